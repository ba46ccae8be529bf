"""Parameter fill of the MobileNetV1 fixtures (tests/golden/mnv1_*.npz, map_mnv1_*.npz; tools/gen_golden_mobilenet.py): the
name-hashed rule of oracle/map_oracle.fill_state applied to a state_dict's own names and shapes, so that the fixture generator
(reference classes) and the GPU tests (this package's containers) fill identical states without shipping them."""
import math
import zlib
from collections import OrderedDict

import numpy as np
import torch


def fill_state(shapes, seed=0):
    """shapes: OrderedDict name -> shape (a state_dict's); returns the filled state_dict (bp_index: the triu index of its size)"""
    sd = OrderedDict()
    for name, shape in shapes.items():
        shape = tuple(shape)
        rs = np.random.RandomState((zlib.crc32(name.encode()) + 7919 * seed) & 0x7FFFFFFF)
        leaf = name.rsplit('.', 1)[-1]
        if leaf == 'num_batches_tracked':
            sd[name] = torch.zeros((), dtype=torch.int64)
            continue
        if leaf == 'bp_index':
            bp = int(round(math.sqrt(2 * shape[0] + 0.25) - 0.5))
            t = torch.triu_indices(bp, bp)
            sd[name] = t[0] * bp + t[1]
            continue
        if leaf == 'running_mean':
            v = rs.uniform(-0.1, 0.1, shape)
        elif leaf == 'running_var':
            v = rs.uniform(0.5, 1.5, shape)
        elif len(shape) >= 2:
            v = rs.standard_normal(shape) * (1.0 / math.sqrt(int(np.prod(shape[1:]))))
        elif leaf == 'weight':
            v = rs.uniform(0.8, 1.2, shape)
        else:
            v = rs.uniform(-0.1, 0.1, shape)
        sd[name] = torch.tensor(v, dtype=torch.float32)
    return sd


def running_names(names):
    return [n for n in names if n.endswith('running_mean') or n.endswith('running_var')]
