#!/usr/bin/env python3
"""One hash per engine over its recorded launch plans: the proof that a change of the engine code moved no launch.

Builds every engine family at batch 4 (the smallest batch at which the forward still splits into two chains), train and eval,
bf16 and fp32, under the default schedule and the serial one of tests/_spread.py, and prints one line per engine.  The hash covers
the prep, fwd, bwd and DropPath plans after finalize(): per recorded call the function name, the label, the lane and the arguments,
the pseudo calls (join / mark / signal / wait) included, then the plan's marks.  Descriptors passed by reference and the batched
descriptor arrays of flush() are expanded field by field.  Which values are pointers comes from _lib._SIGS and the descriptor
field types; a pointer is replaced by the ordinal of its first appearance in the engine, so addresses do not matter while
aliasing and slicing do.  Plans are built only; no kernel runs.

    python tools/plan_fingerprint.py [--dump DIR] > new.txt      # at both commits, then: diff old.txt new.txt
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import imagenet_models_amd as A  # noqa: E402
from _spread import SERIAL  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NAMED = [('ga_convnext_tiny_768', {}), ('ga_convnext_tiny_768', dict(gram_fp64=True)), ('ga_convnext_tiny_688', {}),
         ('ga_CSWin_64_12211_tiny_224', {}), ('map_convnext_tiny', {}), ('map_vit_small_patch16_224', {}), ('map_pit_s', {}),
         ('pit_s', {}), ('convnext_tiny', {}), ('mobilenet_v1', {}), ('map_mobilenet_v1', {}), ('map_resnet50', {})]


def _golden_cfg(name, tuples):
    cfg = json.loads(str(np.load(os.path.join(GOLDEN, name))['cfg']))
    cfg.update({k: tuple(cfg[k]) for k in tuples})
    return cfg


def models():
    """(tag, factory) of every engine family and option the fingerprint covers"""
    for name, kw in NAMED:
        for dp in (None, 0.1):          # without DropPath sites, and with (create_model drops a None)
            tag = name + ''.join(f'+{k}' for k in kw) + ('+droppath' if dp else '')
            yield tag, lambda name=name, kw=kw, dp=dp: A.create_model(name, drop_path_rate=dp, **kw)
    c = _golden_cfg('cswin_v6b_eval.npz', ('depth', 'split_size', 'num_heads', 'dims'))       # narrow, SE-Bottleneck stage 5
    yield 'cswin_narrow_bottleneck', lambda: A.GA_CSWinTransformer(
        num_classes=c['num_classes'], embed_dim=c['embed_dim'], depth=c['depth'], split_size=c['split_size'], num_heads=c['num_heads'],
        dims=c['dims'], stage3_naggre=c['naggre'], ga_mlp_groups=c['ga_mlp_groups'], ga_layer_mlp_groups=c['ga_layer_mlp_groups'],
        branches=c['branches'], gram_dim=c['gram_dim'], stage5=c['stage5'], stage5_mlp_groups=c['stage5_mlp_groups'], drop_path_rate=0.1)
    for tag in ('split', 'nosdt', 'linear', 'inter', 'mismatch'):
        v = _golden_cfg(f'mapvar_{tag}_eval.npz', ('dims', 'depths'))
        yield 'mapvar_' + tag, lambda v=v: A.MAP_ConvNeXt(
            num_classes=v['num_classes'], depths=v['depths'], dims=v['dims'], last_dim=v['last_dim'], n_groups=v['n_groups'],
            n_tokens=v['n_tokens'], gram_group=v['gram_group'], bp_dim=v['bp_dim'], ca_dim=v['ca_dim'], num_heads=v['num_heads'],
            head_fn=v['head_fn'], self_distill_token=v['self_distill_token'], interactive=v['interactive'], gram_dim=v['gram_dim'])


class Canon:
    """canonical text of an engine's plans"""

    def __init__(self):
        self.ids, self.lines = {}, []

    def ref(self, v, kind='p'):
        return 'null' if not v else f'{kind}{self.ids.setdefault((kind, v), len(self.ids))}'

    def value(self, v, typ):
        if typ is C.c_void_p:
            return self.ref(v.value if isinstance(v, C.c_void_p) else v)
        if isinstance(typ, type) and issubclass(typ, C.Array):
            return [self.value(x, typ._type_) for x in v]
        if isinstance(typ, type) and issubclass(typ, C._Pointer):       # a descriptor passed with byref()
            return self.struct(v._obj)
        return repr(v)      # sizes, strides, scalars

    def struct(self, s):
        return {name: self.value(getattr(s, name), typ) for name, typ in s._fields_}

    def plan(self, p):
        p.finalize()
        batches = {t.data_ptr(): arr for t, arr in zip(p.keep, p.keep[1:]) if isinstance(t, torch.Tensor) and isinstance(arr, C.Array)}
        self.lines.append(f'== {p.name}: {len(p.calls)} calls')
        for (fn, args, label), lane in zip(p.calls, p.lanes):
            types = getattr(fn, 'argtypes', None)
            if types is None:      # join / mark / signal / wait: tags and lanes as they are, events by identity
                vals = [a if isinstance(a, (str, int)) else self.ref(id(a), 'e') for a in args]
            else:
                vals = [self.value(a, t) for a, t in zip(args, types)]
                if fn.__name__.endswith('_batch'):
                    vals.append([self.struct(d) for d in batches[args[0]]])
            self.lines.append(json.dumps([fn.__name__, label, lane, vals]))
        self.lines.append('marks ' + json.dumps(sorted(p.marks.items())))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--only', default='', help='substring of the model tags to build')
    ap.add_argument('--dump', default='', help='directory for the canonical text of every engine (to locate a difference)')
    a = ap.parse_args()
    for tag, make in models():
        if a.only not in tag:
            continue
        torch.manual_seed(0)
        m = make().cuda()
        for sched in ('default', 'serial'):
            for k, v in SERIAL.items():
                os.environ.pop(k, None)
                if sched == 'serial':
                    os.environ[k] = v
            for training in (True, False):
                for mode in ('bf16', 'fp32'):
                    eng = m.make_engine(a.batch, training, mode)
                    c = Canon()
                    for p in (eng.prep, eng.fwd, eng.bwd, vars(eng).get('dp_plan')):
                        if p is not None:
                            c.plan(p)
                    text = '\n'.join(c.lines) + '\n'
                    key = f"{tag} {'train' if training else 'eval'} {mode} {sched}"
                    print(f'{key}: {hashlib.sha256(text.encode()).hexdigest()[:16]} ({len(c.lines)} lines)', flush=True)
                    if a.dump:
                        os.makedirs(a.dump, exist_ok=True)
                        open(os.path.join(a.dump, key.replace(' ', '_') + '.txt'), 'w').write(text)
                    del eng, c
        del m
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
