"""mixup / cutmix on the device for the training step (timm.data.Mixup, mode 'batch', as /root/reference/GA/train.py:544-557
builds it and :727-728 applies it to every batch when --mixup / --cutmix are set -- the reference's defaults 0.2 / 1.0 have it
on).  lam and the cut box are drawn on the host from numpy's generator exactly as timm draws them; the blend / box copy and
the dense smoothed target are HIP kernels (ga_mixup_batch, ga_mixup_target).  The dense (B, num_classes) target goes to
ga_loss / map_loss / TrainStep, which then evaluate SoftTargetCrossEntropy (or BinaryCrossEntropy) on it (train.py:616-621).

Mixup is the --no-prefetcher order of the reference (mix the normalised fp32 batch on the device); no recipe runs it.  With the
prefetcher on, which every recipe has (MAP/train.py:383), timm mixes at COLLATE time: FastCollateMixup blends the uint8 images
and rounds every blended value back to uint8, PrefetchLoader normalises on the device, RandomErasing comes last on the mixed
image.  FastCollateMixup below is that order as one HIP pass (ga_input_collate): a per-sample table {kind, box, lam, 1 - lam}
drawn on the host, so timm's modes 'batch', 'elem' and 'pair' are the same kernel.  Given an fp32 batch it is timm's Mixup in
those modes (no rounding to integers, no normalisation).  Mode 'half' halves the batch the engine was planned for: refused.

timm is not vendored in the reference and not installed: the samplers restate its published algorithm, parity with timm itself
is unpinned (as for oracle/mixup_oracle.py)."""
import numpy as np
import torch

from . import ops, staging

KIND_NONE, KIND_MIXUP, KIND_CUTMIX = 0, 1, 2


class Mixup:
    def __init__(self, mixup_alpha=1.0, cutmix_alpha=0.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                 correct_lam=True, label_smoothing=0.1, num_classes=1000, rng=None):
        if mode != 'batch':
            raise NotImplementedError(f"Mixup mode {mode!r}: only 'batch' is built here; FastCollateMixup runs 'elem' and 'pair' "
                                      '(on uint8 and on fp32 batches)')
        self.mixup_alpha, self.cutmix_alpha, self.cutmix_minmax = mixup_alpha, cutmix_alpha, cutmix_minmax
        if cutmix_minmax is not None:
            assert len(cutmix_minmax) == 2
            self.cutmix_alpha = 1.0          # force cutmix alpha == 1.0 when minmax active to keep logic simple & safe
        self.mix_prob, self.switch_prob = prob, switch_prob
        self.label_smoothing, self.num_classes, self.correct_lam = label_smoothing, num_classes, correct_lam
        self.mixup_enabled = True            # set False to turn it off (--mixup-off-epoch, train.py:705-709)
        self.rng = rng if rng is not None else np.random      # timm draws from the global numpy generator
        self.last = None                     # (lam, use_cutmix, box) of the last call, for logging / tests

    def _params_per_batch(self):
        lam, use_cutmix = 1.0, False
        if self.mixup_enabled and self.rng.rand() < self.mix_prob:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = self.rng.rand() < self.switch_prob
                lam_mix = self.rng.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else \
                    self.rng.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.0:
                lam_mix = self.rng.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.cutmix_alpha > 0.0:
                use_cutmix = True
                lam_mix = self.rng.beta(self.cutmix_alpha, self.cutmix_alpha)
            else:
                raise AssertionError('one of mixup_alpha > 0, cutmix_alpha > 0, cutmix_minmax not None must be true')
            lam = float(lam_mix)
        return lam, use_cutmix

    def _box(self, H, W, lam):
        if self.cutmix_minmax is not None:
            lo, hi = self.cutmix_minmax
            cut_h = self.rng.randint(int(H * lo), int(H * hi))
            cut_w = self.rng.randint(int(W * lo), int(W * hi))
            yl = self.rng.randint(0, H - cut_h)
            xl = self.rng.randint(0, W - cut_w)
            box = (yl, yl + cut_h, xl, xl + cut_w)
        else:
            ratio = np.sqrt(1 - lam)
            cut_h, cut_w = int(H * ratio), int(W * ratio)
            cy, cx = self.rng.randint(0, H), self.rng.randint(0, W)
            box = (int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H)),
                   int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W)))
        if self.correct_lam or self.cutmix_minmax is not None:
            lam = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / float(H * W)
        return box, lam

    def __call__(self, x, target):
        """x: (B, C, H, W) fp32 on the device, target: (B,) int64 -> (mixed x (a new tensor), dense target (B, num_classes))"""
        if not x.is_cuda:
            raise RuntimeError('Mixup runs on the HIP kernels only (no CPU fallback)')
        if not x.is_floating_point():
            raise TypeError(f'Mixup expects a normalised floating-point batch, got {x.dtype}: normalise uint8 input first '
                            '(TrainStep does; engine.normalize_u8)')
        B, _, H, W = x.shape
        assert B % 2 == 0, 'Batch size should be even when using this'
        lam, use_cutmix = self._params_per_batch()
        box = (0, 0, 0, 0)
        x = x.float().contiguous()
        p = ops.Plan(eager=True)
        if lam != 1.0:
            if use_cutmix:
                box, lam = self._box(H, W, lam)
            out = torch.empty_like(x)
            p.mixup_batch(x, out, lam, use_cutmix, box)
        else:
            out = x
        dense = torch.empty(B, self.num_classes, device=x.device, dtype=torch.float32)
        p.mixup_target(target.contiguous(), dense, self.num_classes, lam, self.label_smoothing)
        self.last = (lam, use_cutmix, box)
        return out, dense


class FastCollateMixup(Mixup):
    """timm's FastCollateMixup + PrefetchLoader order on the device: mix the uint8 batch (rounded back to uint8), normalise,
    erase -- one pass (ga_input_collate).  Same constructor as Mixup; mode 'batch' | 'elem' | 'pair'.  The partner of sample i
    is B-1-i.  Parameters are drawn on the host from self.rng in timm's order (sample())."""

    def __init__(self, mixup_alpha=1.0, cutmix_alpha=0.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                 correct_lam=True, label_smoothing=0.1, num_classes=1000, rng=None):
        if mode == 'half':
            raise ValueError("FastCollateMixup mode 'half' returns half of the batch: the engine is planned for the full batch size, "
                             "so it is not built ('batch', 'elem' or 'pair')")
        if mode not in ('batch', 'elem', 'pair'):
            raise ValueError(f"FastCollateMixup mode {mode!r}: 'batch', 'elem' or 'pair'")
        super().__init__(mixup_alpha, cutmix_alpha, cutmix_minmax, prob, switch_prob, 'batch', correct_lam, label_smoothing,
                         num_classes, rng)
        self.mode = mode
        self.last = None                     # the int32 (B, 8) table of the last call, for logging / tests
        self._ring, self._dev, self._out, self._dense = staging.Ring(), None, None, None

    def _params_per_elem(self, n):
        lam = np.ones(n, dtype=np.float32)
        use_cutmix = np.zeros(n, dtype=bool)
        if self.mixup_enabled:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = self.rng.rand(n) < self.switch_prob
                lam_mix = np.where(use_cutmix, self.rng.beta(self.cutmix_alpha, self.cutmix_alpha, size=n),
                                   self.rng.beta(self.mixup_alpha, self.mixup_alpha, size=n))
            elif self.mixup_alpha > 0.0:
                lam_mix = self.rng.beta(self.mixup_alpha, self.mixup_alpha, size=n)
            elif self.cutmix_alpha > 0.0:
                use_cutmix = np.ones(n, dtype=bool)
                lam_mix = self.rng.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
            else:
                raise AssertionError('one of mixup_alpha > 0, cutmix_alpha > 0, cutmix_minmax not None must be true')
            lam = np.where(self.rng.rand(n) < self.mix_prob, lam_mix.astype(np.float32), lam)
        return lam, use_cutmix

    def _draw(self, B, H, W):
        """-> (int32 (B, 8) table {kind, yl, yh, xl, xh, bits(l), bits(m), 0}, lam): lam is the python float of 'batch' mode (the
        target kernel forms its complement in double) or the float32 (B,) vector of 'elem' / 'pair'"""
        assert B % 2 == 0, 'Batch size should be even when using this'
        tab = np.zeros((B, 8), dtype=np.int32)
        lm = tab[:, 5:7].view(np.float32)                     # l, m as their bit patterns
        if self.mode == 'batch':
            lam, use_cutmix = self._params_per_batch()
            if lam != 1.0:
                if use_cutmix:
                    box, lam = self._box(H, W, lam)
                    tab[:, 0] = KIND_CUTMIX
                    tab[:, 1:5] = box
                else:
                    tab[:, 0] = KIND_MIXUP
            lm[:, 0] = np.float32(lam)
            lm[:, 1] = np.float32(1.0 - lam)                  # numpy with a scalar lam: the complement in double, rounded once
            return tab, lam
        n = B if self.mode == 'elem' else B // 2
        lam, use_cutmix = self._params_per_elem(n)
        for i in range(n):
            if lam[i] == 1.0:
                continue
            rows = (i,) if self.mode == 'elem' else (i, B - 1 - i)
            if use_cutmix[i]:
                box, lam[i] = self._box(H, W, lam[i])         # the corrected lam goes back into the float32 vector
                for r in rows:
                    tab[r, 0] = KIND_CUTMIX
                    tab[r, 1:5] = box
            else:
                for r in rows:
                    tab[r, 0] = KIND_MIXUP
        if self.mode == 'pair':
            lam = np.concatenate((lam, lam[::-1]))
        lm[:, 0] = lam
        lm[:, 1] = np.float32(1.0) - lam                      # numpy with a float32 lam vector: subtracted in fp32
        return tab, lam

    def sample(self, B, H, W):
        """the per-sample mix table of one batch (host only): int32 (B, 8) rows {kind, yl, yh, xl, xh, bits(l), bits(m), 0};
        `table[:, 5:7].view(np.float32)` are l and m"""
        return self._draw(B, H, W)[0]

    def __call__(self, x, target, random_erasing=None, mean=None, std=None):
        """x: (B, C, H, W) uint8 on the device (mixed in uint8, then normalised with mean / std, 0..255 units) or fp32 (mixed as
        it is); target: (B,) int64; random_erasing: an imagenet_models_amd.RandomErasing whose boxes are filled in the same
        pass, on the mixed image -> (fp32 batch, dense target (B, num_classes)), both in buffers this object owns and reuses"""
        x = staging.check_batch(x, 'FastCollateMixup', stats=(mean, std))
        B, _, H, W = x.shape
        tab, lam = self._draw(B, H, W)
        # one staging block: the (B, 8) table and, behind it, bits(l) once more: the fp32 lam[B] of ga_mixup_target_elem
        self._dev = staging.buffer(self._dev, (B * 9,), torch.int32, x.device)
        self._ring.upload(np.concatenate((tab.reshape(-1), tab[:, 5])), self._dev)
        self._out = staging.buffer(self._out, x.shape, torch.float32, x.device)
        self._dense = staging.buffer(self._dense, (B, self.num_classes), torch.float32, x.device)
        p = ops.Plan(eager=True)
        boxes, max_count, mode, seed, offset = random_erasing.stage(x) if random_erasing is not None else (None, 0, 0, 0, 0)
        p.input_collate(x, self._out, self._dev[:B * 8], boxes, max_count, mode, seed, offset, mean, std)
        target = target.contiguous()
        if self.mode == 'batch':
            p.mixup_target(target, self._dense, self.num_classes, lam, self.label_smoothing)
        else:
            p.mixup_target_elem(target, self._dense, self.num_classes, self._dev[B * 8:].view(torch.float32), self.label_smoothing)
        self.last = tab
        return self._out, self._dense
