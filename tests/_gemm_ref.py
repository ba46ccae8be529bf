"""Float64 reference of ga_gemm's NT product with its epilogue (include/gaext.h), the ONE gate the kernel tests hold csrc/gemm.hip's
forms to, fp32 restatements of the accumulation in its documented order and roundings, wrong restatements the gate has to reject,
and the case table shared by tests/test_gemm_ref_cpu.py, tests/test_gemm_forms_edges_gpu.py and tools/gemm_forms.py.

    C[z][m][n] = epilogue(alpha * sum_k A[za][m][k] B[z][n][k]),  za = z % a_batch_mod (0: z); tensors are [Z][M][K], [Z][N][K], [Z][M][N]
    epilogue order: v = alpha acc; v += bias[n]; (C2 store); v = act(v); v *= gelu'(H) | H; v *= rowscale[m / rows_per_scale]; v += R;
                    relu_after; colsum[n] += v; colsumsq[n] += v v; store
Everything is float64 on the CPU, from inputs that are exactly representable in the dtype the kernel reads them in.  The fused fc1
epilogue of the bf16 forms is the logistic (tanh-form) GELU  x s(1.5957691216 (x + 0.044715 x^3))  and its exact derivative, the
operation gelu_both_fast (csrc/common.h) computes; the generic epilogue and the fp32 mode use the exact-erf GELU.
Every output comes with the per-element absolute sum A of its terms, |alpha| (|a| @ |b|^T) + |bias| carried through the epilogue
(times |H|, |rowscale|, plus |R|; a column sum: the sum of its rows' A; a column sum of squares: 3 sum A^2, which covers
2 |v| t + t^2 for an element error t <= A), and with E, the allowance of a GELU evaluated in fp32 (below), carried the same way.

gate(): per element  |got - ref| <= r |ref| + u A + E,  nothing relative to the tensor's maximum.
    r = 2^-8 for an output stored as bf16 (ONE round-to-nearest); 0 for fp32 outputs (c_f32, fp32 mode, colsum, colsumsq)
    u = 2^-24 L, L = the longest chain of fp32 roundings in the form that ran.  From csrc/gemm.hip, for every form in the table:
        staged128 / 96 / 64, big, dma128, dma256x128 / x96, t256 (gemm_nt_kernel), pp (gemm_nt_pp_kernel), r3 (gemm_nt_r3_kernel):
          one accumulator per output element and wave, chained v_mfma_f32_16x16x32_bf16 over K, which gemm_nt_kernel and pp bring
          in as slabs of 64 bf16 (two MFMAs; nk = ceil(K / 64), ring of 1, 2 or 3 slots) and r3 as stages of 32 (one MFMA;
          nk = ceil(K / 32), ring of three); the chunks of a ragged last slab / stage beyond K read as zeros, so the number of
          roundings is the same; no form splits K over waves or workgroups, and no partial tiles meet: K products
          + ceil(K / 32) accumulates; fp32 mode (staged only): v_mfma_f32_16x16x4f32, K + ceil(K / 4)
          epilogue: alpha, bias, activation (counted 3), H, row scale, residual: at most 8 more
          L_gemm = K + ceil(K / 32 | 4) + 8
        column sums: a thread adds the rows it owns of a tile (at most the tile's 256), the row groups / lanes of the workgroup meet
          (at most 64 partials), one fp32 atomic per tile row (ceil(M / 128) at most): L_col = 256 + 64 + ceil(M / 128), on top of
          L_gemm for the elements themselves.  This is the issue's recipe taken literally and it is loose: u (L_gemm + L_col) sum A is
          about 5 % of a typical column sum at M = 8200, K = 264 (3 sum A^2: 2.5 % of a sum of squares), the GPU ratios are 0.001,
          and a wrong term is certain to be seen only where it is large (colsum_rows: through the outlier bias columns).  A tighter
          bound would take the depth of the sum times the partial sums instead of its length times sum A.
      (with K <= 520 u A is far below r |ref| unless the sum cancels -- at K = 264 it is 4e-3 for |ref| of 14 on average -- so a few
      units of generosity cost nothing; where a term has to be found in an element that cancelled, the impulse kind finds it)
    E = g max(1, |x|) for a GELU or GELU' of x evaluated in fp32 through v_exp_f32 / v_rcp_f32.  g is the one constant that cannot
        be derived: it is MEASURED, on the reference's side only -- the torch fp32 restatements gelu_fast_f32 / gelu_erf_f32 below
        against the float64 forms on 2^21 + 1 points of [-13, 13] and on the cases' own pre-activations, worst |err| / max(1, |x|):
            logistic GELU   1.41e-07   allowed G_FAST_ACT  = 5.7e-07          logistic GELU'  5.59e-07   allowed G_FAST_GRAD = 2.3e-06
            erf GELU        1.82e-07   allowed G_ERF_ACT   = 7.3e-07          erf GELU'       2.91e-07   allowed G_ERF_GRAD  = 1.2e-06
        (allowed = 4 x measured: the hardware instructions are 1-ulp approximations where torch's are correctly rounded; the erf
        form is Abramowitz-Stegun 7.1.26, |erf error| <= 1.5e-7, which the measurement contains).  tests/test_gemm_ref_cpu.py
        measures them again and asserts they stay below the allowance.

Input kinds:
    plain    |a| in [0.5, 2], |b| in [0.25, 1], |R|, |H| in [0.5, 2], |bias| in [0.25, 1], random signs, values of the dtype; every row,
             column and batch element carries its own values, so a read from a neighbour is off by O(1).  Four columns carry a bias
             of +8, -8, +12, -12 (exp2 of the logistic form overflows to inf and underflows there); the row-scale vector cycles
             through 1.25, 0, 2, 1, 0.5, 1.5: every sixth group is a dropped DropPath sample whose rows must equal R bit for bit
    impulse  (the GPU module) each row of A is one-hot at k = (7 m + 3) % K, no bias: the plain output equals B[n, k_m] bit for bit
a_act = GELU rounds gelu(a) to bf16 while staging: `aact` inputs keep every a whose gelu lies within 2^-12 of a rounding boundary out
of A, so that the staged operand is the same bf16 value on both sides.
"""
import math

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
R_BF16, U = 2.0 ** -8, 2.0 ** -24
G_MEASURED = dict(fast_act=1.41e-07, fast_grad=5.59e-07, erf_act=1.82e-07, erf_grad=2.91e-07)
G_FAST_ACT, G_FAST_GRAD, G_ERF_ACT, G_ERF_GRAD = 5.7e-07, 2.3e-06, 7.3e-07, 1.2e-06
ALPHA = 0.75          # alpha of the generic cases


def rnd_to(t, dt):
    """the values of float64 `t` rounded to dtype dt, as float64"""
    return t.to(F32).to(dt).to(F64)


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------------------
# GELU: float64 forms and the fp32 restatements of csrc/common.h
# ------------------------------------------------------------------------------------------------------------------------------
def gelu_tanh64(x):
    """logistic (tanh-form) GELU and its exact derivative"""
    z = 1.5957691216 * (x + 0.044715 * x ** 3)
    s = torch.sigmoid(z)
    return x * s, s + x * s * (1 - s) * 1.5957691216 * (1 + 3 * 0.044715 * x * x)


def gelu_erf64(x):
    cdf = 0.5 * (1 + torch.erf(x / math.sqrt(2.0)))
    return x * cdf, cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _fmaf(a, b, c):
    """fmaf on fp32 tensors: one rounding (b, c may be Python floats, taken as the fp32 constants the kernel holds)"""
    f = lambda v: v.to(F64) if torch.is_tensor(v) else float(torch.tensor(v, dtype=F32))
    return (f(a) * f(b) + f(c)).to(F32)


def gelu_fast_f32(x):
    """gelu_both_fast: x fp32 -> (act, grad) fp32"""
    x2 = x * x
    e = torch.exp2(x * _fmaf(x2, -0.10294324, -2.3022082))
    s = 1.0 / (1.0 + e)
    zp = _fmaf(x2, 0.21406186, 1.5957691)
    return x * s, _fmaf(x * (s - s * s), zp, s)


def gelu_erf_f32(x):
    """gelu_both_f / gelu_f / gelu_grad_f (Abramowitz-Stegun 7.1.26): x fp32 -> (act, grad) fp32"""
    z = x.abs() * torch.tensor(0.70710678118654752, dtype=F32)
    t = 1.0 / _fmaf(z, 0.3275911, 1.0)
    p = _fmaf(t, 1.061405429, -1.453152027)
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = _fmaf(p, t, c)
    e = torch.exp(-z * z)
    h = 0.5 * p * t * e
    cdf = torch.where(x >= 0, 1.0 - h, h)
    return x * cdf, _fmaf(x * torch.tensor(0.3989422804014327, dtype=F32), e, cdf)


def gelu_constants(extra=None):
    """the measured g of the four fp32 GELU evaluations: dense grid of [-13, 13] plus the fp32 tensor `extra`"""
    x = torch.linspace(-13, 13, 2 ** 21 + 1, dtype=F64).to(F32)
    if extra is not None:
        x = torch.cat([x, extra.reshape(-1).to(F32)])
    den = x.to(F64).abs().clamp(min=1.0)
    out = []
    for f32, f64 in ((gelu_fast_f32, gelu_tanh64), (gelu_erf_f32, gelu_erf64)):
        got, ref = f32(x), f64(x.to(F64))
        out += [float(((g.to(F64) - r).abs() / den).max()) for g, r in zip(got, ref)]
    return dict(zip(('fast_act', 'fast_grad', 'erf_act', 'erf_grad'), out))


# ------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------
OFF = dict(NT_R3=0, NT_DMA=0, NT_PP=0, NT_T256=0, NT_DMA2=0, NT_BIG=0, FEWROWS=0)
FAMILIES = {
    'staged': dict(OFF), 'big': dict(OFF, NT_BIG=1), 'dma128': dict(OFF, NT_DMA2=15, NT_DMA2_MINK=8), 'dma256': dict(OFF, NT_DMA=2),
    't256': dict(OFF, NT_T256=15), 'pp': dict(OFF, NT_PP=15), 'r3': dict(NT_R3=15),
}
TILE_M = {'staged': 128, 'big': 256, 'dma128': 128, 'dma256': 256, 't256': 256, 'pp': 256, 'r3': 256}
CLS = {'plain': 'plain', 'fc1': 'fc1', 'fc1_noc2': 'fc1', 'fc2': 'fc2', 'fc2_nors': 'fc2', 'dg2': 'dg2',
       'gen_full': 'generic', 'gen_full_cf32': 'generic', 'gen_aact': 'generic'}
FUSED = ('plain', 'fc1', 'fc1_noc2', 'fc2', 'fc2_nors', 'dg2')
GENERIC = ('gen_full', 'gen_full_cf32', 'gen_aact')


class Case:
    """one product M x N x K (batch Z) and the families it runs on: fams maps a family to the form name's prefix at 256 CUs"""

    def __init__(self, M, N, K, Z, fams, edge, rps=7, pad=True, grouped=False, dt=BF, epis=FUSED):
        self.M, self.N, self.K, self.Z, self.fams, self.edge = M, N, K, Z, fams, edge
        self.rps, self.pad, self.grouped, self.dt, self.epis = rps, pad, grouped, dt, epis
        self.label = f'{M}x{N}x{K}' + (f'z{Z}' if Z > 1 else '') + ('g' if grouped else '') + ('' if pad else 't') + \
            ('-f32' if dt == F32 else '') + ('-gen' if epis is GENERIC else '')

    def __repr__(self):
        return self.label

    def epis_of(self, fam):
        return tuple(e for e in self.epis if fam != 'big' or CLS[e] in ('fc2', 'dg2'))

    def tile_n(self):
        """column-tile width of the staged / LDS-DMA forms (gemm_select.h nt_tile_width)"""
        N = self.N
        for w in (128, 96, 64):
            if N % w == 0:
                return w
        waste = {w: _cdiv(N, w) * w for w in (128, 96, 64)}
        return 128 if waste[128] <= waste[96] and waste[128] <= waste[64] else (96 if waste[96] <= waste[64] else 64)

    def want(self, fam, epi):
        """the form name ga_gemm_form must give"""
        name = f'{self.fams[fam]}:{CLS[epi]}'
        if fam == 'staged':
            pre = self.dt == BF and (CLS[epi] in ('fc2', 'dg2') or epi in ('gen_full', 'gen_full_cf32'))
            name += ('+pre' if pre else '') + ('+f32' if self.dt == F32 else '')
        return name


S128 = dict(staged='staged128', big='big', dma128='dma128')
S96, S64 = dict(staged='staged96'), dict(staged='staged64')
SIX = dict(staged='staged128', big='big', dma128='dma128', dma256='dma256x128', pp='pp', r3='r3')
FOUR = dict(staged='staged128', big='big', dma128='dma128', dma256='dma256x128')
D96 = dict(staged='staged96', dma256='dma256x96')
ALL7 = dict(SIX, t256='t256')

CASES = [
    # ---- a few tiles: the 128-row forms (staged, dma128) and the 256-row big form
    Case(257, 128, 8, 1, S128, 'K = one chunk; M one row over two 128-row tiles and over one 256-row tile'),
    Case(129, 128, 64, 1, S128, 'K = exactly one slab; M one row over a 128-row tile', pad=False),
    Case(255, 128, 128, 1, S128, 'K = two slabs = the ring slots of dma128; M one row short of two 128-row tiles / one 256-row tile'),
    Case(300, 100, 200, 1, S128, 'N % 8 != 0 with ldc > N; K = three slabs and a ragged one'),
    Case(7, 128, 136, 1, S128, 'M < 8; K = two slabs and a ragged one', rps=100),
    Case(300, 136, 72, 1, S96, 'staged 96-column tiles, last one mostly empty; K = slab plus ragged tail'),
    Case(257, 132, 72, 1, S96, 'staged 96-column tiles, N % 8 != 0'),
    Case(5, 40, 96, 1, S64, 'staged 64-column tile, M < 8'),
    # ---- thin batched launches: M < 8 on every form, the K ladder of the ring forms at little cost (one tile per batch element,
    # fewer tiles than workgroups)
    Case(7, 256, 8, 128, FOUR, 'M < 8, K = one chunk, batch 128', rps=100),
    Case(5, 256, 64, 128, dict(FOUR, r3='r3'), 'K = one slab: fewer slabs than ring slots'),
    Case(7, 256, 72, 128, dict(FOUR, r3='r3'), 'K = slab plus ragged tail', pad=False, rps=100),
    Case(7, 256, 128, 128, dict(FOUR, r3='r3'), 'K = two slabs', rps=100),
    Case(7, 256, 96, 128, dict(FOUR, r3='r3'), 'r3: exactly three whole stages of 32 = its ring; the others: a ragged slab of 4 chunks', rps=100),
    Case(7, 256, 104, 128, dict(FOUR, r3='r3'), 'a ragged tail of several chunks: 40 of 64 (r3: 8 of 32 after three stages)', rps=100),
    Case(7, 250, 200, 128, FOUR, 'N % 8 != 0 (ldc 256 + pad), K = three slabs and a ragged one', rps=100),
    Case(7, 256, 520, 256, ALL7, 'M < 8 on all seven families; K = eight slabs and a ragged one; batch 256: grid cap 8', rps=100),
    Case(7, 512, 328, 128, dict(t256='t256', pp='pp'), 'K = five slabs and a ragged one on the 256 x 256 forms', rps=100),
    Case(7, 2048, 296, 32, ALL7, 'batch 32, exactly one tile per workgroup: pp and t256 8 tiles on 8, r3 and dma128 16 on 16 '
         '(dma256: 16 on 8); K = four slabs and a tail of 5 chunks', rps=100),
    Case(7, 2560, 264, 32, ALL7, 'batch 32, more tiles than workgroups on every family: pp and t256 10 on 8, r3 and dma128 20 on 16, '
         'dma256 20 on 8', rps=100),
    # ---- the 256-row forms at their grid edges
    Case(8200, 1024, 264, 1, SIX, 'unbatched: 33 tile rows, the last of 8 rows; 264 tiles of 256 x 128 on a grid of 256 (dma256: the slab '
         'stream crosses a tile boundary, xcd_remap wraps), 520 of 128 x 128 on 512 (dma128); fewer tiles than workgroups for pp, r3'),
    Case(520, 1000, 328, 11, SIX, 'last column tile 104 of 128 (pp: 232 of 256); batch 11'),
    Case(520, 1004, 136, 11, FOUR, 'N % 8 != 0 on the forms that accept it, ldc 1008 + pad'),
    Case(257, 288, 104, 43, D96, 'dma256x96: M one row over a 256-row tile, three full 96-column tiles; K tail of 5 chunks'),
    Case(513, 260, 136, 29, D96, 'dma256x96 with N % 8 != 0: last tile 68 of 96'),
    Case(520, 264, 264, 32, dict(D96, pp='pp', r3='r3'), 'batch 32: grid cap 8, 9 tiles of 256 x 96 (wraps); pp 6 tiles, r3 9 of 16'),
    Case(513, 520, 264, 17, dict(D96, pp='pp'), 'batch 17: grid cap 8; pp 9 full-height tiles on 8 workgroups: its K-tile stream crosses '
         'a tile boundary and xcd_remap wraps; dma256x96 18 on 8'),
    Case(1023, 264, 296, 17, dict(staged='staged96', pp='pp'), 'batch 17: pp 8 full-height tiles on 8 workgroups, exactly one each, the '
         'second column tile 8 of 256; K tail of 5 chunks'),
    Case(513, 264, 200, 64, dict(D96, r3='r3'), 'batch 64: r3 capped at 8 workgroups, 9 tiles: the ring crosses a tile boundary'),
    Case(1023, 256, 264, 32, SIX, 'a_batch_mod = 2, every batch writes its own column block of one C; M one row short of four '
         '256-row tiles; dma256: 8 tiles on 8 workgroups, exactly one each (pp 4 on 8, r3 8 on 16, dma128 16 on 16)', grouped=True),
    Case(1025, 256, 256, 32, SIX, 'M one row over four 256-row tiles; dma256: 10 tiles on 8 workgroups (pp 5 on 8, r3 10 on 16, dma128 18 on 16); '
         'K = exactly four slabs', rps=100),
    Case(257, 256, 256, 128, dict(t256='t256'), 't256 at its hard K bound, M one row over a tile'),
    Case(257, 1280, 264, 32, dict(t256='t256'), 't256: 10 tiles on 8 workgroups', rps=100),
    Case(511, 512, 264, 64, dict(t256='t256'), 't256: M one row short of two tiles (a 256 x 256 form needs 256 tiles: no smaller shape)', rps=100),
    # ---- generic epilogue and fp32 mode (staged only), the three tile widths
    Case(257, 128, 72, 2, dict(staged='staged128'), 'generic, 128-column tile, batch 2', epis=GENERIC),
    Case(300, 136, 200, 1, S96, 'generic, 96-column tiles', epis=GENERIC),
    Case(5, 40, 96, 1, S64, 'generic, 64-column tile, M < 8', epis=GENERIC),
    Case(257, 128, 72, 2, dict(staged='staged128'), 'fp32 mode, generic, batch 2', rps=100, dt=F32, epis=GENERIC),
    Case(300, 132, 200, 1, S96, 'fp32 mode, 96-column tiles, N % 8 != 0', dt=F32, epis=GENERIC),
    Case(5, 40, 96, 1, S64, 'fp32 mode, 64-column tile', dt=F32, epis=GENERIC),
    Case(129, 128, 64, 1, dict(staged='staged128'), 'fp32 mode, fused epilogues', dt=F32),
]
assert len({c.label for c in CASES}) == len(CASES)
assert all(c.rps in (7, 100) and c.M % c.rps and 128 % c.rps and 256 % c.rps for c in CASES)      # divides neither a tile height nor M
PAIRS = [(c, f) for c in CASES for f in c.fams]

# workgroups per CU of the families whose occupancy follows from their LDS (gemm.hip: 160 / 120 KiB dma256, 144 KiB t256, 160 KiB pp:
# one; 80 KiB r3 and dma128: two).  staged and big ask the runtime (hipOccupancyMaxActiveBlocksPerMultiprocessor); by their
# registers big holds one workgroup per CU and staged two to four, which the table does not rely on
PER_CU = {'pp': 1, 't256': 1, 'dma256': 1, 'r3': 2, 'dma128': 2}


def grid(c, fam, cus=256):
    """(tiles per batch element, workgroups per batch element) of a launch: launch_nt_, launch_nt_pp, launch_nt_r3_"""
    bn = {'pp': 256, 't256': 256, 'r3': 128, 'dma128': 128}.get(fam) or c.tile_n()
    return _cdiv(c.M, TILE_M[fam]) * _cdiv(c.N, bn), max(8, PER_CU[fam] * cus // c.Z // 8 * 8)


def layout(c):
    """leading dimensions and strides (elements): wider than the matrices unless the case is `tight`"""
    N8 = _cdiv(c.N, 8) * 8
    p = 8 if c.pad else 0
    d = dict(lda=c.K + p, ldb=c.K + 2 * p, ldc=N8 + p, ldr=N8 + 2 * p, ldh=N8 + 3 * p, strideBias=c.N + (3 if c.pad else 0),
             strideCol=c.N + (5 if c.pad else 0))
    if c.grouped:
        d['ldc'] = c.Z * c.N + p
    d.update(strideA=c.M * d['lda'], strideB=c.N * d['ldb'], strideC=c.N if c.grouped else c.M * d['ldc'],
             strideR=c.M * d['ldr'], strideH=c.M * d['ldh'])
    return d


def gemm_kwargs(c, epi, ops, impulse=False):
    """keyword arguments of ops.Plan.gemm after (A, B, C, M, N, K, dtype) for one launch; operands are named by strings ('bias', 'R',
    'H', 'C2', 'rowscale', 'colsum', 'colsumsq') that the caller replaces by its tensors"""
    L = layout(c)
    kw = dict(lda=L['lda'], ldb=L['ldb'], ldc=L['ldc'], batch=c.Z, strideA=L['strideA'], strideB=L['strideB'], strideC=L['strideC'],
              a_batch_mod=2 if c.grouped else 0)
    bias = {} if impulse else dict(bias='bias', strideBias=L['strideBias'])
    cs = dict(colsum='colsum', strideCol=L['strideCol'])
    R = dict(R='R', ldr=L['ldr'], strideR=L['strideR'])
    H = dict(H='H', ldh=L['ldh'], strideH=L['strideH'])
    rs = dict(rowscale='rowscale', rows_per_scale=c.rps)
    if epi == 'plain':
        kw.update(bias, **cs, colsumsq='colsumsq')
    elif epi == 'fc1':
        kw.update(bias, act=ops.ACT_GELU, C2='C2', c2_mode=2)
    elif epi == 'fc1_noc2':
        kw.update(bias, act=ops.ACT_GELU)
    elif epi == 'fc2':
        kw.update(bias, **rs, **R)
    elif epi == 'fc2_nors':
        kw.update(bias, **R)
    elif epi == 'dg2':
        kw.update(H, h_is_deriv=True, **cs)
    elif epi in ('gen_full', 'gen_full_cf32'):
        # the whole documented order at once; ga_gemm takes a second output only beside a dtype-typed C, so the order runs twice:
        # with C2 (c2_mode 1) and with c_f32
        kw.update(bias, alpha=ALPHA, act=ops.ACT_RELU, **H, **rs, **R, relu_after=True, **cs, colsumsq='colsumsq')
        kw.update(dict(C2='C2', c2_mode=1) if epi == 'gen_full' else dict(c_f32=True))
    else:
        assert epi == 'gen_aact'
        kw.update(bias, a_act=ops.ACT_GELU)
    return kw


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def _mag(shape, lo, hi, g):
    return (lo + (hi - lo) * torch.rand(shape, generator=g, dtype=F64)) * (torch.randint(0, 2, shape, generator=g).to(F64) * 2 - 1)


RS_CYCLE = [1.25, 0.0, 2.0, 1.0, 0.5, 1.5]
OUTLIERS = (8.0, -8.0, 12.0, -12.0)


def outlier_columns(N):
    return sorted({1 % N, N // 3, N // 2, N - 2 if N > 2 else 0})


def make_inputs(c, kind='plain', seed=0):
    """float64 tensors holding values of c.dt: a [Za][M][K], b [Z][N][K], R, H [Z][M][N]; fp32 values: bias [Z][N], rowscale"""
    g = torch.Generator().manual_seed(7000 + seed)
    Za = 2 if c.grouped else c.Z
    i = dict(b=rnd_to(_mag((c.Z, c.N, c.K), 0.25, 1.0, g), c.dt))
    if kind == 'impulse':
        a = torch.zeros(Za, c.M, c.K, dtype=F64)
        a[:, torch.arange(c.M), (7 * torch.arange(c.M) + 3) % c.K] = 1.0
        i['a'] = a
        return i
    i['a'] = rnd_to(_mag((Za, c.M, c.K), 0.5, 2.0, g), c.dt)
    i['R'] = rnd_to(_mag((c.Z, c.M, c.N), 0.5, 2.0, g), c.dt)
    i['H'] = rnd_to(_mag((c.Z, c.M, c.N), 0.5, 2.0, g), c.dt)
    bias = _mag((c.Z, c.N), 0.25, 1.0, g)
    for col, v in zip(outlier_columns(c.N), OUTLIERS):
        bias[:, col] = v
    i['bias'] = bias.to(F32).to(F64)
    i['rowscale'] = torch.tensor((RS_CYCLE * (_cdiv(c.M, c.rps) // 6 + 1))[:_cdiv(c.M, c.rps)], dtype=F64)
    if 'gen_aact' in c.epis and c.dt == BF:         # keep gelu(a) away from the bf16 rounding boundaries
        a = i['a']
        for _ in range(20):
            ga = gelu_erf64(a)[0]
            bad = (rnd_to(ga * (1 + 2.0 ** -12), BF) != rnd_to(ga * (1 - 2.0 ** -12), BF))
            if not bool(bad.any()):
                break
            a = torch.where(bad, rnd_to(_mag(a.shape, 0.5, 2.0, g), BF), a)
        assert not bool(bad.any())
        i['a_aact'] = a
    else:
        i['a_aact'] = i['a']
    return i


def _a_of(c, a):
    """[Z][M][K]: the A each batch element reads"""
    return a[torch.arange(c.Z) % a.shape[0]] if a.shape[0] != c.Z else a


# ------------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------------------------------------
class Out:
    """one output: the reference, its absolute sum A, the GELU allowance E, and r of its storage type"""

    def __init__(self, ref, A, E, r):
        self.ref, self.A, self.E, self.r = ref, A, E, r


def product(c, inp, aact=False):
    """acc = a @ b^T and |a| @ |b|^T, [Z][M][N]; aact: A := gelu(a) rounded to the dtype (fp32 mode: not rounded), also returned as
    the third value: max(1, |a|) @ |b|^T for E"""
    a = _a_of(c, inp['a_aact'] if aact else inp['a'])
    bt = inp['b'].transpose(1, 2)
    if not aact:
        return a @ bt, a.abs() @ bt.abs(), None
    ga = gelu_erf64(a)[0]
    ga = rnd_to(ga, BF) if c.dt == BF else ga
    return ga @ bt, ga.abs() @ bt.abs(), a.abs().clamp(min=1.0) @ bt.abs()


def _rs_rows(c, inp, cd, tile_local=0):
    """row scale of every row [M]; tile_local = BM: the group index restarts at every tile (the wrong restatement)"""
    m = torch.arange(c.M)
    idx = m // c.rps
    if tile_local:
        m0 = m // tile_local * tile_local
        idx = m0 // c.rps + (m - m0) // c.rps
    return inp['rowscale'].to(cd)[idx][None, :, None]


def epilogue(c, inp, epi, acc, cd=F64, wrong=None, tile=(128, 128)):
    """the epilogue on acc [Z][M][N] in compute dtype cd: F64 is the reference (outputs unrounded), F32 a restatement (fp32 GELUs of
    common.h, outputs rounded to their storage type, returned as float64).  wrong: one of WRONG; tile = (BM, BN) of the form"""
    t = lambda x: x.to(cd)
    Z, M, N = acc.shape
    BM, BN = tile
    st = (lambda v: v) if cd == F64 else (lambda v: v.to(c.dt).to(F64))       # storage rounding of a restatement
    f32o = (lambda v: v) if cd == F64 else (lambda v: v.to(F64))
    total = lambda v: v.to(F64).sum(1) if cd == F64 else v.to(F64).sum(1).to(F32).to(F64)
    fast = (CLS[epi] == 'fc1' and c.dt == BF) != (wrong == 'gelu_swap')
    gelu = {(F64, True): gelu_tanh64, (F64, False): gelu_erf64, (F32, True): gelu_fast_f32, (F32, False): gelu_erf_f32}[(cd, fast)]
    bias = t(inp['bias'])[:, None, :]
    if wrong == 'bias_batch0':
        bias = bias[0:1].expand(Z, 1, N)
    if wrong == 'bias_tile':
        bias = bias.clone()
        bias[..., (_cdiv(N, BN) - 1) * BN:] = 0
    R, H = t(inp['R']), t(inp['H'])
    out = {}
    if epi in ('plain', 'gen_aact'):
        v = acc + bias
        out['C'] = st(v)
        if epi == 'plain':
            out['colsum'], out['colsumsq'] = total(v), total(v * v)
            if wrong == 'colsum_rows':        # the rows >= M of the last tile hold the bias
                extra = _cdiv(M, BM) * BM - M
                out['colsum'] = out['colsum'] + extra * bias[:, 0].to(F64)
                out['colsumsq'] = out['colsumsq'] + extra * bias[:, 0].to(F64) ** 2
    elif CLS[epi] == 'fc1':
        out['C'], dg = gelu(acc + bias)
        out['C'] = st(out['C'])
        if epi == 'fc1':
            out['C2'] = st(dg)
    elif CLS[epi] == 'fc2':
        p = acc + bias
        rs = _rs_rows(c, inp, cd, BM if wrong == 'rs_tile' else 0) if epi == 'fc2' else 1.0
        if wrong == 'res_first':
            v = (p + R) * rs
        elif wrong == 'round_twice':
            v = t((p * rs).to(c.dt)) + R
        else:
            v = p * rs + R
        out['C'] = st(v)
    elif epi == 'dg2':
        v = acc * H
        out['C'], out['colsum'] = st(v), total(v)
    else:
        assert epi in ('gen_full', 'gen_full_cf32')
        v = acc * ALPHA + bias
        if epi == 'gen_full':
            out['C2'] = st(v)
        v = torch.relu(v) * gelu(H)[1] * _rs_rows(c, inp, cd)
        v = torch.relu(v + R)
        out['C'] = st(v) if epi == 'gen_full' else f32o(v)
        out['colsum'], out['colsumsq'] = total(v), total(v * v)
    return out


def reference(c, inp, epi, base=None):
    """{name: Out} of one launch; base = product(c, inp[, aact]) when the caller shares it"""
    aact = epi == 'gen_aact'
    acc, Aab, Eab = base or product(c, inp, aact)
    ref = epilogue(c, inp, epi, acc)
    r = R_BF16 if c.dt == BF else 0.0
    ab, aR, aH = inp['bias'].abs()[:, None, :], inp['R'].abs(), inp['H'].abs()
    zero = torch.zeros(())
    sums = lambda A, E: (A.sum(1), E.sum(1) if E.dim() else zero, 3 * (A * A).sum(1), 3 * (A * E).sum(1) if E.dim() else zero)
    o = {}
    if epi in ('plain', 'gen_aact'):
        A = Aab + ab
        E = G_ERF_ACT * Eab if (aact and c.dt == F32) else zero
        o['C'] = Out(ref['C'], A, E, r)
        if epi == 'plain':
            As, Es, Aq, Eq = sums(A, E)
            o['colsum'], o['colsumsq'] = Out(ref['colsum'], As, Es, 0.0), Out(ref['colsumsq'], Aq, Eq, 0.0)
    elif CLS[epi] == 'fc1':
        x = acc + inp['bias'][:, None, :]
        ga, gg = (G_FAST_ACT, G_FAST_GRAD) if c.dt == BF else (G_ERF_ACT, G_ERF_GRAD)
        den = x.abs().clamp(min=1.0)
        o['C'] = Out(ref['C'], 1.2 * (Aab + ab), ga * den, r)          # |gelu'| <= 1.13, |gelu''| <= 0.8
        if epi == 'fc1':
            o['C2'] = Out(ref['C2'], Aab + ab, gg * den, r)
    elif CLS[epi] == 'fc2':
        rs = _rs_rows(c, inp, F64).abs() if epi == 'fc2' else 1.0
        o['C'] = Out(ref['C'], (Aab + ab) * rs + aR, zero, r)
    elif epi == 'dg2':
        A = Aab * aH
        o['C'], o['colsum'] = Out(ref['C'], A, zero, r), Out(ref['colsum'], A.sum(1), zero, 0.0)
    else:
        A0 = ALPHA * Aab + ab
        rs = _rs_rows(c, inp, F64).abs()
        if epi == 'gen_full':
            o['C2'] = Out(ref['C2'], A0, zero, r)
        A = A0 * gelu_erf64(inp['H'])[1].abs() * rs + aR
        E = G_ERF_GRAD * aH.clamp(min=1.0) * torch.relu(acc * ALPHA + inp['bias'][:, None, :]) * rs
        o['C'] = Out(ref['C'], A, E, r if epi == 'gen_full' else 0.0)
        As, Es, Aq, Eq = sums(A, E)
        o['colsum'], o['colsumsq'] = Out(ref['colsum'], As, Es, 0.0), Out(ref['colsumsq'], Aq, Eq, 0.0)
    return o


# ------------------------------------------------------------------------------------------------------------------------------
# the gate
# ------------------------------------------------------------------------------------------------------------------------------
def chain(c, name):
    """L of one output of case c (the same for every form of the table: see the module docstring)"""
    L = c.K + _cdiv(c.K, 32 if c.dt == BF else 4) + 8
    return L + (256 + 64 + _cdiv(c.M, 128) if name.startswith('colsum') else 0)


def gate(got, ref, A, r, u, E=0.0):
    """worst err / allowed over the elements of one tensor (float64 tensors); inf if an element is off where nothing is allowed"""
    err = (got - ref).abs()
    allowed = r * ref.abs() + u * A + E
    ratio = torch.where(err > 0, err / allowed, torch.zeros_like(err))      # 0 / 0 = 0, x / 0 = inf
    ratio = torch.nan_to_num(ratio, nan=float('inf'))
    return float(ratio.max()) if ratio.numel() else 0.0


def gate_out(c, name, got, o):
    return gate(got, o.ref, o.A, o.r, U * chain(c, name), o.E)


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 restatements of the accumulation, for tests/test_gemm_ref_cpu.py
# ------------------------------------------------------------------------------------------------------------------------------
def accumulate(c, inp, aact=False):
    """the fp32 accumulator as every form of the table builds it: K walked in slabs of 64 elements (bf16; a ragged last slab is
    zero-filled), one fp32 rounding per MFMA of 32 exact products (fp32 mode: 4).  Returns (acc, acc before the last MFMA, the last
    MFMA's exact products, those of the last 8 elements of K alone) as fp32 / float64 tensors.  (None of the NT forms splits K over its waves: no
    restatement of a cross-wave meeting applies.)"""
    a = _a_of(c, inp['a_aact'] if aact else inp['a'])
    if aact:
        a = gelu_erf64(a)[0]
        a = rnd_to(a, BF) if c.dt == BF else a.to(F32).to(F64)
    bt = inp['b'].transpose(1, 2)
    grp = 32 if c.dt == BF else 4
    acc = torch.zeros(c.Z, c.M, c.N, dtype=F32)
    prev = p = None
    for k0 in range(0, c.K, grp):
        prev = acc
        p = a[:, :, k0:k0 + grp] @ bt[:, k0:k0 + grp]
        acc = (acc.to(F64) + p).to(F32)
    return acc, prev, p, a[:, :, c.K - 8:] @ bt[:, c.K - 8:]


# name -> (the epilogue it is judged on, the outputs judged, applies(c, fam) -> reason it does not apply or None)
def _min_elems(c, n=20000):
    return None if c.Z * c.M * c.N >= n else f'fewer than {n} elements: a rounding coincidence is not certain'


def _rs_tile_applies(c, fam):
    m = torch.arange(c.M)
    m0 = m // TILE_M[fam] * TILE_M[fam]
    cyc = torch.tensor(RS_CYCLE)
    differs = cyc[(m // c.rps) % 6] != cyc[(m0 // c.rps + (m - m0) // c.rps) % 6]
    return None if bool(differs.any()) else 'the tile-local group index is the right one on every row'


WRONG = {
    'drop_chunk': ('plain', ('C',), lambda c, f: None if c.K % (32 if f == 'r3' else 64) else 'K has no ragged slab / stage'),
    'pad_chunk': ('plain', ('C',), lambda c, f: None if c.K % (32 if f == 'r3' else 64) else 'K has no ragged slab / stage'),
    'bias_tile': ('plain', ('C',), lambda c, f: None),
    'rs_tile': ('fc2', ('C',), _rs_tile_applies),
    'colsum_rows': ('plain', ('colsum', 'colsumsq'), lambda c, f: None if c.M % TILE_M[f] else 'no partial tile'),
    'res_first': ('fc2', ('C',), lambda c, f: None),
    # the two GELUs differ by at most 5e-4; u A (A <= 1.2 * 2 K) has to stay below a fifth of that for the gate to see it: K = 8 only
    'gelu_swap': ('fc1', ('C', 'C2'), lambda c, f: _min_elems(c, 2000) if U * chain(c, 'C') * 2.4 * c.K < 1e-4 else
                  'u A exceeds the 5e-4 by which the two forms differ'),
    'round_twice': ('fc2', ('C',), lambda c, f: 'fp32 mode' if c.dt == F32 else _min_elems(c)),
    'bias_batch0': ('plain', ('C',), lambda c, f: None if c.Z > 1 else 'batch 1'),
}


def restate(c, inp, epi, accs, wrong=None, fam='staged'):
    """one launch as an fp32 restatement: the accumulator of accumulate(), the epilogue in fp32, one rounding to the storage type.
    wrong: the name of a wrong restatement (WRONG)"""
    acc, prev, p, p8 = accs
    if wrong == 'drop_chunk':         # the ragged slab's last 16-byte chunk (8 elements) never arrives
        acc = (prev.to(F64) + p - p8).to(F32)
    elif wrong == 'pad_chunk':        # one chunk beyond K is read: a pad chunk of 1.0 on both operands
        acc = (prev.to(F64) + p + 8.0).to(F32)
    tile = (TILE_M[fam], c.tile_n() if fam in ('staged', 'dma256') else (256 if fam in ('pp', 't256') else 128))
    return epilogue(c, inp, epi, acc, F32, wrong, tile)
