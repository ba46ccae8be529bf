"""Float64 reference, bf16 rounding model, error metric and the shared case lists for the global-attention kernel tests
(csrc/attn.hip).  Pure torch on the CPU; tests/test_attn_ref_cpu.py validates it and tests/test_attn_edges_gpu.py gates
the kernels with it.

Layouts: `qkv` [B*N][3C] (q | k | v column blocks, head h owns columns h*hd.. of each block) and `dout` [B*N][C] as the
kernels take them; everything `exact()` / `rounding_model()` return is per head, [B][H][N][hd] (lse [B][H][N]).
"""
import functools
import math

import torch

F64 = torch.float64
KINDS = ('plain', 'sharp', 'ramp', 'offset')


def rnd(x, dt):
    """x (float64) rounded to dt, held as float64"""
    return x.to(torch.float32).to(dt).to(F64)


def case_seed(B, N, H, hd):
    return 100003 * B + 1009 * N + 101 * H + hd


def make_inputs(B, N, H, hd, kind='plain', seed=0, dt=torch.bfloat16):
    """qkv [B*N][3C] and dout [B*N][C], rounded to dt and held as float64.
    plain:  0.7 * randn (scores with std ~0.5: a nearly uniform softmax)
    sharp:  q and k times 4 (scores with std ~8: saturated rows)
    ramp:   q += a u, key n += a (n / N) u for a unit vector u, a = 0.75 sqrt(hd) (6 at hd 64): the row maximum rises
            with n, so the online softmax rescales its accumulator on every key block
    offset: q += a u, k += a u, a = 2 sqrt(hd) (16 at hd 64): a common +4 sqrt(hd) on every score (+32 at hd 64),
            harmless only if the maximum is subtracted
    The amplitudes follow sqrt(hd) so that the shifted component keeps the same size next to the 0.7 * randn part
    (norm 0.7 sqrt(hd)) at every head width: the bf16 rounding of dS and of delta is multiplied by that ratio in dq
    and dk, and with a fixed 16u the rounding model itself left its 2e-2 validity bound at hd 16 and 48."""
    assert kind in KINDS, kind
    g = torch.Generator().manual_seed(seed)
    x = 0.7 * torch.randn(B, N, 3, H, hd, generator=g, dtype=F64)
    dout = torch.randn(B, N, H, hd, generator=g, dtype=F64)
    u = torch.randn(hd, generator=g, dtype=F64)
    u = u / u.norm()
    if kind == 'sharp':
        x[:, :, 0:2] *= 4.0
    elif kind == 'ramp':
        a = 0.75 * math.sqrt(hd)
        x[:, :, 0] += a * u
        x[:, :, 1] += a * (torch.arange(N, dtype=F64) / N).view(1, N, 1, 1) * u
    elif kind == 'offset':
        x[:, :, 0:2] += 2.0 * math.sqrt(hd) * u
    C = H * hd
    return rnd(x.reshape(B * N, 3 * C), dt), rnd(dout.reshape(B * N, C), dt)


def split_heads(x, B, N, H, hd):
    """[B*N][>= H*hd] (a column block of qkv / dqkv, or out / dout) -> [B][H][N][hd]"""
    return x[:, :H * hd].reshape(B, N, H, hd).permute(0, 2, 1, 3)


def _qkvg(qkv, dout, B, N, H, hd):
    C = H * hd
    q, k, v = (split_heads(qkv[:, j * C:(j + 1) * C].to(F64), B, N, H, hd) for j in range(3))
    return q, k, v, split_heads(dout.to(F64), B, N, H, hd)


def exact(qkv, dout, B, N, H, hd):
    """out, lse, dq, dk, dv in float64 from the closed form (no autograd):
    P = softmax(q k^T / sqrt(hd)),  out = P v,  delta = rowsum(dO * out),  dS = P * (dO v^T - delta),
    dq = dS k / sqrt(hd),  dk = dS^T q / sqrt(hd),  dv = P^T dO"""
    q, k, v, g = _qkvg(qkv, dout, B, N, H, hd)
    scale = hd ** -0.5
    S = q @ k.transpose(-1, -2) * scale
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse[..., None])
    out = P @ v
    delta = (g * out).sum(-1, keepdim=True)
    dS = P * (g @ v.transpose(-1, -2) - delta)
    return out, lse, dS @ k * scale, dS.transpose(-1, -2) @ q * scale, P.transpose(-1, -2) @ g


def rounding_model(qkv, dout, B, N, H, hd, dt=torch.bfloat16):
    """The same computation with a rounding to dt at every point where the kernel header (csrc/attn.hip) says a value
    passes through dt: S stays in fp32; P is rounded before P v and before P^T dO; out is rounded; delta comes from
    the rounded out; dS is rounded before dS k and dS^T q; the results are rounded.  Sums are exact (float64)."""
    q, k, v, g = _qkvg(qkv, dout, B, N, H, hd)
    f32 = torch.float32
    scale = rnd(torch.tensor(hd ** -0.5, dtype=F64), f32)
    S = rnd(rnd(q @ k.transpose(-1, -2), f32) * scale, f32)
    lse = rnd(torch.logsumexp(S, dim=-1), f32)
    P = rnd(torch.exp(S - lse[..., None]), f32)
    Pr = rnd(P, dt)
    out = rnd(Pr @ v, dt)
    delta = rnd((g * out).sum(-1, keepdim=True), f32)
    dP = rnd(g @ v.transpose(-1, -2), f32)
    dS = rnd(P * (dP - delta), dt)
    return (out, lse, rnd(dS @ k * scale, dt), rnd(dS.transpose(-1, -2) @ q * scale, dt), rnd(Pr.transpose(-1, -2) @ g, dt))


def block_err(got, ref, N):
    """max over (b, h) and over blocks of 16 consecutive rows (the last one may be shorter) of
        ||got - ref||_F over the block / (||ref||_F over the whole (b, h) slice * sqrt(rows_in_block / N)):
    an error confined to one 16-row MFMA tile is not diluted by the rest of the tensor, and a block whose reference
    is tiny next to its head's norm does not blow the metric up.  got, ref: [..][N][hd].  A NaN in got gives inf; a
    head whose reference is identically zero gives 0 where got is zero too and inf otherwise."""
    got, ref = got.to(F64), ref.to(F64)
    assert got.shape == ref.shape and ref.shape[-2] == N, (got.shape, ref.shape, N)
    d2 = ((got - ref) ** 2).sum(-1)                                   # [..][N]
    nb = (N + 15) // 16
    d2 = torch.nn.functional.pad(d2, (0, 16 * nb - N)).reshape(*d2.shape[:-1], nb, 16).sum(-1)
    rows = torch.full((nb,), 16.0, dtype=F64)
    rows[-1] = N - 16 * (nb - 1)
    den = ref.pow(2).sum((-1, -2)).sqrt()[..., None] * (rows / N).sqrt()
    e = d2.sqrt() / den
    e = torch.where((d2 == 0) & (den == 0), torch.zeros_like(e), e)
    return float(torch.nan_to_num(e, nan=math.inf, posinf=math.inf).max())


@functools.lru_cache(maxsize=None)
def reference(B, N, H, hd, kind='plain', dt=torch.bfloat16):
    """inputs, exact() and, for bf16, block_err(rounding_model, exact) per tensor of one case; computed once and shared:
    callers must not modify what it returns"""
    qkv, dout = make_inputs(B, N, H, hd, kind, case_seed(B, N, H, hd), dt)
    names = ('out', 'lse', 'dq', 'dk', 'dv')
    ex = dict(zip(names, exact(qkv, dout, B, N, H, hd)))
    r = dict(qkv=qkv, dout=dout, exact=ex)
    if dt == torch.bfloat16:
        mo = dict(zip(names, rounding_model(qkv, dout, B, N, H, hd, dt)))
        r['model_err'] = {n: block_err(mo[n], ex[n], N) for n in ('out', 'dq', 'dk', 'dv')}
    return r


# ------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_attn_edges_gpu.py ((B, N, H, hd) unless said otherwise); tests/test_attn_ref_cpu.py checks
# the validity condition of the rounding-model gate for every one that is gated by it
# ------------------------------------------------------------------------------------------------------------------
THRESH_N = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 193, 255, 256, 257)      # at B = H = 2, hd 64
FORCED_N = (17, 65, 129, 257)                                                      # ATTN_QT x ATTN_KT in {1, 2}^2
WALK = {(3, 3, 129): 18, (1, 7, 64): 7, (3, 3, 65): 18, (3, 3, 64): 9, (1, 1, 64): 1}   # (B, H, N) -> forward workgroups
HEAD_WIDTHS = tuple((2, N, 3, hd) for hd in (16, 32, 48) for N in (65, 129))
LD_PADS = ((8, 8), (24, 0), (0, 40))                                               # (ldq - 3C, ldo - C)
LD_SHAPES = ((2, 129, 2, 48), (2, 129, 2, 64))
KIND_SHAPES = ((2, 257, 1, 64), (1, 130, 2, 64), (1, 129, 2, 48), (1, 65, 1, 16))
MISALIGNED = (2, 129, 2, 64)                                                       # dout / dqkv 8 bytes off a 16-byte boundary
SIMPLE_HD48 = (2, 129, 2, 48)                                                      # ATTN_MFMA = 0
GENERIC_BF16 = tuple((2, N, 2, hd) for hd in (40, 80, 128) for N in (50, 130))
GENERIC_F32 = tuple((2, N, 2, hd) for hd in (12, 20, 40, 64, 96, 128) for N in (1, 50, 130))
GENERIC_F32_ODD_LD = ((2, 50, 2, 64), 3, 2)                                        # shape, ldq - 3C, ldo - C
SUB_BATCH = (4, 129, 2, 64)


def bf16_gated_cases():
    """every (B, N, H, hd, kind) whose bf16 kernels are held to F * block_err(rounding_model, exact)"""
    s = [(2, N, 2, 64) for N in THRESH_N] + [(2, N, 2, 64) for N in FORCED_N] + [(B, N, H, 64) for (B, H, N) in WALK]
    s += list(HEAD_WIDTHS) + list(LD_SHAPES) + [MISALIGNED, SIMPLE_HD48, SUB_BATCH] + list(GENERIC_BF16)
    cases = {c + ('plain',) for c in s}
    cases |= {c + (kind,) for c in KIND_SHAPES for kind in ('sharp', 'ramp', 'offset')}
    return sorted(cases)
