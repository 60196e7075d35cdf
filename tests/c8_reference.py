"""Layout, float64 references, the 16-bit criterion, cases and refusals of the op-level tests of the 16-bit END-TO-END ("C8") operators:
csrc/c8_ops.hip (InstanceNorm statistics / normalise + activation / backward, MaxPool3d(2) and its backward + skip add, C8 -> fp32, the 64 -> 1
head and its backward), csrc/convt_h.hip (ConvTranspose3d(2, 2) forward / dgrad / wgrad / dbias) and the fused fp32 -> fp32 + C8 norm passes of
csrc/norm_act.hip.  tests/test_gpu_c8_ops.py runs the kernels against this file; tests/test_c8_reference.py holds this file to torch's float64
operators on the CPU.  Nothing here calls the library; every function runs on whatever device its operands live on.

LAYOUT.  C8 = [N][C/8][S voxels][8 channels] 16-bit.  A tensor argument (buffer, ctot, c0) means channels [c0, c0 + C) of a ctot-channel buffer.

REFERENCES.  float64, evaluated on the EXACT 16-bit input values widened to float64.  The normalise pass and the backward take `mean` and `rstd`
as the fp32 values the ABI receives (they are arguments of those calls).  The transposed convolution rounds its fp32 weights to the operand type
in the kernel (k_pack_wT), so its references take the rounded weights.

THE 16-BIT CRITERION.  A kernel that evaluates the operator in fp32 and rounds ONCE, to nearest even, stores a value within
    |got - ref| <= 1/2 ulp_T(max(|got|, |ref|)) + e          (within_half_ulp)
of the float64 value, where ulp_T is the spacing of bf16 (8 significand bits) or fp16 (11 bits; never below 2^-24) and e bounds the error of the
fp32 evaluation.  e is computed in float64 from ABSOLUTE VALUES of the operands, by the standard forward bounds (u = 2^-24) -- never from what a
kernel returns:
    reduction over n products of 16-bit operands   the products are exact in fp32, only the accumulation rounds: e = 2 n u A, A the same operator
                                                   on absolute values (sum|w||x| + |bias|).  n = C (forward), 8 K (data gradient), 64 (the dot).
                                                   The factor 2 covers the matrix cores' grouped summation (not one rounding per addition).
    pointwise expression                           (roundings + 1) u sum|terms|.
                                                   normalise: 3 u (|x| + |mean|) rstd  (+ u of it where the LeakyReLU product rounds once more)
                                                   pool backward + skip, outer product: u sum|terms|
    backward of the normalise + activation pair    dx = r ((g' - m1) - xhat m2): four roundings, and the errors of its inputs,
                                                       e = r (5 u (|g'| + |m1| + |xhat m2|) + u_s |g'| + |m2| d_xhat + d_m1 + |xhat| d_m2)
                                                   d_xhat = 3 u (|x| + |mean|) r                      (xhat = fl(fl(x - mean) r))
                                                   u_s    = u where g' = slope g is a rounded product (slope not 0 or 1), else 0
                                                   d_m1   = u |m1| + (L u + u_s) mean|g'|             (m1 = fl32 of a sum of fp32 chains of length <= L)
                                                   d_m2   = u |m2| + mean(|g'| d_xhat) + (L u + u_s) mean|g' xhat|
                                                   L = ceil(ceil(S / splits) / 256) <= 64, the longest per-thread fp32 chain of k_bwd_sums_c8.
                                                   The sign of xhat is the sign of x - mean, which fp32 has exactly: no element changes its mask.
`excess` = max(0, |got - ref| - 1/2 ulp) / e is the share of e a result uses.  A TRUNCATING conversion, a double rounding or a value moved by one
ulp leaves the criterion (tests/test_c8_reference.py shows each).

FP32 OUTPUTS (mean, rstd, dw, db, the dot, the fp32 twin of the fused passes): the project's rule of tests/convt_reference.py unchanged
(err / within / ratios: rms <= 3 rms_oracle + 2^-23, max <= 3 max_oracle + 2^-21), the oracle torch's fp32 operator on the CPU on the same
16-bit-rounded operands.  (tests/norm_reference.py offers limits for nc_instnorm_stats, but no fp32 oracle; the statistics take torch's.)

DBIAS of the norm backward is the per-channel sum of dx, whose true value is exactly zero (an instance's dx sums to zero), so there is no
reference value to be close to and nothing sharper than a bound on the rounding exists: |dbias[c]| <= n u sum|dx| over the channel, n = N S its
number of terms (dbias_limit).  What a lost or doubled partial sum does is caught by the second bound, dbias_chain_limit: the kernel sums the
fp32 values d_i = dx_i + err_i (|err_i| <= e_i) in chains of 8 and then in fp64, so |dbias - sum dx_i| <= sum e_i + 9 u sum|dx|, with the float64
sum of the reference dx (zero up to what the fp32 rounding of `mean` leaves in sum xhat)."""
import functools
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convt_reference as CR  # noqa: E402

FP, BF = 1, 2                    # NC_DT_F16, NC_DT_BF16
DTS = (BF, FP)
U = 2.0 ** -24
EPS = 9.999999747378752e-06      # 1e-5f, the float the ABI receives
NC_OK, NC_ERR_SHAPE, NC_ERR_WS, NC_ERR_ARG = 0, -1, -2, -4
GRID_Y_MAX = 65535


def tdt(dt):
    return torch.bfloat16 if dt == BF else torch.float16


def dt_name(dt):
    return 'bf16' if dt == BF else 'fp16'


def f32(v):
    """the fp32 value of a Python float (the ABI takes the slope as a float: 0.2f is not 0.2)"""
    return torch.tensor(v, dtype=torch.float32).item()


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------------------------------
def pack(x):
    """[N, C, ...] -> [N, C/8, S, 8], same dtype"""
    N, C = x.shape[:2]
    return x.reshape(N, C // 8, 8, -1).permute(0, 1, 3, 2).contiguous()


def unpack(xh, shape):
    """[N, C/8, S, 8] -> shape = [N, C, ...], same dtype"""
    return xh.permute(0, 1, 3, 2).reshape(shape).contiguous()


def view(buf, c0, C):
    """channels [c0, c0 + C) of a C8 buffer [N, ctot/8, S, 8] (a view)"""
    return buf[:, c0 // 8:(c0 + C) // 8]


def pack_into(buf, x, c0):
    view(buf, c0, x.shape[1]).copy_(pack(x))
    return buf


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the criterion
# ---------------------------------------------------------------------------------------------------------------------------------------------
def ulp16(v, dt):
    """spacing of the 16-bit type at |v| (float64, finite): 2^(e - p + 1) for the binade e of |v|, the smallest normal's below it"""
    p, emin = (8, -126) if dt == BF else (11, -14)
    a = v.abs().double()
    _, ex = torch.frexp(a)                                   # a = m 2^ex, m in [0.5, 1)
    e = torch.where(a > 0, ex - 1, torch.full_like(ex, emin)).clamp_min(emin)
    return torch.ldexp(torch.ones_like(a), e - (p - 1))


def _classes(t):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    return torch.isposinf(t) * 1 + torch.isneginf(t) * 2 + torch.isnan(t) * 3


def half_ulp_excess(got, ref, e, dt):
    """per element: max(0, |got - ref| - 1/2 ulp) / e (0 where within half an ulp, inf where beyond it with e == 0); non-finite elements: 0 where
    class and sign agree, inf where not"""
    g = got.to(ref.device).double().reshape(ref.shape)
    e = torch.as_tensor(e, dtype=torch.float64, device=ref.device).expand(ref.shape)
    cg, cr = _classes(g), _classes(ref)
    fin = (cg == 0) & (cr == 0)
    g0, r0 = torch.where(fin, g, torch.zeros_like(g)), torch.where(fin, ref, torch.zeros_like(ref))
    over = ((g0 - r0).abs() - 0.5 * ulp16(torch.maximum(g0.abs(), r0.abs()), dt)).clamp_min(0.0)
    inf = torch.full_like(over, math.inf)
    x = torch.where(over == 0, torch.zeros_like(over), torch.where(e > 0, over / e.clamp_min(1e-300), inf))
    return torch.where(fin, x, torch.where(cg == cr, torch.zeros_like(over), inf))


def within_half_ulp(got, ref, e, dt):
    """(ok, excess): the criterion of the module text for every element, and the largest share of e used"""
    x = half_ulp_excess(got, ref, e, dt)
    m = x.max().item() if x.numel() else 0.0
    return m <= 1.0, m


def bound_excess(got, ref, e):
    """an fp32 output against a rigorous bound: (ok, max |got - ref| / e)"""
    d = (got.to(ref.device).double().reshape(ref.shape) - ref).abs()
    e = torch.as_tensor(e, dtype=torch.float64, device=ref.device).expand(ref.shape)
    x = torch.where(d == 0, torch.zeros_like(d), torch.where(e > 0, d / e.clamp_min(1e-300), torch.full_like(d, math.inf)))
    m = x.max().item()
    return m <= 1.0, m


def truncated(v32, dt):
    """fp32 -> 16-bit by TRUNCATION (toward zero) instead of round-to-nearest-even: what the criterion must reject"""
    h = v32.to(tdt(dt))
    away = h.float().abs() > v32.abs()
    bits = h.view(torch.int16)
    return torch.where(away, bits - 1, bits).view(tdt(dt))    # one ulp toward zero: sign-magnitude, so bits - 1


def one_ulp_moved(h, index):
    """a copy of the 16-bit tensor with the element at flat `index` moved by one ulp (away from zero)"""
    o = h.clone()
    o.view(torch.int16).reshape(-1)[index] += 1
    return o


def units_swapped(h, n, cb, s):
    """a copy of the C8 tensor [N, C/8, S, 8] with the 8-channel units of voxels s and s + 1 exchanged"""
    o = h.clone()
    o[n, cb, s], o[n, cb, s + 1] = h[n, cb, s + 1], h[n, cb, s]
    return o


# ---------------------------------------------------------------------------------------------------------------------------------------------
# InstanceNorm: x [N, C, S] (16-bit values in any dtype), mean / rstd [N, C] fp32
# ---------------------------------------------------------------------------------------------------------------------------------------------
def ref_stats(x):
    """mean, var (biased, two-pass), rstd in float64"""
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = (xd - mean).pow(2).mean(-1)
    return mean.squeeze(-1), var, 1.0 / (var + EPS).sqrt()


def oracle_stats(x):
    """torch's fp32 statistics on the CPU of the same values"""
    xf = x.float().cpu()
    var, mean = torch.var_mean(xf, -1, unbiased=False)
    return mean, torch.rsqrt(var + torch.tensor(EPS, dtype=torch.float32))


def stats32(x):
    """the fp32 mean and rstd the pass-2 tests hand to the kernels: the float64 statistics rounded once (not a kernel's output)"""
    m, _, r = ref_stats(x)
    return m.float(), r.float()


def _rounds_slope(slope):
    return 0.0 if f32(slope) in (0.0, 1.0) else U


def _xhat(x, mean, rstd):
    m, r = mean.double().unsqueeze(-1), rstd.double().unsqueeze(-1)
    xd = x.double()
    return (xd - m) * r, r, 3 * U * (xd.abs() + m.abs()) * r


def ref_norm_act(x, mean, rstd, slope):
    """y, e"""
    xhat, _, d = _xhat(x, mean, rstd)
    return torch.where(xhat > 0, xhat, f32(slope) * xhat), d + _rounds_slope(slope) * xhat.abs()


def emu_norm_act(x, mean, rstd, slope):
    """the same expression in torch's fp32"""
    t = (x.float() - mean.float().unsqueeze(-1)) * rstd.float().unsqueeze(-1)
    return torch.where(t > 0, t, t * torch.tensor(slope, dtype=torch.float32, device=t.device))


def splits_for(S):
    """csrc/c8_ops.hip splits_for"""
    return max(1, min(cdiv(S, 256 * 64), 256))


def nbx(S):
    """csrc/c8_ops.hip: blocks of k_bwd_apply_c8 (256 threads x 8 voxels)"""
    return cdiv(S, 256 * 8)


def chain_len(S):
    """the longest per-thread fp32 chain of k_stats_c8 / k_bwd_sums_c8"""
    return cdiv(cdiv(S, splits_for(S)), 256)


def ref_norm_bwd(g, x, mean, rstd, slope, L=None):
    """dx, e for the gradient g [N, C, S] (bf16 values) at the activation's output; m1, m2 from the float64 sums"""
    S = x.shape[-1]
    L = chain_len(S) if L is None else L
    us = _rounds_slope(slope)
    xhat, r, d = _xhat(x, mean, rstd)
    gd = g.double()
    gp = torch.where(xhat > 0, gd, f32(slope) * gd)
    m1 = gp.mean(-1, keepdim=True)
    m2 = (gp * xhat).mean(-1, keepdim=True)
    p = xhat * m2
    dx = r * ((gp - m1) - p)
    d_m1 = U * m1.abs() + (L * U + us) * gp.abs().mean(-1, keepdim=True)
    d_m2 = U * m2.abs() + (gp.abs() * d).mean(-1, keepdim=True) + (L * U + us) * (gp * xhat).abs().mean(-1, keepdim=True)
    e = r * (5 * U * (gp.abs() + m1.abs() + p.abs()) + us * gp.abs() + m2.abs() * d + d_m1 + xhat.abs() * d_m2)
    return dx, e


def emu_norm_bwd(g, x, mean, rstd, slope):
    """the backward in torch's fp32, means by torch's fp32 mean"""
    m, r = mean.float().unsqueeze(-1), rstd.float().unsqueeze(-1)
    xh = (x.float() - m) * r
    gp = torch.where(xh > 0, g.float(), g.float() * torch.tensor(slope, dtype=torch.float32, device=xh.device))
    m1 = gp.double().mean(-1, keepdim=True).float()
    m2 = (gp * xh).double().mean(-1, keepdim=True).float()
    return r * ((gp - m1) - xh * m2)


def dbias_limit(dx):
    """[C]: n u sum|dx| over the channel, n = N S (module text, DBIAS)"""
    N, _, S = dx.shape
    return N * S * U * dx.abs().sum((0, 2))


def dbias_chain_limit(dx, e, chain=8):
    """[C]: sum e_i + (chain + 1) u sum|dx|"""
    return e.sum((0, 2)) + (chain + 1) * U * (dx.abs() + e).sum((0, 2))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# MaxPool3d(2): x [N, C, D, H, W] 16-bit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def windows(x):
    """[N, C, D, H, W] -> [N, C, D/2, H/2, W/2, 8], the window in scan order t = 4 a + 2 b + c"""
    N, C, D, H, W = x.shape
    return x.reshape(N, C, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(N, C, D // 2, H // 2, W // 2, 8)


def unwindows(w):
    N, C, Do, Ho, Wo, _ = w.shape
    return w.reshape(N, C, Do, Ho, Wo, 2, 2, 2).permute(0, 1, 2, 5, 3, 6, 4, 7).reshape(N, C, 2 * Do, 2 * Ho, 2 * Wo)


def ref_pool(x, last=False):
    """(y, arg): a plain scan in the order (a, b, c) that keeps the FIRST maximum; a NaN always wins, so the LAST NaN's position takes the
    gradient.  y has the bits of the chosen element (-0.0 stays -0.0, a window of eight -inf gives -inf).  last=True: the LAST maximum instead
    (what the tests must be able to tell apart)."""
    cols = windows(x)
    f = cols.double()
    best, arg = f[..., 0].clone(), torch.zeros(f.shape[:-1], dtype=torch.long, device=x.device)
    for t in range(1, 8):
        v = f[..., t]
        take = ((v >= best) if last else (v > best)) | torch.isnan(v)
        best = torch.where(take, v, best)
        arg = torch.where(take, torch.full_like(arg, t), arg)
    return torch.gather(cols, -1, arg.unsqueeze(-1)).squeeze(-1), arg


def ref_pool_bwd_add(dp, arg, skip):
    """dx = skip + the pool's gradient routed to `arg`; e = u sum|terms|"""
    gw = torch.zeros(arg.shape + (8,), dtype=torch.float64, device=dp.device)
    gw.scatter_(-1, arg.unsqueeze(-1), dp.double().unsqueeze(-1))
    gfull = unwindows(gw)
    return skip.double() + gfull, U * (skip.double().abs() + gfull.abs())


def plant_nonfinite(x):
    """Plants, in every channel of sample 0, windows (od, oh, ow) of a [1, C, 4, 4, 4] tensor: (0,0,0) a single NaN at t = 3; (0,0,1) NaNs at
    t = 2 and 5; (0,1,0) +inf at t = 4; (0,1,1) all -inf; (1,0,0) +0.0 then -0.0 ties; (1,0,1) -0.0 first, then +0.0."""
    w = windows(x).clone()
    nan, inf = float('nan'), float('inf')
    w[0, :, 0, 0, 0, 3] = nan
    w[0, :, 0, 0, 1, 2] = nan
    w[0, :, 0, 0, 1, 5] = nan
    w[0, :, 0, 1, 0, 4] = inf
    w[0, :, 0, 1, 1, :] = -inf
    w[0, :, 1, 0, 0, :] = torch.tensor([0.0, -0.0, 0.0, -0.0, -1.0, 0.0, -0.0, -2.0], dtype=x.dtype)
    w[0, :, 1, 0, 1, :] = torch.tensor([-0.0, 0.0, 0.0, -0.0, -1.0, 0.0, -0.0, -2.0], dtype=x.dtype)
    return unwindows(w)


PLANTED_ARGS = {(0, 0, 0): 3, (0, 0, 1): 5, (0, 1, 0): 4, (0, 1, 1): 0, (1, 0, 0): 0, (1, 0, 1): 0}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the 64 -> 1 head: x [N, 64, S] 16-bit, w [64] fp32, bias [1] fp32 or None, g [N, S] fp32
# ---------------------------------------------------------------------------------------------------------------------------------------------
def ref_dot64(x, w, bias):
    """out [N, S], e = 2 n u A with n = 64"""
    wd = w.double().view(1, 64, 1)
    out = (wd * x.double()).sum(1)
    A = (wd.abs() * x.double().abs()).sum(1)
    if bias is not None:
        out, A = out + bias.double(), A + bias.double().abs()
    return out, 2 * 64 * U * A


def oracle_dot64(x, w, bias):
    o = (w.float().cpu().view(1, 64, 1) * x.float().cpu()).sum(1)
    return o if bias is None else o + bias.float().cpu()


def ref_outer64(g, x, w):
    """dx [N, 64, S] = w (x) g with e = u |w g|; dw [64] = sum g x; db = sum g"""
    gd = g.double().unsqueeze(1)
    dx = w.double().view(1, 64, 1) * gd
    return dx, U * dx.abs(), (gd * x.double()).sum((0, 2)), g.double().sum().reshape(1)


def oracle_outer64(g, x):
    gc = g.float().cpu().unsqueeze(1)
    return (gc * x.float().cpu()).sum((0, 2)), gc.sum().reshape(1)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# ConvTranspose3d(2, 2): x [N, C, D, H, W] 16-bit, w [C, K, 2, 2, 2] ROUNDED to the operand type, bias fp32
# ---------------------------------------------------------------------------------------------------------------------------------------------
def ref_convt_fwd(x, w, b):
    """y, e = 2 C u (sum|w||x| + |bias|)"""
    C = x.shape[1]
    return CR.ref_fwd(x, w, b), 2 * C * U * CR.ref_fwd(x.double().abs(), w.double().abs(), None if b is None else b.double().abs())


def ref_convt_dgrad(dy, w):
    """dx, e = 2 (8 K) u sum|w||dy|"""
    K = w.shape[1]
    return CR.ref_dgrad(dy, w), 2 * 8 * K * U * CR.ref_dgrad(dy.double().abs(), w.double().abs())


def oracle_convt_wgrad(x, w, dy):
    """dw, db of torch's fp32 operator on the CPU"""
    wz = w.float().cpu().clone().requires_grad_(True)
    bz = torch.zeros(w.shape[1], requires_grad=True)
    return tuple(t.detach() for t in torch.autograd.grad(F.conv_transpose3d(x.float().cpu(), wz, bz, stride=2), (wz, bz), dy.float().cpu()))


def taps_permuted(y):
    """a forward result with the taps (a, b, c) read as (c, a, b): what the criterion must reject"""
    N, K, D2, H2, W2 = y.shape
    t = y.reshape(N, K, D2 // 2, 2, H2 // 2, 2, W2 // 2, 2)
    return t.permute(0, 1, 2, 7, 4, 3, 6, 5).reshape(N, K, D2, H2, W2)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# dispatch of csrc/convt_h.hip, restated
# ---------------------------------------------------------------------------------------------------------------------------------------------
def convt_fwd_grid(N, C, K, n):
    """(workgroups along x, tiles of 32 voxels, most tiles one wave walks, is the last tile partial)"""
    S = n[0] * n[1] * n[2]
    tiles = cdiv(S, 32) * N
    gx = min(cdiv(tiles, 4), cdiv(2048, K // 32))
    return gx, tiles, cdiv(tiles, gx * 4), S % 32 != 0


def convt_fwd_lds(C):
    return 8 * (C // 16) * 64 * 16


def convt_dgrad_kernel(C):
    return 'dgrad<4>' if (C // 32) % 4 == 0 else 'dgrad<1>'


def convt_wgrad_kernel(C):
    """the NW rule: a workgroup of C / 32 waves shares dY where C / 32 is 1, 2, 4 or 8"""
    return 'wgrad_h2' if C // 32 in (1, 2, 4, 8) else 'wgrad_h'


# ---------------------------------------------------------------------------------------------------------------------------------------------
# cases.  Every one names what it reaches; tests/test_c8_reference.py asserts that from the restated dispatch.
# ---------------------------------------------------------------------------------------------------------------------------------------------
S_CLAMP = 256 * 16384 + 777
# (name, N, C, S, ctot, c0, slope, dtypes, kind): statistics, normalise + activation into (ctot, c0), backward with g in (ctot, c0)
NORM_CASES = [
    ('S1', 2, 8, 1, 8, 0, 0.0, DTS, None),                # variance 0: rstd = 1 / sqrt(eps), y = 0, dx = 0
    ('S255', 1, 16, 255, 16, 0, 0.2, DTS, None),          # one ragged block of 256
    ('S256', 2, 8, 256, 8, 0, 0.0, DTS, None),            # exactly one block
    ('S257', 1, 8, 257, 8, 0, 0.2, DTS, None),            # a second block with one voxel
    ('S2047', 1, 8, 2047, 8, 0, 0.0, DTS, None),          # k_bwd_apply_c8: eight voxels per thread, the last thread's eighth missing
    ('S2048', 1, 8, 2048, 8, 0, 0.2, DTS, None),          # exactly one eight-per-thread block
    ('S2049', 2, 8, 2049, 8, 0, 0.0, DTS, None),          # a second block with one voxel: two partials per channel block for dbias
    ('S16384', 1, 8, 16384, 8, 0, 0.0, DTS, None),        # one split, the longest fp32 chain (64)
    ('S16385', 1, 8, 16385, 8, 0, 0.2, DTS, None),        # two splits
    ('clamp', 1, 8, S_CLAMP, 8, 0, 0.0, DTS, None),       # cdiv(S, 16384) = 257 > 256: the clamp of splits_for
    ('view', 3, 24, 300, 40, 8, 0.2, DTS, None),          # N = 3, three channel blocks, a channel range of a wider buffer
    ('offset', 1, 8, 16384, 8, 0, 0.0, (FP,), 'offset'),  # fp16, mean 100, standard deviation 1: q / S - m^2 from fp32 partials (the longest chain)
]

# (name, N, C, S): nc_instnorm_act_fwd_c8 / nc_instnorm_act_bwd_c8 (fp32 in, fp32 + C8 out)
FWD_STRIDE, BWD_STRIDE = 2048 * 256, 1024 * 1024
FUSED_CASES = [
    ('S300', 2, 8, 300),                                   # short instance
    ('fwd-stride', 1, 8, FWD_STRIDE + 300),                # the forward's grid-stride loop takes a second round
    ('bwd-stride', 1, 8, BWD_STRIDE + 300),                # the backward's
]

# (name, N, C, dims, ctot, c0, kind)
POOL_CASES = [
    ('ties', 2, 16, (6, 8, 10), 24, 8, 'ties'),            # coarse values: ties inside windows
    ('one-window', 1, 8, (2, 2, 2), 8, 0, None),           # a single output voxel
    ('view-514', 1, 24, (2, 4, 514), 40, 16, None),        # 514 output voxels: three blocks, the last with two; a channel range
    ('planted', 1, 8, (4, 4, 4), 8, 0, 'planted'),         # NaN, two NaNs, +inf, all -inf, signed-zero ties
]

# (N, C, S, ctot, c0): nc_from_c8 (exact: every 16-bit value is an fp32 value)
FROM_C8_CASES = [(1, 8, 1, 8, 0), (1, 8, 257, 8, 0), (2, 16, 300, 32, 8)]

# (N, C, K, coarse dims, what it reaches)
CONVT_CASES = [
    (1, 32, 32, (1, 1, 1), 'one voxel: 31 of 32 lanes clamped'),
    (2, 64, 32, (3, 5, 7), 'N = 2, S % 32 != 0'),
    (1, 96, 64, (3, 4, 5), 'C / 32 = 3: k_convT_wgrad_h, dgrad<1>'),
    (1, 160, 32, (2, 3, 5), 'C / 32 = 5: k_convT_wgrad_h, dgrad<1>'),
    (1, 320, 32, (2, 2, 9), 'C / 32 = 10: the 160 KiB LDS limit of the forward, k_convT_wgrad_h, dgrad<1>'),
    (1, 256, 128, (6, 6, 6), "the network's t_conv2"),
    (1, 128, 64, (4, 9, 10), "the network's t_conv1"),
    (1, 32, 256, (17, 40, 50), '34 000 voxels against a cap of 256 workgroups: two tiles per wave, the last one partial'),
]
CONVT_BIG = 1 << 23   # outputs above this many elements are run on the GPU only

# (N, S, what)
HEAD_CASES = [(1, 1, 'one voxel'), (2, 255, 'N = 2, a ragged block'), (1, 4096, 'one 16-per-thread block'),
              (2, 4097, 'N = 2, a second block of k_outer64_c8 with one voxel')]


def case_id(c):
    return '-'.join('x'.join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c if isinstance(v, (int, tuple)) or (isinstance(v, str) and ' ' not in v and ':' not in v))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inputs (seeded; the tests only read them)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


@functools.lru_cache(maxsize=2)
def norm_inputs(N, C, S, kind, dt, device='cpu'):
    """x [N, C, S] in the operand type, g [N, C, S] bf16"""
    g = _gen(device, 11 * S + N * C + dt)
    x = torch.randn(N, C, S, generator=g, device=device)
    x = 100.0 + x if kind == 'offset' else 1.7 * x + 0.6
    return x.to(tdt(dt)), torch.randn(N, C, S, generator=g, device=device).to(torch.bfloat16)


@functools.lru_cache(maxsize=2)
def fused_inputs(N, C, S, device='cpu'):
    """x, dy [N, C, S] fp32"""
    g = _gen(device, 13 * S + N * C)
    return 1.7 * torch.randn(N, C, S, generator=g, device=device) + 0.6, torch.randn(N, C, S, generator=g, device=device)


@functools.lru_cache(maxsize=None)
def pool_inputs(N, C, dims, kind, dt):
    """x in the operand type, dp and skip bf16 (CPU)"""
    g = _gen('cpu', 17 * C + dims[2] + dt)
    if kind in ('ties', 'planted'):
        x = torch.randint(-3, 4, (N, C) + dims, generator=g).float() * 0.5
    else:
        x = torch.randn((N, C) + dims, generator=g)
    x = x.to(tdt(dt))
    if kind == 'planted':
        x = plant_nonfinite(x)
    dp = torch.randn((N, C) + tuple(d // 2 for d in dims), generator=g).to(torch.bfloat16)
    return x, dp, torch.randn((N, C) + dims, generator=g).to(torch.bfloat16)


@functools.lru_cache(maxsize=2)
def convt_inputs(N, C, K, n, device='cpu'):
    """x, w, b, dy fp32 (to be rounded by the caller): randn, the weights scaled by (2 / (8 C))^0.5, a bias of order 1 of alternating sign"""
    g = _gen(device, 1000 * C + 10 * K + N + n[0] * n[1] * n[2])
    x = torch.randn(N, C, *n, generator=g, device=device)
    w = torch.randn(C, K, 2, 2, 2, generator=g, device=device) * (2.0 / (8 * C)) ** 0.5
    b = (1.0 + 0.25 * torch.randn(K, generator=g, device=device)) * (1.0 - 2.0 * (torch.arange(K, device=device) % 2))
    dy = torch.randn(N, K, 2 * n[0], 2 * n[1], 2 * n[2], generator=g, device=device)
    return x, w, b, dy


@functools.lru_cache(maxsize=None)
def head_inputs(N, S, dt):
    """x [N, 64, S] in the operand type, w [64], bias [1], g [N, S] fp32 (CPU)"""
    g = _gen('cpu', 19 * S + N + dt)
    return (torch.randn(N, 64, S, generator=g).to(tdt(dt)), torch.randn(64, generator=g) / 8, torch.tensor([0.75]),
            torch.randn(N, S, generator=g))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# refusals, as pure predicates of the arguments: the code the entry point returns, in the order it checks.  'null' = a NULL pointer among the
# required ones, dt = the dtype argument, ws = workspace bytes passed (None: the exact need), need = the *_ws_bytes of the shape.
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _dt_bad(dt):
    return dt not in (FP, BF)


def _range_bad(ctot, c0, C):
    return C % 8 != 0 or ctot % 8 != 0 or c0 % 8 != 0 or c0 < 0 or c0 + C > ctot


def _grid_bad(N, C):
    return N < 1 or N * (C // 8) > GRID_Y_MAX or N * (C // 8) < 1


def _ws_bad(a):
    return a.get('ws', 0) < 0    # ws = -1: one byte less than the need


def expect_stats(a):
    if a.get('null') or _dt_bad(a['dt']):
        return NC_ERR_ARG
    if a['C'] % 8 or a['N'] < 1 or a['S'] < 1 or _grid_bad(a['N'], a['C']):
        return NC_ERR_SHAPE
    return NC_ERR_WS if _ws_bad(a) else NC_OK


def expect_apply(a):
    if a.get('null') or _dt_bad(a['dt']) or a['N'] < 1 or a['S'] < 1:
        return NC_ERR_ARG
    return NC_ERR_SHAPE if _range_bad(a['ctot'], a['c0'], a['C']) or _grid_bad(a['N'], a['C']) else NC_OK


def expect_bwd(a):
    e = expect_apply(a)
    return e if e else NC_ERR_WS if _ws_bad(a) else NC_OK


def expect_pool(a):
    if a.get('null') or _dt_bad(a['dt']):
        return NC_ERR_ARG
    odd = any(d < 2 or d % 2 for d in a['dims'])
    bad = _range_bad(a['ctot'], a['c0'], a['C']) or odd or _grid_bad(a['N'], a['C'])
    if 'sctot' in a:
        bad = bad or _range_bad(a['sctot'], a['sc0'], a['C'])
    return NC_ERR_SHAPE if bad else NC_OK


def expect_from_c8(a):
    return expect_apply(a)


def _convt_bad(a):
    return a['C'] % 32 != 0 or a['K'] % 32 != 0 or a['C'] < 32 or a['K'] < 32


def expect_convt_fwd(a):
    if a.get('null') or _dt_bad(a['dt']):
        return NC_ERR_ARG
    if _convt_bad(a) or a['ctot'] % 8 or a['c0'] % 32 or a['c0'] + a['K'] > a['ctot']:
        return NC_ERR_SHAPE
    if _ws_bad(a):
        return NC_ERR_WS
    return NC_ERR_SHAPE if a['C'] > 320 else NC_OK


def expect_convt_grad(a):
    """dgrad and wgrad: no dtype argument (bf16), no limit on C"""
    if a.get('null'):
        return NC_ERR_ARG
    if _convt_bad(a) or a['ctot'] % 8 or a['c0'] % 8 or a['c0'] + a['K'] > a['ctot']:
        return NC_ERR_SHAPE
    return NC_ERR_WS if _ws_bad(a) else NC_OK


def expect_head(a):
    if a.get('null') or _dt_bad(a['dt']):
        return NC_ERR_ARG
    if a['S'] < 1 or a['N'] < 1 or a['N'] > GRID_Y_MAX:
        return NC_ERR_SHAPE
    return NC_ERR_WS if _ws_bad(a) else NC_OK


def expect_fused_fwd(a):
    if a.get('null'):
        return NC_ERR_ARG
    if a['N'] < 1 or a['C'] < 8 or a['C'] % 8 or a['S'] < 1 or a['N'] * a['C'] // 8 > GRID_Y_MAX:
        return NC_ERR_SHAPE
    return NC_ERR_ARG if _dt_bad(a['dt']) else NC_OK


def expect_fused_bwd(a):
    if a.get('null'):
        return NC_ERR_ARG
    if a['N'] < 1 or a['C'] < 8 or a['C'] % 8 or a['S'] < 1 or a['N'] * a['C'] > GRID_Y_MAX:
        return NC_ERR_SHAPE
    if _dt_bad(a['dt']):
        return NC_ERR_ARG
    return NC_ERR_WS if _ws_bad(a) else NC_OK


EXPECT = {'stats': expect_stats, 'apply': expect_apply, 'bwd': expect_bwd, 'pool': expect_pool, 'pool_bwd': expect_pool, 'from_c8': expect_from_c8,
          'convt_fwd': expect_convt_fwd, 'convt_dgrad': expect_convt_grad, 'convt_wgrad': expect_convt_grad, 'dot64': expect_head,
          'outer64': expect_head, 'fused_fwd': expect_fused_fwd, 'fused_bwd': expect_fused_bwd}

# a small valid call per entry point; a refusal row changes some of its arguments
_NORM = dict(N=1, C=8, S=4, ctot=8, c0=0, dt=BF)
_POOL = dict(N=1, C=8, dims=(2, 2, 2), ctot=8, c0=0, dt=BF)
_CONVT = dict(N=1, C=32, K=32, dims=(1, 1, 1), ctot=32, c0=0, dt=BF)
BASE = {'stats': _NORM, 'apply': _NORM, 'bwd': _NORM, 'from_c8': _NORM, 'pool': _POOL, 'pool_bwd': dict(_POOL, sctot=8, sc0=0),
        'convt_fwd': _CONVT, 'convt_dgrad': _CONVT, 'convt_wgrad': _CONVT, 'dot64': dict(N=1, S=4, dt=BF), 'outer64': dict(N=1, S=4, dt=BF),
        'fused_fwd': dict(N=1, C=8, S=4, dt=BF), 'fused_bwd': dict(N=1, C=8, S=4, dt=BF)}
HUGE_C = 8 * 65536     # N * C / 8 = 65536 > 65535 at N = 1

# (entry, what, changed arguments, code)
REFUSALS = [(op, 'N * C / 8 = 65536', dict(C=HUGE_C, ctot=HUGE_C, S=1), NC_ERR_SHAPE) for op in ('stats', 'apply', 'bwd', 'from_c8')] + [
    ('pool', 'N * C / 8 = 65536', dict(C=HUGE_C, ctot=HUGE_C), NC_ERR_SHAPE),
    ('pool_bwd', 'N * C / 8 = 65536', dict(C=HUGE_C, ctot=HUGE_C, sctot=HUGE_C), NC_ERR_SHAPE),
    ('fused_fwd', 'N * C / 8 = 65536', dict(C=HUGE_C, S=1), NC_ERR_SHAPE),
    ('fused_bwd', 'N * C = 65536', dict(C=65536, S=1), NC_ERR_SHAPE),
    ('dot64', 'N = 65536', dict(N=65536, S=1), NC_ERR_SHAPE),
    ('outer64', 'N = 65536', dict(N=65536, S=1), NC_ERR_SHAPE),
] + [(op, 'C % 8', dict(C=12, ctot=16), NC_ERR_SHAPE) for op in ('stats', 'apply', 'bwd', 'from_c8', 'pool', 'fused_fwd', 'fused_bwd')] + [
    (op, 'c0 + C > ctot', dict(ctot=8, c0=8), NC_ERR_SHAPE) for op in ('apply', 'bwd', 'from_c8', 'pool', 'pool_bwd')] + [
    (op, 'c0 % 8', dict(ctot=24, c0=4), NC_ERR_SHAPE) for op in ('apply', 'bwd', 'from_c8', 'pool', 'pool_bwd')] + [
    ('pool_bwd', 'skip range', dict(sctot=8, sc0=8), NC_ERR_SHAPE),
    ('pool', 'odd W', dict(dims=(2, 2, 3)), NC_ERR_SHAPE),
    ('pool', 'odd D', dict(dims=(1, 2, 2)), NC_ERR_SHAPE),
    ('pool_bwd', 'odd H', dict(dims=(2, 3, 2)), NC_ERR_SHAPE),
    ('pool', 'N = 0', dict(N=0), NC_ERR_SHAPE),
    ('pool_bwd', 'N = 0', dict(N=0), NC_ERR_SHAPE),
    ('stats', 'N = 0', dict(N=0), NC_ERR_SHAPE),
    ('stats', 'S = 0', dict(S=0), NC_ERR_SHAPE),
    ('apply', 'S = 0', dict(S=0), NC_ERR_ARG),
    ('dot64', 'S = 0', dict(S=0), NC_ERR_SHAPE),
    ('outer64', 'N = 0', dict(N=0), NC_ERR_SHAPE),
    ('convt_fwd', 'C % 32', dict(C=48), NC_ERR_SHAPE),
    ('convt_fwd', 'K % 32', dict(K=48, ctot=48), NC_ERR_SHAPE),
    ('convt_fwd', 'out_c0 % 32', dict(ctot=48, c0=16), NC_ERR_SHAPE),
    ('convt_fwd', 'out_c0 + K > out_ctot', dict(ctot=32, c0=32), NC_ERR_SHAPE),
    ('convt_fwd', 'C = 352 > 320', dict(C=352), NC_ERR_SHAPE),
    ('convt_dgrad', 'C % 32', dict(C=48), NC_ERR_SHAPE),
    ('convt_dgrad', 'dy_c0 % 8', dict(ctot=48, c0=4), NC_ERR_SHAPE),
    ('convt_wgrad', 'K % 32', dict(K=16, ctot=16), NC_ERR_SHAPE),
    ('convt_wgrad', 'dy_c0 + K > dy_ctot', dict(ctot=32, c0=8), NC_ERR_SHAPE),
] + [(op, 'dtype fp32', dict(dt=0), NC_ERR_ARG) for op in ('stats', 'apply', 'bwd', 'from_c8', 'pool', 'pool_bwd', 'convt_fwd', 'dot64', 'outer64',
                                                           'fused_fwd', 'fused_bwd')] + [
    (op, 'NULL input', dict(null='in'), NC_ERR_ARG) for op in sorted(EXPECT)] + [
    (op, 'NULL output', dict(null='out'), NC_ERR_ARG) for op in sorted(EXPECT)] + [
    (op, 'workspace one byte short', dict(ws=-1), NC_ERR_WS) for op in ('stats', 'bwd', 'convt_fwd', 'convt_dgrad', 'convt_wgrad', 'outer64',
                                                                        'fused_bwd')]


def refusal_args(op, changed):
    return dict(BASE[op], **changed)


def refusal_id(r):
    return '%s-%s' % (r[0], r[1].replace(' ', '_'))
