"""Reference, yardstick, dispatch rules and cases of the op-level tests of the fp32 convolution entry points nc_conv_fwd / nc_conv_dgrad /
nc_conv_wgrad on their OLDEST kernels: the gather GEMM (csrc/conv_gemm.hip), the VALU kernels and bias_grad (conv_direct.hip), the fp32 brick
kernels (conv_mfma_fwd.hip, conv_mfma_wgrad.hip), the pointwise kernels (conv_1x1.hip) and the single-channel / K = 1 kernels (conv_c1.hip).
tests/test_gpu_conv_fp32.py runs the cases; tests/test_conv_fp32_reference.py checks this module on the CPU.  Nothing here calls the library.

A 2-D layer is the 3-D layer with D = 1, kd = 1 and stride 1 / padding 0 along D -- the C ABI's own convention (common.hpp make_dims) -- so
every tensor below is 5-D and one set of functions serves both.

REFERENCE: the definitions as float64 tap loops (on whatever device the operands live), zero outside the input:
    y[n,k,o] = b[k] + sum_(c,t) x[n,c,s o - p + t] w[k,c,t]        dx = its adjoint        dw[k,c,t] = sum_(n,o) x[n,c,s o - p + t] dy[n,k,o]
    db[k] = sum_(n,o) dy[n,k,o]
YARDSTICK ("chain oracle", as tests/conv2d_reference.py): a one-accumulator fp32 chain -- the terms of an output element added one at a time,
every product and every partial sum rounded to fp32 -- in the order the kernels' header comments give: forward over (c, tap), the bias last; data
gradient over (k, tap); weight gradient over (n, position); bias gradient over (n, position).  torch's CPU operator sums in blocks and is closer
to float64: a correct single-accumulator matrix-core kernel would fail a factor-3 limit against it (conv2d_reference.py).
ERROR MEASURE and LIMIT: tests/convt_reference.py's, unchanged -- maximum and rms of the error over the rms of the reference;
rms <= FACTOR rms_chain + RMS_FLOOR and max <= FACTOR max_chain + MAX_FLOOR with FACTOR = 3, RMS_FLOOR = 2^-23, MAX_FLOOR = 2^-21."""
import collections
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from convt_reference import FACTOR, MAX_FLOOR, RMS_FLOOR, err, ratios, within  # noqa: E402,F401

Dims = collections.namedtuple('Dims', 'N C D H W K kd kh kw sd sh sw pd ph pw Do Ho Wo')


def cdiv(a, b):
    return -(-a // b)


def make_dims(N, C, K, sp, k, stride, pad):
    """common.hpp make_dims: sp = (D, H, W) with a k^3 kernel, or (H, W) with a 1 x k x k kernel; stride and padding leave a depth of kernel 1 alone."""
    D, H, W = sp if len(sp) == 3 else (1,) + tuple(sp)
    kd = k if len(sp) == 3 else 1
    sd, pd = (stride, pad) if kd > 1 else (1, 0)
    Do, Ho, Wo = (D + 2 * pd - kd) // sd + 1, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    assert min(N, C, K, D, H, W, Do, Ho, Wo) >= 1 and D + 2 * pd >= kd and H + 2 * pad >= k and W + 2 * pad >= k
    return Dims(N, C, D, H, W, K, kd, k, k, sd, stride, stride, pd, pad, pad, Do, Ho, Wo)


# ---- float64 reference and the chain oracle -------------------------------------------------------------------------------------------------
def _padded(x, d):
    """x with its zero border, and room for every window the output positions reach."""
    N, C = x.shape[:2]
    p = torch.zeros(N, C, d.D + 2 * d.pd, d.H + 2 * d.ph, d.W + 2 * d.pw, dtype=x.dtype, device=x.device)
    p[:, :, d.pd:d.pd + d.D, d.ph:d.ph + d.H, d.pw:d.pw + d.W] = x
    return p


def _taps(d):
    return [(tz, ty, tx) for tz in range(d.kd) for ty in range(d.kh) for tx in range(d.kw)]


def _window(d, t):
    """Index of the padded positions tap t meets, one per output position: x[s o - p + t]."""
    return (slice(None), slice(None), slice(t[0], t[0] + d.sd * (d.Do - 1) + 1, d.sd), slice(t[1], t[1] + d.sh * (d.Ho - 1) + 1, d.sh),
            slice(t[2], t[2] + d.sw * (d.Wo - 1) + 1, d.sw))


def _crop(p, d):
    return p[:, :, d.pd:d.pd + d.D, d.ph:d.ph + d.H, d.pw:d.pw + d.W].contiguous()


def ref_fwd(x, w, b, d):
    xp, w = _padded(x.double(), d), w.double()
    y = torch.zeros(d.N, d.K, d.Do, d.Ho, d.Wo, dtype=torch.float64, device=x.device)
    for t in _taps(d):
        y += torch.einsum('nczyx,kc->nkzyx', xp[_window(d, t)], w[:, :, t[0], t[1], t[2]])
    return y if b is None else y + b.double().view(1, -1, 1, 1, 1)


def ref_dgrad(dy, w, d):
    dy, w = dy.double(), w.double()
    dxp = torch.zeros(d.N, d.C, d.D + 2 * d.pd, d.H + 2 * d.ph, d.W + 2 * d.pw, dtype=torch.float64, device=dy.device)
    for t in _taps(d):
        dxp[_window(d, t)] += torch.einsum('nkzyx,kc->nczyx', dy, w[:, :, t[0], t[1], t[2]])
    return _crop(dxp, d)


def ref_wgrad(x, dy, d):
    xp, dy = _padded(x.double(), d), dy.double()
    dw = torch.zeros(d.K, d.C, d.kd, d.kh, d.kw, dtype=torch.float64, device=x.device)
    for t in _taps(d):
        dw[:, :, t[0], t[1], t[2]] = torch.einsum('nkzyx,nczyx->kc', dy, xp[_window(d, t)])
    return dw


def ref_dbias(dy):
    return dy.double().sum((0, 2, 3, 4))


def chain_fwd(x, w, b, d, dtype=torch.float32):
    """One accumulator per output element over (c, tap), the bias last.  dtype = float64 turns it into the reference summed in that order."""
    xp, w = _padded(x.to(dtype), d), w.to(dtype)
    acc = torch.zeros(d.N, d.K, d.Do, d.Ho, d.Wo, dtype=dtype, device=x.device)
    wins = [_window(d, t) for t in _taps(d)]
    for c in range(d.C):
        for t, win in zip(_taps(d), wins):
            acc = acc + xp[win][:, c:c + 1] * w[:, c, t[0], t[1], t[2]].view(1, -1, 1, 1, 1)
    return acc if b is None else acc + b.to(dtype).view(1, -1, 1, 1, 1)


def chain_dgrad(dy, w, d, dtype=torch.float32):
    """One accumulator per input element over (k, tap): an element takes the terms of the taps that reach it, in that order."""
    dy, w = dy.to(dtype), w.to(dtype)
    accp = torch.zeros(d.N, d.C, d.D + 2 * d.pd, d.H + 2 * d.ph, d.W + 2 * d.pw, dtype=dtype, device=dy.device)
    wins = [_window(d, t) for t in _taps(d)]
    for k in range(d.K):
        for t, win in zip(_taps(d), wins):
            accp[win] = accp[win] + dy[:, k:k + 1] * w[k, :, t[0], t[1], t[2]].view(1, -1, 1, 1, 1)
    return _crop(accp, d)


def chain_wgrad(x, dy, d, dtype=torch.float32):
    """One accumulator per weight over (n, output position); a window position outside the input adds a zero."""
    xp, dy = _padded(x.to(dtype), d), dy.to(dtype)
    P = d.Do * d.Ho * d.Wo
    xcol = torch.stack([xp[_window(d, t)].reshape(d.N, d.C, P) for t in _taps(d)], 2)    # [N, C, taps, P]
    xcol = xcol.permute(0, 3, 1, 2).reshape(d.N * P, 1, d.C * len(_taps(d))).contiguous()
    g = dy.reshape(d.N, d.K, P).permute(0, 2, 1).reshape(d.N * P, d.K, 1).contiguous()
    acc = torch.zeros(d.K, xcol.shape[2], dtype=dtype, device=x.device)
    for i in range(d.N * P):
        acc = acc + g[i] * xcol[i]
    return acc.reshape(d.K, d.C, d.kd, d.kh, d.kw)


def chain_dbias(dy, dtype=torch.float32):
    g = dy.to(dtype).permute(0, 2, 3, 4, 1).reshape(-1, dy.shape[1])
    acc = torch.zeros(dy.shape[1], dtype=dtype, device=dy.device)
    for i in range(g.shape[0]):
        acc = acc + g[i]
    return acc


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(N, C, K, sp, k, stride, pad):
    """x, w, b, dy on the CPU in float32: seeded randn, the weights scaled by (2 / (C taps))^0.5, a bias of order 1 that is nowhere near zero
    and alternates in sign (a dropped or doubled bias shows in every channel).  Computed once per layer; the tests only read them."""
    d = make_dims(N, C, K, sp, k, stride, pad)
    g = torch.Generator().manual_seed(100003 * N + 1009 * C + 13 * K + 7 * d.D * d.H * d.W + 3 * k + 2 * stride + pad)
    taps = d.kd * d.kh * d.kw
    x = torch.randn(N, C, d.D, d.H, d.W, generator=g)
    w = torch.randn(K, C, d.kd, d.kh, d.kw, generator=g) * (2.0 / (C * taps)) ** 0.5
    b = (1.0 + 0.25 * torch.randn(K, generator=g)) * (1.0 - 2.0 * (torch.arange(K) % 2))
    dy = torch.randn(N, K, d.Do, d.Ho, d.Wo, generator=g)
    return x, w, b, dy


FWD, DGRAD, WGRAD = 0, 1, 2


def reference(op, layer, device='cpu'):
    """The float64 reference of an op (FWD with the bias, DGRAD, WGRAD or 'dbias') at a layer (N, C, K, spatial, k, stride, pad)."""
    d = make_dims(*layer)
    x, w, b, dy = (t.to(device) for t in inputs(*layer))
    return (ref_fwd(x, w, b, d) if op == FWD else ref_dgrad(dy, w, d) if op == DGRAD else ref_wgrad(x, dy, d) if op == WGRAD else ref_dbias(dy))


@functools.lru_cache(maxsize=None)
def oracle_err(op, layer):
    """(max, rms) error of the fp32 chain oracle of an op at a layer against the float64 reference, both on the CPU; computed once."""
    d = make_dims(*layer)
    x, w, b, dy = inputs(*layer)
    o = (chain_fwd(x, w, b, d) if op == FWD else chain_dgrad(dy, w, d) if op == DGRAD else chain_wgrad(x, dy, d) if op == WGRAD else chain_dbias(dy))
    return err(o, reference(op, layer))


# ---- the dispatch, restated (pure functions of the layer; each names its source) ----------------------------------------------------------
DIRECT, NO_SPLIT, NO_WS = 'force-direct', 'no-split', 'no-workspace'


def taps(d):
    return d.kd * d.kh * d.kw


def Rf(d):
    return d.C * taps(d)


def Rd(d):
    return d.K * taps(d)


def Po(d):
    return d.N * d.Do * d.Ho * d.Wo


def Pi(d):
    return d.N * d.D * d.H * d.W


def padded_ok(M, N, R):
    """conv_gemm.hip padded_ok: fewer than 16 rows only with a long reduction on a small padded problem."""
    return M >= 16 or (R >= 256 and 2.0 * cdiv(M, 64) * 64 * cdiv(N, 64) * 64 * R <= 30e9)


def gemm_supported(op, d):
    """conv_gemm.hip gemm_fwd / dgrad / wgrad_supported (the 2^31 index ranges hold for every case here)."""
    M, N, R = gemm_mnr(op, d)
    return max(Pi(d), Po(d), Rf(d), Rd(d)) < 1 << 31 and padded_ok(M, N, R)


def gemm_mnr(op, d):
    """Rows, columns and reduction of the plain GEMM of an op (conv_gemm.hip header comment)."""
    return {FWD: (d.K, Po(d), Rf(d)), DGRAD: (d.C, Pi(d), Rd(d)), WGRAD: (d.K, Rf(d), Po(d))}[op]


def pick_splits(M, N, R):
    """conv_gemm.hip pick_splits."""
    tiles = cdiv(M, 64) * cdiv(N, 64)
    if tiles >= 256:
        return 1
    return max(1, min(cdiv(512, tiles), cdiv(R, 128), 256))


def fill_splits(M, cols64, R, s):
    """conv_gemm.hip fill_splits."""
    if M >= 128:
        t128 = cdiv(M, 128) * cols64
        while t128 * s < 768 and s * 2 <= cdiv(R, 128) and s * 2 <= 256:
            s *= 2
    return s


def dgrad_as_fwd(d):
    """conv_gemm.hip dgrad_as_fwd: the flip-transpose path."""
    return (d.sd == d.sh == d.sw == 1 and d.kd - 1 - d.pd >= 0 and d.kh - 1 - d.ph >= 0 and d.kw - 1 - d.pw >= 0 and d.ph == d.pw and
            (d.kd == 1 or d.pd == d.ph) and d.C >= 16)


def dgrad_parity_ok(d):
    """conv_gemm.hip dgrad_parity_ok."""
    def pow2(v):
        return v > 0 and v & (v - 1) == 0
    return (max(d.sd, d.sh, d.sw) > 1 and d.kd % d.sd == 0 and d.kh % d.sh == 0 and d.kw % d.sw == 0 and pow2(d.sd) and pow2(d.sh) and pow2(d.sw))


def tile_rows(M, N, splits, ncls):
    """conv_gemm.hip tile_rows."""
    cols = cdiv(N, 64) * splits * ncls
    if M >= 256 and cdiv(M, 256) * cols >= 384:
        return 256
    if M >= 128 and cdiv(M, 128) * cols >= 512:
        return 128
    return 64


def gemm_plan(op, d):
    """What conv_fwd_gemm / conv_dgrad_gemm / conv_wgrad_gemm launch: (mode, M, N, R, splits, tile rows, elements of the output)."""
    if op == FWD:
        M, N, R = gemm_mnr(FWD, d)
        s = fill_splits(M, cdiv(N, 64), R, pick_splits(M, N, R))
        return 'G_FWD', M, N, R, s, tile_rows(M, N, s, 1), M * N
    if op == WGRAD:
        M, N, R = gemm_mnr(WGRAD, d)
        s = fill_splits(M, cdiv(N, 64), R, pick_splits(M, N, R))
        return 'G_WGRAD', M, N, R, s, tile_rows(M, N, s, 1), M * N
    M, N, R = gemm_mnr(DGRAD, d)
    if dgrad_as_fwd(d):
        s = fill_splits(M, cdiv(N, 64), R, pick_splits(M, N, R))
        return 'flip G_FWD', M, N, R, s, tile_rows(M, N, s, 1), M * N
    if dgrad_parity_ok(d):
        ncls = d.sd * d.sh * d.sw
        npar = d.N * cdiv(d.D, d.sd) * cdiv(d.H, d.sh) * cdiv(d.W, d.sw)
        s = fill_splits(M, cdiv(npar, 64) * ncls, R // ncls, pick_splits(M, npar * ncls, R // ncls))
        return 'G_DGRAD_P', M, npar, R // ncls, s, tile_rows(M, npar, s, ncls), M * N
    s = pick_splits(M, N, R)
    return 'G_DGRAD', M, N, R, s, tile_rows(M, N, s, 1), M * N


def gemm_branch(op, d):
    """The name a gather-GEMM case carries: mode / tile rows / one launch or a split reduction and the form of its reduce kernel
    (gemm_split_reduce: float4 when the output's element count is a multiple of 4) / padded rows."""
    mode, M, N, R, s, tm, n = gemm_plan(op, d)
    name = '%s/%d/%s' % (mode, tm, 'one' if s == 1 else 'split-v4' if n % 4 == 0 else 'split-scalar')
    return name + ('/padded' if M < 16 else '')


def brick_shape_ok(d, Cin, Cout):
    """conv_mfma_fwd.hip shape_ok (whether a tile plan exists on top of it is the library's to say: nc_conv_mfma_plan_debug)."""
    if not (d.kd == d.kh == d.kw) or d.kd not in ((3, 7) if Cin == 1 else (3, 5)):
        return False
    return (d.sd == d.sh == d.sw == 1 and d.pd == d.ph == d.pw == d.kd // 2 and (Cin == 1 or Cin % 4 == 0) and Cout % 64 == 0 and d.W <= 192)


def brick_wgrad_shape_ok(d):
    """conv_mfma_wgrad.hip wg_shape_ok + the channel multiples of plan_wgrad / plan_wgrad_rows (32 | C)."""
    return (d.kd == d.kh == d.kw and d.kd in (3, 5) and d.sd == d.sh == d.sw == 1 and d.pd == d.ph == d.pw == d.kd // 2 and d.W <= 192 and
            d.K % 64 == 0 and d.C % 32 == 0)


def flat_1x1_shape(d):
    """conv_1x1.hip flat_1x1_shape == wgrad_1x1_supported."""
    S = d.D * d.H * d.W
    return (taps(d) == 1 and d.sh == d.sw == 1 and d.ph == d.pw == 0 and d.K <= 64 and d.C <= 64 and S % 4 == 0 and S >= 16384 and S * 64 < 1 << 31)


def k1_fwd_supported(d):
    """conv_c1.hip k1_fwd_supported."""
    return d.K == 1 and Rf(d) >= 256 and Po(d) >= 1024


def k1_wgrad_supported(d):
    """conv_c1.hip k1_wgrad_supported."""
    return k1_fwd_supported(d) and d.kh == 4 and d.kw == 4 and d.kd in (1, 4)


def _c1k64(d, ks):
    return (d.C == 1 and d.K == 64 and d.kd == d.kh == d.kw and d.kd in ks and d.sd == d.sh == d.sw == 1 and d.pd == d.ph == d.pw == d.kd // 2)


def c1_wgrad_supported(d):
    """conv_c1.hip c1w_plan: 1 -> 64 channels, 3^3 or 7^3, W % 4 == 0, W >= 16 (its LDS and DMA-piece limits hold up to W = 192)."""
    return _c1k64(d, (3, 7)) and d.W % 4 == 0 and 16 <= d.W <= 192


def to1_mfma_supported(d):
    """conv_c1.hip to1_mfma_supported."""
    return _c1k64(d, (7,)) and d.W % 4 == 0 and 16 <= d.W <= 208


def to1_dgrad_supported(d):
    """conv_c1.hip to1_dgrad_supported."""
    return d.C == 1 and d.K >= 8 and d.kd == d.kh == d.kw == 7 and d.sd == d.sh == d.sw == 1 and d.pd == d.ph == d.pw == 3


def direct_branch(op, d):
    """conv_direct.hip: conv_fwd_direct / conv_dgrad_direct block pick_tile(K or C) channels per lane, conv_wgrad_direct 16 taps per workgroup."""
    def pick_tile(n):
        return 8 if n % 8 == 0 else 4 if n % 4 == 0 else 2 if n % 2 == 0 else 1
    return ('k_conv_fwd<%d>' % pick_tile(d.K) if op == FWD else 'k_conv_dgrad<%d>' % pick_tile(d.C) if op == DGRAD else
            'k_conv_wgrad<%d>' % (1 if taps(d) <= 1 else 16))


def newer_family(op, d, mode):
    """True where a kernel family that has its own op-level file may take the layer in front of the ladder below (api.hip kRungs: the
    paths 9 .. 11, 13, 8 and 7, and conv_c1k3.hip): stated as the NECESSARY conditions of those predicates, so that False is certain.
    The case lists stay out of them."""
    cubic_same = d.kd == d.kh == d.kw and d.sd == d.sh == d.sw == 1 and d.pd == d.ph == d.pw == d.kd // 2
    red, out = (d.C, d.K) if op != DGRAD else (d.K, d.C)
    if mode != NO_SPLIT:
        if cubic_same and d.kd in (3, 5) and (d.C % 32 == 0 and d.K % 64 == 0 if op == WGRAD else red % 8 == 0 and out % 64 == 0):
            return True    # conv_split.hip ws_shape_ok / s_shape_ok
        if op != WGRAD and _c1k64(d, (7,)):
            return True    # conv_s3x.hip c1k7_h2_supported
    pg = d.D == 1 and d.kd == 1 and d.kh == 4 and d.kw == 4 and d.ph == 1 and d.pw == 1 and d.sh in (1, 2)
    if pg and d.C == 1 and d.sh == 2:
        return True        # patchgan_edge.hip pg1_supported (rung 8): tests/test_gpu_patchgan_fp32.py
    if pg and (d.K % 128 == 0 and d.C % 8 == 0 if op == WGRAD else red % 2 == 0 and red >= 16 and out % 64 == 0):
        return True        # conv2d_img.hip sconv_*_supported (rung 7): tests/test_gpu_patchgan_fp32.py; conv_p2d.hip p2_shape, wgrad_p2d.hip q_shape
    if op != WGRAD and d.D == 1 and d.kd == 1 and d.kh == 3 and d.sh == 1 and d.ph == 1 and red % 2 == 0 and red >= 16 and out % 64 == 0:
        return True        # conv2d_k3.hip k3_shape_ok
    if op == FWD and d.C == 1 and d.K % 64 == 0 and cubic_same and d.kd == 3 and d.W >= 8:
        return True        # conv_c1k3.hip c1k3_fwd_supported
    return False


def dispatch(op, d, mode):
    """(path, branch): the path of the rung of api.hip's kRungs (conv_route) a layer reaches under a mode -- the number the profiler reports in
    cls -- and the kernel behind it.  Brick variants are left to nc_conv_mfma_plan_debug ('brick'); NO_WS changes no path."""
    if mode == DIRECT:
        return 0, direct_branch(op, d)
    assert not newer_family(op, d, mode), 'a newer kernel family may take this layer: not a case for this file'
    if op == FWD:
        if brick_shape_ok(d, d.C, d.K):
            return 1, 'brick'
        if flat_1x1_shape(d):
            return 3, 'flat_1x1'
        if k1_fwd_supported(d):
            return 5, 'k1_fwd'
    elif op == DGRAD:
        if d.K != 1 and brick_shape_ok(d, d.K, d.C):    # conv_mfma_fwd.hip dgrad_shape_ok: the single-channel mode is forward only
            return 1, 'brick'
        if flat_1x1_shape(d):
            return 3, 'flat_1x1'
        if to1_mfma_supported(d):
            return 6, 'to1_mfma/%d' % (1 if d.W <= 112 else 2)
        if to1_dgrad_supported(d):
            return 0, 'to1_dgrad'
    else:
        if brick_wgrad_shape_ok(d):
            return 1, 'brick'
        if flat_1x1_shape(d):
            return 3, 'wgrad_1x1'
        if c1_wgrad_supported(d):
            return 4, 'c1_wgrad/%d' % d.kd
        if k1_wgrad_supported(d):
            return 5, 'k1_wgrad/%d' % d.kd
    if gemm_supported(op, d):
        return 2, gemm_branch(op, d)
    return 0, direct_branch(op, d)


# ---- the fp32 brick kernels: what nc_conv_mfma_plan_debug reports, as the name a case carries ---------------------------------------------
NUM_WG = 256    # conv_mfma_fwd.hip kNumWG: the persistent workgroups of the stream-K loop


def streamk_regimes(units, nchunks):
    """How k_conv_mfma's shares [units w / 256, units (w + 1) / 256) cut the tiles (a tile = nchunks consecutive units) -- the arithmetic of
    the kernel's prologue and of k_conv_fixup, not the planner's cost model: 'few' = fewer units than workgroups (every tile with nchunks > 1
    is split over many workgroups, some shares are empty); 'whole' = a share that ends one tile, holds whole tiles and starts another (both of
    its partial slots are used); 'cut3' = a tile cut by three or more boundaries (the fix-up's "an earlier boundary already cuts this tile")."""
    B = [units * w // NUM_WG for w in range(NUM_WG + 1)]
    out = ['few'] if units < NUM_WG else []
    if any(B[w] % nchunks and B[w + 1] % nchunks and B[w + 1] // nchunks - cdiv(B[w], nchunks) >= 1 for w in range(NUM_WG)):
        out.append('whole')
    cuts = collections.Counter(b // nchunks for b in B[1:NUM_WG] if b % nchunks)   # (boundaries of empty shares coincide: each one counts)
    if any(v >= 3 for v in cuts.values()):
        out.append('cut3')
    return '+'.join(out) if out else 'plain'


def brick_fwd_name(d, plan):
    """plan: the 8 ints of nc_conv_mfma_plan_debug(what = 0 | 1)."""
    cfg, CK, Tz, Ty, tail, nchunks, units, tiles = plan
    return 'brick/KS%d/CK%d/cfg%d/%s/W%d/%s' % (d.kd, CK, cfg, 'tail' if tail else 'whole-rows', 64 if d.W <= 64 else 128 if d.W <= 128 else 192,
                                               streamk_regimes(units, nchunks))


def brick_wgrad_name(plan):
    """plan: the 8 ints of nc_conv_mfma_plan_debug(what = 2)."""
    kern, KS, AB, NXB = plan[:4]
    return ('brick/k_wgrad_rows<%d>/rows%d' % (KS, AB) if kern == 0 else 'brick/k_wgrad_dma<%d,%d>/blocks%d' % (KS, AB, NXB) if kern == 1 else
            'brick/k_wgrad_mfma<%d,%d>' % (KS, AB))


# ---- the cases: (N, C, K, spatial, k, stride, pad, mode, branch) ---------------------------------------------------------------------------
# spatial (D, H, W) with a k^3 kernel or (H, W) with a 1 x k x k one.  mode: None = the default switches, DIRECT = under nc_set_force_direct(1),
# NO_SPLIT = under nc_set_conv_split(0) (the split-operand and two-term kernels, api.hip's rungs 9 .. 11, would take the layer otherwise),
# NO_WS = default switches and ws = NULL.  branch: what dispatch() above says the case reaches; for the brick kernels the variant
# nc_conv_mfma_plan_debug reports, named by brick_fwd_name / brick_wgrad_name.  Each case is the smallest layer found that reaches its branch
# with a ragged edge: rows that are no multiple of the tile, columns that are no multiple of 64, odd extents under a stride.
#
# The gather GEMM (conv_gemm.hip): mode / tile rows / 'one' launch or a 'split' reduction with the float4 or the scalar reduce kernel / padded
# rows (M < 16).  The tall tiles need M >= 128 (256) rows and 512 (384) workgroups: few channels on the reduction side and 12 .. 16 thousand
# columns for 'one'; for 'split' a long reduction over few columns, which fill_splits then cuts further.  G_DGRAD (a stride that does not
# divide the kernel) calls pick_splits alone: with a split its tiles never pass 64 rows (test_conv_fp32_reference.py counts it out).
FWD_CASES = [
    (2, 2, 24, (9, 10, 11), 4, 2, 1, None, 'G_FWD/64/one'),               # the 4^3 stride-2 PatchGAN layer; M = 24, 200 columns, R = 128
    (2, 2, 24, (9, 10, 11), 4, 2, 1, NO_WS, 'G_FWD/64/one'),
    (2, 16, 24, (9, 10, 11), 4, 2, 1, None, 'G_FWD/64/split-v4'),         # R = 1024: 8 splits
    (1, 16, 25, (7, 7, 7), 4, 2, 1, None, 'G_FWD/64/split-scalar'),       # 25 x 27 outputs: odd
    (2, 4, 5, (9, 10, 11), 4, 2, 1, None, 'G_FWD/64/split-v4/padded'),    # M = 5 with R = 256
    (3, 24, 40, (9, 11), 4, 2, 1, None, 'G_FWD/64/split-v4'),             # kd = 1, kh = kw = 4
    (1, 64, 32, (6, 6, 6), 1, 1, 0, None, 'G_FWD/64/one'),                # k = 1: qdiv's d == 1 branch
    (1, 16, 16, (15, 26, 42), 1, 1, 0, None, 'G_FWD/64/one'),             # S = 16380: just below the pointwise kernels' 16384
    (1, 2, 160, (130, 128), 4, 1, 1, None, 'G_FWD/128/one'),              # M = 160: a ragged second row tile; 16383 columns
    (1, 2, 320, (112, 112), 4, 1, 1, None, 'G_FWD/256/one'),              # M = 320; 12321 columns
    (1, 128, 160, (51, 51), 4, 1, 1, None, 'G_FWD/128/split-v4'),         # 2500 columns, R = 2048: 10 splits
    (1, 512, 328, (23, 23), 4, 1, 1, None, 'G_FWD/256/split-v4'),         # 484 columns, R = 8192: 44 splits
    # conv_direct.hip: under force-direct, and by default where the GEMM declines (M < 16 and R < 256)
    (2, 2, 24, (9, 10, 11), 4, 2, 1, DIRECT, 'k_conv_fwd<8>'),
    (3, 24, 40, (9, 11), 4, 2, 1, DIRECT, 'k_conv_fwd<8>'),
    (2, 3, 5, (9, 10, 11), 3, 2, 1, None, 'k_conv_fwd<1>'),
    (2, 5, 12, (10, 11), 3, 1, 1, None, 'k_conv_fwd<4>'),
    (2, 5, 12, (10, 11), 3, 1, 1, DIRECT, 'k_conv_fwd<4>'),
    (2, 7, 6, (5, 6, 7), 3, 1, 1, DIRECT, 'k_conv_fwd<2>'),
    (2, 16, 1, (5, 6, 7), 3, 1, 1, DIRECT, 'k_conv_fwd<1>'),              # K = 1
    (2, 1, 6, (5, 6, 7), 3, 1, 1, DIRECT, 'k_conv_fwd<2>'),               # C = 1
    # conv_1x1.hip k_flat_1x1: S = 16428 = 16384 + 4 * 11 voxels, a last chunk of 44
    (1, 64, 32, (12, 37, 37), 1, 1, 0, None, 'flat_1x1'),
    (2, 16, 1, (12, 37, 37), 1, 1, 0, None, 'flat_1x1'),                  # both channel counts padded, batch 2
    # conv_c1.hip k_conv_k1_fwd
    (9, 16, 1, (12, 13), 4, 1, 1, None, 'k1_fwd'),                        # C taps = 256 exactly, one channel per group
    (3, 100, 1, (9, 10, 11), 4, 1, 1, None, 'k1_fwd'),                    # 7 channels per group, the last two groups ragged / empty
    # conv_mfma_fwd.hip
    (1, 16, 64, (3, 5, 4), 3, 1, 1, NO_SPLIT, 'brick/KS3/CK4/cfg0/whole-rows/W64/few+cut3'),
    (1, 16, 64, (7, 7, 7), 3, 1, 1, NO_SPLIT, 'brick/KS3/CK4/cfg0/tail/W64/few+cut3'),
    (1, 16, 64, (4, 5, 68), 3, 1, 1, NO_SPLIT, 'brick/KS3/CK4/cfg0/whole-rows/W128/few+cut3'),
    (1, 16, 64, (4, 5, 66), 3, 1, 1, NO_SPLIT, 'brick/KS3/CK4/cfg0/tail/W128/few+cut3'),
    (1, 16, 64, (3, 4, 132), 3, 1, 1, NO_SPLIT, 'brick/KS3/CK4/cfg0/whole-rows/W192/few+cut3'),
    (1, 16, 64, (3, 4, 130), 3, 1, 1, NO_SPLIT, 'brick/KS3/CK4/cfg0/tail/W192/few+cut3'),
    (1, 1, 64, (3, 5, 4), 3, 1, 1, None, 'brick/KS3/CK1/cfg1/whole-rows/W64/few'),           # W < 8: conv_c1k3.hip leaves it
    (1, 32, 256, (3, 5, 4), 3, 1, 1, NO_SPLIT, 'brick/KS3/CK8/cfg4/whole-rows/W64/few+cut3'),
    (1, 32, 256, (7, 7, 7), 3, 1, 1, NO_SPLIT, 'brick/KS3/CK8/cfg4/tail/W64/few+cut3'),
    (2, 32, 256, (9, 10, 27), 3, 1, 1, NO_SPLIT, 'brick/KS3/CK8/cfg2/tail/W64/few+cut3'),
    (2, 64, 256, (6, 5, 54), 3, 1, 1, NO_SPLIT, 'brick/KS3/CK8/cfg3/tail/W64/few+cut3'),
    (1, 8, 64, (3, 5, 4), 5, 1, 2, NO_SPLIT, 'brick/KS5/CK2/cfg0/whole-rows/W64/few+cut3'),
    (1, 16, 256, (3, 5, 4), 5, 1, 2, NO_SPLIT, 'brick/KS5/CK4/cfg4/whole-rows/W64/few+cut3'),
    (1, 16, 256, (7, 7, 7), 5, 1, 2, NO_SPLIT, 'brick/KS5/CK4/cfg4/tail/W64/few+cut3'),
    (2, 64, 256, (5, 6, 16), 5, 1, 2, NO_SPLIT, 'brick/KS5/CK4/cfg1/whole-rows/W64/cut3'),   # 256 units of 16 tiles: one unit per workgroup
    (1, 1, 64, (3, 5, 4), 7, 1, 3, NO_SPLIT, 'brick/KS7/CK1/cfg1/whole-rows/W64/few'),
    (1, 1, 64, (4, 5, 68), 7, 1, 3, NO_SPLIT, 'brick/KS7/CK1/cfg1/whole-rows/W128/few'),
    (3, 12, 256, (34, 25, 4), 3, 1, 1, None, 'brick/KS3/CK4/cfg4/whole-rows/W64/whole'),     # 408 tiles of 3 units, 4.78 units per workgroup
]

DGRAD_CASES = [
    (2, 24, 4, (9, 10, 11), 3, 2, 1, None, 'G_DGRAD/64/one'),             # 3^3 stride 2: no parity classes
    (2, 24, 4, (9, 10, 11), 3, 2, 1, NO_WS, 'G_DGRAD/64/one'),
    (2, 24, 40, (9, 10, 11), 3, 2, 1, None, 'G_DGRAD/64/split-v4'),
    (1, 25, 40, (9, 9, 11), 3, 2, 1, None, 'G_DGRAD/64/split-scalar'),
    (2, 8, 300, (6, 6, 6), 1, 1, 0, None, 'G_DGRAD/64/split-v4/padded'),  # k = 1, C < 16: not the flipped forward
    (1, 160, 2, (130, 127), 3, 2, 1, None, 'G_DGRAD/128/one'),
    (1, 320, 2, (111, 111), 3, 2, 1, None, 'G_DGRAD/256/one'),
    (2, 24, 4, (9, 11, 13), 4, 2, 1, None, 'G_DGRAD_P/64/one'),           # 8 classes of 5 x 6 x 7 down to 4 x 5 x 6 positions
    (2, 24, 40, (9, 11, 13), 4, 2, 1, None, 'G_DGRAD_P/64/split-v4'),
    (1, 25, 40, (9, 11, 13), 4, 2, 1, None, 'G_DGRAD_P/64/split-scalar'),
    (2, 24, 40, (9, 11), 4, 2, 1, None, 'G_DGRAD_P/64/split-v4'),         # 4 classes
    (2, 5, 4, (9, 11, 13), 4, 2, 1, None, 'G_DGRAD_P/64/one/padded'),
    (1, 160, 2, (125, 129), 4, 2, 1, None, 'G_DGRAD_P/128/one'),
    (1, 320, 2, (111, 109), 4, 2, 1, None, 'G_DGRAD_P/256/one'),
    (1, 160, 512, (49, 47), 4, 2, 1, None, 'G_DGRAD_P/128/split-v4'),     # 600 columns per class, R = 2048 per class: 10 splits
    (1, 328, 512, (37, 33), 4, 2, 1, None, 'G_DGRAD_P/256/split-v4'),
    (2, 24, 2, (10, 11), 4, 1, 1, None, 'flip G_FWD/64/one'),             # dgrad_as_fwd
    (2, 24, 40, (10, 11), 4, 1, 1, None, 'flip G_FWD/64/split-v4'),
    (1, 25, 40, (9, 11), 4, 1, 1, None, 'flip G_FWD/64/split-scalar'),
    (1, 64, 32, (6, 6, 6), 1, 1, 0, None, 'flip G_FWD/64/one'),
    (1, 16, 16, (15, 26, 42), 1, 1, 0, None, 'flip G_FWD/64/one'),
    (1, 160, 2, (129, 127), 4, 1, 1, None, 'flip G_FWD/128/one'),
    (1, 64, 1, (5, 6, 8), 3, 1, 1, None, 'flip G_FWD/64/one'),            # 3^3 with K = 1: NOT the brick kernel, whose one-channel mode is forward only
    (2, 24, 4, (9, 10, 11), 3, 2, 1, DIRECT, 'k_conv_dgrad<8>'),
    (2, 24, 40, (9, 11), 4, 2, 1, DIRECT, 'k_conv_dgrad<8>'),
    (2, 3, 5, (9, 10, 11), 3, 2, 1, None, 'k_conv_dgrad<1>'),
    (2, 12, 5, (10, 11), 3, 1, 1, None, 'k_conv_dgrad<4>'),
    (2, 12, 5, (10, 11), 3, 1, 1, DIRECT, 'k_conv_dgrad<4>'),
    (2, 6, 7, (5, 6, 7), 3, 1, 1, DIRECT, 'k_conv_dgrad<2>'),
    (2, 1, 6, (5, 6, 7), 3, 1, 1, DIRECT, 'k_conv_dgrad<1>'),             # C = 1
    (2, 16, 1, (5, 6, 7), 3, 1, 1, DIRECT, 'k_conv_dgrad<8>'),            # K = 1
    (1, 64, 32, (12, 37, 37), 1, 1, 0, None, 'flat_1x1'),
    (2, 16, 1, (12, 37, 37), 1, 1, 0, None, 'flat_1x1'),
    # conv_c1.hip k_dgrad_to1: W = 16; two column segments (W > 112); 300 rows over 64 workgroups (row ranges that split planes)
    (1, 1, 64, (5, 6, 16), 7, 1, 3, NO_SPLIT, 'to1_mfma/1'),
    (1, 1, 64, (7, 8, 116), 7, 1, 3, NO_SPLIT, 'to1_mfma/2'),
    (2, 1, 64, (5, 30, 24), 7, 1, 3, NO_SPLIT, 'to1_mfma/1'),
    # conv_c1.hip k_conv_to1<7> (reported as path 0, its own rung)
    (1, 1, 8, (5, 6, 18), 7, 1, 3, NO_SPLIT, 'to1_dgrad'),
    (1, 1, 64, (5, 6, 18), 7, 1, 3, NO_SPLIT, 'to1_dgrad'),
    # conv_mfma_fwd.hip as the data gradient (Cin = K, Cout = C)
    (1, 64, 16, (7, 7, 7), 3, 1, 1, NO_SPLIT, 'brick/KS3/CK4/cfg0/tail/W64/few+cut3'),
    (1, 256, 32, (3, 5, 4), 3, 1, 1, NO_SPLIT, 'brick/KS3/CK8/cfg4/whole-rows/W64/few+cut3'),
    (1, 64, 8, (3, 5, 4), 5, 1, 2, NO_SPLIT, 'brick/KS5/CK2/cfg0/whole-rows/W64/few+cut3'),
    (2, 256, 32, (9, 10, 27), 3, 1, 1, NO_SPLIT, 'brick/KS3/CK8/cfg2/tail/W64/few+cut3'),
    (3, 256, 12, (34, 25, 4), 3, 1, 1, None, 'brick/KS3/CK4/cfg4/whole-rows/W64/whole'),
]

# every case also takes dbias (bias_grad, conv_direct.hip) in a second call
WGRAD_CASES = [
    (1, 24, 24, (7, 7, 7), 4, 2, 1, None, 'G_WGRAD/64/one'),              # 27 positions
    (3, 24, 40, (9, 11), 4, 2, 1, None, 'G_WGRAD/64/one'),
    (2, 3, 24, (9, 10, 11), 4, 2, 1, None, 'G_WGRAD/64/split-v4'),
    (2, 5, 5, (9, 10, 11), 3, 2, 1, None, 'G_WGRAD/64/split-scalar/padded'),   # K = 5 with 300 positions
    (1, 64, 32, (6, 6, 6), 1, 1, 0, None, 'G_WGRAD/64/split-v4'),
    (1, 16, 16, (15, 26, 42), 1, 1, 0, None, 'G_WGRAD/64/split-v4'),      # 128 splits of 128 positions
    (1, 607, 160, (5, 5, 5), 3, 2, 1, None, 'G_WGRAD/128/one'),           # 16389 columns
    (1, 455, 320, (5, 5, 5), 3, 2, 1, None, 'G_WGRAD/256/one'),
    (1, 93, 160, (21, 21, 21), 3, 2, 1, None, 'G_WGRAD/128/split-v4'),    # 2511 columns, 1331 positions
    (1, 56, 328, (25, 25, 25), 3, 2, 1, None, 'G_WGRAD/256/split-v4'),
    (1, 24, 24, (7, 7, 7), 4, 2, 1, DIRECT, 'k_conv_wgrad<16>'),
    (1, 5, 5, (9, 10, 11), 3, 2, 1, None, 'k_conv_wgrad<16>'),            # K = 5 with 150 positions: the GEMM declines
    (3, 4, 7, (4, 4), 4, 1, 0, None, 'k_conv_wgrad<16>'),                 # ONE output position per image (bias_grad: S = 1)
    (2, 5, 5, (10, 11), 3, 1, 1, DIRECT, 'k_conv_wgrad<16>'),
    (2, 7, 3, (6, 6, 6), 1, 1, 0, DIRECT, 'k_conv_wgrad<1>'),
    (2, 16, 1, (5, 6, 7), 3, 1, 1, DIRECT, 'k_conv_wgrad<16>'),           # K = 1
    (2, 1, 6, (5, 6, 7), 3, 1, 1, DIRECT, 'k_conv_wgrad<16>'),            # C = 1
    (1, 64, 32, (12, 37, 37), 1, 1, 0, None, 'wgrad_1x1'),                # bias_grad: 16428 positions in 5 splits
    (2, 16, 1, (12, 37, 37), 1, 1, 0, None, 'wgrad_1x1'),
    (2, 1, 64, (7, 11, 36), 3, 1, 1, None, 'c1_wgrad/3'),
    (1, 1, 64, (10, 9, 20), 7, 1, 3, None, 'c1_wgrad/7'),
    (9, 16, 1, (12, 13), 4, 1, 1, None, 'k1_wgrad/1'),
    (3, 100, 1, (9, 10, 11), 4, 1, 1, None, 'k1_wgrad/4'),
    # conv_mfma_wgrad.hip
    (1, 64, 64, (6, 7, 60), 5, 1, 2, NO_SPLIT, 'brick/k_wgrad_dma<5,1>/blocks1'),
    (1, 64, 64, (5, 6, 96), 3, 1, 1, NO_SPLIT, 'brick/k_wgrad_dma<3,2>/blocks2'),
    (1, 32, 64, (5, 6, 70), 3, 1, 1, NO_SPLIT, 'brick/k_wgrad_mfma<3,1>'),
    (2, 32, 64, (6, 5, 54), 3, 1, 1, NO_SPLIT, 'brick/k_wgrad_rows<3>/rows2'),
]

CASES = {FWD: FWD_CASES, DGRAD: DGRAD_CASES, WGRAD: WGRAD_CASES}

# where the source shows the size check in front of every launch (conv_gemm.hip split_setup -- not the flipped forward, whose weight transpose
# is launched first --, conv_mfma_fwd.hip run, conv_1x1.hip launch_flat): (op, case, bytes passed)
def first_case(op, branch, mode=None):
    return next(c for c in CASES[op] if c[8] == branch and c[7] == mode)


UNDERSIZED = [
    (FWD, first_case(FWD, 'G_FWD/64/split-v4'), 256), (DGRAD, first_case(DGRAD, 'G_DGRAD/64/split-v4'), 256),
    (DGRAD, first_case(DGRAD, 'G_DGRAD_P/64/split-v4'), 256), (WGRAD, first_case(WGRAD, 'G_WGRAD/64/split-v4'), 256),
    (FWD, first_case(FWD, 'brick/KS3/CK4/cfg0/tail/W64/few+cut3', NO_SPLIT), 256),
    (DGRAD, first_case(DGRAD, 'brick/KS3/CK8/cfg4/whole-rows/W64/few+cut3', NO_SPLIT), 256),
    (FWD, first_case(FWD, 'flat_1x1'), 128), (DGRAD, first_case(DGRAD, 'flat_1x1'), 128),
]


def case_id(c):
    return '-'.join('x'.join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c if v is not None).replace(' ', '')
