"""Cases, references and limits of the op-level tests of the small kernels every training step runs through: the four losses and Adam
(csrc/misc.hip) and the spectral norm (csrc/spectral.hip).  tests/test_gpu_small_ops.py holds the kernels to them; tests/test_small_ops_reference.py
checks them on the CPU.  Nothing here calls the library; the references run on whatever device their operands live on.

REFERENCES, in float64, of the fp32 values the ABI receives (a target of 0.9 is 0.9f, beta1 = 0.1 is 0.1f, ...):
    mse     mean((p - t)^2)                                   d/dp = gscale 2 (p - t) / n
    l1      mean|a - b|                                        d/da = gscale sign(a - b) / n      (0 where a == b)
    bce     mean(max(p, 0) - p t + log1p(exp(-|p|)))           d/dp = gscale (sigmoid(p) - t) / n
    mean    mean(p)                                            d/dp = gscale / n
    Adam    m' = b1 m + (1 - b1) g;  v' = b2 v + (1 - b2) g^2;  p' = p - lr / (1 - b1^step) m' / (sqrt(v') / sqrt(1 - b2^step) + eps)
    spectral norm, W [K, M]:  v' = W^T u / max(|W^T u|, eps);  s = W v';  u' = s / max(|s|, eps);  sigma = u' . s;  W / sigma
                    (power_iteration = 0: s = W v, sigma = u . s, u and v untouched)
            backward, u and v constants:  dW = (G - <G, W / sigma> u v^T) / sigma, of the fp32 W / sigma, u, v, sigma the op is handed

LIMITS, with u = 2^-24 (one correctly rounded fp32 operation: relative error <= u), from the rounding points the kernels spell out, never from
what the kernels return.  Worst-case sums of the first-order terms; the products of two such terms are covered by a factor 1 + 4u (losses),
1 + 64u (Adam: up to ten roundings in a chain) or 1 + 4 gamma_max (spectral norm).  A result in the denormal range is off by up to 2^-149 per
operation whatever its size (TINY); where an intermediate may be flushed or overflow on the way (exp of |p| > 87) by up to 2^-126 (MINN).
  loss forward   out = fl32((sum_i v_i) / n), the v_i rounded in fp32, summed in fp64 (k_loss_partial / k_loss_final):
                     |out - ref| <= u |ref| + (sum_i e_i + 2^-44 sum_i |v_i|) / n + 2^-149
                 2^-44: fewer than 2^9 fp64 additions lie between any v_i and the result (32 per thread at the largest n, 8 levels of
                 the workgroup tree, 256 partials), 2^-53 each.  e_i per mode:
                     mse    fl(p - t) squared in fp64: (2u + u^2) d^2          l1   fl(a - b): u |d|          mean   0
                     bce    u (|p t| + |max(p, 0) - p t|)         the product and the difference (one rounding less if contracted to an fma)
                            + 2u (EXP_ULP e / (1 + e) + LOG1P_ULP L) + 2^-126     e = exp(-|p|), L = log1p(e); 1 ulp <= 2u relative
                            + u |v|                               the last addition
                 EXP_ULP = 2 and LOG1P_ULP = 1 are the largest errors the public CUDA and HIP math tables state for expf and log1pf.
  loss backward  g = fl(gscale / fl(n)) (mse: fl(gscale fl(2 / fl(n)))); n < 2^24, so fl(n) is n
                     mse   4u |ref| (p - t, two roundings in g, the product)        l1, mean   u |ref|
                     bce   ABSOLUTE: |g / n| (ds + 3u |s - t|), ds = u (2 EXP_ULP s (1 - s) + 2 s) + 2^-126: sigmoid(p) - t cancels (in the
                           reference's own fp32 formula too), so the error is a few u of g / n, not of the result.
  Adam           m'   u (|m'| + 3 wl |g - m|) where wl = fl(1 - b1) < 0.5 (m + wl (g - m): wl, g - m, the product; the sum),
                      u (|m'| + (wl + 3 b1) |g - m|) else (g - (g - m) fl(1 - wl): fl(1 - wl) is off b1 by up to u (wl + b1))
                 v'   u (|v'| + |v b2| + 3 |g^2 (1 - b2)|) + 3 2^-149
                 p'   propagated through sqrt (|sqrt a - sqrt b| <= min(|a - b| / sqrt a, sqrt|a - b|)), / fl32(sqrt(bc2)), + eps, m' / denom,
                      * fl32(lr / bc1), p - .: one u per operation on its own result, see adam_ref
  spectral norm  a dot product of n sequential fmaf (or n additions in a tree: fewer) is within gamma_n sum|w||x|, gamma_n = n u / (1 - n u),
                 of the exact one.  The kernel's lengths: K for W^T u (one thread per column); ceil(M / 64) + 6 per row of W v (a lane's
                 share, then the wave tree); ceil(L / 1024) + 22 for the three workgroup sums (a thread's share, the wave tree, the 16 wave
                 partials); ceil(K M / 1024) + 22 for <G, W / sigma> in the backward.  Each result's limit carries the limits of what it was
                 computed from (spectral_fwd_ref).  A norm below eps / 2 is replaced by eps on both sides (SPECTRAL_TINY); no case has a
                 norm within a factor 2 of eps.
No limit here is a multiple of torch's own fp32 distance: every constant above is derived or, for the two ulp figures, a published statement."""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -149
MINN = 2.0 ** -126
EXP_ULP, LOG1P_ULP = 2.0, 1.0
SN_EPS = 1e-12


def f32(v):
    """the fp32 value of a Python float, as a Python float (the ABI takes floats: 0.9f is not 0.9)"""
    return float(np.float32(v))


def share(err, lim):
    """(max, rms) of err / lim over all elements; lim == 0 demands err == 0; a NaN counts as inf"""
    err, lim = torch.as_tensor(err, dtype=torch.float64).reshape(-1), torch.as_tensor(lim, dtype=torch.float64).reshape(-1)
    s = torch.where(lim > 0, err / lim.clamp_min(1e-320), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    s = torch.where(torch.isnan(s), torch.full_like(s, math.inf), s)
    return s.max().item(), s.pow(2).mean().sqrt().item()


def diff(out, ref):
    """|out - ref| in float64; equal infinities are no error"""
    out, ref = out.double(), ref.double()
    return torch.where(out == ref, torch.zeros_like(ref), (out - ref).abs())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------------------------------------
LOSS_MODES = ('mse', 'l1', 'bce', 'mean')
# the wave, workgroup and cdiv(n, 1024) edges; where k_loss_partial's cap of 256 workgroups starts to bind; where the backward grid (8192 x 256) wraps
LOSS_SIZES = (1, 63, 64, 65, 255, 257, 1023, 1025, 262144, 262145, 8192 * 256 + 257)
TARGETS = (0.0, 1.0, 0.9)
GSCALES = (1.0, -1.0, 0.37)
LOGIT_EDGES = (0.0, 1e-6, -1e-6, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4)


@functools.lru_cache(maxsize=None)
def loss_inputs(mode, n, target=0.0):
    """(a, b) fp32 on the CPU; b only for l1.  bce: logits 3 randn with LOGIT_EDGES at the front and at the back; mse: every tenth input within
    1e-6 of the target; l1: every tenth pair exactly equal, and every tenth (offset 5) two denormals, alternately a > b and a < b;
    mean: 1000 + noise"""
    g = torch.Generator().manual_seed(1000 * LOSS_MODES.index(mode) + n % 9973 + int(10 * target))
    a = torch.randn(n, generator=g)
    b = None
    if mode == 'bce':
        a = 3.0 * a
        e = torch.tensor(LOGIT_EDGES)
        k = min(n, e.numel())
        a[:k] = e[:k]
        if n >= 2 * e.numel():
            a[n - e.numel():] = e.flip(0)
    elif mode == 'mse':
        a = a + target
        a[::10] = torch.tensor(target) + 1e-6 * (2.0 * torch.rand(a[::10].numel(), generator=g) - 1.0)
    elif mode == 'l1':
        b = torch.randn(n, generator=g)
        b[::10] = a[::10]
        a[5::20], b[5::20] = 3e-40, 1e-40
        a[15::20], b[15::20] = 1e-40, 3e-40
    else:
        a = 1000.0 + a
    return a, b


def loss_terms(mode, a, b, target):
    """v_i and the bound e_i of its fp32 evaluation, float64"""
    t = f32(target)
    x = a.double()
    if mode == 'mse':
        v = (x - t) ** 2
        return v, (2 * U + U * U) * v
    if mode == 'l1':
        v = (x - b.double()).abs()
        return v, U * v
    if mode == 'mean':
        return x, torch.zeros_like(x)
    m, xt, ex = x.clamp_min(0.0), x * t, torch.exp(-x.abs())
    lg = torch.log1p(ex)
    v = m - xt + lg
    return v, U * (xt.abs() + (m - xt).abs()) + 2 * U * (EXP_ULP * ex / (1.0 + ex) + LOG1P_ULP * lg) + MINN + U * v.abs()


def loss_fwd(mode, a, b, target):
    """(ref, limit), 0-d float64"""
    v, e = loss_terms(mode, a, b, target)
    n = a.numel()
    ref = v.sum() / n
    return ref, U * ref.abs() + (1 + 4 * U) * (e.sum() + 2.0 ** -44 * v.abs().sum()) / n + TINY


def loss_bwd(mode, a, b, target, gscale):
    """(ref, limit) [n] float64"""
    t, n = f32(target), a.numel()
    G = f32(gscale) / n
    x = a.double()
    if mode == 'mse':
        ref = 2.0 * G * (x - t)
        return ref, 4 * U * (1 + 4 * U) * ref.abs() + TINY
    if mode == 'l1':
        ref = G * torch.sign(x - b.double())
        return ref, U * ref.abs() + TINY
    if mode == 'mean':
        ref = torch.full_like(x, G)
        return ref, U * ref.abs() + TINY
    s = torch.sigmoid(x)
    ds = U * (2 * EXP_ULP * s * (1.0 - s) + 2.0 * s) + MINN
    return (s - t) * G, abs(G) * (ds + 3 * U * (s - t).abs()) * (1 + 4 * U) + TINY


def emu_loss_fwd(mode, a, b, target, variant=None):
    """numpy fp32 restatement of k_loss_partial / k_loss_final.  variants: 'no_max' (bce without max(p, 0)), 'n_minus_1'"""
    x, t = a.numpy(), np.float32(target)
    with np.errstate(all='ignore'):
        if mode == 'mse':
            d = x - t
            v = d.astype(np.float64) ** 2
        elif mode == 'l1':
            v = np.abs(x - b.numpy()).astype(np.float64)
        elif mode == 'mean':
            v = x.astype(np.float64)
        else:
            m = np.zeros_like(x) if variant == 'no_max' else np.maximum(x, np.float32(0))
            v = ((m - x * t) + np.log1p(np.exp(-np.abs(x)))).astype(np.float64)
        n = x.size - 1 if variant == 'n_minus_1' else x.size
        return torch.tensor(float(np.float32(np.float64(v.sum()) / np.float64(n))), dtype=torch.float64)


def emu_loss_bwd(mode, a, b, target, gscale, variant=None):
    """numpy fp32 restatement of k_mse_bwd / k_l1_bwd / k_logit_bwd.  variant: 'plus_g_at_equal' (l1: +g where a == b)"""
    x, t, gs = a.numpy(), np.float32(target), np.float32(gscale)
    nf = np.float32(x.size)
    with np.errstate(all='ignore'):
        if mode == 'mse':
            out = (x - t) * (gs * (np.float32(2) / nf))
        elif mode == 'l1':
            d, g = x - b.numpy(), gs / nf
            out = np.where(d > 0, g, np.where(d < 0, -g, g if variant == 'plus_g_at_equal' else np.float32(0))).astype(np.float32)
        elif mode == 'mean':
            out = np.full_like(x, gs / nf)
        else:
            out = (np.float32(1) / (np.float32(1) + np.exp(-x)) - t) * (gs / nf)
    assert out.dtype == np.float32
    return torch.from_numpy(out)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------------------------
ADAM_BETA1 = (0.0, 0.1, 0.5, 0.9)     # fl(1 - b1) = 1, 0.9, 0.5 (the boundary: not < 0.5), 0.1: the second lerp form three times, the first once
ADAM_BETA2 = (0.9, 0.999)
ADAM_STEPS = (1, 2, 10, 100000)
ADAM_EPS = (1e-8, 1e-3)
ADAM_SIZES = (1, 257, 8192 * 256 + 3)    # the last wraps the 8192 x 256 grid
ADAM_LR = 1e-4
ADAM_SMALL = [(n, b1, b2, st, ep) for n in ADAM_SIZES[:2] for b1 in ADAM_BETA1 for b2 in ADAM_BETA2 for st in ADAM_STEPS for ep in ADAM_EPS]
# at the wrapping size every beta1 (both lerp forms and the boundary), every step, both beta2 and both eps appear
ADAM_LARGE = [(ADAM_SIZES[2], b1, ADAM_BETA2[i % 2], ADAM_STEPS[i], ADAM_EPS[(i + 1) % 2]) for i, b1 in enumerate(ADAM_BETA1)]


@functools.lru_cache(maxsize=4)
def adam_inputs(n):
    """p, g, m, v fp32 [n], v >= 0.  g holds 0, +-1e-30 (g^2 underflows; with v = 0 the denominator is eps alone), +-1e3, 1e-30 at v > 0, and
    an all-zero element, where n allows"""
    gen = torch.Generator().manual_seed(77 + n % 1009)
    p = 0.05 * torch.randn(n, generator=gen)
    g = 0.1 * torch.randn(n, generator=gen)
    m = 0.1 * torch.randn(n, generator=gen)
    v = (0.1 * torch.randn(n, generator=gen)) ** 2
    if n >= 7:
        g[:7] = torch.tensor([0.0, 1e-30, -1e-30, 1e3, -1e3, 1e-30, 0.0])
        v[1], v[2], v[6], m[6] = 0.0, 0.0, 0.0, 0.0
    return p, g, m, v


def adam_ref(p, g, m, v, lr, b1, b2, eps, step):
    """{'p' | 'm' | 'v': (ref, limit)} of one step, float64"""
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    pd, gd, md, vd = p.double(), g.double(), m.double(), v.double()
    D = gd - md
    m1 = md * b1 + (1.0 - b1) * gd          # (not m + (1 - b1)(g - m): at b1 = 0 and |g| << |m| that form loses g even in float64)
    wl = float(np.float32(1) - np.float32(b1))
    lim_m = U * (m1.abs() + (3 * wl if wl < 0.5 else wl + 3 * b1) * D.abs()) * (1 + 64 * U) + TINY
    gg = gd * gd * (1.0 - b2)
    v1 = vd * b2 + gg
    lim_v = U * (v1.abs() + (vd * b2).abs() + 3 * gg.abs()) * (1 + 64 * U) + 3 * TINY
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    ss = lr / bc1
    sq = v1.sqrt()
    dsq = torch.minimum(lim_v / sq.clamp_min(1e-300), lim_v.sqrt())
    q = sq / math.sqrt(bc2)                          # sqrtf (u), fl32(sqrt(bc2)) (u), the division (u)
    dq = dsq / math.sqrt(bc2) + 3 * U * q
    den = q + eps
    dden = dq + U * den
    r = m1 / den
    dr = lim_m / den + r.abs() * dden / den + U * r.abs()
    upd = ss * r                                     # fl32(lr / bc1) (u), the product (u)
    dupd = abs(ss) * dr + 2 * U * upd.abs()
    p1 = pd - upd
    return {'p': (p1, (dupd + U * p1.abs()) * (1 + 64 * U) + TINY), 'm': (m1, lim_m), 'v': (v1, lim_v)}


def emu_adam(p, g, m, v, lr, b1, b2, eps, step, variant=None):
    """numpy fp32 restatement of nc_adam_step / k_adam -> (p, m, v).  variants: 'other_branch' (the lerp form of the other side of
    wl < 0.5), 'no_eps', 'bc2' (bias correction by bc2 instead of its root)"""
    f = np.float32
    p, g, m, v = p.numpy(), g.numpy(), m.numpy(), v.numpy()
    b1, b2, eps = f(b1), f(b2), f(eps)
    bc1 = 1.0 - float(b1) ** step
    bc2 = 1.0 - float(b2) ** step
    ss = f(float(f(lr)) / bc1)
    bc2s = f(bc2 if variant == 'bc2' else math.sqrt(bc2))
    wl = f(1) - b1
    first = bool(wl < f(0.5)) != (variant == 'other_branch')
    with np.errstate(all='ignore'):
        mi = m + wl * (g - m) if first else g - (g - m) * (f(1) - wl)
        vi = v * b2 + g * g * (f(1) - b2)
        den = np.sqrt(vi) / bc2s
        if variant != 'no_eps':
            den = den + eps
        po = p - ss * (mi / den)
    assert po.dtype == mi.dtype == vi.dtype == np.float32
    return torch.from_numpy(po), torch.from_numpy(mi), torch.from_numpy(vi)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# spectral norm
# ---------------------------------------------------------------------------------------------------------------------------------------------
# (K, M): K = 1 (the last PatchGAN layer); M < 64 (less than a wave per row); M = 1; neither a multiple of anything; M past the 1024 threads; K past
# them (and past the 16 waves); the largest 2-D layer; M = 16384, the 3-D layers
SPECTRAL_CASES = [(1, 8192), (64, 16), (3, 1), (17, 65), (128, 1025), (1025, 3), (512, 8192), (64, 16384)]
SPECTRAL_TINY = (17, 65, 1e-20)     # W scaled to 1e-20: both norms fall below eps


def gamma(n):
    return n * U / (1.0 - n * U)


def _cdiv(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def spectral_inputs(K, M, scale=1.0):
    """W [K, M], u [K] (NOT normalised: 2 randn), v [M] (unit length, as the buffers are kept), G [K, M]"""
    gen = torch.Generator().manual_seed(31 * K + M)
    W = torch.randn(K, M, generator=gen) * scale
    u = 2.0 * torch.randn(K, generator=gen)
    v = torch.randn(M, generator=gen)
    v = v / v.norm()
    return W, u, v, torch.randn(K, M, generator=gen)


def _norm_limit(vec, dvec, L, eps):
    """(max(|vec|, eps), its limit): the sum of squares over L-long chains, sqrtf; |vec| < eps / 2 is eps on both sides"""
    N = float(vec.norm())
    if N < 0.5 * eps:
        return eps, 0.0
    return max(N, eps), float(dvec.norm()) + (0.5 * gamma(L) + U) * N


def spectral_fwd_ref(W, u, v, power_iteration, eps=SN_EPS):
    """{'u' | 'v' | 'sigma' | 'w': (ref, limit)} float64, and the two norms (None without the power iteration)"""
    eps = f32(eps)
    K, M = W.shape
    Wd, aW, ud, vd = W.double(), W.double().abs(), u.double(), v.double()
    Ls, Lk, Lm = _cdiv(M, 64) + 6, _cdiv(K, 1024) + 22, _cdiv(M, 1024) + 22
    g2 = 1.0 + 4.0 * gamma(max(K, Ls, Lk, Lm))
    norms = None
    if power_iteration:
        t = Wd.t() @ ud
        dt = gamma(K) * (aW.t() @ ud.abs()) + K * TINY
        Nt, dNt = _norm_limit(t, dt, Lm, eps)
        v1 = t / Nt
        dv = dt / Nt + v1.abs() * (dNt / Nt + 2 * U) + TINY
    else:
        v1, dv = vd, torch.zeros_like(vd)
    s = Wd @ v1
    ds = gamma(Ls) * (aW @ v1.abs()) + aW @ dv + Ls * TINY
    if power_iteration:
        Nsn, dNs = _norm_limit(s, ds, Lk, eps)
        u1 = s / Nsn
        du = ds / Nsn + u1.abs() * (dNs / Nsn + 2 * U) + TINY
        norms = (float(t.norm()), float(s.norm()))
    else:
        u1, du = ud, torch.zeros_like(ud)
    sigma = (u1 * s).sum()
    dsig = gamma(Lk) * (u1 * s).abs().sum() + (du * s.abs() + u1.abs() * ds).sum() + Lk * TINY
    w = Wd / sigma
    dw = w.abs() * (dsig / sigma.abs() + U) + TINY
    return {'u': (u1, du * g2), 'v': (v1, dv * g2), 'sigma': (sigma.reshape(1), (dsig * g2).reshape(1)), 'w': (w, dw * g2)}, norms


def spectral_bwd_ref(G, wsn, u, v, sigma):
    """(dW, limit) float64, of the fp32 operands the backward is handed"""
    K, M = G.shape
    Gd, wd = G.double(), wsn.double()
    L = _cdiv(K * M, 1024) + 22
    c = (Gd * wd).sum()
    dc = gamma(L) * (Gd * wd).abs().sum() + L * TINY
    uv = torch.outer(u.double(), v.double())
    sg = sigma.double().reshape(())
    num = Gd - c * uv
    ref = num / sg
    return ref, (((dc + 2 * U * c.abs()) * uv.abs() + U * num.abs()) / sg.abs() + U * ref.abs()) * (1 + 4 * gamma(L)) + TINY


def spectral_G(kind, G, wsn):
    """the three incoming gradients of the backward: 'random'; 'orthogonal' to W / sigma (c is rounding noise); 'parallel' = W / sigma itself
    (the two terms of the numerator cancel as far as W is rank one)"""
    if kind == 'random':
        return G
    if kind == 'parallel':
        return wsn.clone()
    wd = wsn.double()
    return (G.double() - (G.double() * wd).sum() / (wd * wd).sum() * wd).float()


def emu_spectral_fwd(W, u, v, power_iteration, eps=SN_EPS, variant=None):
    """numpy fp32 restatement of k_spectral_fwd -> (u, v, sigma, w).  variants: 'no_u_update', 'sigma_old_u' (u updated, sigma from the old)"""
    f = np.float32
    W, u0, v0, eps = W.numpy(), u.numpy(), v.numpy(), f(eps)
    u1, v1 = u0, v0
    with np.errstate(all='ignore'):
        if power_iteration:
            t = W.T @ u0
            v1 = t * (f(1) / np.maximum(np.sqrt((t * t).sum(dtype=f)), eps))
        s = W @ v1
        if power_iteration and variant != 'no_u_update':
            u1 = s * (f(1) / np.maximum(np.sqrt((s * s).sum(dtype=f)), eps))
        sigma = ((u0 if variant == 'sigma_old_u' else u1) * s).sum(dtype=f)
        w = W / sigma
    assert w.dtype == u1.dtype == v1.dtype == np.float32
    return torch.from_numpy(np.array(u1)), torch.from_numpy(np.array(v1)), torch.tensor([float(sigma)]), torch.from_numpy(w)


def emu_spectral_bwd(G, wsn, u, v, sigma, variant=None):
    """numpy fp32 restatement of k_spectral_bwd.  variants: 'no_rank_one', 'sigma_twice' (the rank-one term divided by sigma twice)"""
    f = np.float32
    G, wsn, u, v, sg = G.numpy(), wsn.numpy(), u.numpy(), v.numpy(), f(float(sigma))
    with np.errstate(all='ignore'):
        c = (G * wsn).sum(dtype=f)
        r = np.outer(c * u, v)
        if variant == 'sigma_twice':
            r = r / sg
        out = (G if variant == 'no_rank_one' else G - r) / sg
    assert out.dtype == np.float32
    return torch.from_numpy(out)
