"""Cases, references and limits of the op-level tests of csrc/norm_act.hip and the MIP kernels of csrc/misc.hip (tests/test_gpu_norm.py; checked
on the CPU by tests/test_norm_reference.py).  Nothing here calls the library; every function runs on whatever device its operands live on.

REFERENCES, in float64.  Pass 1 (statistics) is computed from the fp32 input values.  Pass 2 (everything else) takes the fp32 `mean` and `rstd`
the op is given as INPUTS, because the ABI does (nc_instnorm_act_fwd / _bwd take them as fp32 arguments), and evaluates the rest in float64:
    InstanceNorm   xhat = (x - mean) rstd,  y = xhat > 0 ? xhat : slope xhat
                   g = xhat > 0 ? dy : slope dy,  m1 = mean(g),  m2 = mean(g xhat),  dx = rstd ((g - m1) - xhat m2),  dbias[c] = sum_(n, voxels) dx
    BatchNorm      z = xhat gamma + beta (the mask is on z),  dbeta = sum gz,  dgamma = sum gz xhat,  M = N S
                   training:   dx = gamma rstd ((gz - dbeta / M) - xhat dgamma / M)        evaluation: dx = gamma rstd gz
                   running statistics: (1 - mom) old + mom new, the variance unbiased (var M / (M - 1); var at M = 1)
    inference tail sigmoid(w2 (b1 + sum_c w1[c] relu(xhat_c)) + b2)
    max-pool, MIP  a plain scan that keeps the FIRST maximum (pool: window order (a, b, c); MIP: ascending along the axis).  NaN beats numbers;
                   in the pool the LAST NaN's position wins (the kernel's `v != v` clause always takes a NaN), in the MIP the first NaN sticks
                   (`v != v && best == best`: a NaN is taken only while the best is a number).

LIMITS, with u = 2^-24, from the fp32 rounding points the kernels spell out (in_bwd_value, bn_value), never from what the kernels return:
    mean           |m - mean64| <= 2u |mean64| + 2^-40 mean|x|
    rstd           |r / rstd64 - 1| <= 4u + 2^-46 E[x^2] / (var64 + eps)         (the second term: fp64 cancellation in q / S - m^2)
    forward        |y - y_ref| <= d_xhat + 1e-30,  d_xhat = 4u (|xhat| + rstd |mean|);  BatchNorm adds 4u (|gamma xhat| + |beta|)
    sums           dgamma, dbeta, dbias, and m1, m2 (which are such sums over their count): fp64 sums on the device, so one fp32 rounding of
                   the result plus the per-element errors of the terms in quadrature,
                       |err| <= 2u |ref| + sqrt(sum_i e_i^2),
                   e_i = |g_i| (d_xhat_i + u' |xhat_i|) for a term g xhat, u' |g_i| for a term g (u' = u where g = slope dy is rounded, slope
                   not 0 or 1; else 0), the dx limit below for dbias.
                   dbias adds u sum_(n, voxels) rstd |g - m1|: quadrature assumes independent errors, and one rounding of in_bwd_value is
                   not -- g is fp32 data (dy, or slope dy) and m1 one constant per instance, so fl(g - m1) is off by the SAME amount for every
                   element of a binade (what m1 has below that binade's ulp), and in the sum of dx these errors add linearly.  The kernel's
                   dbias is also held to the fp64 sum of the dx it stored (dbias_plumbing_limit): that is what catches a lost partial.
    backward       |dx - dx_ref| <= rstd (4u (|g| + |m1| + |xhat m2|) + |m2| d_xhat + d_m1 + |xhat| d_m2);  BatchNorm: times |gamma|, with gz;
                   d_m1, d_m2: the quadrature part of the sums' limit over the count.
    What a first derivation had differently, and what showed it (the fp32 emulation of in_bwd_value on the CPU, tests/test_norm_reference.py
    -- not the kernels):
      * sums as 2u |ref| + 2u sum|terms| / sqrt(count), i.e. 2u mean|term| sqrt(count).  That is not the quadrature sum it was meant to be:
        the root of the sum of squares is rms(term) sqrt(count) >= mean|term| sqrt(count) (1.6 x for a product of two Gaussians, 2.2 x behind
        a ReLU mask), and the per-element error of a term g xhat is |g| d_xhat >= 4u |g xhat|, not 2u.  The emulation reaches 1.27 of that
        form for dgamma at (N, C, S) = (2, 3, 5000).  first_form() still reports the share of it.
      * dx without d_m1 and d_m2: only 4u |m1| and 4u |xhat m2|, roundings RELATIVE to m1 and m2.  But every term of m2 holds the fp32
        roundings of xhat, and m2 is a mean that cancels to ~ 1 / sqrt(S) of its terms' size: its error does not shrink with it.  1.27 of
        that limit at (NC, S) = (3, 2052), slope 0, on an element with g = 0, where nothing else is left in the limit.
      * dbias without the linear term: 3.5 of the quadrature form at S = 2049, 17 at 8196, 85 at 524292 -- growing as sqrt(S), as a linear
        sum does against a quadrature one.  (dgamma's terms carry the random sign of gz; dbeta's are exact or independently rounded.)
    running stats  (not set by the forward limits: an fp32 store of an fp64 expression of the statistics)
                   mean: 2u |ref| + mom (2^-40 mean|x|);  var: 2u |ref| + mom 2^-45 E[x^2] M / (M - 1)    (2^-45 E[x^2]: the rstd limit's
                   cancellation term, as an absolute error of the variance)
    tail           2u (|b1| + sum|w1 t|) |w2| / 4 + 4u     (the sigmoid's slope is at most 1 / 4; 4u on the output)
    pool, MIP      bit-equal

MASK FLIPS.  An element whose float64 xhat lies within d_xhat of zero may take the other branch of the activation in fp32; its dx then differs
by (1 - slope) |dy| rstd, which no rounding limit covers.  Exactly those elements are left out of the element-wise dx comparison (they stay
in the sums); BatchNorm: z within its forward limit of zero.  One refinement, needed by the constant instance: xhat64 == 0 means x == mean
bit for bit, where fp32 computes an exact zero too -- such an element is compared.  The share left out is capped per case (EXCL_CAP; by hand:
a Gaussian xhat has density 0.4 at zero, d_xhat there is 4u rstd |mean| ~ 1e-7 .. 1e-6: a share of ~ 4e-7; the offset-mean case has
rstd |mean| ~ 3.5e3, d_xhat ~ 8e-4 and a uniform xhat of density 0.29: ~ 5e-4 .. 1e-3) and tests/test_norm_reference.py checks it from the
inputs alone.  (For InstanceNorm the exclusion is in fact conservative: near xhat = 0 the fp32 difference x - mean is exact, so the fp32 sign
is the float64 sign.  BatchNorm's z = xhat gamma + beta can really flip.)"""
import functools
import math

import torch

U = 2.0 ** -24
EPS = 9.999999747378752e-06   # 1e-5f, the float the ABI receives
MOMENTUM = 0.10000000149011612   # 0.1f, likewise
SLOPES = (0.0, 0.2)
EXCL_CAP, EXCL_CAP_OFFSET = 1e-4, 5e-3


def f32(v):
    """the fp32 value of a Python float (the ABI takes the slope as a float: 0.2f is not 0.2)"""
    return torch.tensor(v, dtype=torch.float32).item()


# ---- InstanceNorm, long path (S > 2048).  (N, C, S, kind, branch); kind: None (x = 2 randn + 0.5), 'unaligned' (every pointer one float off a
# 16-byte boundary, and a run with only y off), 'offset' (x = 100 + 0.05 uniform(-1, 1)), 'constant' (instance 0 is 1.7 everywhere), 'huge' (the
# NC > 65535 recursion: inputs made on the device, reference in slices).  splits = min(ceil(2048 / NC), ceil(S / 8192)) clamped to [1, 64];
# chunk = ceil(S / splits) rounded up to 4; 16-byte loads when S % 4 == 0 and the base pointers are aligned.
IN_CASES = [
    (2, 1, 2049, None, 'smallest long instance, scalar, 1 split'),
    (1, 3, 2052, None, 'float4, 1 split'),
    (2, 1, 8193, None, '2 splits, scalar, chunk 4097 -> 4100'),
    (2, 1, 8196, None, '2 splits, float4, short last chunk'),
    (1, 5, 13824, None, '24^3, 2 splits'),
    (1, 1, 531441, None, '81^3: cap 65 clamps to 64, scalar'),
    (1, 1, 524292, None, 'clamp to 64, float4, chunk 8193 -> 8196'),
    (4, 275, 24580, None, 'want (2) < cap (4)'),
    (3, 700, 8196, None, 'want = 1 at a multi-chunk length'),
    (1, 1, 1048580, None, 'backward apply wraps its 1024-block grid'),
    (1, 1, 4194308, None, 'forward wraps its 1024-block grid'),
    (1, 3, 8196, 'unaligned', 'unaligned scalar fallback'),
    (2, 1, 16384, 'offset', 'offset mean'),
    (2, 1, 8196, 'constant', 'var = 0, rstd = 1 / sqrt(eps)'),
]
HUGE_CASE = (1, 65537, 2052, 'huge', 'the NC > 65535 recursion')

# (N, C, S, kind); kind 'signs': gamma of mixed sign, beta large enough to move the mask
BN_CASES = [(2, 3, 5000, None), (4, 8, 8196, None), (4, 8, 8193, None), (3, 5, 1, None), (1, 1, 1, None), (2, 4, 2049, 'signs')]

TAIL_C = (1, 64, 256)
TAIL_S = (1, 255, 257, 4099)

# (NC, D, H, W)
POOL_CASES = [(3, 4, 6, 8), (2, 5, 7, 9), (4, 1, 6, 10)]
MIP_SHAPE = (2, 5, 6, 7)


def pick_splits(NC, S):
    """csrc/norm_act.hip pick_splits"""
    return max(1, min(-(-2048 // NC), -(-S // 8192), 64))


def chunk_len(S, splits):
    """csrc/norm_act.hip chunk_range"""
    return (-(-S // splits) + 3) & ~3


def case_id(c):
    return '-'.join(str(v) for v in c[:4] if v is not None)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inputs (on the CPU, seeded; computed once per case, the tests only read them)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def in_inputs(N, C, S, kind):
    """x, dy [N * C, S] fp32 and the noise [N * C] the deliberately wrong statistics are made with."""
    g = torch.Generator().manual_seed(7 * S + N * C)
    NC = N * C
    if kind == 'offset':
        x = 100.0 + 0.05 * (2.0 * torch.rand(NC, S, generator=g) - 1.0)
    else:
        x = torch.randn(NC, S, generator=g) * 2.0 + 0.5
    if kind == 'constant':
        x[0] = 1.7
    dy = torch.randn(NC, S, generator=g)
    return x, dy, torch.randn(NC, generator=g)


def wrong_stats(mean, rstd, noise):
    """Statistics that are deliberately not the instance's: the channel sums of dx are then O(1) instead of rounding noise."""
    return (mean + 0.3 * noise.to(mean.device) / rstd).float(), (rstd * 1.2).float()


@functools.lru_cache(maxsize=None)
def bn_inputs(N, C, S, kind):
    """x, dy [N, C, S], gamma, beta, running_mean, running_var [C]"""
    g = torch.Generator().manual_seed(11 * S + 100 * N + C)
    x = torch.randn(N, C, S, generator=g) * 1.5 + torch.linspace(-1.0, 2.0, C).view(1, C, 1)
    dy = torch.randn(N, C, S, generator=g)
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    if kind == 'signs':
        gamma = gamma * (1.0 - 2.0 * (torch.arange(C) % 2))
        beta = torch.tensor([0.8, -0.9, 1.1, -0.7])[:C] * gamma.abs()
    rm = 0.2 * torch.randn(C, generator=g)
    rv = 0.5 + torch.rand(C, generator=g)
    return x, dy, gamma, beta, rm, rv


@functools.lru_cache(maxsize=None)
def tail_inputs(C, S):
    g = torch.Generator().manual_seed(13 * S + C)
    x = torch.randn(C, S, generator=g) * 2.0 + 0.5
    w1 = torch.randn(C, generator=g) * (2.0 / C) ** 0.5
    b1, w2, b2 = torch.tensor([0.3]), torch.tensor([-1.7]), torch.tensor([0.4])
    return x, w1, b1, w2, b2


def tied(shape, seed):
    """relu(uniform(-1, 1)): about half zeros (the network pools behind a ReLU), and a quarter of the 2 x 2 x 2 blocks zero as a whole, so
    that whole windows tie"""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(2.0 * torch.rand(*shape, generator=g) - 1.0)
    keep = (torch.rand(*shape[:-3], *(-(-v // 2) for v in shape[-3:]), generator=g) > 0.25).float()
    for d in (-3, -2, -1):
        keep = keep.repeat_interleave(2, d)
    return x * keep[..., :shape[-3], :shape[-2], :shape[-1]]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# shares of a limit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def share(err, lim, keep=None):
    """(max, rms) of err / lim over the elements of `keep` (all by default).  lim == 0 demands err == 0 (share 0, else inf)."""
    s = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    if keep is not None:
        s = s[keep]
    if s.numel() == 0:
        return 0.0, 0.0
    return s.max().item(), s.pow(2).mean().sqrt().item()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# statistics (pass 1)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def stats64(x, dims=(1,)):
    """mean64, var64 (biased, two-pass), rstd64, mean|x|, E[x^2] over `dims` of the fp32 x, in float64"""
    xd = x.double()
    mean = xd.mean(dims, keepdim=True)
    var = (xd - mean).pow(2).mean(dims)
    mean = mean.reshape(var.shape)
    return mean, var, 1.0 / (var + EPS).sqrt(), xd.abs().mean(dims), xd.pow(2).mean(dims)


def mean_share(m, st):
    return share((m.double() - st[0]).abs(), 2 * U * st[0].abs() + 2.0 ** -40 * st[3])


def rstd_share(r, st):
    return share((r.double() / st[2] - 1.0).abs(), 4 * U + 2.0 ** -46 * st[4] / (st[1] + EPS))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# InstanceNorm (pass 2): x, dy [NC, S]; mean, rstd [NC] fp32
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _xhat(x, mean, rstd):
    m, r = mean.double().unsqueeze(-1), rstd.double().unsqueeze(-1)
    xhat = (x.double() - m) * r
    return xhat, r, 4 * U * (xhat.abs() + r * m.abs())


def in_fwd(x, mean, rstd, slope):
    """y_ref, limit"""
    xhat, _, d = _xhat(x, mean, rstd)
    return torch.where(xhat > 0, xhat, f32(slope) * xhat), d + 1e-30


def in_bwd(dy, x, mean, rstd, slope):
    """dx_ref, limit, the elements that may flip their mask (left out of the element-wise comparison), and per instance the linear bound of the
    correlated rounding of g - m1 in the sum of dx (u rstd sum|g - m1|: see LIMITS, sums)"""
    xhat, r, d = _xhat(x, mean, rstd)
    dyd = dy.double()
    g = torch.where(xhat > 0, dyd, f32(slope) * dyd)
    m1 = g.mean(1, keepdim=True)
    m2 = (g * xhat).mean(1, keepdim=True)
    p = xhat * m2
    dx = r * ((g - m1) - p)
    S = x.shape[1]
    d_m1 = quad(_u1(slope) * g, (1,)) / S
    d_m2 = quad(g * (d + _u1(slope) * xhat.abs()), (1,)) / S
    lim = r * (4 * U * (g.abs() + m1.abs() + p.abs()) + m2.abs() * d + d_m1 + xhat.abs() * d_m2)
    return dx, lim, (xhat != 0) & (xhat.abs() <= d), U * r.squeeze(-1) * (g - m1).abs().sum(1)


def _u1(slope):
    """u where g = slope dy is a rounded product, 0 where it is dy or zero"""
    return 0.0 if f32(slope) in (0.0, 1.0) else U


def quad(e, dims):
    """root of the sum of squares over dims (kept)"""
    return e.pow(2).sum(dims, keepdim=True).sqrt()


def first_form(ref, terms, dims):
    """the sums' limit as first derived (see the module text): 2u |ref| + 2u sum|terms| / sqrt(count); reported, not asserted"""
    count = math.prod(terms.shape[d] for d in dims)
    return 2 * U * ref.abs() + 2 * U * terms.abs().sum(dims) / math.sqrt(count)


def dbias_ref(dx, lim, corr, N, C):
    """dx, lim [N * C, S] float64 and corr [N * C] of in_bwd -> (dbias [C], limit, the first form of the limit)"""
    d3 = dx.reshape(N, C, -1)
    ref = d3.sum((0, 2))
    return ref, 2 * U * ref.abs() + quad(lim.reshape(N, C, -1), (0, 2)).reshape(C) + corr.reshape(N, C).sum(0), first_form(ref, d3, (0, 2))


def dbias_plumbing_limit(dx_stored, N, C):
    """the kernel's dbias against the fp64 sum of the fp32 dx it stored: (sum [C], limit) -- the partial sums are fp64 on the device, so one fp32
    rounding of the result and the fp64 summation error (2^-53 per addition, taken as 2^-40 of the sum of magnitudes)"""
    d3 = dx_stored.double().reshape(N, C, -1)
    ref = d3.sum((0, 2))
    return ref, U * ref.abs() + 2.0 ** -40 * d3.abs().sum((0, 2))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm: x, dy [N, C, S]; mean, rstd, gamma, beta [C] fp32
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _bn_z(x, mean, rstd, gamma, beta):
    v = lambda t: t.double().view(1, -1, 1)  # noqa: E731
    m, r, ga, be = v(mean), v(rstd), v(gamma), v(beta)
    xhat = (x.double() - m) * r
    d = 4 * U * (xhat.abs() + r * m.abs())
    return xhat, xhat * ga + be, r, ga, d, d + 4 * U * ((ga * xhat).abs() + be.abs()) + 1e-30


def bn_fwd(x, mean, rstd, gamma, beta, slope):
    _, z, _, _, _, lim = _bn_z(x, mean, rstd, gamma, beta)
    return torch.where(z > 0, z, f32(slope) * z), lim


def bn_bwd(dy, x, mean, rstd, gamma, beta, slope, training):
    """dx_ref, its limit, the elements left out, (dgamma, limit, first form), (dbeta, limit, first form)"""
    xhat, z, r, ga, d, zlim = _bn_z(x, mean, rstd, gamma, beta)
    dyd = dy.double()
    gz = torch.where(z > 0, dyd, f32(slope) * dyd)
    M = x.shape[0] * x.shape[2]
    dbeta = gz.sum((0, 2))
    dgamma = (gz * xhat).sum((0, 2))
    m1 = (dbeta / M).view(1, -1, 1) if training else torch.zeros_like(r)
    m2 = (dgamma / M).view(1, -1, 1) if training else torch.zeros_like(r)
    p = xhat * m2
    dx = ga * r * ((gz - m1) - p)
    q1 = quad(_u1(slope) * gz, (0, 2))
    q2 = quad(gz * (d + _u1(slope) * xhat.abs()), (0, 2))
    lim = ga.abs() * r * (4 * U * (gz.abs() + m1.abs() + p.abs()) + m2.abs() * d)
    if training:
        lim = lim + ga.abs() * r * (q1 + xhat.abs() * q2) / M
    return (dx, lim, z.abs() <= zlim, (dgamma, 2 * U * dgamma.abs() + q2.reshape(-1), first_form(dgamma, gz * xhat, (0, 2))),
            (dbeta, 2 * U * dbeta.abs() + q1.reshape(-1), first_form(dbeta, gz, (0, 2))))


def bn_running(rm, rv, st, M, mom=MOMENTUM):
    """(running_mean, limit), (running_var, limit) after one training step; st = stats64(x, (0, 2))"""
    unb = M / (M - 1.0) if M > 1 else 1.0
    nm = (1.0 - mom) * rm.double() + mom * st[0]
    nv = (1.0 - mom) * rv.double() + mom * st[1] * unb
    return (nm, 2 * U * nm.abs() + mom * 2.0 ** -40 * st[3]), (nv, 2 * U * nv.abs() + mom * 2.0 ** -45 * st[4] * unb)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the inference tail: x [C, S]; mean, rstd, w1 [C]; b1, w2, b2 [1]
# ---------------------------------------------------------------------------------------------------------------------------------------------
def tail(x, mean, rstd, w1, b1, w2, b2):
    xhat, _, _ = _xhat(x, mean, rstd)
    wt = w1.double().unsqueeze(-1) * torch.relu(xhat)
    a = b1.double() + wt.sum(0)
    y = torch.sigmoid(w2.double() * a + b2.double())
    return y, 2 * U * (b1.double().abs() + wt.abs().sum(0)) * w2.double().abs() * 0.25 + 4 * U


# ---------------------------------------------------------------------------------------------------------------------------------------------
# max-pool (window 2, or 1 x 2 x 2 at D == 1; floor mode) and MIP: first maximum in scan order
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _windows(x):
    """x [NC, D, H, W] -> [NC, Do, Ho, Wo, wd * 4], the window elements in scan order (a, b, c), and wd"""
    NC, D, H, W = x.shape
    wd = 2 if D > 1 else 1
    Do, Ho, Wo = D // wd, H // 2, W // 2
    xc = x[:, :Do * wd, :Ho * 2, :Wo * 2]
    return xc.reshape(NC, Do, wd, Ho, 2, Wo, 2).permute(0, 1, 3, 5, 2, 4, 6).reshape(NC, Do, Ho, Wo, wd * 4), wd


def _scan(cols, pool_rule):
    """(best, index) of the scan over the last axis.  pool_rule: start at -inf, a NaN is always taken; else (MIP) start at the first element, a
    NaN is taken only while the best is a number."""
    if pool_rule:
        best = torch.full_like(cols[..., 0], -math.inf)
        arg = torch.zeros(cols.shape[:-1], dtype=torch.int64, device=cols.device)
        first = 0
    else:
        best, arg, first = cols[..., 0].clone(), torch.zeros(cols.shape[:-1], dtype=torch.int64, device=cols.device), 1
    for k in range(first, cols.shape[-1]):
        v = cols[..., k]
        take = (v > best) | (torch.isnan(v) if pool_rule else (torch.isnan(v) & ~torch.isnan(best)))
        best = torch.where(take, v, best)
        arg = torch.where(take, torch.full_like(arg, k), arg)
    return best, arg


def pool_fwd(x):
    cols, _ = _windows(x)
    return _scan(cols, True)[0]


def pool_bwd(dy, x, skip=None):
    """dx [NC, D, H, W] fp32: dy at the first maximum of each window, zero elsewhere (an odd size's border included); skip: added (fp32)"""
    NC, D, H, W = x.shape
    cols, wd = _windows(x)
    _, arg = _scan(cols, True)
    gw = torch.zeros_like(cols).scatter_(-1, arg.unsqueeze(-1), dy.reshape(arg.shape).unsqueeze(-1))
    Do, Ho, Wo = D // wd, H // 2, W // 2
    dx = torch.zeros_like(x)
    dx[:, :Do * wd, :Ho * 2, :Wo * 2] = gw.reshape(NC, Do, Ho, Wo, wd, 2, 2).permute(0, 1, 4, 2, 5, 3, 6).reshape(NC, Do * wd, Ho * 2, Wo * 2)
    return dx if skip is None else skip + dx


def mip_fwd(vol, axis, start, depth):
    """vol [NC, D, H, W]; (out, arg) over vol[start : start + depth] along `axis` (0 / 1 / 2 = D / H / W); arg is the absolute coordinate"""
    cols = vol.narrow(axis + 1, start, depth).movedim(axis + 1, -1)
    best, arg = _scan(cols, False)
    return best, (arg + start).to(torch.int32)


def mip_bwd(dout, arg, shape, axis):
    dvol = torch.zeros(shape, dtype=dout.dtype, device=dout.device)
    return dvol.scatter_(axis + 1, arg.long().unsqueeze(axis + 1), dout.unsqueeze(axis + 1))


def plant_nans(x, positions):
    """a copy of x [NC, ...] with a NaN at each of `positions` (index tuples)"""
    x = x.clone()
    for p in positions:
        x[p] = math.nan
    return x


def bits(t):
    """int32 view: bit equality that also holds NaN to NaN"""
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels' arithmetic (every operation rounded to fp32, the sums in fp64): the limits are checked against it on the CPU,
# with deliberately wrong variants that must fail them
# ---------------------------------------------------------------------------------------------------------------------------------------------
def emu_in_fwd(x, mean, rstd, slope, bf16_mean=False):
    m = mean.bfloat16().float() if bf16_mean else mean
    v = (x - m.unsqueeze(-1)) * rstd.unsqueeze(-1)
    return torch.where(v > 0, v, v * slope)


def emu_in_bwd(dy, x, mean, rstd, slope, splits=1, bf16_mean=False, drop_last_split=False):
    """in_bwd_value with m1, m2 from fp64 sums over `splits` chunks (chunk_len); drop_last_split: m2 without its last chunk"""
    S = x.shape[1]
    m = (mean.bfloat16().float() if bf16_mean else mean).unsqueeze(-1)
    r = rstd.unsqueeze(-1)
    xh = (x - m) * r
    g = torch.where(xh > 0, dy, dy * slope)
    ch = chunk_len(S, splits)
    s1 = torch.zeros(x.shape[0], dtype=torch.float64)
    s2 = torch.zeros(x.shape[0], dtype=torch.float64)
    for k in range(splits):
        b, e = min(k * ch, S), min((k + 1) * ch, S)
        s1 += g[:, b:e].double().sum(1)
        if not (drop_last_split and k == splits - 1):
            s2 += (g[:, b:e].double() * xh[:, b:e].double()).sum(1)
    m1, m2 = (s1 / S).float().unsqueeze(-1), (s2 / S).float().unsqueeze(-1)
    p = xh * m2
    return r * ((g - m1) - p)
