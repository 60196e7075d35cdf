"""Geometry, plan, references, yardsticks, limits and cases of the stage-level tests of the fused KernelGAN discriminator (csrc/kgan.hip:
nc_kgan_fwd / nc_kgan_bwd).  tests/test_gpu_kernelgan_fp64.py runs the cases through the C ABI; tests/test_kgan_reference.py checks this module
on the CPU.  Nothing here calls the library; every function runs on whatever device its operands live on.

LAYOUT (kgan.hip): every 64-channel map is [B][64][P], the statistics [B][64][2] = (mean, 1 / sqrt(var + eps)), x is [B][D][H][W], the collapsed
weights W' are [64][T] with the taps in (tz, ty, tx) order, T = 7^nd.  geo(), plan() and saved_layout() restate kgan.hip's geo(), plan() and
saved_floats() as pure functions; branches() names what a case reaches in each kernel.

REFERENCES, in float64, one function per stage; each takes the stage's inputs as given (fp32 tensors from the device are fed in as they are, so
no error compounds from one stage into the next):
    z2 = W2 (W1 * x + b1) + b2 by the layered definition, the 64-channel z1 formed;  st = (mean, rstd) of a map;  z3, z4 = W relu(IN(z)) + b;
    y = W5 relu(IN(z4)) + b5;  gz = rstd (gn - mean(gn) - n mean(gn n)) with gn = W5[c] dy [n > 0] at the top, the masked data gradient below;
    da = (W^T gz) [n > 0];  dW = sum gz relu(IN(z below))^T, db = sum gz;  G = sum gz2 patch(x)^T, s = sum gz2;  dW1 = W2^T G, db1 = W2^T s,
    dW2 = G W1^T + s b1^T, db2 = s;  dW5 = sum dy relu(IN(z4)), db5 = sum dy;  dx = the full correlation of gz2 with W2 W1.
RELU MASKS of the backward references are the kernels': ((z - mu) * rs) > 0 evaluated in float32 from the saved float32 z and st (n32()) -- a
subtraction followed by a multiplication, two roundings nothing can contract -- so the device's masks are reproduced bit for bit and no element
is left out of any comparison.  (The sign of that product is the sign of z - mu, which fp32 gets exactly, so the float64 forward has the same
mask too.)

YARDSTICKS for the GEMM stages (z2, z3, z4, y, the data gradients, every dW / G, dW1, dW2, dx): the one-accumulator fp32 chain of the stage in
the order kgan.hip's comments give, every product and every partial sum rounded to fp32 (chain_* below, as chain_* of conv_fp32_reference.py):
z2 in the collapsed order -- W' over the 64 channels, then the taps, the bias last; the 1 x 1 layers over the input channels, the bias last;
weight gradients over (b, p); dx over (tz, c, ty, tx).  ERROR MEASURE and LIMIT: tests/convt_reference.py's, unchanged (err, within, FACTOR = 3,
MAX_FLOOR = 2^-21, RMS_FLOOR = 2^-23).  Where a tensor is compared with the whole float64 backward from `saved` (errors of several stages in
it), the yardstick is the same stages composed in fp32: emu_backward(), the chains and the row kernels' arithmetic.  The maps gz2 and gz3 can
only be read behind a data gradient AND k_kg_norm_bwd (the workspace keeps no data gradient), so they are GEMM stages with the row kernel's
arithmetic in the yardstick -- and they are compared DIVIDED BY THE ROW'S rstd (per_row(): an fp32 input, the same number on both sides).  A
row of gz is rstd times a difference of order one, and rstd spans 2.6 (median) to 50 over the rows of a small case: 70 to 83 % of the squared
error of such a map then sits in three of its 64 .. 128 rows, its maximum and rms are statistics of those three rows, and two correct summation
orders differ by more than the factor 3 in them (first run on the device, undivided: 1.03 of the limit for gz2 from gz3 at P = 3, 1.17 for gz2
at P = 4, with gz3 of the same calls at 0.3; the CPU emulations of three orders spread as widely).  Divided, the rows have one scale.
The same holds one step on, for what is compared with the WHOLE backward and has one row per channel of a gz (r4 / dW4, r3 / dW3, r7 / G, dW2):
row c carries the scale of gz's rows c, and on a plane of four pixels every element of G's row c is driven by the same four rounding errors of
gz2 (undivided, second run: G at P = 4 at 1.31 of the limit in the maximum, 0.63 in the rms, G from the device's own gz2 at 0.2).  They are
compared with row c divided by row_scale(): sqrt(sum_b rstd[b][c]^2) of that layer's saved statistics.  Fed with the device's own gz these
tensors are plain GEMM stages and are compared as they are; so are dW1 and dx, which mix the channels.

LIMITS of the row kernels (k_kg_stats, k_kg_norm_bwd: fp64 sums on the device), u = 2^-24, tests/norm_reference.py's wherever the function fits:
    mean           norm_reference.mean_share:  2u |mean64| + 2^-40 mean|z|
    rstd           4u + 2^-46 E[(z - z0)^2] / (var64 + eps).  norm_reference.rstd_share has E[z^2] in the second term, the cancellation of
                   q / S - m^2 over the raw values; k_kg_stats sums the values SHIFTED by the row's first one (z0), so the cancellation it can
                   have is that of the shifted values.  Same terms, the shifted second moment: it does not fit as imported, this is why.
    gz             norm_reference.in_bwd's dx limit, rstd (4u (|gn| + |m1| + |n m2|) + |m2| d_n + d_m1 + |n| d_m2), d_n = 4u (|n| + rstd |mean|),
                   d_m1, d_m2 the quadrature part of the sums' limit over P.  in_bwd itself does not fit: it takes its mask from the float64 n
                   and its g from dy alone, the kernel's g below the top layer is a tensor.  u' = u at the top layer (gn = W5 dy is a rounded
                   product), 0 below.
    sums           pw5[b][c] = sum_p dy relu(n), pb5[b] = sum_p dy (fp64 sums, one fp32 rounding):  2u |ref| + sqrt(sum e_i^2) + 2^-40 sum|term|,
                   e_i = |dy_i| d_n_i [n_i > 0] (norm_reference's sums' limit, and the fp64 summation error of its dbias_plumbing_limit).
    fp32 sums      s = db2, db3, db4 (k_kg_wgrad's per-lane fp32 sums of gz, added in a fixed order) and dW5, db5 (k_kg_grads adds pw5 / pb5 over
                   b in fp32) are sums of fp32 terms IN fp32, which norm_reference's fp64 form does not cover; from the same terms, with every
                   partial sum rounded:  2u |ref| + 2u sum|terms|.  A serial chain of n terms of size sigma errs by about u sigma n / sqrt(2)
                   = 0.9 u sum|terms|; every blocked order is below it.  The sums of gz are analytically zero (the InstanceNorm in front of them
                   removes any constant), so this is a limit on sum|gz|, not a relative measure.  db1 = W2^T s: |W2|^T of s's limit, and for its own
                   chain of 64 terms of very unequal size the worst case 64 u sum|terms| (fed with the device's own s it is a GEMM stage).  That holds for the sums of the gz the device itself stored (db3 from its gz3, s from its gz2).
                   Against the whole float64 backward the terms differ too -- the device's gz carries k_kg_norm_bwd's own rounding, and on planes
                   of two to four pixels gz is a cancellation residue far below that rounding -- so there the limit adds the gz limit above,
                   summed over the terms (linearly: the roundings of n repeat along a row), as norm_reference.dbias_ref adds the dx limit."""
import collections
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_reference as N  # noqa: E402
from convt_reference import FACTOR, MAX_FLOOR, RMS_FLOOR, err, ratios, within  # noqa: E402,F401

U = N.U
EPS = N.EPS
C = 64            # kC
THREADS = 256     # kThreads
TILE7 = 128       # kTile: pixels per k_kg_conv7 workgroup, 16 per (wave, nt)
TILE1 = 256       # kTile1: pixels per k_kg_1x1 workgroup, 4 per lane
UNIT = 64         # kUnit
WG = C * C + C    # kWg
DX_R, DX_C = 16, 64
NC_OK, NC_ERR_SHAPE, NC_ERR_WS, NC_ERR_ARG = 0, -1, -2, -4

Geo = collections.namedtuple('Geo', 'B D H W nd T Tp nblk Do Ho Wo S P')
Plan = collections.namedtuple('Plan', 'cp units per p1 p7 o_wc o_bc o_a o_b o_pw5 o_pb5 o_r3 o_r4 o_r7 o_part total')


def cdiv(a, b):
    return -(-a // b)


def geo(B, D, H, W, nd, ndf=C):
    """kgan.hip geo(): (Geo, NC_OK) or (None, the refusal)."""
    if nd not in (2, 3):
        return None, NC_ERR_ARG
    if ndf != C or (nd == 2 and D != 1) or B < 1 or H < 7 or W < 7 or (nd == 3 and D < 7):
        return None, NC_ERR_SHAPE
    T = 343 if nd == 3 else 49
    Do, Ho, Wo = (D - 6 if nd == 3 else 1), H - 6, W - 6
    P = Do * Ho * Wo
    if P < 2 or B > 65535 or B * D > 65535 or P > 1 << 30 or B * C * P > 1 << 40:
        return None, NC_ERR_SHAPE
    return Geo(B, D, H, W, nd, T, (T + 3) // 4 * 4, cdiv(T, 64), Do, Ho, Wo, D * H * W, P), NC_OK


def al(n):
    return (n + 63) // 64 * 64


def plan(g):
    """kgan.hip plan(): the weight-gradient split and every workspace offset, in floats."""
    cp = cdiv(g.P, UNIT)
    units = g.B * cp
    per = cdiv(units, min(1024 // g.nblk, units))
    p1 = cdiv(units, per)
    sizes = [('o_wc', al(C * g.Tp)), ('o_bc', al(C)), ('o_a', al(g.B * C * g.P)), ('o_b', al(g.B * C * g.P)), ('o_pw5', al(g.B * C)),
             ('o_pb5', al(g.B)), ('o_r3', al(WG)), ('o_r4', al(WG)), ('o_r7', al(g.nblk * WG)), ('o_part', p1 * g.nblk * WG)]
    off, o = {}, 0
    for k, n in sizes:
        off[k] = o
        o += n
    return Plan(cp=cp, units=units, per=per, p1=p1, p7=p1, total=o, **off)


def saved_layout(g):
    """Offsets of z2, z3, z4, st2, st3, st4 in `saved` and its size (kgan.hip saved_floats and the pointer arithmetic of nc_kgan_fwd)."""
    m, s = g.B * C * g.P, 2 * g.B * C
    return dict(z2=0, z3=m, z4=2 * m, st2=3 * m, st3=3 * m + s, st4=3 * m + 2 * s, total=3 * m + 3 * s)


def param_floats(nd):
    T = 343 if nd == 3 else 49
    return C * T + C + 3 * WG + C + 1


LABELS = ['1x1/V', '1x1/scalar', '1x1/one-tile', '1x1/tiles', '1x1/last-full', '1x1/last-partial', '1x1/quads-out', '1x1/ragged-quad',
          'conv7/full', 'conv7/partial', 'conv7/16-off', 'conv7/Wo1', 'conv7/Ho1', 'conv7/Do1',
          'rows/P2', 'rows/P<256', 'rows/P>256',
          'wgrad/per1', 'wgrad/per2-3', 'wgrad/per>=5', 'wgrad/short-last', 'wgrad/ragged-unit', 'wgrad/cp1', 'wgrad/tapblocks1',
          'wgrad/tapblocks6',
          'reduce/<16', 'reduce/16', 'reduce/>16+tail',
          'dx/xtiles1', 'dx/xtiles>1', 'dx/W%4', 'dx/H%16', 'dx/depth-low', 'dx/depth-high',
          'grads/B1', 'grads/B>1']


def branches(case):
    """The labels a case (B, D, H, W, nd, ...) reaches, from the launch arithmetic of kgan.hip alone."""
    g, code = geo(*case[:5])
    assert code == NC_OK, case
    pl = plan(g)
    out = set()

    def add(cond, label):
        if cond:
            out.add(label)
    # k_kg_1x1: 256 pixels per workgroup, a lane holds 4 consecutive ones; V (16-byte accesses) when P % 4 == 0
    last1 = g.P - TILE1 * (cdiv(g.P, TILE1) - 1)
    add(g.P % 4 == 0, '1x1/V')
    add(g.P % 4 != 0, '1x1/scalar')
    add(g.P <= TILE1, '1x1/one-tile')
    add(g.P > TILE1, '1x1/tiles')
    add(last1 == TILE1, '1x1/last-full')
    add(last1 < TILE1, '1x1/last-partial')
    add(TILE1 - last1 >= 4, '1x1/quads-out')      # a lane with all four pixels outside
    add(g.P % 4 != 0, '1x1/ragged-quad')           # a lane with some pixels inside and some outside
    # k_kg_conv7: 128 pixels per workgroup in 8 tiles of 16
    last7 = g.P - TILE7 * (cdiv(g.P, TILE7) - 1)
    add(last7 == TILE7, 'conv7/full')
    add(last7 < TILE7, 'conv7/partial')
    add(TILE7 - last7 >= 16, 'conv7/16-off')
    add(g.Wo == 1, 'conv7/Wo1')
    add(g.Ho == 1, 'conv7/Ho1')
    add(g.nd == 3 and g.Do == 1, 'conv7/Do1')
    # k_kg_stats, k_kg_norm_bwd: one workgroup of 256 threads per row
    add(g.P == 2, 'rows/P2')
    add(g.P < THREADS, 'rows/P<256')
    add(g.P > THREADS, 'rows/P>256')
    # k_kg_wgrad: a workgroup takes `per` units, wave w every fourth
    add(pl.per == 1, 'wgrad/per1')
    add(pl.per in (2, 3), 'wgrad/per2-3')
    add(pl.per >= 5, 'wgrad/per>=5')
    add(pl.units % pl.per != 0, 'wgrad/short-last')
    add(g.P % UNIT != 0, 'wgrad/ragged-unit')
    add(pl.cp == 1, 'wgrad/cp1')
    add(g.nblk == 1, 'wgrad/tapblocks1')
    add(g.nblk == 6, 'wgrad/tapblocks6')
    # k_kg_reduce: 16 parts at a time, then a tail
    add(pl.p1 < 16, 'reduce/<16')
    add(pl.p1 == 16, 'reduce/16')
    add(pl.p1 > 16 and pl.p1 % 16 != 0, 'reduce/>16+tail')
    # k_kg_dx: 16 rows x 64 columns of one input plane
    add(cdiv(g.W, DX_C) == 1, 'dx/xtiles1')
    add(cdiv(g.W, DX_C) > 1, 'dx/xtiles>1')
    add(g.W % 4 != 0, 'dx/W%4')
    add(g.H % DX_R != 0, 'dx/H%16')
    add(g.nd == 3, 'dx/depth-low')                 # qz < 6: taps with qz - tz < 0
    add(g.nd == 3, 'dx/depth-high')                # qz >= Do: taps with qz - tz >= Do
    add(g.B == 1, 'grads/B1')
    add(g.B > 1, 'grads/B>1')
    return out


# (B, D, H, W, nd, offset of the input).  The smallest shapes per label; what each is for stands beside it (P, and the plan where it matters).
CASES = [
    (1, 1, 8, 7, 2, 0.0),        # P = 2: the InstanceNorm worst case; every lane quad ragged, conv7's second 16-pixel tile off
    (1, 1, 12, 49, 2, 1e5),      # P = 258 with a mean some 3e5 times the spread: k_kg_stats' shifted sums.  (Not at P = 2: the square of an fp32
                                 # value is exact in fp64 and so is a sum of up to 32 of them -- unshifted fp64 sums lose 2^-53 mean^2 / var only
                                 # from P = 33 on, and only then can a test tell the shift is there.)
    (16, 1, 8, 7, 2, 0.0),       # 16 units: exactly 16 partial slabs
    (2, 1, 7, 9, 2, 0.0),        # Ho = 1, P = 3
    (3, 1, 10, 7, 2, 0.0),       # Wo = 1, P = 4: the V path with whole quads out
    (1, 1, 22, 22, 2, 0.0),      # P = 256: one full 1x1 tile, two conv7 tiles, four units; H crosses a 16-row dx tile
    (2, 1, 7, 263, 2, 0.0),      # P = 257 (prime): one past the tile, scalar, five 64-column dx tiles, W % 4 = 3
    (1, 1, 19, 26, 2, 0.0),      # P = 260: V with a partial last tile
    (2, 1, 12, 49, 2, 0.0),      # P = 258: scalar, ragged unit
    (1, 1, 33, 71, 2, 0.0),      # P = 1755: several tiles of every kind, the row kernels' strided loops, dx tiles ragged both ways
    (513, 1, 11, 19, 2, 0.0),    # P = 65, cp = 2: 1026 units, per = 2, 513 slabs = 32 x 16 + 1
    (2049, 1, 11, 19, 2, 0.0),   # P = 65, cp = 2: 4098 units, per = 5, 820 workgroups, the last with 3 units: every wave takes two units
    (1, 7, 8, 8, 3, 0.0),        # Do = 1, P = 4: only tz = qz lands in range
    (1, 8, 9, 10, 3, 0.0),       # P = 24
    (2, 13, 13, 13, 3, 0.0),     # P = 343, P % 4 = 3; six tap blocks, the last with 23 of 64 taps
    (5, 20, 20, 20, 3, 0.0),     # P = 2744, 215 units on 170 workgroups: per = 2
    (33, 17, 17, 17, 3, 0.0),    # P = 1331, 693 units on 170: per = 5, p7 = 139, the last workgroup short
]


def case_id(c):
    return '%dd-%d-%s%s' % (c[4], c[0], 'x'.join(str(v) for v in (c[1:4] if c[4] == 3 else c[2:4])), '+%g' % c[5] if c[5] else '')


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def rnd(seed, shape):
    return np.random.default_rng(int(seed)).random(tuple(int(s) for s in shape), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def params(nd, seed=5):
    """The ten tensors in state-dict order, packed (fp32, on the CPU): the seeded weights every KernelGAN test here uses."""
    from neuroclear_amd.util import seed as S
    w = S.weights_from_seed(S.kernelgan_spec(nd), seed)
    return torch.from_numpy(np.concatenate([v.ravel() for v in w.values()]))


@functools.lru_cache(maxsize=2)
def inputs(case):
    """x [B, D, H, W] = rnd - 0.5 (+ the case's offset) and dy [B, P] standard normal, fp32 on the CPU."""
    g, _ = geo(*case[:5])
    seed = 7 * g.B + 11 * g.S + g.nd
    x = torch.from_numpy(rnd(seed, (g.B, g.D, g.H, g.W)) - np.float32(0.5)) + np.float32(case[5])
    dy = torch.from_numpy(np.random.default_rng(seed + 1).standard_normal((g.B, g.P)).astype(np.float32))
    return x, dy


def unpack(prm, nd):
    """kgan.hip unpack(): W1 [64, T], b1, W2 [64, 64], b2, W3, b3, W4, b4, W5 [64], b5 [1] -- views of the packed parameters."""
    T = 343 if nd == 3 else 49
    out, o = {}, 0
    for k, shape in (('W1', (C, T)), ('b1', (C,)), ('W2', (C, C)), ('b2', (C,)), ('W3', (C, C)), ('b3', (C,)), ('W4', (C, C)), ('b4', (C,)),
                     ('W5', (C,)), ('b5', (1,))):
        n = int(np.prod(shape))
        out[k] = prm[o:o + n].view(*shape)
        o += n
    assert o == prm.numel() == param_floats(nd)
    return out


def taps(g):
    return [(tz, ty, tx) for tz in range(7 if g.nd == 3 else 1) for ty in range(7) for tx in range(7)]


def window(x, g, t):
    """[B, P]: the input value tap t meets at every output pixel"""
    return x.view(g.B, g.D, g.H, g.W)[:, t[0]:t[0] + g.Do, t[1]:t[1] + g.Ho, t[2]:t[2] + g.Wo].reshape(g.B, g.P)


def patches(x, g):
    """[B, T, P]"""
    return torch.stack([window(x, g, t) for t in taps(g)], 1)


def n32(z, st):
    """The kernels' nrm(): (z - mu) * rs, two roundings in the dtype of z -- float32 for what the device saved.  z [B, 64, P], st [B, 64, 2]."""
    assert z.dtype == st.dtype
    return (z - st[..., 0:1]) * st[..., 1:2]


def per_row(t, st):
    """a map out of k_kg_norm_bwd with its row's rstd divided out (see YARDSTICKS), in float64"""
    return t.double() / st[..., 1:2].double()


def row_scale(st):
    """[64, 1]: the scale row c of a weight gradient takes from its left factor, the gz of the layer with statistics st (see YARDSTICKS)"""
    return st[..., 1].double().pow(2).sum(0).sqrt().view(C, 1)


def n64(z, st):
    return (z.double() - st[..., 0:1].double()) * st[..., 1:2].double()


def d_n(z, st):
    """norm_reference's d_xhat: what the two fp32 roundings of nrm() can move n by"""
    return 4 * U * (n64(z, st).abs() + (st[..., 1:2] * st[..., 0:1]).double().abs())


# ---- float64 references, one per stage ------------------------------------------------------------------------------------------------------
def ref_z2(x, p, g):
    z1 = torch.einsum('ct,btp->bcp', p['W1'].double(), patches(x.double(), g)) + p['b1'].double().view(1, C, 1)
    return torch.einsum('dc,bcp->bdp', p['W2'].double(), z1) + p['b2'].double().view(1, C, 1)


def ref_stats(z):
    """(mean, rstd) [B, 64] in float64 and the tuple norm_reference.stats64 gives (for mean_share / rstd_limit)"""
    st = N.stats64(z.reshape(-1, z.shape[-1]))
    return st[0].view(z.shape[:2]), st[2].view(z.shape[:2]), st


def rstd_limit(z, st64):
    """see LIMITS: norm_reference's rstd limit with the second moment of the values shifted by the row's first one"""
    r = z.reshape(-1, z.shape[-1]).double()
    return 4 * U + 2.0 ** -46 * (r - r[:, 0:1]).pow(2).mean(1) / (st64[1] + EPS)


def ref_1x1(z, st, W, b):
    return torch.einsum('dc,bcp->bdp', W.double(), torch.relu(n64(z, st))) + b.double().view(1, C, 1)


def ref_y(z4, st4, W5, b5):
    return torch.einsum('c,bcp->bp', W5.double(), torch.relu(n64(z4, st4))) + b5.double()


def ref_norm_bwd(gn, z, st, rounded):
    """(gz, limit) of k_kg_norm_bwd from gn [B, 64, P] (float64, already masked); rounded: gn is a rounded fp32 product on the device"""
    n, r, d = n64(z, st), st[..., 1:2].double(), d_n(z, st)
    P = z.shape[-1]
    m1, m2 = gn.mean(-1, keepdim=True), (gn * n).mean(-1, keepdim=True)
    p = n * m2
    u1 = U if rounded else 0.0
    d_m1 = N.quad(u1 * gn, (-1,)) / P
    d_m2 = N.quad(gn * (d + u1 * n.abs()), (-1,)) / P
    return r * (gn - m1 - p), r * (4 * U * (gn.abs() + m1.abs() + p.abs()) + m2.abs() * d + d_m1 + n.abs() * d_m2)


def top_gn(dy, W5, z4, st4):
    """gn of the top layer in float64: W5[c] dy[b][p] under the fp32 mask"""
    return (W5.double().view(1, C, 1) * dy.double().unsqueeze(1)) * (n32(z4, st4) > 0)


def ref_gz4(dy, W5, z4, st4):
    return ref_norm_bwd(top_gn(dy, W5, z4, st4), z4, st4, True)


def ref_dgrad(gz, W, z, st):
    """da = (W^T gz) [n > 0], the mask of the layer below from its saved fp32 (z, st)"""
    return torch.einsum('dc,bdp->bcp', W.double(), gz.double()) * (n32(z, st) > 0)


def ref_wgrad(gz, z, st):
    """dW [64, 64], db [64] and sum|gz| [64] (the scale of db's limit)"""
    gz = gz.double()
    return torch.einsum('bdp,bcp->dc', gz, torch.relu(n64(z, st))), gz.sum((0, 2)), gz.abs().sum((0, 2))


def ref_w5(dy, z4, st4):
    """pw5 [B, 64], pb5 [B] with their limits, dW5 [64], db5 [1] with theirs"""
    dyd = dy.double().unsqueeze(1)
    n = n64(z4, st4)
    terms = dyd * torch.relu(n)
    pw5, pb5 = terms.sum(-1), dy.double().sum(-1)
    lw = 2 * U * pw5.abs() + N.quad(dyd * d_n(z4, st4) * (n > 0), (-1,)).squeeze(-1) + 2.0 ** -40 * terms.abs().sum(-1)
    lb = 2 * U * pb5.abs() + 2.0 ** -40 * dy.double().abs().sum(-1)
    dW5, db5 = pw5.sum(0), pb5.sum(0, keepdim=True)
    return (pw5, lw), (pb5, lb), (dW5, lw.sum(0) + fp32_sum_limit(dW5, pw5.abs().sum(0))), (db5, lb.sum(0, keepdim=True) + fp32_sum_limit(db5, pb5.abs().sum(0, keepdim=True)))


def fp32_sum_limit(ref, sum_abs):
    """see LIMITS, fp32 sums"""
    return 2 * U * ref.abs() + 2 * U * sum_abs


def ref_G(gz2, x, g):
    """G [64, T], s [64], sum|gz2| [64]"""
    gz2 = gz2.double()
    return torch.einsum('bcp,btp->ct', gz2, patches(x.double(), g)), gz2.sum((0, 2)), gz2.abs().sum((0, 2))


def ref_first(G, s, p):
    """dW1, db1, dW2, db2 by the formulas of kgan.hip's header, from G and s as given"""
    W1, W2, b1 = p['W1'].double(), p['W2'].double(), p['b1'].double()
    G, s = G.double(), s.double()
    return W2.t() @ G, W2.t() @ s, G @ W1.t() + torch.outer(s, b1), s


def db1_limit(s_lim, s, p):
    W2 = p['W2'].double()
    return W2.abs().t() @ s_lim + 2 * U * (W2.t() @ s.double()).abs() + C * U * (W2.abs().t() @ s.double().abs())


def ref_dx(gz2, p, g):
    """the full correlation of gz2 with W' = W2 W1 (float64): dx[q] = sum_t sum_c W'[c][t] gz2[c][q - t]"""
    wc = p['W2'].double() @ p['W1'].double()
    v = torch.einsum('ct,bcp->btp', wc, gz2.double())
    dx = torch.zeros(g.B, g.D, g.H, g.W, dtype=torch.float64, device=gz2.device)
    for i, t in enumerate(taps(g)):
        dx[:, t[0]:t[0] + g.Do, t[1]:t[1] + g.Ho, t[2]:t[2] + g.Wo] += v[:, i].view(g.B, g.Do, g.Ho, g.Wo)
    return dx


def ref_forward(x, p, g):
    """The stage references composed: every map and statistic in float64 (the statistics handed on as float64, nothing rounded)."""
    out = {'z2': ref_z2(x, p, g)}
    for k, nxt, W, b in (('2', 'z3', 'W3', 'b3'), ('3', 'z4', 'W4', 'b4'), ('4', 'y', 'W5', 'b5')):
        m, r, _ = ref_stats(out['z' + k])
        st = out['st' + k] = torch.stack([m, r], -1)
        n = torch.relu((out['z' + k] - m.unsqueeze(-1)) * r.unsqueeze(-1))
        if nxt == 'y':
            out['y'] = torch.einsum('c,bcp->bp', p[W].double(), n) + p[b].double()
        else:
            out[nxt] = torch.einsum('dc,bcp->bdp', p[W].double(), n) + p[b].double().view(1, C, 1)
    return out


def ref_backward(x, dy, saved, p, g):
    """The whole float64 backward from the saved fp32 maps and statistics (saved: dict z2, z3, z4, st2, st3, st4), every intermediate kept."""
    o = {}
    o['gz4'], o['lim4'] = ref_gz4(dy, p['W5'], saved['z4'], saved['st4'])
    o['da3'] = ref_dgrad(o['gz4'], p['W4'], saved['z3'], saved['st3'])
    o['gz3'], o['lim3'] = ref_norm_bwd(o['da3'], saved['z3'], saved['st3'], False)
    o['da2'] = ref_dgrad(o['gz3'], p['W3'], saved['z2'], saved['st2'])
    o['gz2'], o['lim2'] = ref_norm_bwd(o['da2'], saved['z2'], saved['st2'], False)
    o['dW4'], o['db4'], o['abs4'] = ref_wgrad(o['gz4'], saved['z3'], saved['st3'])
    o['dW3'], o['db3'], o['abs3'] = ref_wgrad(o['gz3'], saved['z2'], saved['st2'])
    o['G'], o['s'], o['abs2'] = ref_G(o['gz2'], x, g)
    o['dW1'], o['db1'], o['dW2'], o['db2'] = ref_first(o['G'], o['s'], p)
    o['pw5'], o['pb5'], o['dW5'], o['db5'] = ref_w5(dy, saved['z4'], saved['st4'])
    o['dx'] = ref_dx(o['gz2'], p, g)
    return o


def pack_grads(o):
    """the ten gradients of ref_backward / emu_backward in state-dict order"""
    dW5 = o['dW5'][0] if isinstance(o['dW5'], tuple) else o['dW5']
    db5 = o['db5'][0] if isinstance(o['db5'], tuple) else o['db5']
    return [o['dW1'], o['db1'], o['dW2'], o['db2'], o['dW3'], o['db3'], o['dW4'], o['db4'], dW5, db5]


GRAD_NAMES = ['dW1', 'db1', 'dW2', 'db2', 'dW3', 'db3', 'dW4', 'db4', 'dW5', 'db5']


def split_grads(dprm, nd):
    """the packed dparams of nc_kgan_bwd as the ten tensors"""
    q = unpack(dprm, nd)
    return [q[k] for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'W4', 'b4', 'W5', 'b5')]


# ---- the fp32 yardsticks: one-accumulator chains, every product and partial sum rounded (dtype = float64 turns each into the reference summed
# in that order) ---------------------------------------------------------------------------------------------------------------------------------
def chain_matmul(A, Bm, dtype=torch.float32, drop=None):
    """sum_k A[..., k] Bm[k, ...] as a chain over k: A [M, K], Bm [K, N] -> [M, N].  drop: one k left out (the deliberately wrong variant)."""
    A, Bm = A.to(dtype), Bm.to(dtype)
    acc = torch.zeros(A.shape[0], Bm.shape[1], dtype=dtype, device=A.device)
    for k in range(A.shape[1]):
        if k != drop:
            acc = acc + A[:, k:k + 1] * Bm[k:k + 1]
    return acc


def chain_collapse(p, dtype=torch.float32):
    """k_kg_collapse: W' = W2 W1 and b' = W2 b1 + b2, each a chain over the 64 channels"""
    wc = chain_matmul(p['W2'], p['W1'], dtype)
    bc = chain_matmul(p['W2'], p['b1'].view(C, 1), dtype).view(C) + p['b2'].to(dtype)
    return wc, bc


def chain_z2(x, p, g, dtype=torch.float32):
    """k_kg_conv7 in the collapsed order: W' by its chain, then one accumulator per element over the taps, the bias last"""
    wc, bc = chain_collapse(p, dtype)
    x = x.to(dtype)
    acc = torch.zeros(g.B, C, g.P, dtype=dtype, device=x.device)
    for i, t in enumerate(taps(g)):
        acc = acc + window(x, g, t).unsqueeze(1) * wc[:, i].view(1, C, 1)
    return acc + bc.view(1, C, 1)


def chain_1x1(a, W, b=None, dtype=torch.float32, drop=None, transpose=False):
    """out[d] = sum_c W[d][c] a[c] (+ b) over c in order; transpose: out[c] = sum_d W[d][c] a[d] over d (the data gradient).  a [B, 64, P]."""
    a, W = a.to(dtype), (W.t() if transpose else W).to(dtype)
    acc = torch.zeros_like(a)
    for c in range(C):
        if c != drop:
            acc = acc + a[:, c:c + 1] * W[:, c].view(1, C, 1)
    return acc if b is None else acc + b.to(dtype).view(1, C, 1)


def act32(z, st):
    """relu(IN(z)) as the kernels' prologues form it, in float32"""
    return torch.relu(n32(z, st))


def chain_y(z4, st4, W5, b5, dtype=torch.float32):
    a = act32(z4, st4).to(dtype)
    acc = torch.zeros(a.shape[0], a.shape[2], dtype=dtype, device=a.device)
    for c in range(C):
        acc = acc + a[:, c] * W5[c].to(dtype)
    return acc + b5.to(dtype)


def chain_dgrad(gz, W, z, st, dtype=torch.float32):
    return chain_1x1(gz, W, None, dtype, transpose=True) * (n32(z, st) > 0)


def rows_bp(m):
    """[B, K, P] -> [B P, K]: one row per (b, p), b outermost"""
    return m.permute(0, 2, 1).reshape(-1, m.shape[1])


def chain_outer(pairs, dtype=torch.float32):
    """For every (left [n, 64], right [n, N_k]) of pairs: sum_i left[i] right[i]^T as ONE chain over i = (b, p), all pairs in the same loop (the
    loop is what costs).  Returns a list of [64, N_k]."""
    n = pairs[0][0].shape[0]
    Nmax = max(r.shape[1] for _, r in pairs)
    dev = pairs[0][0].device
    L = torch.stack([a.to(dtype) for a, _ in pairs], 1).unsqueeze(-1).contiguous()                     # [n, K, 64, 1]
    R = torch.zeros(n, len(pairs), 1, Nmax, dtype=dtype, device=dev)
    for k, (_, r) in enumerate(pairs):
        R[:, k, 0, :r.shape[1]] = r.to(dtype)
    acc = torch.zeros(len(pairs), C, Nmax, dtype=dtype, device=dev)
    for l, r in zip(L.unbind(0), R.unbind(0)):
        acc = acc + l * r
    return [acc[k, :, :r.shape[1]] for k, (_, r) in enumerate(pairs)]


def chain_dx(gz2, wc, g, dtype=torch.float32):
    """k_kg_dx's terms as one chain per input element over (tz, c, ty, tx); gz2 [B', 64, P] (B' any multiple of the geometry's B), wc = W'."""
    gz2, wc = gz2.to(dtype), wc.to(dtype)
    Bn = gz2.shape[0]
    gv = gz2.view(Bn, C, g.Do, g.Ho, g.Wo)
    acc = torch.zeros(Bn, g.D, g.H, g.W, dtype=dtype, device=gz2.device)
    for tz in range(7 if g.nd == 3 else 1):
        for c in range(C):
            for ty in range(7):
                for tx in range(7):
                    acc[:, tz:tz + g.Do, ty:ty + g.Ho, tx:tx + g.Wo] += gv[:, c] * wc[c, tz * 49 + ty * 7 + tx]
    return acc


def chain_first(G, s, p, dtype=torch.float32):
    """k_kg_grads: dW1 = W2^T G over c2, db1 = W2^T s over c2, dW2 = G W1^T over t and then s b1^T"""
    G, s = G.to(dtype), s.to(dtype)
    dW1 = chain_matmul(p['W2'].t(), G, dtype)
    db1 = chain_matmul(p['W2'].t(), s.view(C, 1), dtype).view(C)
    dW2 = chain_matmul(G, p['W1'].t(), dtype) + s.view(C, 1) * p['b1'].to(dtype).view(1, C)
    return dW1, db1, dW2


# ---- the row kernels' arithmetic in fp32 with fp64 sums, as the kernels have it ----------------------------------------------------------------
def emu_stats(z, shift=True):
    """k_kg_stats: fp64 sums of the values shifted by the row's first one; shift = False: the deliberately wrong variant (sh = 0)"""
    r = z.double()
    sh = r[..., 0:1] if shift else torch.zeros_like(r[..., 0:1])
    d = r - sh
    P = z.shape[-1]
    m1, m2 = d.sum(-1, keepdim=True) / P, (d * d).sum(-1, keepdim=True) / P
    return torch.cat([(sh + m1).float(), (1.0 / ((m2 - m1 * m1).clamp_min(0.0) + EPS).sqrt()).float()], -1)


def emu_norm_bwd(gn, z, st):
    """k_kg_norm_bwd from gn in float32 (masked): n in fp32, the two means from fp64 sums, the result one fp64 expression rounded once"""
    n = n32(z, st)
    P = z.shape[-1]
    m1 = gn.double().sum(-1, keepdim=True) / P
    m2 = (gn.double() * n.double()).sum(-1, keepdim=True) / P
    return (st[..., 1:2].double() * (gn.double() - m1 - n.double() * m2)).float()


def emu_top_gn(dy, W5, z4, st4):
    return (W5.view(1, C, 1) * dy.unsqueeze(1)) * (n32(z4, st4) > 0)


def emu_backward(x, dy, saved, p, g, fed=None):
    """The fp32 stages composed, from the saved fp32 maps: the yardstick of everything compared with ref_backward.  fed: {'gz3': .., 'gz2': ..}
    fp32 maps (the device's own) whose dW3 / G / dx chains run in the same loops; returned under 'fed_dW3', 'fed_G', 'fed_dx'."""
    o = {}
    o['gz4'] = emu_norm_bwd(emu_top_gn(dy, p['W5'], saved['z4'], saved['st4']), saved['z4'], saved['st4'])
    o['gz3'] = emu_norm_bwd(chain_dgrad(o['gz4'], p['W4'], saved['z3'], saved['st3']), saved['z3'], saved['st3'])
    o['gz2'] = emu_norm_bwd(chain_dgrad(o['gz3'], p['W3'], saved['z2'], saved['st2']), saved['z2'], saved['st2'])
    a3, a2, pt = rows_bp(act32(saved['z3'], saved['st3'])), rows_bp(act32(saved['z2'], saved['st2'])), rows_bp(patches(x, g))
    pairs = [(rows_bp(o['gz4']), a3), (rows_bp(o['gz3']), a2), (rows_bp(o['gz2']), pt)]
    if fed is not None:
        pairs += [(rows_bp(fed['gz3']), a2), (rows_bp(fed['gz2']), pt)]
    res = chain_outer(pairs)
    o['dW4'], o['dW3'], o['G'] = res[:3]
    if fed is not None:
        o['fed_dW3'], o['fed_G'] = res[3:]
    o['s'] = o['gz2'].double().sum((0, 2)).float()
    o['dW1'], o['db1'], o['dW2'] = chain_first(o['G'], o['s'], p)
    wc = chain_collapse(p)[0]
    if fed is not None:           # both dx chains in one loop
        both = chain_dx(torch.cat([o['gz2'], fed['gz2']]), wc, g)
        o['dx'], o['fed_dx'] = both[:g.B], both[g.B:]
    else:
        o['dx'] = chain_dx(o['gz2'], wc, g)
    return o
