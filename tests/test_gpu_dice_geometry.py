"""The index arithmetic of the dice and assemble kernels (csrc/dice.hip), bit for bit against the numpy oracle (oracle/dice.py), at the
geometries the golden volumes do not reach: a grid of step 1 (overlap = roi - 1), (L + overlap) % step == 0, an axis shorter than the roi,
overlap 1, a border of roi - 1 and one within one of the smallest padded length, three different grid counts per axis, uint8 and uint16 --
all small enough for the oracle to run in milliseconds.  Per geometry: every cube of nc_dice_cut_cube; nc_assemble_scatter_add over all cubes
in index order and nc_assemble_finalize; nc_assemble_merge on the whole padded volume; nc_assemble_finalize_slab for EVERY slab (z0, nz) and
every accumulator origin za <= z0; nc_assemble_rescale_finalize for lo >= 0 and lo < 0; an accumulator of all-ones cubes.  The entry points
are called through the C ABI directly.  Float outputs are pre-filled with NaN between NaN guard words, integer outputs with the byte 0xA5
between guards of it: an element that is not written, or one written outside the tensor, fails.  Everything is compared, nothing left out.

Values outside [0, 1] at the truncating cast are not tested: the conversion of a float outside the integer type's range is undefined in numpy
and in C++ alike.  (So the lo < 0 rescale, which maps to [-1, 1], is run on a volume whose values lie above the middle of the range.)

On an MI355X the module takes MODULE_SECONDS of wall time; every comparison is bit-exact, so there is no share of a limit to report."""
import ctypes
import math
import os
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import dice as od  # noqa: E402

DEV = 'cuda'
NC_ERR_SHAPE, NC_ERR_ARG = -1, -4
GUARD = 4
SENTINEL = 0xA5
MODULE_SECONDS = '0.8 s'
T0 = [None]

# (L0, L1, L2), roi, overlap, border, what it is there for.  Padded lengths and grid counts: test_geometries_cover_what_they_name
GEOMS = [
    ((3, 10, 6), 6, 5, 1, 'step 1; counts 9, 16, 12'),
    ((8, 8, 8), 4, 2, 2, '(L + overlap) % step == 0'),
    ((13, 4, 9), 8, 2, 3, 'an axis shorter than the roi'),
    ((5, 7, 6), 4, 1, 3, 'overlap 1, border = roi - 1'),
    ((1, 2, 3), 2, 1, 3, 'border = smallest padded length - 1; step 1; counts 3, 4, 5'),
    ((5, 11, 20), 4, 1, 2, 'counts 3, 5, 8'),
]
DTYPES = ('uint8', 'uint16')


def L():
    from neuroclear_amd._lib import lib
    return lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(code, what):
    assert code == 0, (what, code, L().nc_last_error())


@pytest.fixture(scope='module', autouse=True)
def _wall_time():
    T0[0] = time.time()
    yield
    torch.cuda.synchronize()
    print('\nmodule wall time %.1f s' % (time.time() - T0[0]))


class Out:
    """n floats between NaN guards; fill=None: NaN-filled, else holding `fill`"""

    def __init__(self, n, fill=None):
        self.whole = torch.full((n + 2 * GUARD,), math.nan, device=DEV)
        self.t = self.whole[GUARD:GUARD + n]
        if fill is not None:
            self.t.copy_(torch.as_tensor(fill).reshape(-1))

    def intact(self):
        return bool(torch.isnan(self.whole[:GUARD]).all()) and bool(torch.isnan(self.whole[GUARD + self.t.numel():]).all())

    def untouched(self):
        return bool(torch.isnan(self.whole).all())

    def bits(self):
        return self.t.cpu().numpy().view(np.int32)


class IntOut:
    """n elements of uint8 / uint16, every byte 0xA5, between 16 guard bytes of it on each side"""

    def __init__(self, n, dtype):
        self.dtype = np.dtype(dtype)
        self.nbytes = n * self.dtype.itemsize
        self.whole = torch.full((self.nbytes + 32,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.t = self.whole[16:16 + self.nbytes]

    def intact(self):
        return bool((self.whole[:16] == SENTINEL).all()) and bool((self.whole[16 + self.nbytes:] == SENTINEL).all())

    def untouched(self):
        return bool((self.whole == SENTINEL).all())

    def array(self, shape):
        return self.t.cpu().numpy().view(self.dtype).reshape(shape)


class Geom:
    def __init__(self, shape, roi, ov, border):
        self.L, self.roi, self.ov, self.border = tuple(shape), roi, ov, border
        self.step = roi - ov
        self.P = tuple(l + p for l, p in zip(shape, od.pad_amounts(shape, roi, ov)))
        self.steps = od.grid_steps(self.P, roi, ov)
        self.n = self.steps[0] * self.steps[1] * self.steps[2]
        self.E = roi + 2 * border

    def origin(self, index):
        return tuple(i * self.step for i in od.index_to_zyx(index, self.steps))


def test_geometries_cover_what_they_name():
    """the padded lengths and grid counts of the table, by hand, and the properties the cases are there for"""
    want = {(3, 10, 6): ((14, 21, 17), (9, 16, 12)), (8, 8, 8): ((14, 14, 14), (6, 6, 6)), (13, 4, 9): ((20, 14, 14), (3, 2, 2)),
            (5, 7, 6): ((10, 10, 10), (3, 3, 3)), (1, 2, 3): ((4, 5, 6), (3, 4, 5)), (5, 11, 20): ((10, 16, 25), (3, 5, 8))}
    gs = [Geom(*g[:4]) for g in GEOMS]
    for g in gs:
        assert (g.P, g.steps) == want[g.L], g.L
        assert all((n - 1) * g.step + g.roi == p for n, p in zip(g.steps, g.P))       # the last cube ends at the padded length
        assert g.border < min(g.P)
    assert any(g.step == 1 and g.ov == g.roi - 1 for g in gs)
    assert any(all((l + g.ov) % g.step == 0 for l in g.L) for g in gs)
    assert any(min(g.L) < g.roi < max(g.L) for g in gs)
    assert any(g.border == g.roi - 1 for g in gs) and any(g.border == min(g.P) - 1 for g in gs)
    assert any(g.ov == 1 for g in gs)
    assert sum(len(set(g.steps)) == 3 for g in gs) >= 2


def volume(g, dtype, seed):
    """random over the whole range of the type, the extremes at the corners"""
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max
    vol = rng.integers(0, top + 1, size=g.L, dtype=np.int64).astype(dtype)
    vol.flat[0], vol.flat[-1] = top, 0
    return vol


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(DEV) if a.dtype != np.float32 else torch.from_numpy(a).to(DEV)


def np_accumulate(g, cubes):
    """acc and cnt of util/assemble_dice.py:167-173 (the loop of oracle.dice.assemble), fp32, in index order"""
    acc, cnt = np.zeros(g.P, np.float32), np.zeros(g.P, np.float32)
    b, r = g.border, g.roi
    for i in range(g.n):
        z, y, x = g.origin(i)
        acc[z:z + r, y:y + r, x:x + r] += cubes[i][b:-b, b:-b, b:-b] / 8
        cnt[z:z + r, y:y + r, x:x + r] += 1.0
    return acc, cnt


def dev_accumulate(g, cubes):
    """nc_assemble_scatter_add over all cubes in index order into a zeroed, guarded accumulator"""
    cd = to_dev(np.ascontiguousarray(cubes, dtype=np.float32))
    E3 = g.E ** 3
    acc = Out(g.P[0] * g.P[1] * g.P[2], np.zeros(1, np.float32).repeat(g.P[0] * g.P[1] * g.P[2]))
    for i in range(g.n):
        ok(L().nc_assemble_scatter_add(P(cd.view(-1)[i * E3:]), P(acc.t), *g.P, g.roi, g.ov, g.border, i, stream()), 'nc_assemble_scatter_add')
    assert acc.intact()
    return acc


def dev_finalize(g, acc, dtype):
    out = IntOut(g.L[0] * g.L[1] * g.L[2], dtype)
    ok(L().nc_assemble_finalize(P(acc.t), P(out.t), int(dtype == 'uint16'), *g.P, *g.L, g.roi, g.ov, stream()), 'nc_assemble_finalize')
    assert out.intact()
    return out


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMS, ids=['%dx%dx%d-roi%d-ov%d-b%d' % (*g[0], g[1], g[2], g[3]) for g in GEOMS])
def test_dice_and_assemble_bit_exact(geom, dtype):
    g = Geom(*geom[:4])
    u16 = int(dtype == 'uint16')
    top = float(np.iinfo(dtype).max)
    vol = volume(g, dtype, 100 + g.n)
    E3, nP, nL = g.E ** 3, g.P[0] * g.P[1] * g.P[2], g.L[0] * g.L[1] * g.L[2]

    # ---- every cube of nc_dice_cut_cube
    refl = od.reflect_pad(od.pad_for_dicing(vol, g.roi, g.ov), g.border)
    want = np.stack([od.normalize(od.cut_cube(refl, i, g.steps, g.roi, g.ov, g.border)) for i in range(g.n)])
    assert want.shape == (g.n, g.E, g.E, g.E) and want.dtype == np.float32
    vd = to_dev(vol)
    cubes = Out(g.n * E3)
    for i in range(g.n):
        ok(L().nc_dice_cut_cube(P(vd), u16, *g.L, g.roi, g.ov, g.border, i, P(cubes.t[i * E3:]), stream()), 'nc_dice_cut_cube')
    assert cubes.intact()
    got = cubes.bits().reshape(want.shape)
    bad = np.nonzero((got != want.view(np.int32)).reshape(g.n, -1).any(1))[0]
    assert bad.size == 0, ('cubes that differ', bad[:10])

    # ---- scatter-add in index order + finalize: the diced cubes themselves, and random cubes (roundings the diced ones do not have)
    rng = np.random.default_rng(200 + g.n)
    rand = (0.99 * rng.random((g.n, g.E, g.E, g.E))).astype(np.float32)
    for name, cs in (('diced', want), ('random', rand)):
        acc = dev_accumulate(g, cs)
        acc_np, cnt = np_accumulate(g, cs)
        assert cnt.min() >= 1
        assert np.array_equal(acc.bits().reshape(g.P), acc_np.view(np.int32)), name
        out = dev_finalize(g, acc, dtype)
        full = od.assemble(list(cs), g.P, g.L, g.roi, g.ov, g.border, dtype)
        assert full.shape == g.L and full.dtype == np.dtype(dtype)
        assert np.array_equal(out.array(g.L), full), name
        # ---- merge: (acc / cnt) * 8 on the whole padded volume
        merged = Out(nP)
        ok(L().nc_assemble_merge(P(acc.t), P(merged.t), *g.L, g.roi, g.ov, stream()), 'nc_assemble_merge')
        assert merged.intact()
        assert np.array_equal(merged.bits().reshape(g.P), ((acc_np / cnt) * 8).astype(np.float32).view(np.int32)), name
    if dtype == 'uint16':     # (the diced cubes come back as the volume up to the truncation of v / 65535 * 65535)
        back = od.assemble(list(want), g.P, g.L, g.roi, g.ov, g.border, dtype)
        assert int(np.abs(back.astype(np.int64) - vol.astype(np.int64)).max()) <= 1

    # ---- finalize_slab: every slab [z0, z0 + nz) from an accumulator that starts at plane za <= z0 (`acc`, `out`: the random cubes)
    isz = np.dtype(dtype).itemsize
    plane, splane = g.L[1] * g.L[2] * isz, g.P[1] * g.P[2]
    slabs = 0
    for z0 in range(g.L[0]):
        for nz in range(1, g.L[0] - z0 + 1):
            for za in range(z0 + 1):
                so = IntOut(nz * g.L[1] * g.L[2], dtype)
                ok(L().nc_assemble_finalize_slab(P(acc.t[za * splane:]), P(so.t), u16, *g.P, *g.L, g.roi, g.ov, z0, nz, za, stream()), 'nc_assemble_finalize_slab')
                assert so.intact() and torch.equal(so.t, out.t[z0 * plane:(z0 + nz) * plane]), (z0, nz, za)
                slabs += 1
    assert slabs == sum((g.L[0] - z0) * (z0 + 1) for z0 in range(g.L[0]))

    # ---- rescale_finalize: skimage's rescale_intensity and the truncating cast; lo >= 0 maps to [0, 1], lo < 0 to [-1, 1]
    m = (0.1 + 0.8 * rng.random(g.P)).astype(np.float32)
    md = to_dev(m)
    for lo, hi in ((0.25, 0.75), (-0.75, 0.875)):     # (binary fractions: v - lo and hi - lo are exact, the clipped top maps to 1.0)
        r = od.rescale_intensity_f32(m, lo, hi)
        assert r.dtype == np.float32 and r.min() >= 0.0 and r.max() <= 1.0 and (lo >= 0) == (r.min() == 0.0)
        wantr = (r * np.float32(top)).astype(dtype)[:g.L[0], :g.L[1], :g.L[2]]
        ro = IntOut(nL, dtype)
        ok(L().nc_assemble_rescale_finalize(P(md), P(ro.t), u16, *g.L, g.roi, g.ov, np.float32(lo), np.float32(hi), np.float32(hi - lo), stream()),
           'nc_assemble_rescale_finalize')
        assert ro.intact() and np.array_equal(ro.array(g.L), wantr), (lo, hi)
        if lo < 0:     # the lower end of the output range is -1: an output range of [0, 1] would give other numbers
            other = ((np.clip(m, np.float32(lo), np.float32(hi)) - np.float32(lo)) / np.float32(hi - lo) * np.float32(top)).astype(dtype)
            assert not np.array_equal(other[:g.L[0], :g.L[1], :g.L[2]], wantr)

    # ---- an accumulator of all-ones cubes finalizes to the top of the type
    ones = dev_finalize(g, dev_accumulate(g, np.ones((g.n, g.E, g.E, g.E), np.float32)), dtype)
    assert bool((ones.array(g.L) == int(top)).all())


def test_dice_and_assemble_refuse_bad_geometry():
    g = Geom((5, 7, 6), 4, 1, 3)
    vd = to_dev(volume(g, 'uint16', 1))
    cube, acc = Out(g.E ** 3), Out(g.P[0] * g.P[1] * g.P[2])
    merged, out = Out(g.P[0] * g.P[1] * g.P[2]), IntOut(g.L[0] * g.L[1] * g.L[2], 'uint16')
    src = torch.ones(g.E ** 3, device=DEV)
    zero = torch.zeros(g.P[0] * g.P[1] * g.P[2], device=DEV)
    st = stream()
    cut = lambda roi, ov, b, i, Ls=g.L: L().nc_dice_cut_cube(P(vd), 1, *Ls, roi, ov, b, i, P(cube.t), st)  # noqa: E731
    sca = lambda roi, ov, b, i, Ps=g.P: L().nc_assemble_scatter_add(P(src), P(acc.t), *Ps, roi, ov, b, i, st)  # noqa: E731
    fin = lambda Ps, roi, ov: L().nc_assemble_finalize(P(zero), P(out.t), 1, *Ps, *g.L, roi, ov, st)  # noqa: E731
    slab = lambda Ps, roi, ov, z0, nz, za: L().nc_assemble_finalize_slab(P(zero), P(out.t), 1, *Ps, *g.L, roi, ov, z0, nz, za, st)  # noqa: E731
    mer = lambda roi, ov: L().nc_assemble_merge(P(zero), P(merged.t), *g.L, roi, ov, st)  # noqa: E731
    res = lambda roi, ov, lo, hi, rng: L().nc_assemble_rescale_finalize(P(zero), P(out.t), 1, *g.L, roi, ov, lo, hi, rng, st)  # noqa: E731
    # a border of a padded length or more (np.pad's reflect would fold twice), and none at all
    assert cut(4, 1, min(g.P), 0) == NC_ERR_SHAPE and cut(4, 1, min(g.P) + 5, 0) == NC_ERR_SHAPE and cut(4, 1, 0, 0) == NC_ERR_SHAPE
    assert cut(2, 1, 4, 0, (1, 2, 3)) == NC_ERR_SHAPE        # (padded lengths 4, 5, 6: a border of 3 is the last one accepted)
    # overlap 0 (the reference assembler adds nothing then) and overlap >= roi
    for ov in (0, 4, 5):
        assert sca(4, ov, 3, 0) == NC_ERR_SHAPE and fin(g.P, 4, ov) == NC_ERR_SHAPE and slab(g.P, 4, ov, 0, 1, 0) == NC_ERR_SHAPE
        assert mer(4, ov) == NC_ERR_SHAPE and res(4, ov, 0.2, 0.7, 0.5) == NC_ERR_SHAPE
    assert cut(4, 4, 3, 0) == NC_ERR_SHAPE and cut(4, 5, 3, 0) == NC_ERR_SHAPE
    # a cube index equal to n, and below zero
    assert cut(4, 1, 3, g.n) == NC_ERR_SHAPE and cut(4, 1, 3, -1) == NC_ERR_SHAPE
    assert sca(4, 1, 3, g.n) == NC_ERR_SHAPE and sca(4, 1, 3, -1) == NC_ERR_SHAPE
    # a padded size that is not pad_for_dicing of the original size
    for k in range(3):
        for d in (1, -1):
            Ps = tuple(p + d * (i == k) for i, p in enumerate(g.P))
            assert fin(Ps, 4, 1) == NC_ERR_SHAPE and slab(Ps, 4, 1, 0, 1, 0) == NC_ERR_SHAPE
    # a slab outside the volume, an empty one, an accumulator that starts behind it
    for z0, nz, za in ((0, g.L[0] + 1, 0), (g.L[0], 1, 0), (-1, 2, 0), (2, 0, 0), (2, 1, 3), (2, 1, -1)):
        assert slab(g.P, 4, 1, z0, nz, za) == NC_ERR_SHAPE, (z0, nz, za)
    # hi <= lo, an empty range
    assert res(4, 1, 0.5, 0.5, 0.1) == NC_ERR_SHAPE and res(4, 1, 0.7, 0.2, 0.5) == NC_ERR_SHAPE and res(4, 1, 0.2, 0.7, 0.0) == NC_ERR_SHAPE
    # null pointers
    assert L().nc_dice_cut_cube(P(None), 1, *g.L, 4, 1, 3, 0, P(cube.t), st) == NC_ERR_ARG
    assert L().nc_assemble_scatter_add(P(src), P(None), *g.P, 4, 1, 3, 0, st) == NC_ERR_ARG
    assert L().nc_assemble_finalize(P(zero), P(None), 1, *g.P, *g.L, 4, 1, st) == NC_ERR_ARG
    assert L().nc_assemble_merge(P(None), P(merged.t), *g.L, 4, 1, st) == NC_ERR_ARG
    torch.cuda.synchronize()
    assert cube.untouched() and acc.untouched() and merged.untouched() and out.untouched()
    # ... and the same calls with good arguments go through
    assert cut(4, 1, 3, g.n - 1) == 0 and fin(g.P, 4, 1) == 0 and slab(g.P, 4, 1, g.L[0] - 1, 1, g.L[0] - 1) == 0
    assert mer(4, 1) == 0 and res(4, 1, 0.2, 0.7, 0.5) == 0
    torch.cuda.synchronize()
