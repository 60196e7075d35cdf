"""The boundary kernels of csrc/dl_bnd.hip against the ones of csrc/dl_typed.hip they restate, BIT BY BIT: same products, same FMAs, same
additions in the same order per output, so every word of the result is equal (compared through uint32 views: no tolerance).  The pieces run
alone through nc_dl_bnd_piece_debug (include/nc_hip.h) from the same seeded inputs with variant 0 (dl_typed.hip), 1 (dl_bnd.hip) and -1 (what
the whole-network calls take), at dl_typed.hip's index boundaries (tests/deep_linear_reference.py TYPED_CASES A .. I) and dl_bnd.hip's own
(tests/dl_bnd_plan.py OWN_CASES; the planning itself is checked on the CPU by tests/test_dl_bnd_plan.py).

dl_bnd.hip has kernels for dL/dact0 (piece 1) and for the R set's part of the type sums (piece 2).  For the forward (0) the library's choice is
dl_typed.hip's kernels, the default-variant query answers 0 and variant 1 is refused; that is asserted here, so a piece that gains kernels has to
gain its bit comparison too.  For that piece nothing here compares kernels.

No end-to-end case forced to dl_typed.hip's kernels: the whole-network calls take no variant argument, and forcing one would need process state
(a switch), which tests/test_switches.py pins.  tests/test_gpu_deep_linear_types.py holds the whole calls to float64, type by type."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dl_bnd_plan as B  # noqa: E402
from neuroclear_amd import ops  # noqa: E402

DEV = 'cuda'
GUARD = 256          # bytes behind the scratch, which is allocated at its exact size
GUARD_BYTE = 0xA5
NC_ERR_SHAPE, NC_ERR_WS, NC_ERR_ARG = -1, -2, -4
F_SEED, A_SEED, DY_SEED, IO_SEED = 51, 52, 53, 54


def _lib():
    from neuroclear_amd._lib import lib
    return lib()


def _io_shape(piece, shape):
    N, _, D, H, W = shape
    return {0: (N, 1, D, H, W), 1: (N, 64, D, H, W), 2: (64, 32, 125)}[piece]


_IN = {}


def _inputs(shape):
    """F, act0, dy on the device, uniform in [-0.5, 0.5) from fixed seeds (as deep_linear_reference.inputs draws x and r); shared, left unchanged"""
    if shape not in _IN:
        N, _, D, H, W = shape
        def u(seed, shp):
            return torch.from_numpy(np.random.default_rng(seed).random(shp, dtype=np.float32) - np.float32(0.5)).to(DEV)
        _IN[shape] = (u(F_SEED, (27, 64, 125)), u(A_SEED, (N, 64, D, H, W)), u(DY_SEED, shape))
    return _IN[shape]


@pytest.fixture(scope='module', autouse=True)
def _leave_nothing_behind():
    yield
    _IN.clear()


def _prefill(piece, shape, nan=False):
    shp = _io_shape(piece, shape)
    if nan:
        return torch.full(shp, float('nan'), dtype=torch.float32, device=DEV)
    return torch.from_numpy(np.random.default_rng(IO_SEED).random(shp, dtype=np.float32) - np.float32(0.5)).to(DEV)


def _run(piece, shape, variant, io):
    """one call of the debug entry on a scratch of the exact size with guard bytes behind it -> rc, io's bits, the scratch's bytes"""
    L = _lib()
    N, _, D, H, W = shape
    nb = L.nc_dl_typed_scratch_bytes_debug(N, D, H, W)
    assert nb > 0
    buf = torch.full((nb + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    F, act0, dy = _inputs(shape)
    rc = L.nc_dl_bnd_piece_debug(piece, ops._ptr(F), ops._ptr(act0), ops._ptr(dy), ops._ptr(io), ops._ptr(buf), nb, N, D, H, W, variant, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.nc_last_error())
    assert bool((buf[nb:] == GUARD_BYTE).all()), 'the call wrote behind its scratch'
    return io.cpu().numpy().view(np.uint32), buf[:nb]


@pytest.mark.parametrize('case', list(B.CASES))
def test_dgrad_bits(case):
    """g, pre-filled with the same random values: dl_bnd.hip's kernels, twice, and the library's own choice give dl_typed.hip's bits in every
    word -- the voxels neither touches included"""
    shape = B.CASES[case]
    N, _, D, H, W = shape
    assert _lib().nc_dl_bnd_variant_debug(1, N, D, H, W) == 1
    fill = _prefill(1, shape)
    g0, _ = _run(1, shape, 0, fill.clone())
    g1, _ = _run(1, shape, 1, fill.clone())
    g1b, _ = _run(1, shape, 1, fill.clone())
    gd, _ = _run(1, shape, -1, fill.clone())
    f = fill.cpu().numpy().view(np.uint32)
    changed = int((g0 != f).sum())
    print('\n%s %s: %d of %d words of g changed by the boundary terms; words that differ: variant 1 %d, second call %d, default %d' %
          (case, shape, changed, g0.size, int((g1 != g0).sum()), int((g1b != g0).sum()), int((gd != g0).sum())))
    assert changed > 0
    assert np.array_equal(g1, g0)
    assert np.array_equal(g1b, g1)
    assert np.array_equal(gd, g0)
    # out of every source's reach nothing is written: rows (uz, uy) out of reach of the R set, without the four columns next to either x face
    far = np.array([[not B.in_reach(uz, uy, D, H) for uy in range(H)] for uz in range(D)])
    if far.any() and W > 8:
        assert np.array_equal(g1[:, :, far][..., 4:W - 4], f[:, :, far][..., 4:W - 4])


@pytest.mark.parametrize('case', list(B.CASES))
def test_sums_bits(case):
    """the type sums: Pq and the WHOLE scratch -- partA, partB and dHb among its regions, next to the typed kernels and the transposed copies --
    equal in every byte between dl_typed.hip's kernels, dl_bnd.hip's (twice) and the library's choice"""
    shape = B.CASES[case]
    N, _, D, H, W = shape
    assert _lib().nc_dl_bnd_variant_debug(2, N, D, H, W) == 1
    fill = _prefill(2, shape)
    p0, s0 = _run(2, shape, 0, fill.clone())
    assert not np.array_equal(p0, fill.cpu().numpy().view(np.uint32)) and bool(np.isfinite(p0.view(np.float32)).all())
    for variant in (1, 1, -1):
        p1, s1 = _run(2, shape, variant, fill.clone())
        print('%s %s variant %2d: words of Pq that differ %d, bytes of the scratch that differ %d of %d' %
              (case, shape, variant, int((p1 != p0).sum()), int((s1 != s0).sum()), s0.numel()))
        assert np.array_equal(p1, p0)
        assert torch.equal(s1, s0)


@pytest.mark.parametrize('piece', [p for p in range(3) if p not in B.NEW_PIECES])
@pytest.mark.parametrize('case', ['B', 'K'])
def test_pieces_without_new_kernels_run_the_parents(case, piece):
    """the forward has no kernels in dl_bnd.hip, so there is no bit comparison for it here: variants 0 and -1 run the SAME kernels of dl_typed.hip.
    What this checks is the debug export for that piece (the two calls agree, scratch included), that it writes every boundary voxel and no
    other (NaN pre-fill), and that variant 1 is refused before anything is written"""
    L = _lib()
    shape = B.CASES[case]
    N, _, D, H, W = shape
    assert L.nc_dl_bnd_variant_debug(piece, N, D, H, W) == 0
    fill = _prefill(piece, shape)
    a, sa = _run(piece, shape, 0, fill.clone())
    b, sb = _run(piece, shape, -1, fill.clone())
    assert np.array_equal(a, b) and torch.equal(sa, sb)
    assert not np.array_equal(a, fill.cpu().numpy().view(np.uint32))
    if piece == 0:   # every boundary voxel is written, no other: a NaN pre-fill leaves NaN exactly inside
        y, _ = _run(0, shape, -1, _prefill(0, shape, nan=True))
        nan = np.isnan(y.view(np.float32))[:, 0]
        inside = np.zeros((D, H, W), bool)
        inside[1:-1, 1:-1, 1:-1] = True
        assert (nan == inside[None]).all()
    io = fill.clone()
    F, act0, dy = _inputs(shape)
    nb = L.nc_dl_typed_scratch_bytes_debug(N, D, H, W)
    buf = torch.full((nb + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    rc = L.nc_dl_bnd_piece_debug(piece, ops._ptr(F), ops._ptr(act0), ops._ptr(dy), ops._ptr(io), ops._ptr(buf), nb, N, D, H, W, 1, ops._stream())
    torch.cuda.synchronize()
    assert rc == NC_ERR_SHAPE
    assert torch.equal(io, fill) and bool((buf == GUARD_BYTE).all())


def test_refusals_write_nothing():
    L = _lib()
    shape = B.CASES['B']
    N, _, D, H, W = shape
    F, act0, dy = _inputs(shape)
    nb = L.nc_dl_typed_scratch_bytes_debug(N, D, H, W)
    fill = _prefill(1, shape)
    io = fill.clone()
    buf = torch.full((nb + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    p = ops._ptr
    null = p(None)

    def call(piece=1, F_=p(F), a=p(act0), d=p(dy), o=p(io), sc=p(buf), n=nb, dims=(N, D, H, W), variant=1):
        return L.nc_dl_bnd_piece_debug(piece, F_, a, d, o, sc, n, *dims, variant, ops._stream())

    assert call(piece=3) == NC_ERR_ARG and call(piece=-1) == NC_ERR_ARG and call(variant=2) == NC_ERR_ARG and call(variant=-2) == NC_ERR_ARG
    assert call(F_=null) == NC_ERR_ARG and call(a=null) == NC_ERR_ARG and call(d=null) == NC_ERR_ARG and call(o=null) == NC_ERR_ARG
    assert call(sc=null) == NC_ERR_ARG
    assert call(n=nb - 1) == NC_ERR_WS and call(n=0) == NC_ERR_WS
    for dims in ((N, 7, H, W), (N, D, 7, W), (N, D, H, 18), (N, D, 196, W), (0, D, H, W)):
        assert call(dims=dims) == NC_ERR_SHAPE, dims
        assert L.nc_dl_typed_scratch_bytes_debug(*dims) == 0
        assert L.nc_dl_bnd_variant_debug(1, *dims) == NC_ERR_SHAPE
    assert L.nc_dl_bnd_variant_debug(3, N, D, H, W) == NC_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(io, fill) and bool((buf == GUARD_BYTE).all())
    # (the forward takes no dy)
    y = _prefill(0, shape)
    assert L.nc_dl_bnd_piece_debug(0, p(F), p(act0), null, p(y), p(buf), nb, N, D, H, W, 0, ops._stream()) == 0
    torch.cuda.synchronize()
