"""CPU: the numpy restatement of the 2-D dice / assemble path (tests/dice2d_reference.py) anchored, bit for bit, to the 3-D oracle
(oracle/dice.py), which is pinned to the reference's golden volumes.

For an image I, the volume V with V[z] = I for z < R + b dices into cubes whose z-layer 0 sees only copies of I (the reflect border
and the roi of that layer read the planes -b .. R + b - 1, none of them in the dicing pad): every plane of such a cube is the 2-D tile.
Plane 0 of an assembled volume is covered by the cubes of z-layer 0 only, once along z: for cubes that are constant along z it is the 2-D
assembly of their planes -- which is why the 2-D path keeps the / 8 ... * 8 of the 3-D assembler."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dice2d_reference as D2  # noqa: E402
from oracle import dice as od  # noqa: E402

# (L1, L2), roi, overlap, border, what it is there for
GEOMS = [
    ((31, 40), 12, 3, 2, '4 x 5 tiles; E = 16, which the nets accept'),
    ((5, 7), 12, 3, 2, 'both axes shorter than the roi'),
    ((10, 6), 6, 5, 1, 'step 1'),
    ((2, 3), 2, 1, 3, 'border larger than image and roi'),
    ((11, 20), 4, 1, 2, 'overlap 1'),
]
IDS = ['%dx%d-roi%d-ov%d-b%d' % (*g[0], g[1], g[2], g[3]) for g in GEOMS]
DTYPES = ('uint8', 'uint16')


def image(shape, dtype, seed):
    """random over the whole range of the type, the extremes at the corners"""
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max
    img = rng.integers(0, top + 1, size=shape, dtype=np.int64).astype(dtype)
    img.flat[0], img.flat[-1] = top, 0
    return img


def test_geometries_by_hand():
    """P = step * ((L + ov) // step) + R and n = (P - ov) // step, worked out by hand"""
    want = {(31, 40): ((39, 48), (4, 5)), (5, 7): ((12, 21), (1, 2)), (10, 6): ((21, 17), (16, 12)), (2, 3): ((5, 6), (4, 5)),
            (11, 20): ((16, 25), (5, 8))}
    for shape, roi, ov, b, _ in GEOMS:
        P, n = D2.geometry(shape, roi, ov)
        assert (P, n) == want[shape], shape
        assert all((k - 1) * (roi - ov) + roi == p for k, p in zip(n, P))     # the last tile ends at the padded length
        assert b < min(P)
    assert GEOMS[0][1] + 2 * GEOMS[0][3] == 16
    assert all(l < GEOMS[1][1] for l in GEOMS[1][0])
    assert GEOMS[2][1] - GEOMS[2][2] == 1
    assert GEOMS[3][3] >= max(GEOMS[3][0]) and GEOMS[3][3] > GEOMS[3][1]     # the border reaches across the whole image, and past the roi
    assert GEOMS[4][2] == 1


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMS, ids=IDS)
def test_tiles_are_the_planes_of_the_cubes_of_z_layer_0(geom, dtype):
    shape, roi, ov, b, _ = geom
    img = image(shape, dtype, 11 + shape[0])
    tiles = D2.tiles2d(img[None], roi, ov, b)
    vol = np.repeat(img[None], roi + b, axis=0)
    padded = od.pad_for_dicing(vol, roi, ov)
    steps = od.grid_steps(padded.shape, roi, ov)
    assert steps[1:] == D2.geometry(shape, roi, ov)[1] and tiles.shape[0] == steps[1] * steps[2]
    refl = od.reflect_pad(padded, b)
    for t in range(steps[1] * steps[2]):
        assert od.index_to_zyx(t, steps)[0] == 0
        cube = od.normalize(od.cut_cube(refl, t, steps, roi, ov, b))
        assert cube.shape == (roi + 2 * b,) * 3 and cube.dtype == np.float32
        assert np.array_equal(cube.view(np.int32), np.broadcast_to(tiles[t].view(np.int32), cube.shape)), t


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMS, ids=IDS)
def test_assembly_is_plane_0_of_the_3d_assembly(geom, dtype):
    shape, roi, ov, b, _ = geom
    E = roi + 2 * b
    (P1, P2), (n1, n2) = D2.geometry(shape, roi, ov)
    rng = np.random.default_rng(23 + shape[1])
    tiles = rng.random((n1 * n2, E, E), dtype=np.float32)
    vshape = (1,) + tuple(shape)
    padded = tuple(l + p for l, p in zip(vshape, od.pad_amounts(vshape, roi, ov)))
    steps = od.grid_steps(padded, roi, ov)
    assert steps[1:] == (n1, n2) and padded[1:] == (P1, P2)
    # z-layer 0: the tiles, constant along z; the layers above it (which do not reach plane 0): anything
    cubes = [np.broadcast_to(tiles[i], (E, E, E)) if i < n1 * n2 else rng.random((E, E, E), dtype=np.float32)
             for i in range(steps[0] * n1 * n2)]
    want = od.assemble(cubes, padded, vshape, roi, ov, b, dtype)
    acc = D2.assemble2d(tiles, vshape, roi, ov, b)
    got = D2.finalize2d(acc, vshape, roi, ov, dtype)
    assert got.shape == want.shape == vshape and got.dtype == want.dtype == np.dtype(dtype)
    assert np.array_equal(got, want)
    assert got.max() > got.min()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMS, ids=IDS)
def test_round_trip_within_one_lsb(geom, dtype):
    """dice -> assemble gives the input back up to the truncation of (v / top) * top"""
    shape, roi, ov, b, _ = geom
    stack = image((2,) + tuple(shape), dtype, 31 + shape[0])
    back = D2.finalize2d(D2.assemble2d(D2.tiles2d(stack, roi, ov, b), stack.shape, roi, ov, b), stack.shape, roi, ov, dtype)
    d = int(np.abs(back.astype(np.int64) - stack.astype(np.int64)).max())
    print('%s %s: round trip max |diff| %d' % (shape, dtype, d))
    assert d <= 1


@pytest.mark.parametrize('geom', GEOMS, ids=IDS)
def test_planes_of_a_stack_are_independent(geom):
    shape, roi, ov, b, _ = geom
    E = roi + 2 * b
    stack = image((3,) + tuple(shape), 'uint16', 41 + shape[1])
    tiles = D2.tiles2d(stack, roi, ov, b)
    per = tiles.shape[0] // 3
    rng = np.random.default_rng(43)
    rand = rng.random((3 * per, E, E), dtype=np.float32)
    out = D2.finalize2d(D2.assemble2d(rand, stack.shape, roi, ov, b), stack.shape, roi, ov, 'uint16')
    for z in range(3):
        assert np.array_equal(tiles[z * per:(z + 1) * per].view(np.int32), D2.tiles2d(stack[z:z + 1], roi, ov, b).view(np.int32))
        one = (1,) + tuple(shape)
        assert np.array_equal(out[z:z + 1], D2.finalize2d(D2.assemble2d(rand[z * per:(z + 1) * per], one, roi, ov, b), one, roi, ov, 'uint16'))
