"""numpy restatement of the 2-D dice / assemble path (neuroclear_amd/csrc/dice2d.hip): the reference's dicing and assembly
(data/diceImage_dataset.py:91-120, util/assemble_dice.py:130-213) on the two in-plane axes of a stack (L0, L1, L2) of planes.
The geometry is oracle.dice.pad_amounts / grid_steps of (L1, L2), the normalisation oracle.dice.normalize;
tests/test_dice2d_reference.py anchors it bit for bit to the 3-D oracle, which is pinned to the reference's goldens.

Tile t lies in plane t // (n1 n2), at yi = (t % (n1 n2)) // n2, xi = t % n2 (x fastest)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import dice as od  # noqa: E402


def geometry(plane_shape, roi, overlap):
    """(P1, P2), (n1, n2) of one plane (L1, L2)"""
    padded = tuple(int(l) + p for l, p in zip(plane_shape, od.pad_amounts(plane_shape, roi, overlap)))
    return padded, od.grid_steps(padded, roi, overlap)


def tile_origin(t, steps, roi, overlap):
    """(plane, y0, x0) of tile t"""
    n1, n2 = steps
    r = t % (n1 * n2)
    return t // (n1 * n2), (r // n2) * (roi - overlap), (r % n2) * (roi - overlap)


def tiles2d(stack, roi, overlap, border):
    """every tile of the uint8 / uint16 stack (L0, L1, L2), in index order: float32 [L0 n1 n2, E, E]"""
    stack = np.asarray(stack)
    assert stack.ndim == 3
    (P1, P2), steps = geometry(stack.shape[1:], roi, overlap)
    E = roi + 2 * border
    out = []
    refl = [np.pad(np.pad(pl, ((0, P1 - pl.shape[0]), (0, P2 - pl.shape[1]))), ((border, border),) * 2, mode='reflect') for pl in stack]
    for t in range(stack.shape[0] * steps[0] * steps[1]):
        z, y0, x0 = tile_origin(t, steps, roi, overlap)
        out.append(od.normalize(refl[z][y0:y0 + E, x0:x0 + E]))
    out = np.stack(out)
    assert out.shape[1:] == (E, E) and out.dtype == np.float32
    return out


def assemble2d(tiles, stack_shape, roi, overlap, border):
    """acc [L0, P1, P2] float32: acc[z, y0:y0+R, x0:x0+R] += tile[b:-b, b:-b] / 8 in ascending tile index"""
    L0 = int(stack_shape[0])
    (P1, P2), steps = geometry(stack_shape[1:], roi, overlap)
    tiles = np.asarray(tiles, dtype=np.float32)
    assert tiles.shape == (L0 * steps[0] * steps[1], roi + 2 * border, roi + 2 * border)
    acc = np.zeros((L0, P1, P2), np.float32)
    for t in range(tiles.shape[0]):
        z, y0, x0 = tile_origin(t, steps, roi, overlap)
        acc[z, y0:y0 + roi, x0:x0 + roi] += tiles[t][border:-border, border:-border] / 8
    return acc


def finalize2d(acc, stack_shape, roi, overlap, data_type='uint16'):
    """T(((acc / cnt) * 8) * scale), truncating, cropped to (L0, L1, L2); cnt = the number of tiles over each pixel"""
    L0, L1, L2 = (int(s) for s in stack_shape)
    (P1, P2), steps = geometry((L1, L2), roi, overlap)
    assert acc.shape == (L0, P1, P2) and acc.dtype == np.float32
    cnt = np.zeros((P1, P2), np.float32)
    for t in range(steps[0] * steps[1]):
        _, y0, x0 = tile_origin(t, steps, roi, overlap)
        cnt[y0:y0 + roi, x0:x0 + roi] += 1.0
    v = (acc / cnt[None]) * 8
    v *= {'uint8': 255, 'uint16': 2 ** 16 - 1}[str(data_type)]
    return v.astype(data_type)[:, :L1, :L2]
