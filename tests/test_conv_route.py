"""CPU: the convolution layer dispatch (csrc/conv_route.hpp, the rung table of api.hip) through the queries a host can ask.  Every query below
is host arithmetic of the library: none of them touches the device.

1. tests/golden/conv_route_parent.npz holds what the commit BEFORE the dispatch became one table answered -- nc_conv_ws_bytes,
   nc_conv_fwd_path, nc_conv_wgrad_path, nc_conv2d_k3_active, nc_conv2d_split_active, nc_conv_lp_supported over a grid of layers under four
   switch settings (tools/gen_golden_conv_route.py lists the grid).  This tree returns the same numbers.
2. The ladder as tests/conv_fp32_reference.py restates it, until now comparable with the library only through the profiler on a GPU, against
   nc_conv_route for every case of that module.
3. Conv3d(1, 64, 7) called with a workspace that does not hold the pseudo-channel form: routed to the next rung that applies."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import conv_fp32_reference as R  # noqa: E402
import gen_golden_conv_route as G  # noqa: E402
from neuroclear_amd import _lib  # noqa: E402


@pytest.fixture(scope='module')
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_queries_answer_as_the_parent_commit_did(L):
    want = np.load(G.OUT)
    assert list(want['modes']) == G.MODES and list(want['columns']) == G.COLUMNS
    sh = want['shapes']
    assert np.array_equal(sh, G.shapes()), 'the grid of tools/gen_golden_conv_route.py and the fixture differ'
    got = G.answers(L, sh)
    bad = np.argwhere(got != want['answers'])
    assert len(bad) == 0, [(sh[i].tolist(), G.MODES[m], G.COLUMNS[c], int(want['answers'][i, m, c]), int(got[i, m, c])) for i, m, c in bad[:10]]


def _route(L, op, c, mode, ws_bytes=None):
    """nc_conv_route of a case (N, C, K, spatial, k, stride, pad) under a mode of conv_fp32_reference; ws_bytes None: what nc_conv_ws_bytes asks."""
    N, C, D, H, W, K, kd, kh, kw, s, p = G.layer(*c[:7])
    base = (L.nc_get_conv_split(), L.nc_get_conv2d_k3())
    L.nc_set_conv_split(1), L.nc_set_conv2d_k3(1)
    G.set_mode(L, {None: 0, R.NO_WS: 0, R.NO_SPLIT: 1, R.DIRECT: 2}[mode])
    try:
        if ws_bytes is None:
            ws_bytes = L.nc_conv_ws_bytes(N, C, D, H, W, K, kd, kh, kw, s, p)
        return L.nc_conv_route(op, N, C, D, H, W, K, kd, kh, kw, s, p, ws_bytes)
    finally:
        G.set_mode(L, 0, base)


@pytest.mark.parametrize('op', [R.FWD, R.DGRAD, R.WGRAD])
def test_restated_ladder_against_the_route(L, op):
    for c in R.CASES[op]:
        mode = c[7]
        got = _route(L, op, c, mode, 0 if mode == R.NO_WS else None)
        assert got >= 0 and got & 255 == R.dispatch(op, R.make_dims(*c[:7]), mode)[0], (c, got)


# Conv3d(1, 64, 7) at the smallest extent the two-term pseudo-channel kernels and, behind them, to1_mfma take (4 | W, W >= 16)
C1K7 = (1, 1, 64, (5, 6, 16), 7, 1, 3)


@pytest.mark.parametrize('op', [R.FWD, R.DGRAD])
def test_undersized_workspace_routes_past_the_pseudo_channel_kernels(L, op):
    full = L.nc_conv_ws_bytes(1, 1, 5, 6, 16, 64, 7, 7, 7, 1, 3)
    assert _route(L, op, C1K7, None, full) & 255 == 11
    lo, hi = 0, full                       # the rung's own need: the smallest workspace it is taken with
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if _route(L, op, C1K7, None, mid) & 255 == 11 else (mid, hi)
    assert hi > 256
    behind = R.dispatch(op, R.make_dims(*C1K7), R.NO_SPLIT)[0]
    assert behind == (1 if op == R.FWD else 6)
    for ws_bytes in (0, hi - 256):
        got = _route(L, op, C1K7, None, ws_bytes)
        assert got & 255 == behind and got == _route(L, op, C1K7, R.NO_SPLIT, ws_bytes), (ws_bytes, got)


def test_rungs_are_finer_than_paths_and_every_path_has_its_tag(L):
    import ctypes
    buf = ctypes.create_string_buffer(32)
    names = {p: buf.value.decode() for p in range(-1, 17) if L.nc_conv_path_name(p, buf, len(buf)) > 0}
    assert names == {0: 'direct', 1: 'mfma', 2: 'gemm', 3: 'flat', 4: 'taps', 5: 'k1', 6: 'to1', 7: 'img', 8: 'pg1', 9: 'split', 10: 'split2d',
                     11: 'split', 12: 'lk', 13: 'k3img'}
    # c1k3 and the brick kernel both report path 1, k_conv_to1 and the direct kernel both 0: the rung tells them apart
    c1k3, brick = _route(L, R.FWD, (1, 1, 64, (8, 8, 8), 3, 1, 1), None), _route(L, R.FWD, (1, 1, 64, (3, 5, 4), 3, 1, 1), None)
    assert c1k3 & 255 == brick & 255 == 1 and c1k3 >> 8 != brick >> 8
    to1, direct = _route(L, R.DGRAD, (1, 1, 8, (5, 6, 18), 7, 1, 3), R.NO_SPLIT), _route(L, R.DGRAD, (2, 3, 5, (9, 10, 11), 3, 2, 1), None)
    assert to1 & 255 == direct & 255 == 0 and to1 >> 8 != direct >> 8
    assert L.nc_conv_route(3, 1, 1, 8, 8, 8, 1, 3, 3, 3, 1, 1, 0) == -1 and L.nc_conv_route(0, 1, 1, 2, 2, 2, 1, 7, 7, 7, 1, 0, 0) == -1
