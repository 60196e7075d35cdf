"""CPU: the cases, masks and yardstick of the type-by-type tests of deep_linear_gen's position-typed path (tests/deep_linear_reference.py) are
themselves checked -- the types partition the volume, every case has the property it is there for (computed from the constants of
csrc/dl_typed.hip, which are compared with the source text), and the limits of tests/test_gpu_deep_linear_types.py tell the right evaluation
from the one that leaves the faces uncorrected by at least 100 x in every boundary type."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deep_linear_reference as R  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'neuroclear_amd', 'csrc')


@pytest.fixture(scope='module', autouse=True)
def _leave_nothing_behind():
    yield
    R.clear()


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_restated_constants_are_the_sources():
    """the numbers the case properties are computed from, where dl_typed.hip and conv_c1.hip spell them"""
    s = _src('dl_typed.hip')
    assert 'constexpr int kSeg = %d;' % R.K_SEG in s                                          # :128
    assert 'constexpr int kPitch = %d;' % R.K_PITCH in s                                      # :346
    assert 'const int ux = blockIdx.y * %d + lane;' % R.LANES in s                            # :244  k_dl_bnd_dgrad<false>
    assert 'const int uy = seg * %d + lane;' % R.LANES in s                                   # :275  k_dl_bnd_dgrad<true>
    assert 'const int nseg = (int)cdiv(H, %d);' % R.LANES in s                                # :506
    assert s.count('for (int y = threadIdx.x; y < H; y += %d)' % R.Y_LOOP) == 2               # :96, :103  k_dl_gather_x
    assert 'dim3(%d), 0, s, act0, AX' % R.Y_LOOP in s                                         # :491, :504 its launches
    assert 'const size_t lds = (size_t)(64 * kPitch + %d) * 4;' % R.EXT_MAX in s              # :517  dyr[192]
    assert ('return N >= 1 && D >= {0} && H >= {0} && W >= {0} && H <= {1} && W <= {1} && W % 4 == 0;'.format(R.EXT_MIN, R.EXT_MAX)) in s   # :474
    assert re.search(r'__host__ __device__ inline int axis_type\(int coord, int L\) \{ return coord == 0 \? 0 : coord == L - 1 \? 2 : 1; \}', s)  # :27
    c = _src('conv_c1.hip')
    assert 'if (d.W % 4 || d.W < 16) return false;' in c                                      # :585
    assert 'static constexpr int kC1wMaxPD = 6;' in c                                         # :579 (8 * 6 = 48 pieces)
    assert 'return lds_bytes <= 160 * 1024 && p.SD / 256 <= 8 * kC1wMaxPD && 8 * p.PRx / 256 <= 8;' in c   # :597
    assert [w for w in range(4, 260, 4) if R.c1_wgrad_admits(w)] == list(range(R.C1W_W_MIN, R.C1W_W_MAX + 1, 4))
    g = _src('gen_nets.hip')
    assert 'constexpr unsigned kKeptTyped = 1u << 29;' in g and 'constexpr unsigned kKeptNoAct1 = 1u << 30;' in g   # :685-686
    assert 'constexpr unsigned kKeptCollapsed = 1u << 31;' in g                                                      # :684


@pytest.mark.parametrize('dims', sorted({c[0][2:] for c in R.ALL_CASES.values()}))
def test_types_partition_the_volume(dims):
    D, H, W = dims
    t = R.position_types(D, H, W)
    assert t.shape == (D, H, W) and t.min() >= 0 and t.max() <= 26
    masks = R.one_type_masks(D, H, W)
    assert sum(m.astype(np.int64) for m in masks.values()).min() == 1 == sum(m.astype(np.int64) for m in masks.values()).max()
    for tau, m in masks.items():
        assert int(m.sum()) == R.type_count(tau, D, H, W), tau
    assert sum(R.type_count(tau, D, H, W) for tau in range(27)) == D * H * W
    # the numbering: low corner 0, high corner 26, x fastest
    assert t[0, 0, 0] == 0 and t[-1, -1, -1] == 26 and t[0, 0, 1] == 1 and t[0, 1, 0] == 3 and t[1, 0, 0] == 9 and t[1, 1, 1] == R.INTERIOR
    g = R.group_masks(D, H, W)
    assert (g['R'].astype(int) + g['X'].astype(int) + g['interior'].astype(int) == 1).all()
    assert not g['R'][:, :, 0].any() and not g['R'][:, :, -1].any() and g['X'][:, :, 0].all() and g['X'][:, :, -1].all()
    assert int(g['R'].sum()) == (2 * H + 2 * (D - 2)) * (W - 2)   # n_bnd_rows (dl_typed.hip:115) rows without their two end voxels
    assert int(g['X'].sum()) == 2 * D * H


def test_cases_cover_what_they_name():
    T = {k: v[0] for k, v in R.TYPED_CASES.items()}
    for k, (N, _, D, H, W) in T.items():
        assert R.typed_expected(N, D, H, W), k
    N, _, D, H, W = T['A']
    assert D == H == R.EXT_MIN and W == R.C1W_W_MIN     # every voxel within three of both faces on z and y: both faces' windows overlap everywhere
    assert all(min(c, L - 1 - c) <= 3 for L in (D, H) for c in range(L))
    N, _, D, H, W = T['B']
    assert N == 2 and len({D, H, W}) == 3
    N, _, D, H, W = T['C']
    assert N == 3 and H % 2 == 1
    N, _, D, H, W = T['D']
    assert H - 2 == R.K_SEG and W - 2 == R.K_SEG and R.cdiv(H - 2, R.K_SEG) == 1 == R.cdiv(W - 2, R.K_SEG)
    N, _, D, H, W = T['E']
    assert R.cdiv(H - 2, R.K_SEG) == 2 and (H - 2) - R.K_SEG == 1           # the second y segment owns one voxel
    assert R.cdiv(W - 2, R.K_SEG) == 2 and W == R.LANES and R.cdiv(W, R.LANES) == 1
    N, _, D, H, W = T['F']
    assert R.cdiv(H, R.LANES) == 2 and H - R.LANES == 1                      # nseg = 2, one live lane in the second
    assert R.cdiv(W, R.LANES) == 2 and W - R.LANES == 4
    N, _, D, H, W = T['G']
    assert R.cdiv(H, R.Y_LOOP) == 2 and R.cdiv(H, R.LANES) == 3
    N, _, D, H, W = T['H']
    assert H == R.EXT_MAX == R.K_PITCH - 1 and not R.dl_typed_supported(N, D, H + 1, W)
    N, _, D, H, W = T['I']
    assert W == R.C1W_W_MAX and not R.typed_expected(N, D, H, W + 4) and R.dl_typed_supported(N, D, H, W + 4)
    # extents met by no earlier test: the minimum on every axis somewhere, an extent above 128 on H and on W
    assert any(c[2] == 8 for c in T.values()) and any(c[3] == 8 for c in T.values()) and any(c[3] > 128 for c in T.values()) and any(c[4] > 128 for c in T.values())
    F = R.FALLBACK_CASES
    assert min(F['below8'][0][2:]) < R.EXT_MIN
    assert F['w_mod4'][0][4] % 4 != 0 and F['w_mod4'][0] == (2, 1, 9, 14, 21)
    assert F['w196'][0][4] > R.EXT_MAX and min(F['w196'][0][2:]) >= R.EXT_MIN and F['w196'][0][4] % 4 == 0
    assert F['B_terms3'][0] == T['B'] and F['B_terms3'][1] == 3
    for k in ('below8', 'w_mod4', 'w196'):
        assert not R.dl_typed_supported(F[k][0][0], *F[k][0][2:]), k
    for k in ('w8', 'w12', 'w192'):    # the shapes the issue's table named and k_wgrad_c1 refuses
        assert R.dl_typed_supported(F[k][0][0], *F[k][0][2:]) and not R.c1_wgrad_admits(F[k][0][4]), k
    assert F['w8'][0] == (1, 1, 8, 8, 8) and F['w12'][0] == (3, 1, 8, 9, 12) and F['w192'][0] == (1, 1, 8, 8, 192)
    assert all(v[1] == 2 for k, v in F.items() if k != 'B_terms3')


def test_uncorrected_chain_is_the_interior_kernel():
    """run_uncorrected equals the oracle wherever the 3^3 layer reads no padding (type 13), and nowhere else"""
    shape = (1, 1, 8, 9, 16)
    x, r = R.inputs(shape)
    y64 = R.run_oracle(R.weights(), x, r, torch.float64)[0]
    yu = R.run_uncorrected(R.weights(), x, r)[0]
    assert yu.shape == y64.shape
    e = R.per_type_error(yu, y64, R.position_types(*shape[2:]))
    assert e[R.INTERIOR] <= 1e-12 and all(e[t] > 1e-3 for t in range(27) if t != R.INTERIOR)


@pytest.mark.parametrize('case', ['A', 'B'])
def test_the_yardstick_discriminates(case):
    """What the limits of tests/test_gpu_deep_linear_types.py must tell apart, from the inputs alone: the fp32 oracle's worst type leaves the
    forward limit (3 Y + f, capped at FWD_CAP of the scale) room, the uncorrected evaluation misses even the cap by 100 x in every one of the 26
    boundary types and is exact inside; with dy on one boundary type it misses the gradient limit by 100 x in dx and in each weight tensor."""
    shape = R.TYPED_CASES[case][0]
    types = R.position_types(*shape[2:])
    (y64, dx64, g64), (y32, dx32, g32) = R.oracle(shape)
    sdu, xu = R.leaves(R.weights(), R.inputs(shape)[0], torch.float64)
    yu_graph = R.uncorrected_forward(sdu, xu)   # (one forward, a backward per mask)
    yu = yu_graph.detach()
    Y = R.per_type_error(y32, y64, types)
    U = R.per_type_error(yu, y64, types)
    print('case %s fp32 oracle worst type %.2e; uncorrected: least wrong boundary type %.2e, interior %.2e' % (case, Y.max(), np.delete(U, R.INTERIOR).min(), U[R.INTERIOR]))
    assert R.FACTOR * Y.max() <= R.FWD_CAP / 2
    assert U[R.INTERIOR] <= 1e-12
    for tau in range(27):
        if tau != R.INTERIOR:
            assert U[tau] >= 100 * R.FWD_CAP, (tau, U[tau])
    least = {}
    for tau in range(27):
        if tau == R.INTERIOR:
            continue
        (_, dx64, g64), (_, dx32, g32) = R.oracle(shape, tau)
        dxu, gu = R.grads(yu_graph, xu, sdu, R.inputs(shape, tau)[1])
        for k, a, o, ref in [('dx', dxu, dx32, dx64)] + [(k, gu[k], g32[k], g64[k]) for k in g64]:
            lim = R.FACTOR * R.rel(o, ref) + R.GRAD_FLOOR
            ratio = R.rel(a, ref) / lim
            least[k] = min(least.get(k, 1e30), ratio)
            assert ratio >= 100, (tau, k, R.rel(a, ref), R.rel(o, ref))
    print('case %s one-type masks: least ratio of the uncorrected error to the limit %s' % (case, {k: '%.0f' % v for k, v in least.items()}))
