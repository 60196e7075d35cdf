"""CPU: the helper module of the op-level fp32 convolution tests (tests/conv_fp32_reference.py) is itself held to torch's float64 operators, its
chain oracle is a usable yardstick at every case, the restated dispatch gives every case the branch it is labelled with, and the case lists cover
a checked-in set of branches."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_fp32_reference as R  # noqa: E402

ALL = [(op, c) for op in (R.FWD, R.DGRAD, R.WGRAD) for c in R.CASES[op]]
OPS = {R.FWD: 'fwd', R.DGRAD: 'dgrad', R.WGRAD: 'wgrad'}
# every distinct (dimensions, k, stride, pad) of the lists
CONFIGS = sorted({(len(c[3]), c[4], c[5], c[6]) for _, c in ALL})
LAYERS = sorted({(op,) + c[:7] for op, c in ALL})

# The branches the lists must reach: every kernel and variant named in the header of tests/test_gpu_conv_fp32.py.  A case that is deleted, or
# that the dispatch moves elsewhere, fails test_the_lists_cover_every_branch / test_each_case_is_labelled_with_the_branch_it_reaches.
BRANCHES = {
    'fwd': {
        'G_FWD/64/one', 'G_FWD/64/split-v4', 'G_FWD/64/split-scalar', 'G_FWD/64/split-v4/padded', 'G_FWD/128/one', 'G_FWD/128/split-v4',
        'G_FWD/256/one', 'G_FWD/256/split-v4', 'k_conv_fwd<1>', 'k_conv_fwd<2>', 'k_conv_fwd<4>', 'k_conv_fwd<8>', 'flat_1x1', 'k1_fwd',
        'brick/KS3/CK1/cfg1/whole-rows/W64/few', 'brick/KS3/CK4/cfg0/whole-rows/W64/few+cut3', 'brick/KS3/CK4/cfg0/tail/W64/few+cut3',
        'brick/KS3/CK4/cfg0/whole-rows/W128/few+cut3', 'brick/KS3/CK4/cfg0/tail/W128/few+cut3', 'brick/KS3/CK4/cfg0/whole-rows/W192/few+cut3',
        'brick/KS3/CK4/cfg0/tail/W192/few+cut3', 'brick/KS3/CK4/cfg4/whole-rows/W64/whole', 'brick/KS3/CK8/cfg4/whole-rows/W64/few+cut3',
        'brick/KS3/CK8/cfg4/tail/W64/few+cut3', 'brick/KS3/CK8/cfg2/tail/W64/few+cut3', 'brick/KS3/CK8/cfg3/tail/W64/few+cut3',
        'brick/KS5/CK2/cfg0/whole-rows/W64/few+cut3', 'brick/KS5/CK4/cfg4/whole-rows/W64/few+cut3', 'brick/KS5/CK4/cfg4/tail/W64/few+cut3',
        'brick/KS5/CK4/cfg1/whole-rows/W64/cut3', 'brick/KS7/CK1/cfg1/whole-rows/W64/few', 'brick/KS7/CK1/cfg1/whole-rows/W128/few'},
    'dgrad': {
        'G_DGRAD/64/one', 'G_DGRAD/64/split-v4', 'G_DGRAD/64/split-scalar', 'G_DGRAD/64/split-v4/padded', 'G_DGRAD/128/one', 'G_DGRAD/256/one',
        'G_DGRAD_P/64/one', 'G_DGRAD_P/64/split-v4', 'G_DGRAD_P/64/split-scalar', 'G_DGRAD_P/64/one/padded', 'G_DGRAD_P/128/one',
        'G_DGRAD_P/128/split-v4', 'G_DGRAD_P/256/one', 'G_DGRAD_P/256/split-v4', 'flip G_FWD/64/one', 'flip G_FWD/64/split-v4',
        'flip G_FWD/64/split-scalar', 'flip G_FWD/128/one', 'k_conv_dgrad<1>', 'k_conv_dgrad<2>', 'k_conv_dgrad<4>', 'k_conv_dgrad<8>', 'flat_1x1',
        'to1_mfma/1', 'to1_mfma/2', 'to1_dgrad', 'brick/KS3/CK4/cfg0/tail/W64/few+cut3',
        'brick/KS3/CK4/cfg4/whole-rows/W64/whole', 'brick/KS3/CK8/cfg2/tail/W64/few+cut3', 'brick/KS3/CK8/cfg4/whole-rows/W64/few+cut3',
        'brick/KS5/CK2/cfg0/whole-rows/W64/few+cut3'},
    'wgrad': {
        'G_WGRAD/64/one', 'G_WGRAD/64/split-v4', 'G_WGRAD/64/split-scalar/padded', 'G_WGRAD/128/one', 'G_WGRAD/128/split-v4', 'G_WGRAD/256/one',
        'G_WGRAD/256/split-v4', 'k_conv_wgrad<1>', 'k_conv_wgrad<16>', 'wgrad_1x1', 'c1_wgrad/3', 'c1_wgrad/7', 'k1_wgrad/1', 'k1_wgrad/4',
        'brick/k_wgrad_dma<5,1>/blocks1', 'brick/k_wgrad_dma<3,2>/blocks2', 'brick/k_wgrad_mfma<3,1>', 'brick/k_wgrad_rows<3>/rows2'},
}


def close(a, r):
    assert a.shape == r.shape and a.dtype == torch.float64
    assert float((a - r).abs().max()) <= 1e-12 * float(r.abs().max())


def small_layer(nd, k, stride, pad):
    """A small layer of a (dimensions, k, stride, pad): odd extents that leave a remainder under the stride."""
    sp = (k + 4, k + 5, k + 7)[3 - nd:]
    return R.make_dims(2, 3, 4, sp, k, stride, pad)


@pytest.mark.parametrize('cfg', CONFIGS, ids=['%dd-k%d-s%d-p%d' % c for c in CONFIGS])
def test_reference_and_float64_chain_are_the_float64_operator(cfg):
    """Forward (with and without bias) and the three gradients of the tap loops against F.conv3d / F.conv2d + autograd in float64, to 1e-12 of
    the largest magnitude; and the chain oracle run in float64 is the same sum in another order."""
    nd, k, stride, pad = cfg
    d = small_layer(*cfg)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(d.N, d.C, d.D, d.H, d.W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(d.K, d.C, d.kd, d.kh, d.kw, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(d.K, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(d.N, d.K, d.Do, d.Ho, d.Wo, generator=g, dtype=torch.float64)

    def op(bias):
        if nd == 3:
            return F.conv3d(x, w, bias, stride=stride, padding=pad)
        return F.conv2d(x[:, :, 0], w[:, :, 0], bias, stride=stride, padding=pad).unsqueeze(2)
    y = op(b)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), dy)
    xd, wd, bd = x.detach(), w.detach(), b.detach()
    close(R.ref_fwd(xd, wd, bd, d), y.detach())
    close(R.ref_fwd(xd, wd, None, d), op(None).detach())
    close(R.ref_dgrad(dy, wd, d), dx)
    close(R.ref_wgrad(xd, dy, d), dw)
    close(R.ref_dbias(dy), db)
    close(R.chain_fwd(xd, wd, bd, d, torch.float64), y.detach())
    close(R.chain_fwd(xd, wd, None, d, torch.float64), op(None).detach())
    close(R.chain_dgrad(dy, wd, d, torch.float64), dx)
    close(R.chain_wgrad(xd, dy, d, torch.float64), dw)
    close(R.chain_dbias(dy, torch.float64), db)


def torch_fp32(op, layer):
    """torch's CPU fp32 operator and autograd at a layer: a legitimate fp32 order that is none of the kernels'."""
    d = R.make_dims(*layer)
    x, w, b, dy = R.inputs(*layer)
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    if len(layer[3]) == 3:
        y = F.conv3d(x, w, b if op == R.FWD else None, stride=layer[5], padding=layer[6])
    else:
        y = F.conv2d(x[:, :, 0], w[:, :, 0], b if op == R.FWD else None, stride=layer[5], padding=layer[6]).unsqueeze(2)
    if op == R.FWD:
        return y.detach()
    return torch.autograd.grad(y, x if op == R.DGRAD else w, dy)[0]


@pytest.mark.parametrize('layer', LAYERS, ids=[OPS[l[0]] + '-' + R.case_id(l[1:]) for l in LAYERS])
def test_chain_oracle_is_a_yardstick(layer):
    """The fp32 chain against the float64 reference: finite, an fp32 evaluation (a yardstick far off would let anything pass), within the limit
    against itself -- and not accidentally tighter than a legitimate fp32 order: torch's own CPU operator stays within FACTOR times the chain."""
    op, layer = layer[0], layer[1:]
    o = R.oracle_err(op, layer)
    t = R.err(torch_fp32(op, layer), R.reference(op, layer))
    print('%s %s: chain max %.2e rms %.2e | torch fp32 max %.2e rms %.2e' % (OPS[op], layer, o[0], o[1], t[0], t[1]))
    assert math.isfinite(o[0]) and math.isfinite(o[1]) and 0.0 < o[1] <= o[0] < 1e-4, o
    assert R.within(o, o)
    assert R.within(t, o), (t, o)
    if op == R.WGRAD:
        ob = R.oracle_err('dbias', layer)
        assert math.isfinite(ob[0]) and ob[1] <= ob[0] < 1e-4 and R.within(ob, ob), ob


@pytest.mark.parametrize('op,case', ALL, ids=[OPS[op] + '-' + R.case_id(c) for op, c in ALL])
def test_each_case_is_labelled_with_the_branch_it_reaches(op, case):
    d = R.make_dims(*case[:7])
    path, branch = R.dispatch(op, d, case[7])
    if branch == 'brick':      # the variant is the library's to say (nc_conv_mfma_plan_debug, asserted on the GPU); here: the rung and the name's form
        assert path == 1 and case[8].startswith('brick/')
    else:
        assert branch == case[8]
    assert path == (0 if case[7] == R.DIRECT else path)
    if case[7] == R.NO_SPLIT:  # NO_SPLIT only where a newer family would otherwise take the layer (or the two-term 7^3 kernels, rung 11)
        assert R.newer_family(op, d, None) or (d.C == 1 and d.kd == 7)
    if case[7] == R.NO_WS:     # only where the kernel needs no workspace: one launch of the GEMM, nothing transposed
        assert '/one' in branch and not branch.startswith('flip')


def test_the_lists_cover_every_branch():
    for op in OPS:
        assert {c[8] for c in R.CASES[op]} == BRANCHES[OPS[op]], OPS[op]
    # every op: under force-direct, at default switches where the GEMM declines, stride 1 and 2, 2-D and 3-D, K = 1 and C = 1
    for op in OPS:
        direct = [c for c in R.CASES[op] if c[8].startswith('k_conv_')]
        assert {c[7] for c in direct} == {None, R.DIRECT}
        assert {c[5] for c in direct} >= {1, 2} and {len(c[3]) for c in direct} == {2, 3}
        assert any(c[2] == 1 for c in direct) and any(c[1] == 1 for c in direct)
    # a ragged last row tile and ragged columns on every tall tile
    for op in OPS:
        for c in R.CASES[op]:
            if c[8].startswith(('G_', 'flip')) and '/64/' not in c[8]:
                mode, M, N, Rr, s, tm, n = R.gemm_plan(op, R.make_dims(*c[:7]))
                assert M % tm and N % 64, c


def test_the_undersized_workspace_cases_check_before_they_launch():
    for op, c, nbytes in R.UNDERSIZED:
        assert c in R.CASES[op] and ('/split' in c[8] and not c[8].startswith('flip') or c[8].startswith('brick/KS') or c[8] == 'flat_1x1')
        assert nbytes < 256 if c[8] == 'flat_1x1' else nbytes == 256    # launch_flat asks for 256 bytes; a split or a brick for far more


def test_plain_data_gradient_with_a_split_stays_on_64_row_tiles():
    """G_DGRAD calls pick_splits alone (conv_gemm.hip dgrad_splits): at >= 128 rows a split never leaves enough workgroups for a taller tile,
    whatever the reduction -- which is why the lists have no G_DGRAD/128/split and G_DGRAD/256/split."""
    for M in range(128, 2049):
        for cols in range(1, 257):
            s = R.pick_splits(M, cols * 64, 1 << 30)
            if s > 1:
                assert R.tile_rows(M, cols * 64, s, 1) == 64, (M, cols, s)


def test_stream_k_regimes():
    assert R.streamk_regimes(3, 1) == 'few'                      # whole tiles only
    assert R.streamk_regimes(12, 4) == 'few+cut3'                # 256 boundaries over 3 tiles
    assert R.streamk_regimes(256, 16) == 'cut3'                  # one unit per workgroup
    assert R.streamk_regimes(512, 2) == 'plain'                  # one tile per workgroup
    assert R.streamk_regimes(1224, 3) == 'whole'                 # 4.78 units per workgroup: a share [4, 9) ends tile 1, holds tile 2, starts tile 3
    assert (1224 * 1 // 256, 1224 * 2 // 256) == (4, 9)


def test_the_limit_sees_one_dropped_term_at_one_element():
    """What a subtly wrong kernel does, at the longest reduction of the small GEMM cases (1024 terms per element): one (channel, tap) term missing
    at ONE output element, and one split of the reduction added twice into the last 3 elements, both miss the limit."""
    layer = R.first_case(R.FWD, 'G_FWD/64/split-v4')[:7]
    d = R.make_dims(*layer)
    x, w, b, _ = R.inputs(*layer)
    ref, orc = R.reference(R.FWD, layer), R.oracle_err(R.FWD, layer)
    good = R.chain_fwd(x, w, b, d)
    assert R.within(R.err(good, ref), orc)
    bad = good.clone()
    od, oh, ow = d.Do - 1, d.Ho - 1, d.Wo - 1                                  # tap (1, 1, 1) under stride 2, padding 1 meets input voxel 2 o
    bad[-1, -1, od, oh, ow] -= x[-1, -1, 2 * od, 2 * oh, 2 * ow] * w[-1, -1, 1, 1, 1]
    assert (d.sd, d.pd, d.kd) == (2, 1, 4) and 2 * od < d.D and 2 * oh < d.H and 2 * ow < d.W
    assert not R.within(R.err(bad, ref), orc)
    eighth = R.ref_fwd(x[:, :2], w[:, :2], None, d).float()                    # the first of 8 splits: 2 of the 16 channels
    bad = good.clone()
    bad.view(-1)[-3:] += eighth.reshape(-1)[-3:]
    assert not R.within(R.err(bad, ref), orc)


def test_error_measure_and_limit_are_the_projects():
    import convt_reference as T
    assert (R.FACTOR, R.RMS_FLOOR, R.MAX_FLOOR) == (3.0, 2.0 ** -23, 2.0 ** -21)
    assert R.err is T.err and R.within is T.within and R.ratios is T.ratios
