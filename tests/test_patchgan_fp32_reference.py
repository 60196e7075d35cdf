"""CPU: the helper module of the op-level tests of the PatchGAN 4 x 4 kernels (tests/patchgan_fp32_reference.py).  The restated planners give
every case the branch and the switches it is labelled with, the lists cover a counted set of branches and edges, every minimal k_sconv case stops
being one with an image fewer, and the float64 reference is torch's float64 operator on the 4 x 4 layers."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_fp32_reference as R  # noqa: E402
import patchgan_fp32_reference as PG  # noqa: E402
import test_conv_fp32_reference as TC  # noqa: E402

OPS = {R.FWD: 'fwd', R.DGRAD: 'dgrad', R.WGRAD: 'wgrad'}
ALL = [(op, c) for op in OPS for c in PG.CASES[op]] + PG.K65
SCONV = [(op, c) for op in (R.FWD, R.DGRAD) for c in PG.CASES[op] if c[8].startswith('sconv')]
SWGRAD = [c for c in PG.WGRAD_CASES if c[8].startswith('swgrad')]
PG1 = {op: [c for c in PG.CASES[op] if c[8].startswith('pg1')] for op in OPS}
IMG4 = 'sconv fwd/s2/CK4/cfg(8,1,1)/img4'     # the one k_sconv case that is minimal for its branch, not for rung 7


def dims(c):
    return R.make_dims(*c[:7])


def test_error_measure_limit_and_reference_are_the_projects():
    import convt_reference as T
    assert (PG.FACTOR, PG.RMS_FLOOR, PG.MAX_FLOOR) == (3.0, 2.0 ** -23, 2.0 ** -21)
    assert PG.err is T.err and PG.within is T.within and PG.ratios is T.ratios
    assert PG.inputs is R.inputs and PG.reference is R.reference and PG.oracle_err is R.oracle_err and PG.make_dims is R.make_dims


@pytest.mark.parametrize('op,case', ALL, ids=[OPS[op] + '-' + R.case_id(c) for op, c in ALL])
def test_each_case_is_labelled_with_the_branch_and_the_switches_it_reaches(op, case):
    d = dims(case)
    assert case[4:7] == (4, case[5], 1) and len(case[3]) == 2
    rung, branch = PG.dispatch(op, d)
    assert branch == case[8]
    assert rung == (8 if branch.startswith('pg1') else 7 if branch.startswith(('sconv', 'swgrad')) else 2)
    assert rung != 2 or (op, case) in PG.K65 or case in PG.THIN_PLANES
    assert case[7] == PG.mode_of(op, case[:7])
    if case[7] is None:      # default switches: certain that no rung in front of 8 and 7 takes it
        assert not PG.p2d_may_take(op, d)
    # the sibling file's necessary conditions name these layers as another file's -- this one
    assert R.newer_family(op, d, case[7]) or rung == 2 and d.C == 1 and d.K == 65


def test_the_forward_lists_cover_the_enumeration():
    f = [(c, dims(c), PG.sconv_facts(R.FWD, dims(c))) for op, c in SCONV if op == R.FWD]
    assert {d.sh for _, d, _ in f} == {1, 2}
    assert {x['plan']['CK'] for _, _, x in f} == {2, 4, 8, 16}                 # 32: test_no_forward_plan_has_32_channels_per_chunk
    assert {d.K for _, d, _ in f} == {64, 128}
    assert {x['images'] for _, _, x in f} == {2, 3, 4}
    assert all(x['ragged'] for _, _, x in f)                                   # a last tile of fewer than NCT columns, everywhere
    assert sum(d.H % 2 == 1 and d.W % 2 == 1 and d.H != d.W for _, d, _ in f) >= 4
    assert sum(x['wide'] for _, _, x in f) >= 1 and sum(not x['wide'] for _, _, x in f) >= 1
    assert sum(c[7] is None for c, _, _ in f) >= 1 and sum(c[7] == R.NO_SPLIT for c, _, _ in f) >= 1
    # four images need planes of 96 .. 127 pixels under a 256-column tile
    c4 = PG.first_case(R.FWD, IMG4)
    d4 = dims(c4)
    assert 96 <= d4.Ho * d4.Wo <= 127 and PG.sconv_facts(R.FWD, d4)['plan']['NCT'] == 256
    g = [c for c in PG.FWD_CASES if c[8].startswith('pg1')]
    assert len(g) >= 4 and {dims(c).K for c in g} >= {64, 20, 7}
    assert any(c[3][0] == 2 for c in g) and any(c[3][1] == 2 for c in g)
    assert any(dims(c).N * dims(c).Ho * dims(c).Wo > 512 and dims(c).N * dims(c).Ho * dims(c).Wo % 256 for c in g)   # several blocks, the last ragged


def test_the_data_gradient_lists_cover_the_enumeration():
    f = [(c, dims(c), PG.sconv_facts(R.DGRAD, dims(c))) for op, c in SCONV if op == R.DGRAD]
    s1 = [x for x in f if x[1].sh == 1]
    s2 = [x for x in f if x[1].sh == 2]
    assert len(s1) >= 2 and {d.C for _, d, _ in s1} == {64, 128}
    assert {(d.H % 2, d.W % 2) for _, d, _ in s2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for _, d, x in s2:          # classes of different sizes exactly where an extent is odd; then blocks of the smaller ones leave early
        assert (len(set(PG.sconv_classes(R.DGRAD, d))) > 1) == bool(d.H % 2 or d.W % 2)
    assert sum(x['early_exit'] for _, _, x in s2) >= 3
    for group in (s1, s2):
        cks = {x['plan']['CK'] for _, _, x in group}
        assert 2 in cks and max(cks) >= 16
    assert 32 in {x['plan']['CK'] for _, _, x in s2}
    assert {d.C for _, d, _ in s2} == {64, 128}
    assert {x['images'] for _, _, x in f} >= {2, 3} and all(x['ragged'] for _, _, x in f)
    g = PG1[R.DGRAD]
    few = [c for c in g if PG.pg1_dgrad_few(dims(c))]
    big = [c for c in g if not PG.pg1_dgrad_few(dims(c))]

    def blocks(c):
        return c[0] * R.cdiv(c[3][0], 2) * R.cdiv(c[3][1], 2)
    assert max(blocks(c) for c in few) == 128 * 256 - 1 and min(blocks(c) for c in big) == 128 * 256
    for group in (few, big):
        assert {c[3][0] % 2 for c in group} == {0, 1} and {c[3][1] % 2 for c in group} == {0, 1}
    assert {c[2] % 8 != 0 for c in few} == {True, False} and any(c[2] == 20 for c in few) and any(c[2] < 8 for c in few)
    assert any(c[2] == 64 for c in g) and any(c[3][0] == 2 for c in g) and any(c[3][1] == 2 for c in g)


def test_the_weight_gradient_lists_cover_the_enumeration():
    f = [(c, dims(c), PG.plan_swgrad(dims(c)), PG.swgrad_facts(dims(c))) for c in SWGRAD]
    assert {w['NTW'] for _, _, w, _ in f} == {4, 2}
    assert {d.C for _, d, w, _ in f if w['NTW'] == 2} >= {8, 24} and all(d.C % 16 == 0 for _, d, w, _ in f if w['NTW'] == 4)
    for ntw in (4, 2):
        assert {d.sh for _, d, w, _ in f if w['NTW'] == ntw} == {1, 2}
    assert {d.K for _, d, _, _ in f} == {128, 256}
    for edge in ('ragged', 'short', '2img', 'wide', 'xcd'):
        assert sum(edge in e for _, _, _, e in f) >= 1, edge
    for edge in ('ragged', 'xcd', 'wide', 'short'):
        assert sum(edge not in e for _, _, _, e in f) >= 1, edge
    assert {d.sh for _, d, _, e in f if 'wide' in e} == {1, 2}
    assert all(w['splits'] > 1 for _, _, w, _ in f)         # splits == 1 needs C / NCW * K / 128 >= 512: the module says so instead of faking it
    assert PG.plan_swgrad(R.make_dims(10, 4096, 256, (21, 23), 4, 1, 1))['splits'] == 1     # 256 x 2 workgroups: 1 M weights, 270 MB of x
    # a stride-2 weight gradient under the default switches
    assert any(c[5] == 2 and c[7] is None for c, _, _, _ in f) and any(c[7] == R.NO_SPLIT for c, _, _, _ in f)
    # the thin planes are in the list, whatever takes them
    assert {c[:7] for c in PG.THIN_PLANES} == {(32, 8, 128, (130, 4), 4, 2, 1), (32, 8, 128, (130, 5), 4, 2, 1), (64, 8, 128, (65, 2), 4, 1, 1)}
    g = PG1[R.WGRAD]
    npix = {c: c[0] * dims(c).Ho * dims(c).Wo for c in g}
    assert any(n % 128 for n in npix.values()) and any(n % 128 == 0 for n in npix.values())
    assert any(PG.pg1_tiles(dims(c)) > 512 and PG.pg1_blocks(dims(c)) == 512 for c in g)
    assert any(1 < PG.pg1_tiles(dims(c)) < 512 and PG.pg1_blocks(dims(c)) == PG.pg1_tiles(dims(c)) for c in g)
    ks = {c[2] for c in g}
    assert 64 in ks and any(k < 64 and k % 8 == 0 for k in ks) and any(k % 8 and k % 2 == 0 for k in ks) and any(k % 2 for k in ks)
    assert any(c[3][0] == 2 for c in g) and any(c[3][1] == 2 for c in g)


@pytest.mark.parametrize('op,case', SCONV, ids=[OPS[op] + '-' + R.case_id(c) for op, c in SCONV])
def test_one_image_fewer_falls_below_min_tiles(op, case):
    less = R.make_dims(case[0] - 1, *case[1:7])
    if case[8] == IMG4:      # stays on rung 7 under a smaller tile: minimal for the 256-column tile and its four images
        assert PG.sconv_supported(op, less) is not None and PG.sconv_branch(op, less) != case[8]
        return
    pl = PG.plan_sconv(*PG.sconv_problem(op, less))
    assert pl is not None and pl['tiles'] < PG.MIN_TILES and PG.sconv_supported(op, less) is None
    assert PG.sconv_supported(op, dims(case))['tiles'] >= PG.MIN_TILES


def test_no_forward_plan_has_32_channels_per_chunk():
    """Two buffers of 32 channel images fit the 80 KiB only with CS <= 256 floats.  A forward tile stages 4 rows per image and at least
    NCT / Wo - 1 more: enumerated over every output width (Wp > 256 from Wo = 253 on) at the plane height that needs the fewest images per
    tile, both strides, every configuration."""
    for s in (1, 2):
        for Wo in range(1, 257):
            Ho = R.cdiv(512, Wo)
            for g in PG.SCFGS:
                pl = PG.plan_one(g, 1000, 32, 128, Ho, Wo, s, 4, (Wo - 1) * s + 4)
                assert pl is None or pl['CK'] < 32, (s, Wo, g)
    # ... while a class of the stride-2 data gradient stages 2 rows per image
    assert PG.plan_one((2, 1, 2), 39, 32, 64, 12, 13, 1, 2, 14, 4)['CK'] == 32


def test_configuration_tune_and_refusal_cases():
    for op, c in PG.CFG_CASES:
        assert c in PG.CASES[op] and PG.applicable_cfgs(op, dims(c)) == list(range(14))
    assert {op for op, _ in PG.CFG_CASES} == {R.FWD, R.DGRAD} and PG.CFG_CASES[0][1][2] == 128
    assert PG.CFG_CASES[1][1][1] == 128 and PG.CFG_CASES[1][1][5] == 2
    # pinned, the forward layer's 256-column tiles touch other image counts than the heuristic's tile
    d = dims(PG.CFG_CASES[0][1])
    assert len({PG.sconv_facts(R.FWD, d, g)['images'] for g in PG.SCFGS}) >= 2
    op, c = PG.TUNED_CASE
    assert c in PG.CASES[op] and len(PG.applicable_cfgs(op, dims(c))) == 14
    # K = 64 admits only the WN = 1 configurations
    assert PG.applicable_cfgs(R.FWD, dims(PG.FWD_CASES[0])) == [i for i, g in enumerate(PG.SCFGS) if g[1] == 1]
    for op, c, nbytes in PG.UNDERSIZED:
        assert c in PG.CASES[op] and nbytes == 256
    assert {PG.dispatch(op, dims(c))[0] for op, c, _ in PG.UNDERSIZED} == {7, 8}
    for N, C, K, H, W, s in PG.REFUSED:
        assert min(H, W) + 2 < 4
    assert {(C == 1, H == 1) for N, C, K, H, W, s in PG.REFUSED} == {(True, True), (True, False), (False, True), (False, False)}


def test_the_restated_planners_at_known_points():
    # plan_swgrad at the thin plane of the issue: 62 720 B of LDS with NTW = 2 -- and 74 rows for a stage, more than the 64 lanes that decode them
    d = R.make_dims(32, 8, 128, (130, 4), 4, 2, 1)
    w = PG.plan_swgrad(d, row_limit=None)
    assert (w['NTW'], w['lds'], w['pitch']) == (2, 62720, 12) and PG.swgrad_rows(d) == 74
    assert [PG.swgrad_rows(dims(c)) for c in PG.THIN_PLANES] == [74, 74, 73]
    for c in PG.THIN_PLANES:        # accepted in every other respect (mincol, LDS), refused for their rows alone: the gather GEMM, rung 2
        assert PG.plan_swgrad(dims(c), row_limit=None) is not None and c[0] * dims(c).Ho * dims(c).Wo >= PG.MINCOL
        assert PG.plan_swgrad(dims(c)) is None and not PG.sconv_wgrad_supported(dims(c)) and PG.dispatch(R.WGRAD, dims(c))[0] == 2
    # the limit cuts nothing else: from an output width of 3 on a stage has at most 54 rows
    assert max(PG.swgrad_rows(R.make_dims(1, 8, 128, (200, W), 4, s, 1)) for s in (1, 2) for W in range(2 + 2 * s, 200)) == 54
    assert all(PG.swgrad_rows(dims(c)) <= 64 for c in SWGRAD)
    # Athena's layers (tests/test_gpu_ops.py): 216 planes of 54^2 x 64 -> 128 under stride 2
    d = R.make_dims(216, 64, 128, (54, 54), 4, 2, 1)
    assert PG.sconv_fwd_supported(d) and PG.sconv_dgrad_supported(d) and PG.sconv_wgrad_supported(d)
    assert not PG.sconv_fwd_supported(R.make_dims(2, 64, 128, (54, 54), 4, 2, 1))       # Apollo's few planes: the gather GEMM
    assert not PG.sconv_fwd_supported(R.make_dims(600, 64, 128, (18, 18), 4, 2, 1))     # planes of 81 pixels
    assert not PG.sconv_wgrad_supported(R.make_dims(63, 8, 128, (65, 2), 4, 1, 1))      # 4032 columns < mincol
    # patchgan_edge.hip
    assert PG.pg1_supported(R.make_dims(3, 1, 64, (9, 11), 4, 2, 1)) and not PG.pg1_supported(R.make_dims(3, 1, 65, (9, 11), 4, 2, 1))
    assert not PG.pg1_supported(R.make_dims(3, 1, 64, (9, 11), 4, 1, 1)) and not PG.pg1_supported(R.make_dims(3, 2, 64, (9, 11), 4, 2, 1))
    assert PG.pg1_blocks(R.make_dims(216, 1, 64, (108, 108), 4, 2, 1)) == 512 and PG.pg1_blocks(R.make_dims(1, 1, 64, (108, 108), 4, 2, 1)) == 23
    assert PG.pg1_dgrad_few(R.make_dims(4, 1, 64, (108, 108), 4, 2, 1)) and not PG.pg1_dgrad_few(R.make_dims(216, 1, 64, (108, 108), 4, 2, 1))


def test_the_float64_reference_is_the_float64_operator_on_the_4x4_layers():
    """tests/test_conv_fp32_reference.py already holds the tap loops and the float64 chain to F.conv2d + autograd at the two 2-D 4 x 4
    configurations (stride 2 and stride 1, padding 1); run here again, and at the smallest legal plane of the first layer (H = 2: one output
    row, C = 1), which its small layer does not reach."""
    for cfg in ((2, 4, 2, 1), (2, 4, 1, 1)):
        assert cfg in TC.CONFIGS
        TC.test_reference_and_float64_chain_are_the_float64_operator(cfg)
    layer = (3, 1, 7, (2, 9), 4, 2, 1)
    d = R.make_dims(*layer)
    x, w, b, dy = (t.double() for t in R.inputs(*layer))
    x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    y = F.conv2d(x[:, :, 0], w[:, :, 0], b, stride=2, padding=1).unsqueeze(2)
    assert y.shape[3] == 1 == d.Ho
    dx, dw, db = torch.autograd.grad(y, (x, w, b), dy)
    for op, want in ((R.FWD, y.detach()), (R.DGRAD, dx), (R.WGRAD, dw), ('dbias', db)):
        TC.close(R.reference(op, layer), want)
