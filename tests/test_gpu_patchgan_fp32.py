"""The PatchGAN discriminator's own 4 x 4 kernels, op level: the image-staged kernels of csrc/conv2d_img.hip (k_sconv forward and data gradient
at both strides, every channel chunk, tiles that touch two to four images, the four parity classes at all four parities of (H, W), every one of
the 14 tile configurations; k_swgrad<4> and <2> with ragged stages, short last splits, stages across two images, wide rows, either block order)
and the first-layer kernels of csrc/patchgan_edge.hip (forward, weight + bias gradient with one and several tiles per workgroup, both data
gradient kernels either side of their 32 768-thread rule), each against a float64 tap loop of the definition.

The entry points are called through the C ABI directly with the machinery of tests/test_gpu_conv_fp32.py (Out, call, judge and its worst-use
table, imported); reference, yardstick (the one-accumulator fp32 chain), error measure and limit are tests/conv_fp32_reference.py's, unchanged;
the planners restated as pure functions and the case lists: tests/patchgan_fp32_reference.py.  Per case:
  * the rung the call took comes from the library's own profiler (cls = op | path << 4 | kh << 8) and must be the 7 or 8 the restated planner
    gives; cases the two-term kernels (rung 10) could take run under nc_set_conv_split(0), all others -- every stride-2 weight gradient among
    them -- under the default switches;
  * every output (y, dx, dw, db) lives in a NaN-filled buffer with 64 guard floats behind it; the workspace is exactly nc_conv_ws_bytes(...)
    bytes of 0xFF at the head of a larger 0xFF buffer whose tail stays unchanged; an undersized workspace is refused before anything is written;
  * a second call gives the same bits; dw with db = NULL gives the bits of dw with db;
  * k_sconv runs under the heuristic plan (nc_sconv_set_tune(0)); at one forward and one stride-2 data-gradient layer every configuration is
    pinned in turn (nc_sconv_set_cfg), meets the float64 limit itself and is bit-equal to the others; one case runs with tuning on and gives
    the heuristic run's bits.  Pin and tune mode are put back whatever a case did.

Worst use of the limit per branch, 1.0 = at the limit (max / (3 max_chain + 2^-21), rms / (3 rms_chain + 2^-23)), measured on an MI355X -- the
table the module prints at its end.  No branch uses more than 0.4 of the limit.  k_sconv and the first-layer forward and data gradient are one
accumulator chain per element, a third of the limit like the chain itself; the weight gradients, which sum in blocks (k_swgrad's splits, the
first layer's float64 partial sums per workgroup), are far below it:
    G_WGRAD/64/split-v4 (the thin planes)              0.052 0.066  pg1 wgrad/walk/ragged/K64                          0.006 0.008
    K65 dgrad G_DGRAD_P/64/split-scalar/padded         0.234 0.173  pg1 wgrad: db                                      0.256 0.312
    K65 fwd G_FWD/64/one                               0.176 0.193  sconv dgrad/s1/CK16/cfg(2,1,2)/img2                0.344 0.301
    K65 wgrad G_WGRAD/64/one                           0.280 0.246  sconv dgrad/s1/CK2/cfg(2,1,2)/img2                 0.329 0.291
    bias_grad                                          0.038 0.036  sconv dgrad/s2 pinned, each of the 14              0.271 0.261
    pg1 dgrad/p00/K8                                   0.278 0.235  sconv dgrad/s2/p00/CK2/cfg(2,1,2)/img2             0.249 0.258
    pg1 dgrad/p01/K20                                  0.318 0.261  sconv dgrad/s2/p01/CK2/cfg(2,1,2)/img3             0.300 0.257
    pg1 dgrad/p11/K64                                  0.346 0.290  sconv dgrad/s2/p01/CK32/cfg(2,1,2)/img2            0.349 0.274
    pg1 dgrad_few/p00/K64                              0.078 0.123  sconv dgrad/s2/p10/CK16/cfg(2,1,2)/img3            0.325 0.254
    pg1 dgrad_few/p01/K6                               0.286 0.194  sconv dgrad/s2/p11/CK32/cfg(2,1,2)/img2            0.346 0.273
    pg1 dgrad_few/p10/K7                               0.156 0.181  sconv dgrad/s2/p11/CK4/cfg(2,1,2)/img2             0.271 0.261
    pg1 dgrad_few/p10/K8                               0.148 0.161  sconv fwd tuned                                    0.331 0.295
    pg1 dgrad_few/p11/K20                              0.110 0.133  sconv fwd/s1/CK16/cfg(2,1,2)/img2                  0.331 0.295
    pg1 fwd/K20                                        0.240 0.192  sconv fwd/s1/CK2/cfg(2,1,2)/img2                   0.316 0.284
    pg1 fwd/K64                                        0.253 0.198  sconv fwd/s2 pinned, each of the 14                0.352 0.286
    pg1 fwd/K7                                         0.227 0.169  sconv fwd/s2/CK4/cfg(2,1,2)/img2                   0.399 0.286
    pg1 fwd/K8                                         0.207 0.171  sconv fwd/s2/CK4/cfg(8,1,1)/img4                   0.292 0.281
    pg1 wgrad/one-tile/K8                              0.107 0.104  sconv fwd/s2/CK8/cfg(2,1,2)/img2                   0.341 0.290
    pg1 wgrad/one-tile/ragged/K20                      0.084 0.121  sconv fwd/s2/CK8/cfg(2,1,2)/img3                   0.280 0.282
    pg1 wgrad/one-tile/ragged/K6                       0.284 0.244  swgrad<2>/s1/splits66/2img                         0.050 0.058
    pg1 wgrad/one-tile/ragged/K7                       0.071 0.099  swgrad<2>/s2/splits68/ragged+2img+wide+xcd         0.040 0.058
    pg1 wgrad/one-tile/ragged/K8                       0.244 0.217  swgrad<2>/s2/splits69/ragged+2img                  0.038 0.058
    swgrad<4>/s1/splits69/ragged+2img                  0.036 0.058  swgrad<4>/s2/splits33/ragged+2img+xcd              0.044 0.064
    swgrad<4>/s1/splits90/ragged+2img+wide             0.039 0.055  swgrad<4>/s2/splits35/ragged+short+2img+xcd        0.038 0.063
One branch computed wrongly before this file: the thin planes.  k_swgrad decodes the input rows of a 64-column stage with one lane per row
(rowoff, read back with readlane), and plan_swgrad sized LDS for `rows = (urows - 1) s + 8 + s` without asking for rows <= 64.  With an output
width of 2 under stride 2 (W = 4, 5) a stage spans 66 .. 70 rows, with an output width of 1 up to 130; rows 64 and up took the offset of lane
r - 64, another row of the same images.  sconv_wgrad_supported accepted such layers from 4096 columns on, and dw came out wrong, not faulting:
32-8-128-130x4 stride 2: max 1.22 rms 0.244 of the rms of dw (chain 8.7e-06, 1.1e-06), 32-8-128-130x5: 1.27 0.250, 64-8-128-65x2 stride 1:
1.34 0.179.  plan_swgrad now has no plan above 64 rows -- nothing from an output width of 3 on has more than 54 -- and the gather GEMM takes
these layers (WGRAD_CASES' thin planes: rung 2, 'G_WGRAD/64/split-v4', 0.05 0.07 of the limit).  The reading that led here was right.
"""
import contextlib
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_fp32_reference as R  # noqa: E402
import patchgan_fp32_reference as PG  # noqa: E402
import test_gpu_conv_fp32 as T  # noqa: E402  (Out, call, judge, WORST: shared, not forked)

DEV = T.DEV
NC_ERR_SHAPE, NC_ERR_WS = -1, -2
OPS = T.OPS
MINE = set()      # the keys of T.WORST this module wrote


def ids(cases):
    return [R.case_id(c) for c in cases]


def op_ids(pairs):
    return ['%s-%s' % (OPS[p[0]], R.case_id(p[1])) for p in pairs]


@pytest.fixture(autouse=True)
def _switches():
    """Every switch a case touches is put back, whatever the case did."""
    split = T.L().nc_get_conv_split()
    yield
    T.L().nc_set_conv_split(split)
    T.L().nc_sconv_set_cfg(-1)
    T.L().nc_sconv_set_tune(-1)


@contextlib.contextmanager
def sconv(tune=0, cfg=-1):
    """The choice of k_sconv's tile configuration: the heuristic (tune 0), timing on first use (tune 1) or one pinned configuration."""
    T.L().nc_sconv_set_tune(tune)
    T.L().nc_sconv_set_cfg(cfg)
    try:
        yield
    finally:
        T.L().nc_sconv_set_cfg(-1)
        T.L().nc_sconv_set_tune(-1)


@pytest.fixture(scope='module', autouse=True)
def _worst_table():
    yield
    print('\nworst use of the limit per branch (max, rms; 1.0 = at the limit)')
    for k in sorted(MINE):
        if k in T.WORST:
            print('  %-58s %.3f %.3f' % (k, T.WORST[k][0], T.WORST[k][1]))


def judge(kernel, what, got, orc):
    MINE.add(kernel)
    T.judge(kernel, what, got, orc)


def assert_rung(op, case, cls):
    """The rung from the profiler against the restated planner, and the branch the case is labelled with."""
    d = R.make_dims(*case[:7])
    rung, name = PG.dispatch(op, d)
    assert name == case[8] and case[7] == PG.mode_of(op, case[:7])
    assert cls == [op | rung << 4 | d.kh << 8], (cls, op, rung)
    return rung


def run_case(op, case, kernel=None, tune=0, cfg=-1):
    """One case: rung, buffers, the float64 limit on every output, a second call with the same bits."""
    layer, what = case[:7], R.case_id(case)
    kernel = kernel or case[8]
    with sconv(tune, cfg):
        code, outs, cls = T.call(op, case, want_db=True)
        T.ck(code, 'nc_conv_' + OPS[op])
        rung = assert_rung(op, case, cls)
        for o, name in zip(outs, ('out', 'db')):
            o.check('%s %s' % (what, name))
        judge(kernel, what, R.err(outs[0].t, R.reference(op, layer, DEV)), R.oracle_err(op, layer))
        if op == R.WGRAD:
            judge('pg1 wgrad: db' if rung == 8 else 'bias_grad', what, R.err(outs[1].t, R.reference('dbias', layer, DEV)), R.oracle_err('dbias', layer))
        code, again, _ = T.call(op, case, want_db=True)
        T.ck(code, 'nc_conv_' + OPS[op])
    for a, o in zip(again, outs):
        assert torch.equal(a.buf[:a.n], o.buf[:o.n]), '%s: a second call gives other bits' % what
    return outs


def test_the_reference_on_the_gpu_is_the_reference_on_the_cpu():
    """The float64 tap loops run on the GPU below: the same numbers as on the CPU, where tests/test_patchgan_fp32_reference.py and
    tests/test_conv_fp32_reference.py hold them to F.conv2d and autograd."""
    for layer in ((2, 1, 20, (13, 10), 4, 2, 1), (2, 6, 8, (9, 12), 4, 1, 1)):
        for op in (R.FWD, R.DGRAD, R.WGRAD, 'dbias'):
            a, r = R.reference(op, layer, DEV), R.reference(op, layer)
            assert float((a.cpu() - r).abs().max()) <= 1e-12 * float(r.abs().max())


@pytest.mark.parametrize('case', PG.FWD_CASES, ids=ids(PG.FWD_CASES))
def test_forward_against_fp64(case):
    run_case(R.FWD, case)


@pytest.mark.parametrize('case', PG.DGRAD_CASES, ids=ids(PG.DGRAD_CASES))
def test_data_gradient_against_fp64(case):
    run_case(R.DGRAD, case)


@pytest.mark.parametrize('case', PG.WGRAD_CASES, ids=ids(PG.WGRAD_CASES))
def test_weight_and_bias_gradient_against_fp64(case):
    """dw and db of one call; then dw of a call with db = NULL: the same bits."""
    dw, db = run_case(R.WGRAD, case)
    code, outs, _ = T.call(R.WGRAD, case, want_db=False)
    T.ck(code, 'nc_conv_wgrad')
    outs[0].check(R.case_id(case) + ' db=NULL')
    assert torch.equal(outs[0].t, dw.t)


@pytest.mark.parametrize('op,case', PG.CFG_CASES, ids=op_ids(PG.CFG_CASES))
def test_every_tile_configuration_meets_the_limit_with_the_same_bits(op, case):
    """k_sconv's 14 tile shapes, pinned one by one: each against float64 -- not only against each other -- and all bit-equal, the heuristic's
    choice among them."""
    layer, what = case[:7], R.case_id(case)
    d = R.make_dims(*layer)
    assert PG.applicable_cfgs(op, d) == list(range(len(PG.SCFGS)))
    ref, orc = R.reference(op, layer, DEV), R.oracle_err(op, layer)
    with sconv(0, -1):
        code, outs, cls = T.call(op, case)
        T.ck(code, 'nc_conv_' + OPS[op])
    first = outs[0]
    for i, g in enumerate(PG.SCFGS):
        with sconv(0, i):
            code, outs, cls = T.call(op, case)
            T.ck(code, 'nc_conv_%s under configuration %d' % (OPS[op], i))
        assert cls == [op | 7 << 4 | 4 << 8]
        outs[0].check('%s cfg %d' % (what, i))
        f = PG.sconv_facts(op, d, g)
        judge('sconv %s/s%d pinned, each of the 14' % (OPS[op], d.sh), '%s cfg(%d,%d,%d)/CK%d/img%d' % (what, *g, f['plan']['CK'], f['images']),
              R.err(outs[0].t, ref), orc)
        assert torch.equal(outs[0].t, first.t), '%s: configuration %d gives other bits than the heuristic choice' % (what, i)


def test_a_pinned_configuration_that_does_not_apply_is_refused():
    """K = 64 under a WN = 2 configuration (128 output channels per tile): NC_ERR_SHAPE, nothing written to y."""
    case = PG.FWD_CASES[0]
    assert case[2] == 64 and PG.SCFGS[0][1] == 2
    with sconv(0, 0):
        code, outs, _ = T.call(R.FWD, case)
    assert code == NC_ERR_SHAPE and outs[0].untouched(), (code, T.L().nc_last_error())


def test_the_timed_choice_gives_the_bits_of_the_heuristic_choice():
    """nc_sconv_set_tune(1): the first call times every applicable configuration and caches the winner, the second launches it."""
    op, case = PG.TUNED_CASE
    layer, what = case[:7], R.case_id(case)
    with sconv(0, -1):
        code, heur, _ = T.call(op, case)
        T.ck(code, 'nc_conv_fwd')
    with sconv(1, -1):
        for n in ('timing call', 'cached call'):
            code, outs, cls = T.call(op, case)
            T.ck(code, 'nc_conv_fwd')
            assert cls == [op | 7 << 4 | 4 << 8]
            outs[0].check('%s %s' % (what, n))
            assert torch.equal(outs[0].t, heur[0].t), '%s: the %s gives other bits than the heuristic plan' % (what, n)
    judge('sconv fwd tuned', what, R.err(outs[0].t, R.reference(op, layer, DEV)), R.oracle_err(op, layer))


@pytest.mark.parametrize('op,case,nbytes', PG.UNDERSIZED, ids=['%s-%s-%d' % (OPS[op], R.case_id(c), nb) for op, c, nb in PG.UNDERSIZED])
def test_undersized_workspace_is_refused_before_anything_is_written(op, case, nbytes):
    with sconv(0, -1):
        code, outs, cls = T.call(op, case, want_db=False, ws_bytes=nbytes)
    assert code == NC_ERR_WS, (code, T.L().nc_last_error())
    assert all(o.untouched() for o in outs)
    assert_rung(op, case, cls)       # refused by the kernel the case names, not on the way to another


@pytest.mark.parametrize('op,case', PG.K65, ids=op_ids(PG.K65))
def test_65_channels_leave_the_first_layer_kernels_and_meet_the_limit(op, case):
    """patchgan_edge.hip stages at most kMaxK = 64 channels: C = 1 with K = 65 goes to the gather GEMM (rung 2), to the same limit."""
    d = R.make_dims(*case[:7])
    assert not PG.pg1_supported(d) and PG.pg1_supported(d._replace(K=64)) and PG.dispatch(op, d)[0] == 2
    run_case(op, case, kernel='K65 ' + OPS[op] + ' ' + case[8])


@pytest.mark.parametrize('N,C,K,H,W,s', PG.REFUSED, ids=['%d-%d-%d-%dx%d-s%d' % r for r in PG.REFUSED])
def test_a_plane_below_the_kernel_is_refused(N, C, K, H, W, s):
    """H or W = 1: the padded extent 3 is below the 4 x 4 kernel.  Every entry returns NC_ERR_SHAPE, nc_conv_ws_bytes 0, outputs stay NaN."""
    L, P = T.L(), T.P
    assert L.nc_conv_ws_bytes(N, C, 1, H, W, K, 1, 4, 4, s, 1) == 0
    x, w, b = torch.randn(N, C, H, W, device=DEV), torch.randn(K, C, 4, 4, device=DEV), torch.randn(K, device=DEV)
    dy = torch.randn(N * K * 16, device=DEV)
    ws = torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device=DEV)
    y, dx, dw, db = T.Out(N * K * 16), T.Out(N, C, H, W), T.Out(K, C, 4, 4), T.Out(K)
    assert L.nc_conv_fwd(P(x), P(w), P(b), P(y.t), N, C, 1, H, W, K, 1, 4, 4, s, 1, P(ws), ws.numel(), T.stream()) == NC_ERR_SHAPE
    assert L.nc_conv_dgrad(P(dy), P(w), P(dx.t), N, C, 1, H, W, K, 1, 4, 4, s, 1, P(ws), ws.numel(), T.stream()) == NC_ERR_SHAPE
    assert L.nc_conv_wgrad(P(x), P(dy), P(dw.t), P(db.t), N, C, 1, H, W, K, 1, 4, 4, s, 1, P(ws), ws.numel(), T.stream()) == NC_ERR_SHAPE
    torch.cuda.synchronize()
    assert y.untouched() and dx.untouched() and dw.untouched() and db.untouched() and bool((ws == 0xFF).all())
