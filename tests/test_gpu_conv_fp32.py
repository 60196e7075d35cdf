"""nc_conv_fwd / nc_conv_dgrad / nc_conv_wgrad on their oldest kernels, op level: every dispatch branch of the gather GEMM (csrc/conv_gemm.hip:
G_FWD, G_DGRAD, G_DGRAD_P, G_WGRAD and the flipped forward, on 64-, 128- and 256-row tiles, in one launch or split with either reduce kernel,
with padded rows), the VALU kernels and bias_grad (conv_direct.hip), the pointwise kernels (conv_1x1.hip), the single-channel and K = 1 kernels
(conv_c1.hip) and the fp32 brick kernels (conv_mfma_fwd.hip, conv_mfma_wgrad.hip: every instantiated KS / CK, the tail kernels, the three row
widths, the stream-K regimes, the four weight-gradient kernels), each against a float64 tap loop of the definition.

The entry points are called through the C ABI directly, so a case reaches the entry and the switches it names.  Reference, yardstick (a
one-accumulator fp32 chain in the kernels' documented order, against the same float64 reference), error measure, limit (tests/convt_reference.py's,
unchanged), the dispatch rules restated as pure functions, and the case lists: tests/conv_fp32_reference.py.  Per case:
  * the rung the call took comes from the library's own profiler (nc_prof_begin / nc_prof_end: cls = op | path << 4 | kh << 8) and must be the
    one the restated ladder gives; a brick case also asks nc_conv_mfma_plan_debug which variant the planner chose;
  * every output (y, dx, dw, db) lives in a NaN-filled buffer with 64 guard floats behind it: no NaN is left inside, the guard is untouched;
  * the workspace is exactly nc_conv_ws_bytes(...) bytes at the head of a buffer of 0xFF bytes (NaN as fp32 and as fp64: no kernel relies on a
    zeroed workspace); the bytes behind it are unchanged;
  * a second call gives the same bits.
Where two branches compute the same layer (default and force-direct; the brick kernels and the VALU kernels) both meet the float64 limit.

Worst use of the limit per branch, 1.0 = at the limit (max / (3 max_chain + 2^-21), rms / (3 rms_chain + 2^-23)), measured on an MI355X -- the
table the module prints at its end.  No branch uses more than two thirds of the limit.  The highest is the VALU forward, whose accumulators start
at the bias (k_conv_fwd<8>: 0.65); the split GEMMs and the weight gradients, which sum in blocks, are far below the chain:
    bias_grad                                          0.090 0.109  fwd brick/KS3/CK4/cfg0/tail/W128/few+cut3            0.099 0.149
    dgrad G_DGRAD/128/one                              0.209 0.160  fwd brick/KS3/CK4/cfg0/tail/W192/few+cut3            0.105 0.149
    dgrad G_DGRAD/256/one                              0.225 0.160  fwd brick/KS3/CK4/cfg0/tail/W64/few+cut3             0.106 0.151
    dgrad G_DGRAD/64/one                               0.405 0.211  fwd brick/KS3/CK4/cfg0/whole-rows/W128/few+cut3      0.123 0.149
    dgrad G_DGRAD/64/split-scalar                      0.107 0.125  fwd brick/KS3/CK4/cfg0/whole-rows/W192/few+cut3      0.117 0.149
    dgrad G_DGRAD/64/split-v4                          0.086 0.123  fwd brick/KS3/CK4/cfg0/whole-rows/W64/few+cut3       0.119 0.147
    dgrad G_DGRAD/64/split-v4/padded                   0.180 0.184  fwd brick/KS3/CK4/cfg4/whole-rows/W64/whole          0.287 0.257
    dgrad G_DGRAD_P/128/one                            0.237 0.178  fwd brick/KS3/CK8/cfg2/tail/W64/few+cut3             0.113 0.154
    dgrad G_DGRAD_P/128/split-v4                       0.029 0.076  fwd brick/KS3/CK8/cfg3/tail/W64/few+cut3             0.064 0.114
    dgrad G_DGRAD_P/256/one                            0.297 0.178  fwd brick/KS3/CK8/cfg4/tail/W64/few+cut3             0.099 0.153
    dgrad G_DGRAD_P/256/split-v4                       0.047 0.077  fwd brick/KS3/CK8/cfg4/whole-rows/W64/few+cut3       0.079 0.147
    dgrad G_DGRAD_P/64/one                             0.337 0.225  fwd brick/KS5/CK2/cfg0/whole-rows/W64/few+cut3       0.143 0.155
    dgrad G_DGRAD_P/64/one/padded                      0.392 0.221  fwd brick/KS5/CK4/cfg1/whole-rows/W64/cut3           0.042 0.083
    dgrad G_DGRAD_P/64/split-scalar                    0.111 0.173  fwd brick/KS5/CK4/cfg4/tail/W64/few+cut3             0.101 0.154
    dgrad G_DGRAD_P/64/split-v4                        0.199 0.195  fwd brick/KS5/CK4/cfg4/whole-rows/W64/few+cut3       0.152 0.156
    dgrad brick/KS3/CK4/cfg0/tail/W64/few+cut3         0.114 0.155  fwd brick/KS7/CK1/cfg1/whole-rows/W128/few           0.304 0.253
    dgrad brick/KS3/CK4/cfg4/whole-rows/W64/whole      0.279 0.264  fwd brick/KS7/CK1/cfg1/whole-rows/W64/few            0.255 0.214
    dgrad brick/KS3/CK8/cfg2/tail/W64/few+cut3         0.107 0.156  fwd flat_1x1                                         0.282 0.244
    dgrad brick/KS3/CK8/cfg4/whole-rows/W64/few+cut3   0.109 0.154  fwd k1_fwd                                           0.101 0.112
    dgrad brick/KS5/CK2/cfg0/whole-rows/W64/few+cut3   0.137 0.156  fwd k_conv_fwd<1>                                    0.530 0.501
    dgrad flat_1x1                                     0.296 0.232  fwd k_conv_fwd<2>                                    0.352 0.410
    dgrad flip G_FWD/128/one                           0.179 0.178  fwd k_conv_fwd<4>                                    0.270 0.315
    dgrad flip G_FWD/64/one                            0.322 0.234  fwd k_conv_fwd<8>                                    0.651 0.546
    dgrad flip G_FWD/64/split-scalar                   0.109 0.138  wgrad G_WGRAD/128/one                                0.184 0.169
    dgrad flip G_FWD/64/split-v4                       0.094 0.134  wgrad G_WGRAD/128/split-v4                           0.046 0.083
    dgrad k_conv_dgrad<1>                              0.267 0.279  wgrad G_WGRAD/256/one                                0.208 0.169
    dgrad k_conv_dgrad<2>                              0.402 0.296  wgrad G_WGRAD/256/split-v4                           0.035 0.068
    dgrad k_conv_dgrad<4>                              0.265 0.247  wgrad G_WGRAD/64/one                                 0.271 0.249
    dgrad k_conv_dgrad<8>                              0.437 0.306  wgrad G_WGRAD/64/split-scalar/padded                 0.172 0.178
    dgrad to1_dgrad                                    0.313 0.321  wgrad G_WGRAD/64/split-v4                            0.199 0.211
    dgrad to1_mfma/1                                   0.018 0.031  wgrad brick/k_wgrad_dma<3,2>/blocks2                 0.049 0.075
    dgrad to1_mfma/2                                   0.010 0.026  wgrad brick/k_wgrad_dma<5,1>/blocks1                 0.036 0.081
    fwd G_FWD/128/one                                  0.214 0.175  wgrad brick/k_wgrad_mfma<3,1>                        0.040 0.076
    fwd G_FWD/128/split-v4                             0.040 0.080  wgrad brick/k_wgrad_rows<3>/rows2                    0.046 0.072
    fwd G_FWD/256/one                                  0.190 0.176  wgrad c1_wgrad/3                                     0.013 0.033
    fwd G_FWD/256/split-v4                             0.031 0.051  wgrad c1_wgrad/7                                     0.033 0.053
    fwd G_FWD/64/one                                   0.376 0.263  wgrad k1_wgrad/1                                     0.031 0.041
    fwd G_FWD/64/split-scalar                          0.103 0.118  wgrad k1_wgrad/4                                     0.025 0.038
    fwd G_FWD/64/split-v4                              0.207 0.171  wgrad k_conv_wgrad<16>                               0.172 0.160
    fwd G_FWD/64/split-v4/padded                       0.202 0.211  wgrad k_conv_wgrad<1>                                0.047 0.057
    fwd brick/KS3/CK1/cfg1/whole-rows/W64/few          0.241 0.193  wgrad wgrad_1x1                                      0.027 0.036
One branch did not compute before this file: the data gradient of a 3^3 layer with K = 1 and 64 | C went to the brick kernel's single-channel
mode, which is forward only -- nc_conv_ws_bytes sized the packed weights for the forward roles, so the call returned NC_ERR_WS with the library's
own workspace size (and k_pack_w_c1 has no flipped form).  conv_mfma_fwd.hip now leaves K = 1 data gradients to the gather GEMM
(DGRAD_CASES: 'flip G_FWD/64/one' at 1-64-1-5x6x8, 0.24 0.21 of the limit)."""
import contextlib
import ctypes
import functools
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_fp32_reference as R  # noqa: E402

DEV = 'cuda'
GUARD = 64
WS_TAIL = 4096
NC_ERR_WS = -2
OPS = {R.FWD: 'fwd', R.DGRAD: 'dgrad', R.WGRAD: 'wgrad'}
WORST = {}


def L():
    from neuroclear_amd._lib import lib
    return lib()


def ck(code, what):
    from neuroclear_amd._lib import check
    check(code, what)


def P(t):
    from neuroclear_amd import ops
    return ops._ptr(t)


def stream():
    from neuroclear_amd import ops
    return ops._stream()


@pytest.fixture(autouse=True)
def _switches():
    """Every switch a case touches is put back, whatever the case did."""
    split = L().nc_get_conv_split()
    yield
    L().nc_set_force_direct(0)
    L().nc_set_conv_split(split)


@contextlib.contextmanager
def dispatch(mode):
    split = L().nc_get_conv_split()
    if mode == R.DIRECT:
        L().nc_set_force_direct(1)
    if mode == R.NO_SPLIT:
        L().nc_set_conv_split(0)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        L().nc_set_force_direct(0)
        L().nc_set_conv_split(split)


@pytest.fixture(scope='module', autouse=True)
def _worst_table():
    yield
    print('\nworst use of the limit per branch (max, rms; 1.0 = at the limit)')
    for k in sorted(WORST):
        print('  %-58s %.3f %.3f' % (k, WORST[k][0], WORST[k][1]))


@functools.lru_cache(maxsize=None)
def gpu_inputs(layer):
    return tuple(t.to(DEV) for t in R.inputs(*layer))


def judge(kernel, what, got, orc):
    """Print product and oracle figures, keep the worst ratio of the branch, assert the limit of tests/convt_reference.py."""
    r = R.ratios(got, orc)
    print('%-58s %-44s product max %.2e rms %.2e | chain max %.2e rms %.2e | of the limit %.3f %.3f'
          % (kernel, what, got[0], got[1], orc[0], orc[1], r[0], r[1]))
    if math.isfinite(r[0]) and math.isfinite(r[1]):
        w = WORST.get(kernel, (0.0, 0.0))
        WORST[kernel] = (max(w[0], r[0]), max(w[1], r[1]))
    assert R.within(got, orc), (kernel, what, got, orc)


class Out:
    """An output tensor inside a NaN-filled buffer with GUARD floats behind it."""

    def __init__(self, *shape):
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + GUARD,), float('nan'), device=DEV)
        self.t = self.buf[:self.n].view(*shape)

    def check(self, what):
        assert not bool(torch.isnan(self.t).any()), '%s: an element was not written' % what
        assert bool(torch.isnan(self.buf[self.n:]).all()), '%s: a write behind the output' % what

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def conv_args(d):
    return (d.N, d.C, d.D, d.H, d.W, d.K, d.kd, d.kh, d.kw, d.sh, d.ph)


def call(op, case, want_db=False, ws_bytes=None):
    """One call of the entry of `op` at a case, under its mode, bracketed by the profiler.  Returns (code, outputs, cls of the recorded calls).
    ws_bytes: pass that many bytes instead of nc_conv_ws_bytes (the undersized-workspace cases)."""
    layer, mode = case[:7], case[7]
    d = R.make_dims(*layer)
    x, w, b, dy = gpu_inputs(layer)
    with dispatch(mode):
        nb = int(L().nc_conv_ws_bytes(*conv_args(d)))
        assert nb >= 64 * 1024 * 8 and nb % 256 == 0          # common.hpp kBiasGradWsBytes is its floor
        if ws_bytes is not None:
            nb = ws_bytes
        big = torch.full((nb + WS_TAIL,), 0xFF, dtype=torch.uint8, device=DEV)
        ws, wsb = (None, 0) if mode == R.NO_WS else (big, nb)
        cls, flop, ms = (ctypes.c_int * 8)(), (ctypes.c_double * 8)(), (ctypes.c_float * 8)()
        L().nc_prof_begin(0.0)
        if op == R.FWD:
            outs = (Out(d.N, d.K, d.Do, d.Ho, d.Wo),)
            code = L().nc_conv_fwd(P(x), P(w), P(b), P(outs[0].t), *conv_args(d), P(ws), wsb, stream())
        elif op == R.DGRAD:
            outs = (Out(d.N, d.C, d.D, d.H, d.W),)
            code = L().nc_conv_dgrad(P(dy), P(w), P(outs[0].t), *conv_args(d), P(ws), wsb, stream())
        else:
            outs = (Out(d.K, d.C, d.kd, d.kh, d.kw),) + ((Out(d.K),) if want_db else ())
            code = L().nc_conv_wgrad(P(x), P(dy), P(outs[0].t), P(outs[1].t if want_db else None), *conv_args(d), P(ws), wsb, stream())
        torch.cuda.synchronize()
        n = L().nc_prof_end(8, cls, flop, ms)
    assert bool((big[nb:] == 0xFF).all()), 'a write behind the workspace'
    return code, outs, [cls[i] for i in range(min(n, 8))]


def plan_debug(what, d):
    out = (ctypes.c_int * 8)()
    ck(L().nc_conv_mfma_plan_debug(what, d.N, d.C, d.D, d.H, d.W, d.K, d.kd, out), 'nc_conv_mfma_plan_debug')
    return list(out)


def assert_branch(op, case, cls):
    """The rung from the profiler against the restated ladder; the brick variant from the planner's own answer."""
    d, mode, branch = R.make_dims(*case[:7]), case[7], case[8]
    path, name = R.dispatch(op, d, mode)
    assert cls == [op | path << 4 | d.kh << 8], (cls, op, path)
    if name == 'brick':
        with dispatch(mode):
            name = R.brick_wgrad_name(plan_debug(2, d)) if op == R.WGRAD else R.brick_fwd_name(d, plan_debug(op, d))
    assert name == branch


def run_case(op, case):
    layer = case[:7]
    what = R.case_id(case)
    kernel = '%s %s' % (OPS[op], case[8])
    code, outs, cls = call(op, case, want_db=True)
    ck(code, 'nc_conv_' + OPS[op])
    assert_branch(op, case, cls)
    for o, name in zip(outs, ('out', 'db')):
        o.check('%s %s' % (what, name))
    judge(kernel, what, R.err(outs[0].t, R.reference(op, layer, DEV)), R.oracle_err(op, layer))
    if op == R.WGRAD:
        judge('bias_grad', what, R.err(outs[1].t, R.reference('dbias', layer, DEV)), R.oracle_err('dbias', layer))
    code, again, _ = call(op, case, want_db=True)
    ck(code, 'nc_conv_' + OPS[op])
    for a, o in zip(again, outs):
        assert torch.equal(a.buf[:a.n], o.buf[:o.n]), '%s: a second call gives other bits' % what
    return outs


def test_the_reference_on_the_gpu_is_the_reference_on_the_cpu():
    """The float64 tap loops run on the GPU below (torch's own fp64 kernels): the same numbers as on the CPU, where
    tests/test_conv_fp32_reference.py holds them to F.conv3d / F.conv2d and autograd."""
    for layer in ((2, 5, 12, (10, 11), 3, 1, 1), (2, 24, 40, (9, 11, 13), 4, 2, 1)):
        for op in (R.FWD, R.DGRAD, R.WGRAD, 'dbias'):
            a, r = R.reference(op, layer, DEV), R.reference(op, layer)
            assert float((a.cpu() - r).abs().max()) <= 1e-12 * float(r.abs().max())


@pytest.mark.parametrize('case', R.FWD_CASES, ids=[R.case_id(c) for c in R.FWD_CASES])
def test_forward_against_fp64(case):
    run_case(R.FWD, case)


@pytest.mark.parametrize('case', R.DGRAD_CASES, ids=[R.case_id(c) for c in R.DGRAD_CASES])
def test_data_gradient_against_fp64(case):
    run_case(R.DGRAD, case)


@pytest.mark.parametrize('case', R.WGRAD_CASES, ids=[R.case_id(c) for c in R.WGRAD_CASES])
def test_weight_and_bias_gradient_against_fp64(case):
    """dw and dbias of one call; then dw of a call with dbias = NULL: the same bits."""
    dw, db = run_case(R.WGRAD, case)
    code, outs, _ = call(R.WGRAD, case, want_db=False)
    ck(code, 'nc_conv_wgrad')
    outs[0].check(R.case_id(case) + ' dbias=NULL')
    assert torch.equal(outs[0].t, dw.t)


@pytest.mark.parametrize('op,case,nbytes', R.UNDERSIZED, ids=['%s-%s-%d' % (OPS[op], R.case_id(c), nb) for op, c, nb in R.UNDERSIZED])
def test_undersized_workspace_is_refused_before_anything_is_written(op, case, nbytes):
    """conv_gemm.hip split_setup, conv_mfma_fwd.hip run and conv_1x1.hip launch_flat compare the size in front of their first launch."""
    code, outs, cls = call(op, case, want_db=False, ws_bytes=nbytes)
    assert code == NC_ERR_WS, (code, L().nc_last_error())
    assert all(o.untouched() for o in outs)
    assert_branch(op, case, cls)       # refused by the kernel the case names, not on the way to another


BRICK_AND_DIRECT = [(R.FWD, R.first_case(R.FWD, 'brick/KS3/CK4/cfg0/tail/W64/few+cut3', R.NO_SPLIT)),
                    (R.FWD, R.first_case(R.FWD, 'brick/KS5/CK2/cfg0/whole-rows/W64/few+cut3', R.NO_SPLIT)),
                    (R.FWD, R.first_case(R.FWD, 'brick/KS7/CK1/cfg1/whole-rows/W64/few', R.NO_SPLIT)),
                    (R.DGRAD, R.first_case(R.DGRAD, 'brick/KS3/CK8/cfg4/whole-rows/W64/few+cut3', R.NO_SPLIT)),
                    (R.WGRAD, R.first_case(R.WGRAD, 'brick/k_wgrad_rows<3>/rows2', R.NO_SPLIT)),
                    (R.WGRAD, R.first_case(R.WGRAD, 'brick/k_wgrad_mfma<3,1>', R.NO_SPLIT))]


@pytest.mark.parametrize('op,case', BRICK_AND_DIRECT, ids=['%s-%s' % (OPS[op], R.case_id(c)) for op, c in BRICK_AND_DIRECT])
def test_brick_layers_on_the_valu_kernels_meet_the_same_limit(op, case):
    """The layer of a brick case under force-direct: another kernel, another order, the same float64 limit (the brick run itself is held to it
    above); the two need not agree bit for bit, only within the sum of what each is allowed."""
    layer = case[:7]
    d = R.make_dims(*layer)
    direct = layer + (R.DIRECT, R.direct_branch(op, d))
    outs = run_case(op, direct)
    code, brick, _ = call(op, case, want_db=True)
    ck(code, 'nc_conv_' + OPS[op])
    ref, orc = R.reference(op, layer, DEV), R.oracle_err(op, layer)
    both = R.err(outs[0].t, brick[0].t.double())
    scale = float(brick[0].t.double().pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    assert both[0] * scale <= 2 * (R.FACTOR * orc[0] + R.MAX_FLOOR) and both[1] * scale <= 2 * (R.FACTOR * orc[1] + R.RMS_FLOOR), (both, orc)
