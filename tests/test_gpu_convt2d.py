"""ConvTranspose2d(kernel 2, stride 2), op level: every kernel and dispatch branch of csrc/convt2d.hip (k_convT2d_fwd_mfma, k_convT2d_fwd<4 | 2 | 1>,
k_convT2d_dgrad<8 | 4 | 1>, k_convT2d_wgrad<4,4 | 1,1>, the gather-GEMM data and weight gradients, the bias gradient), each against a float64
einsum of the definition.

The entry points are called through the C ABI directly.  References, yardstick (the one-accumulator fp32 chain against the same float64
reference, evaluated with torch on the GPU), error measure, limit and the case lists: tests/conv2d_reference.py.  Every output buffer is
allocated NaN-filled with 64 guard elements behind it: an element that is not written fails, and so does a write past the end.  Every call is made
twice: the two results are bit-equal.

Which kernel a case reaches follows from the dispatch conditions of csrc/convt2d.hip, restated in branch_*() below and asserted against the name
each case carries.  The fallbacks without a workspace are also held bit for bit to the force-direct run of the same kernel."""
import contextlib
import functools
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv2d_reference as R  # noqa: E402

DEV = 'cuda'
GUARD = 64
BIAS_GRAD_WS = 64 * 1024 * 8     # common.hpp kBiasGradWsBytes: nc_convT2d_ws_bytes is the larger of this and the GEMM's need (to 256 bytes)
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


@contextlib.contextmanager
def dispatch(mode):
    if mode == R.DIRECT:
        L().nc_set_force_direct(1)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        L().nc_set_force_direct(0)


@pytest.fixture(scope='module', autouse=True)
def _worst_table():
    yield
    print('\nworst use of the limit per kernel (max, rms; 1.0 = at the limit)')
    for k in sorted(WORST):
        print('  %-28s max %.3f  rms %.3f' % (k, WORST[k][0], WORST[k][1]))


@functools.lru_cache(maxsize=None)
def gpu_inputs(N, C, K, n):
    return tuple(t.to(DEV) for t in R.inputs(N, C, K, n))


@functools.lru_cache(maxsize=None)
def oracle(what, N, C, K, n, with_bias=False):
    """(max, rms) of the fp32 chain against the float64 reference, both on the GPU; computed once per shape."""
    x, w, b, dy = gpu_inputs(N, C, K, n)
    if what == 'fwd':
        return R.err(R.chain_fwd(x, w, b if with_bias else None), R.ref_fwd(x, w, b if with_bias else None))
    if what == 'dgrad':
        return R.err(R.chain_dgrad(dy, w), R.ref_dgrad(dy, w))
    if what == 'wgrad':
        return R.err(R.chain_wgrad(x, dy), R.ref_wgrad(x, dy))
    return R.err(R.chain_dbias(dy), R.ref_dbias(dy))


def judge(kernel, what, got, orc):
    """Print product and oracle figures, keep the worst ratio of the kernel, assert the limit of tests/conv2d_reference.py."""
    r = R.ratios(got, orc)
    print('%-22s %-40s product max %.2e rms %.2e | chain max %.2e rms %.2e | of the limit %.3f %.3f'
          % (kernel, what, got[0], got[1], orc[0], orc[1], r[0], r[1]))
    if math.isfinite(r[0]) and math.isfinite(r[1]):
        w = WORST.get(kernel, (0.0, 0.0))
        WORST[kernel] = (max(w[0], r[0]), max(w[1], r[1]))
    assert R.within(got, orc), (kernel, what, got, orc)


class Out:
    """A NaN-filled output of `shape` with GUARD NaN elements behind it."""

    def __init__(self, *shape):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + GUARD,), float('nan'), device=DEV)
        self.t = self.buf[:n].view(*shape)

    def check(self):
        assert not bool(torch.isnan(self.t).any()), 'an output element was not written'
        assert bool(torch.isnan(self.buf[self.t.numel():]).all()), 'a write past the end of the output'
        return self.t


def test_the_reference_on_the_gpu_is_the_reference_on_the_cpu():
    """The fp64 einsums and the chain run on the GPU below: the einsums give the CPU's numbers (where tests/test_conv2d_reference.py holds them to
    torch's float64 operators), and the float32 chain, whose every step is one correctly rounded multiplication or addition, the CPU's bits."""
    shape = (2, 12, 8, (5, 13))
    x, w, b, dy = R.inputs(*shape)
    xg, wg, bg, dyg = gpu_inputs(*shape)
    for a, r in ((R.ref_fwd(xg, wg, bg), R.ref_fwd(x, w, b)), (R.ref_dgrad(dyg, wg), R.ref_dgrad(dy, w)), (R.ref_wgrad(xg, dyg), R.ref_wgrad(x, dy)),
                 (R.ref_dbias(dyg), R.ref_dbias(dy))):
        assert float((a.cpu() - r).abs().max()) <= 1e-12 * float(r.abs().max())
    for a, r in ((R.chain_fwd(xg, wg, bg), R.chain_fwd(x, w, b)), (R.chain_dgrad(dyg, wg), R.chain_dgrad(dy, w)),
                 (R.chain_wgrad(xg, dyg), R.chain_wgrad(x, dy)), (R.chain_dbias(dyg), R.chain_dbias(dy))):
        assert torch.equal(a.cpu(), r)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# forward, nc_convT2d_k2s2_fwd
# ---------------------------------------------------------------------------------------------------------------------------------------------
def branch_fwd(N, C, K, n, mode):
    """convt2d.hip nc_convT2d_k2s2_fwd: the matrix cores for K % 32 == 0, C % 16 == 0 and C >= 128 unless forced direct, else
    k_convT2d_fwd<pick(K, 4, 2, 1)>."""
    if mode != R.DIRECT and K % 32 == 0 and C % 16 == 0 and C >= 128:
        return 'mfma'
    return 'fwd<%d>' % (4 if K % 4 == 0 else 2 if K % 2 == 0 else 1)


def fwd(x, w, b, mode=None):
    N, C, H, W = x.shape
    K = w.shape[1]
    y = Out(N, K, 2 * H, 2 * W)
    with dispatch(mode):
        ck(L().nc_convT2d_k2s2_fwd(P(x), P(w), P(b), P(y.t), N, C, H, W, K, stream()), 'nc_convT2d_k2s2_fwd')
    return y.check()


@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('case', R.FWD_CASES, ids=[R.case_id(c) for c in R.FWD_CASES])
def test_forward_against_fp64(case, with_bias):
    N, C, K, n, mode, branch = case
    assert branch_fwd(N, C, K, n, mode) == branch
    x, w, b, _ = gpu_inputs(N, C, K, n)
    bb = b if with_bias else None
    y = fwd(x, w, bb, mode)
    judge('k_convT2d_fwd_mfma' if branch == 'mfma' else 'k_convT2d_' + branch, '%s %s' % (R.case_id(case), 'bias' if with_bias else 'nobias'),
          R.err(y, R.ref_fwd(x, w, bb)), oracle('fwd', N, C, K, n, with_bias))
    assert torch.equal(y, fwd(x, w, bb, mode))


def test_forward_matrix_core_and_valu_kernel_agree():
    """The same layer under nc_set_force_direct(1): another kernel, the same values to fp32 rounding (both walk the channels in ascending order, so
    the bits may even agree) -- and the switch is read per call (the third run is the first one's bits)."""
    N, C, K, n = 2, 256, 128, R.P65
    x, w, b, _ = gpu_inputs(N, C, K, n)
    y0, y1, y2 = fwd(x, w, b), fwd(x, w, b, R.DIRECT), fwd(x, w, b)
    assert torch.equal(y0, y2)
    assert float((y0 - y1).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------------------
# data gradient, nc_convT2d_k2s2_dgrad
# ---------------------------------------------------------------------------------------------------------------------------------------------
def ws_for(N, C, K, n):
    nb = int(L().nc_convT2d_ws_bytes(N, C, *n, K))
    assert nb >= BIAS_GRAD_WS and nb % 256 == 0
    return torch.empty(nb, dtype=torch.uint8, device=DEV), nb


def branch_dgrad(N, C, K, n, mode):
    """convt2d.hip nc_convT2d_k2s2_dgrad: the gather GEMM for C >= 64 unless forced direct or the workspace does not cover the GEMM's need, else
    k_convT2d_dgrad<pick(C, 8, 4, 1)>.  (The GEMM's own conditions -- index range, padded_ok -- hold for every shape with C >= 64 here.)"""
    if mode is None and C >= 64:
        return 'gemm'
    return 'dgrad<%d>' % (8 if C % 8 == 0 else 4 if C % 4 == 0 else 1)


def dgrad(dy, w, N, C, K, n, mode):
    ws, nb = ws_for(N, C, K, n)
    dx = Out(N, C, *n)
    with dispatch(mode):
        ck(L().nc_convT2d_k2s2_dgrad(P(dy), P(w), P(dx.t), N, C, *n, K, P(None if mode == R.NO_WS else ws), 0 if mode == R.NO_WS else nb, stream()),
           'nc_convT2d_k2s2_dgrad')
    return dx.check(), nb


@pytest.mark.parametrize('case', R.DGRAD_CASES, ids=[R.case_id(c) for c in R.DGRAD_CASES])
def test_data_gradient_against_fp64(case):
    N, C, K, n, mode, branch = case
    assert branch_dgrad(N, C, K, n, mode) == branch
    x, w, b, dy = gpu_inputs(N, C, K, n)
    dx, nb = dgrad(dy, w, N, C, K, n, mode)
    judge('dgrad gemm' if branch == 'gemm' else 'k_convT2d_' + branch + (' C>=64' if C >= 64 else ''), R.case_id(case),
          R.err(dx, R.ref_dgrad(dy, w)), oracle('dgrad', N, C, K, n))
    assert torch.equal(dx, dgrad(dy, w, N, C, K, n, mode)[0])
    if mode == R.NO_WS:
        # the fall-back is reached only where the GEMM needs a workspace: nc_convT2d_ws_bytes above its floor says it does ...
        assert nb > BIAS_GRAD_WS
        # ... and what ran is the kernel of the force-direct run, bit for bit
        assert torch.equal(dx, dgrad(dy, w, N, C, K, n, R.DIRECT)[0])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# weight and bias gradient, nc_convT2d_k2s2_wgrad
# ---------------------------------------------------------------------------------------------------------------------------------------------
def branch_wgrad(N, C, K, n, mode):
    """convt2d.hip nc_convT2d_k2s2_wgrad: the GEMM when not forced direct, a sufficient workspace is passed and gemm_wgrad_supported holds -- rows
    C >= 16, or a reduction N * H * W >= 256 (conv_gemm.hip padded_ok; the padded problem is far below its 30 GFLOP cap here) -- else
    k_convT2d_wgrad<4, 4> for C % 4 == 0 and K % 4 == 0, else <1, 1>."""
    if mode is None and (C >= 16 or N * n[0] * n[1] >= 256):
        return 'gemm' if C >= 16 else 'gemm, %d rows' % C
    return 'wgrad<4,4>' if C % 4 == 0 and K % 4 == 0 else 'wgrad<1,1>'


def wgrad(x, dy, N, C, K, n, mode, want_db):
    ws, nb = ws_for(N, C, K, n)
    dw = Out(C, K, 2, 2)
    db = Out(K) if want_db else None
    with dispatch(mode):
        ck(L().nc_convT2d_k2s2_wgrad(P(x), P(dy), P(dw.t), P(db.t if want_db else None), N, C, *n, K, P(None if mode == R.NO_WS else ws),
                                     0 if mode == R.NO_WS else nb, stream()), 'nc_convT2d_k2s2_wgrad')
    return dw.check(), (db.check() if want_db else None), nb


@pytest.mark.parametrize('case', R.WGRAD_CASES, ids=[R.case_id(c) for c in R.WGRAD_CASES])
def test_weight_and_bias_gradient_against_fp64(case):
    """dw and dbias of one call, and dw of a call with dbias = NULL (without a workspace the only call: the bias gradient needs one)."""
    N, C, K, n, mode, branch = case
    assert branch_wgrad(N, C, K, n, mode) == branch
    x, w, b, dy = gpu_inputs(N, C, K, n)
    ref = R.ref_wgrad(x, dy)
    orc = oracle('wgrad', N, C, K, n)
    kernel = 'wgrad gemm' if branch.startswith('gemm') else 'k_convT2d_' + branch
    if mode != R.NO_WS:
        dw, db, _ = wgrad(x, dy, N, C, K, n, mode, True)
        judge(kernel, R.case_id(case), R.err(dw, ref), orc)
        judge('bias_grad', R.case_id(case), R.err(db, R.ref_dbias(dy)), oracle('dbias', N, C, K, n))
        dw_b, db_b, _ = wgrad(x, dy, N, C, K, n, mode, True)
        assert torch.equal(dw, dw_b) and torch.equal(db, db_b)
    dw2, _, nb = wgrad(x, dy, N, C, K, n, mode, False)
    judge(kernel, R.case_id(case) + ' dbias=NULL', R.err(dw2, ref), orc)
    if mode == R.NO_WS:   # the GEMM needed a workspace, and what ran is the kernel of the force-direct run, bit for bit
        assert nb > BIAS_GRAD_WS
        assert torch.equal(dw2, wgrad(x, dy, N, C, K, n, R.DIRECT, False)[0])


def test_bias_gradient_without_a_workspace_is_refused():
    N, C, K, n = 2, 10, 6, R.P260
    x, w, b, dy = gpu_inputs(N, C, K, n)
    dw, db = Out(C, K, 2, 2), Out(K)
    code = L().nc_convT2d_k2s2_wgrad(P(x), P(dy), P(dw.t), P(db.t), N, C, *n, K, P(None), 0, stream())
    torch.cuda.synchronize()
    assert code != 0 and bool(torch.isnan(db.buf).all())


def test_bad_arguments_are_refused_before_any_launch():
    x, w, b, dy = gpu_inputs(1, 3, 1, R.P3)
    y = Out(1, 1, 2, 6)
    assert L().nc_convT2d_k2s2_fwd(P(None), P(w), P(b), P(y.t), 1, 3, 1, 3, 1, stream()) != 0
    assert L().nc_convT2d_k2s2_fwd(P(x), P(w), P(b), P(y.t), 1, 3, 0, 3, 1, stream()) != 0
    assert L().nc_convT2d_k2s2_fwd(P(x), P(w), P(b), P(y.t), 1, 3, 1, 3, 70000, stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.buf).all())
