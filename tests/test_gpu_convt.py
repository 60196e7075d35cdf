"""ConvTranspose3d(kernel 2, stride 2), op level: every kernel and dispatch branch of csrc/convt.hip (k_convT_fwd_mfma, k_convT_fwd<4 | 2 | 1>,
k_convT_dgrad<8 | 4 | 1>, k_convT_wgrad<4,4 | 1,1>, the gather-GEMM data and weight gradients, convT_fwd_s3) and the shapes of csrc/convt_s3.hip's
k_convT_s3<8 | 4, 3> that tests/test_gpu_convt_split.py leaves out, each against a float64 einsum of the definition.

The entry points are called through the C ABI directly, so a case reaches the entry it names and not what neuroclear_amd.ops would pick
(ops.conv_transpose_k2s2 takes the split-operand kernel wherever nc_convT_k2s2_split_active holds).  Reference, yardstick (torch's fp32 operator on
the CPU against the same fp64 reference), error measure, limit and the case lists: tests/convt_reference.py.  Every output buffer is pre-filled
with NaN (0xA5 bytes for the 16-bit forms): an element that is not written fails.

Which kernel a case reaches follows from the dispatch conditions of csrc/convt.hip, restated in branch_*() below and asserted against the name
each case carries; where the library can be asked (nc_convT_k2s2_split_supported / _active, nc_convT_ws_bytes) it is.  The fallbacks without a
workspace are also held bit for bit to the force-direct run of the same kernel."""
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
import convt_reference as R  # noqa: E402

DEV = 'cuda'
SENT = 0xA5                      # sentinel byte of the S3 buffers (0xA5A5 is a finite bf16)
BIAS_GRAD_WS = 64 * 1024 * 8     # common.hpp kBiasGradWsBytes: nc_convT_ws_bytes is the larger of this and the GEMM's need (to 256 bytes)
NC_ERR_SHAPE = -1

# Worst use of the limit per kernel, 1.0 = at the limit (max / (3 max_oracle + 2^-21), rms / (3 rms_oracle + 2^-23)), measured on an MI355X
# (the table the module prints at its end).  No kernel needs more than the factor 3:
#   k_convT_fwd_mfma        0.315 0.279     dgrad gemm              0.342 0.282     wgrad gemm           0.383 0.325
#   k_convT_fwd<4>          0.665 0.387     k_convT_dgrad<8> C>=64  0.462 0.282     k_convT_wgrad<4,4>   0.187 0.139
#   k_convT_fwd<2>          0.270 0.202     k_convT_dgrad<8>        0.136 0.146     k_convT_wgrad<1,1>   0.160 0.125
#   k_convT_fwd<1>          0.253 0.160     k_convT_dgrad<4>        0.163 0.147     bias_grad            0.092 0.057
#                                           k_convT_dgrad<1>        0.211 0.193
#   k_convT_s3 against its own limits (max / 3e-6, rms / min(3e-7, 1.5 rms_oracle + 5e-8)): 0.877 0.707
# Before this file two kernels did not meet it: k_convT_fwd<KT> started its accumulators at the bias (0.971 0.959 here, 1.04 of the max limit
# at tests/test_gpu_h2_writers.py's 256 -> 128 case with a randn bias) and k_convT_dgrad<8> at K = 128 summed one chain of 1024 terms
# (1.356 0.761); both now sum as csrc/convt.hip describes.
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
    return tuple(t.to(DEV) if t is not None else None for t in R.inputs(N, C, K, n))


def judge(kernel, what, got, orc):
    """Print product and oracle figures, keep the worst ratio of the kernel, assert the limit of tests/convt_reference.py."""
    r = R.ratios(got, orc)
    print('%-22s %-46s product max %.2e rms %.2e | oracle max %.2e rms %.2e | of the limit %.3f %.3f'
          % (kernel, what, got[0], got[1], orc[0], orc[1], r[0], r[1]))
    if math.isfinite(r[0]) and math.isfinite(r[1]):
        w = WORST.get(kernel, (0.0, 0.0))
        WORST[kernel] = (max(w[0], r[0]), max(w[1], r[1]))
    assert R.within(got, orc), (kernel, what, got, orc)


def nan_like(*shape):
    return torch.full(shape, float('nan'), device=DEV)


def test_the_reference_on_the_gpu_is_the_reference_on_the_cpu():
    """The fp64 einsums run on the GPU below (torch's own fp64 kernels): the same numbers as on the CPU, where tests/test_convt_reference.py holds
    them to F.conv_transpose3d and autograd."""
    shape = (2, 12, 8, R.P260)
    x, w, b, dy = R.inputs(*shape)
    xg, wg, bg, dyg = gpu_inputs(*shape)
    for a, r in ((R.ref_fwd(xg, wg, bg), R.ref_fwd(x, w, b)), (R.ref_dgrad(dyg, wg), R.ref_dgrad(dy, w)), (R.ref_wgrad(xg, dyg), R.ref_wgrad(x, dy)),
                 (R.ref_dbias(dyg), R.ref_dbias(dy))):
        assert float((a.cpu() - r).abs().max()) <= 1e-12 * float(r.abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# forward, nc_convT_k2s2_fwd: the fp32 entry (never the split-operand kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def branch_fwd(N, C, K, n, mode):
    """convt.hip convT_fwd_impl: the matrix cores for C == 128 and K % 32 == 0 unless forced direct, else k_convT_fwd<pick(K, 4, 2, 1)>."""
    S = n[0] * n[1] * n[2]
    if mode != R.DIRECT and K % 32 == 0 and C == 128 and N * K * 8 * S < 1 << 40:
        tiles = -(-S // 32) * N
        cap = -(-2048 // (2 * (K // 32)))
        return 'mfma-capped' if -(-tiles // 4) > cap else 'mfma'
    return 'fwd<%d>' % (4 if K % 4 == 0 else 2 if K % 2 == 0 else 1)


def fwd32(x, w, b, mode=None):
    N, C, D, H, W = x.shape
    K = w.shape[1]
    y = nan_like(N, K, 2 * D, 2 * H, 2 * W)
    with dispatch(mode):
        ck(L().nc_convT_k2s2_fwd(P(x), P(w), P(b), P(y), N, C, D, H, W, K, stream()), 'nc_convT_k2s2_fwd')
    return y


@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('case', R.FWD_CASES, ids=[R.case_id(c) for c in R.FWD_CASES])
def test_forward_fp32_against_fp64(case, with_bias):
    N, C, K, n, mode, branch = case
    assert branch_fwd(N, C, K, n, mode) == branch
    if branch == 'mfma-capped':   # a second sweep of the tile loop that not every workgroup takes
        tiles, per_sweep = -(-(n[0] * n[1] * n[2]) // 32) * N, 4 * -(-2048 // (2 * (K // 32)))
        assert per_sweep < tiles < 2 * per_sweep and (tiles - per_sweep) % 4 == 0 and (tiles, per_sweep) == (1088, 1024)
    # ops.conv_transpose_k2s2 would not come here where the split-operand kernel covers the shape
    assert bool(L().nc_convT_k2s2_split_supported(N, C, *n, K)) == (C % 32 == 0 and K % 16 == 0 and C <= 256)
    x, w, b, _ = gpu_inputs(N, C, K, n)
    y = fwd32(x, w, b if with_bias else None, mode)
    ref = R.ref_fwd(x, w, b if with_bias else None)
    orc = R.err(R.oracle_fwd(N, C, K, n, with_bias), ref)
    assert not bool(torch.isnan(y).any())
    judge('k_convT_fwd_mfma' if branch.startswith('mfma') else 'k_convT_' + branch, '%s %s' % (R.case_id(case), 'bias' if with_bias else 'nobias'),
          R.err(y, ref), orc)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# data gradient, nc_convT_k2s2_dgrad
# ---------------------------------------------------------------------------------------------------------------------------------------------
def ws_for(N, C, K, n):
    nb = int(L().nc_convT_ws_bytes(N, C, *n, K))
    assert nb >= BIAS_GRAD_WS and nb % 256 == 0
    return torch.empty(nb, dtype=torch.uint8, device=DEV), nb


def branch_dgrad(N, C, K, n, mode):
    """convt.hip nc_convT_k2s2_dgrad: the gather GEMM for C >= 64 unless forced direct or the workspace does not cover the GEMM's need, else
    k_convT_dgrad<pick(C, 8, 4, 1)>.  (The GEMM's own conditions -- index range, padded_ok -- hold for every shape with C >= 64 here.)"""
    if mode is None and C >= 64:
        return 'gemm'
    return 'dgrad<%d>' % (8 if C % 8 == 0 else 4 if C % 4 == 0 else 1)


def dgrad(dy, w, N, C, K, n, mode):
    ws, nb = ws_for(N, C, K, n)
    dx = nan_like(N, C, *n)
    with dispatch(mode):
        ck(L().nc_convT_k2s2_dgrad(P(dy), P(w), P(dx), N, C, *n, K, P(None if mode == R.NO_WS else ws), 0 if mode == R.NO_WS else nb, stream()),
           'nc_convT_k2s2_dgrad')
    return dx, nb


@pytest.mark.parametrize('case', R.DGRAD_CASES, ids=[R.case_id(c) for c in R.DGRAD_CASES])
def test_data_gradient_against_fp64(case):
    N, C, K, n, mode, branch = case
    assert branch_dgrad(N, C, K, n, mode) == branch
    x, w, b, dy = gpu_inputs(N, C, K, n)
    dx, nb = dgrad(dy, w, N, C, K, n, mode)
    ref = R.ref_dgrad(dy, w)
    orc = R.err(R.oracle_bwd(N, C, K, n)[0], ref)
    assert not bool(torch.isnan(dx).any())
    judge('dgrad gemm' if branch == 'gemm' else 'k_convT_' + branch + (' C>=64' if C >= 64 else ''), R.case_id(case), R.err(dx, ref), orc)
    if mode == R.NO_WS:
        # the fall-back is reached only where the GEMM needs a workspace: nc_convT_ws_bytes above its floor says it does ...
        assert nb > BIAS_GRAD_WS
        # ... and what ran is the kernel of the force-direct run, bit for bit
        assert torch.equal(dx, dgrad(dy, w, N, C, K, n, R.DIRECT)[0])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# weight and bias gradient, nc_convT_k2s2_wgrad
# ---------------------------------------------------------------------------------------------------------------------------------------------
def branch_wgrad(N, C, K, n, mode):
    """convt.hip nc_convT_k2s2_wgrad: the GEMM when not forced direct, a sufficient workspace is passed and gemm_wgrad_supported holds -- rows
    C >= 16, or a reduction N * S >= 256 (conv_gemm.hip padded_ok; the padded problem is far below its 30 GFLOP cap here) -- else
    k_convT_wgrad<4, 4> for C % 4 == 0 and K % 4 == 0, else <1, 1>."""
    S = n[0] * n[1] * n[2]
    if mode is None and (C >= 16 or N * S >= 256):
        return 'gemm' if C >= 16 else 'gemm, %d rows' % C
    return 'wgrad<4,4>' if C % 4 == 0 and K % 4 == 0 else 'wgrad<1,1>'


def wgrad(x, dy, N, C, K, n, mode, want_db):
    ws, nb = ws_for(N, C, K, n)
    dw = nan_like(C, K, 2, 2, 2)
    db = nan_like(K) if want_db else None
    with dispatch(mode):
        ck(L().nc_convT_k2s2_wgrad(P(x), P(dy), P(dw), P(db), N, C, *n, K, P(None if mode == R.NO_WS else ws), 0 if mode == R.NO_WS else nb, stream()),
           'nc_convT_k2s2_wgrad')
    return dw, db


@pytest.mark.parametrize('case', R.WGRAD_CASES, ids=[R.case_id(c) for c in R.WGRAD_CASES])
def test_weight_and_bias_gradient_against_fp64(case):
    """dw and dbias of one call, and dw of a call with dbias = NULL (without a workspace the only call: the bias gradient needs one)."""
    N, C, K, n, mode, branch = case
    assert branch_wgrad(N, C, K, n, mode) == branch
    x, w, b, dy = gpu_inputs(N, C, K, n)
    ref = R.ref_wgrad(x, dy)
    _, odw, odb = R.oracle_bwd(N, C, K, n)
    orc = R.err(odw, ref)
    kernel = 'wgrad gemm' if branch.startswith('gemm') else 'k_convT_' + branch
    if mode != R.NO_WS:
        dw, db = wgrad(x, dy, N, C, K, n, mode, True)
        assert not bool(torch.isnan(dw).any()) and not bool(torch.isnan(db).any())
        judge(kernel, R.case_id(case), R.err(dw, ref), orc)
        rdb = R.ref_dbias(dy)
        judge('bias_grad', R.case_id(case), R.err(db, rdb), R.err(odb, rdb))
    dw2, _ = wgrad(x, dy, N, C, K, n, mode, False)
    assert not bool(torch.isnan(dw2).any())
    judge(kernel, R.case_id(case) + ' dbias=NULL', R.err(dw2, ref), orc)
    if mode == R.NO_WS:   # the kernel of the force-direct run, bit for bit
        assert torch.equal(dw2, wgrad(x, dy, N, C, K, n, R.DIRECT, False)[0])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# three-term forward, nc_convT_k2s2_fwd_split (csrc/convt_s3.hip): what tests/test_gpu_convt_split.py lacks
# ---------------------------------------------------------------------------------------------------------------------------------------------
def from_s3(raw, N, C, S):
    from test_gpu_convt_split import _from_s3
    return _from_s3(raw, N, C, S)


def s3_buffer(N, ctot, S2):
    return torch.full((int(L().nc_s3_bytes(N, ctot, S2)),), SENT, dtype=torch.uint8, device=DEV)


def fwd_split(x, w, b, want_y=True, want_s3=False):
    N, C, D, H, W = x.shape
    K = w.shape[1]
    nb = int(L().nc_convT_k2s2_split_ws_bytes(N, C, D, H, W, K))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    y = nan_like(N, K, 2 * D, 2 * H, 2 * W) if want_y else None
    ys = s3_buffer(N, K, 8 * D * H * W) if want_s3 else None
    ck(L().nc_convT_k2s2_fwd_split(P(x), P(None), P(w), P(b), P(y), P(ys), K, 0, N, C, D, H, W, K, P(ws), nb, stream()), 'nc_convT_k2s2_fwd_split')
    torch.cuda.synchronize()
    return y, ys


def judge_split(what, got, orc):
    """The limits the project already has for this kernel (tests/test_gpu_convt_split.py), the fp32 figure now the CPU oracle's."""
    print('%-22s %-46s product max %.2e rms %.2e | oracle max %.2e rms %.2e' % ('k_convT_s3', what, got[0], got[1], orc[0], orc[1]))
    w = WORST.get('k_convT_s3 (own limits)', (0.0, 0.0))
    WORST['k_convT_s3 (own limits)'] = (max(w[0], got[0] / R.SPLIT_MAX), max(w[1], got[1] / min(R.SPLIT_RMS, R.SPLIT_FACTOR * orc[1] + R.SPLIT_FLOOR)))
    assert got[1] < R.SPLIT_RMS and got[0] < R.SPLIT_MAX, (what, got)
    assert got[1] <= R.SPLIT_FACTOR * orc[1] + R.SPLIT_FLOOR, (what, got, orc)


@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('case', R.SPLIT_CASES, ids=[R.case_id(c) for c in R.SPLIT_CASES])
def test_forward_three_term_against_fp64(case, with_bias):
    N, C, K, n, QN = case
    assert QN == (8 if (C // 32) * 8 * 3 * 1024 <= 128 * 1024 else 4)     # convt_s3.hip qn_for
    ngroups = (K // 16) * (8 // QN)
    slots, tiles = 8 * max(32 // ngroups, 1), N * -(-(n[0] * n[1] * n[2]) // 512)   # convT_fwd_s3x's grid, k_convT_s3's nslots and ntiles
    if C == 128:
        assert (slots, tiles) == (64, 66)
    assert L().nc_convT_k2s2_split_supported(N, C, *n, K) == 1
    assert L().nc_convT_k2s2_split_active(N, C, *n, K) == (1 if L().nc_get_conv_split() else 0)
    x, w, b, _ = gpu_inputs(N, C, K, n)
    y, _ = fwd_split(x, w, b if with_bias else None)
    ref = R.ref_fwd(x, w, b if with_bias else None)
    assert not bool(torch.isnan(y).any())
    judge_split('%s %s' % (R.case_id(case), 'bias' if with_bias else 'nobias'), R.err(y, ref), R.err(R.oracle_fwd(N, C, K, n, with_bias), ref))


def test_forward_three_term_s3_output_alone():
    """y = NULL, only the S3 form requested: it decodes to the y of a second call, bit for bit, and that y is held to fp64 above."""
    N, C, K, n, _ = R.SPLIT_CASES[1]
    x, w, b, _ = gpu_inputs(N, C, K, n)
    none, ys = fwd_split(x, w, b, want_y=False, want_s3=True)
    y, _ = fwd_split(x, w, b)
    S2 = 8 * n[0] * n[1] * n[2]
    assert none is None and not bool(torch.isnan(y).any())
    assert torch.equal(from_s3(ys, N, K, S2), y.reshape(N, K, S2))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# nc_convT_k2s2_fwd_s3_debug: the three-term output of the fp32 matrix-core kernel (convT_fwd_s3, used by the whole-network calls only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def fwd_s3(x, w, b, ctot, c0, want_y=True):
    N, C, D, H, W = x.shape
    K = w.shape[1]
    y = nan_like(N, K, 2 * D, 2 * H, 2 * W) if want_y else None
    ys = s3_buffer(N, ctot, 8 * D * H * W)
    code = L().nc_convT_k2s2_fwd_s3_debug(P(x), P(w), P(b), P(y), P(ys), ctot, c0, N, C, D, H, W, K, stream())
    torch.cuda.synchronize()
    return code, y, ys


@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('case', R.S3_CASES, ids=[R.case_id(c) for c in R.S3_CASES])
def test_forward_fp32_three_term_output(case, with_bias):
    """Channels [K, 2K) of a 2K-channel S3 tensor: the three terms decode to the y of the same call bit for bit, y meets the fp32 limit, channels
    [0, K) keep the sentinel, and y = NULL gives the same S3 bytes."""
    N, C, K, n = case
    assert branch_fwd(N, C, K, n, None) == 'mfma'
    x, w, b, _ = gpu_inputs(N, C, K, n)
    bb = b if with_bias else None
    S2 = 8 * n[0] * n[1] * n[2]
    code, y, ys = fwd_s3(x, w, bb, 2 * K, K)
    ck(code, 'nc_convT_k2s2_fwd_s3_debug')
    ref = R.ref_fwd(x, w, bb)
    assert not bool(torch.isnan(y).any())
    judge('k_convT_fwd_mfma', '%s %s, with S3 output' % (R.case_id(case), 'bias' if with_bias else 'nobias'), R.err(y, ref),
          R.err(R.oracle_fwd(N, C, K, n, with_bias), ref))
    assert torch.equal(from_s3(ys, N, 2 * K, S2)[:, K:], y.reshape(N, K, S2))
    assert bool((ys[:N * 2 * K * S2 * 6].view(N, 2 * K // 8, 3 * S2 * 16)[:, :K // 8] == SENT).all())
    code, none, ys2 = fwd_s3(x, w, bb, 2 * K, K, want_y=False)
    ck(code, 'nc_convT_k2s2_fwd_s3_debug')
    assert none is None and torch.equal(ys, ys2)


def test_forward_fp32_three_term_output_refuses_what_the_kernel_does_not_cover():
    """C = 256 (the VALU kernel's layer), K % 32 != 0, force-direct, a slice outside the tensor: NC_ERR_SHAPE, nothing written."""
    n = (3, 4, 5)
    for (C, K, ctot, c0, mode) in ((256, 128, 128, 0, None), (128, 48, 48, 0, None), (128, 64, 64, 0, R.DIRECT), (128, 64, 64, 8, None),
                                   (128, 64, 68, 0, None)):
        x, w, b, _ = gpu_inputs(1, C, K, n)
        with dispatch(mode):
            code, y, ys = fwd_s3(x, w, b, ctot, c0)
        assert code == NC_ERR_SHAPE, (C, K, ctot, c0, mode, code)
        assert bool(torch.isnan(y).all()) and bool((ys == SENT).all())
