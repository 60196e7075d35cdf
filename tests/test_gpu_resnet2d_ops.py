"""The kernels of the ResNet generators, op level (csrc/conv2d_k3.hip's reflect mode, csrc/resnet2d.hip), each against float64.

REFLECT CONVOLUTION (nc_conv2d_k3_reflect_fwd / _dgrad): reference, yardstick (the one-accumulator fp32 chain in the kernel's order, the data
gradient's through the documented fold), error measure, limit (FACTOR 3 with tests/convt_reference.py's floors) and cases:
tests/resnet2d_reference.py.  Which path a call takes is asked of the library (nc_conv2d_k3_reflect_active) and held to the zero-padded kernel's
coverage rule (conv2d_reference.k3_covered).  Outputs are NaN-filled with guard elements behind them; the workspace has a guard behind it too.

PAD KERNELS: the forward is a copy (torch.equal); the backward is an fp32 sum of t <= 9 terms: per element within (t - 1) 2^-24 sum|terms| of
float64.

nc_instnorm_res_fwd, y = skip + (x - mean) rstd: the existing bound of nc_instnorm_act_fwd (tests/norm_reference.py in_fwd: 4 u (|xhat| +
rstd |mean|)) covers the normalised term; the residual add is one more correctly rounded fp32 operation on a DIFFERENT magnitude, so its half ulp
u |y| is added -- without it no fp32 output could meet the bound wherever |skip| is large against |xhat| (y = 3 is stored to within 2 u, the
bare bound there is u).  Both shares are printed; measured on an MI355X: of the bare norm bound max 12.8 at (6, 35) and 2.1 at (128, 8192), with
the half ulp of the sum 0.74 and 0.66.

DROPOUT: exact statements only (identity in eval(), survivors 2 x, dx = 2 dy mask, the seed fixes the mask) and the zero fraction within five
standard deviations of a fair coin."""
import contextlib
import functools
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_reference as NR  # noqa: E402
import resnet2d_reference as R  # noqa: E402

DEV = 'cuda'
GUARD = 64
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
def k3(on=1, cfg=-1):
    prev = L().nc_get_conv2d_k3()
    L().nc_set_conv2d_k3(on)
    L().nc_conv2d_k3_set_cfg(cfg)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        L().nc_set_conv2d_k3(prev)
        L().nc_conv2d_k3_set_cfg(-1)


@pytest.fixture(scope='module', autouse=True)
def _worst_table():
    yield
    print('\nworst use of the limit per path (max, rms; 1.0 = at the limit)')
    for k in sorted(WORST):
        print('  %-28s max %.3f  rms %.3f' % (k, WORST[k][0], WORST[k][1]))


def out_buffer(shape):
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), float('nan'), device=DEV)
    return buf, buf[:n].view(shape)


def intact(buf, out):
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()), 'an output element was not written'
    assert bool(torch.isnan(buf[out.numel():]).all()), 'a write past the end of the output'


@functools.lru_cache(maxsize=None)
def gpu_inputs(N, C, K, H, W):
    return tuple(t.to(DEV) for t in R.inputs3(N, C, K, H, W))


@functools.lru_cache(maxsize=None)
def reference(what, N, C, K, H, W):
    """(float64 reference, (max, rms) of the fp32 chain against it), on the GPU, once per shape; the forward reference carries the bias."""
    x, w, b, dy = gpu_inputs(N, C, K, H, W)
    if what == 0:
        ref = R.refr_fwd(x, w, b)
        return ref, R.err(R.chainr_fwd(x, w, b), ref)
    ref = R.refr_dgrad(dy, w)
    return ref, R.err(R.chainr_dgrad(dy, w), ref)


def judge(path, what, got, orc):
    r = R.ratios(got, orc)
    print('%-14s %-34s product max %.2e rms %.2e | chain max %.2e rms %.2e | of the limit %.3f %.3f' % (path, what, got[0], got[1], orc[0], orc[1], r[0], r[1]))
    if math.isfinite(r[0]) and math.isfinite(r[1]):
        w = WORST.get(path, (0.0, 0.0))
        WORST[path] = (max(w[0], r[0]), max(w[1], r[1]))
    assert R.within(got, orc), (path, what, got, orc)


def run(what, N, C, K, H, W):
    """nc_conv2d_k3_reflect_fwd (what 0, with bias) or _dgrad (what 1) under the current switches -> the output, checked for unwritten elements
    and writes past its end or past the end of the workspace."""
    x, w, b, dy = gpu_inputs(N, C, K, H, W)
    nb = int(L().nc_conv2d_k3_reflect_ws_bytes(N, C, H, W, K))
    assert nb >= N * C * (H + 2) * (W + 2) * 4
    ws = torch.full((nb + 4 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    buf, out = out_buffer((N, K if what == 0 else C, H, W))
    if what == 0:
        ck(L().nc_conv2d_k3_reflect_fwd(P(x), P(w), P(b), P(out), N, C, H, W, K, P(ws), nb, stream()), 'nc_conv2d_k3_reflect_fwd')
    else:
        ck(L().nc_conv2d_k3_reflect_dgrad(P(dy), P(w), P(out), N, C, H, W, K, P(ws), nb, stream()), 'nc_conv2d_k3_reflect_dgrad')
    intact(buf, out)
    assert bool((ws[nb:] == 0xA5).all()), 'a write past the end of the workspace'
    return out


def active(what, N, C, K, H, W):
    return L().nc_conv2d_k3_reflect_active(what, N, C, H, W, K)


@pytest.mark.parametrize('what', [0, 1], ids=['fwd', 'dgrad'])
@pytest.mark.parametrize('case', R.KR_CASES, ids=[R.case_id(c[:5]) for c in R.KR_CASES])
def test_reflect_convolution_against_fp64_switch_on_and_off(case, what):
    """Every case is covered by the tiled kernel (asserted, and equal to the coverage rule); with the switch off the same entry point pads
    explicitly.  Both meet the limit; two runs are bit-equal; the first case runs under both pinned tile configurations with equal bits."""
    N, C, K, H, W = case[:5]
    assert R.k3_covered(what, N, C, K, H, W) and active(what, N, C, K, H, W) == 1
    ref, orc = reference(what, N, C, K, H, W)
    name = '%s %s' % (R.case_id(case[:5]), 'fwd' if what == 0 else 'dgrad')
    with k3(on=1):
        y = run(what, N, C, K, H, W)
        judge('k_conv2d_k3 reflect', name, R.err(y, ref), orc)
        assert torch.equal(y, run(what, N, C, K, H, W))
    if case is R.KR_CASES[0]:
        for cfg in range(L().nc_conv2d_k3_num_cfgs()):
            with k3(on=1, cfg=cfg):
                assert torch.equal(run(what, N, C, K, H, W), y), 'tile configuration %d' % cfg
    with k3(on=0):
        assert active(what, N, C, K, H, W) == 0
        judge('explicit pad', name + ' (switch off)', R.err(run(what, N, C, K, H, W), ref), orc)


@pytest.mark.parametrize('case', R.KR_OUTSIDE, ids=[R.case_id(c[:5]) for c in R.KR_OUTSIDE])
def test_shapes_outside_the_coverage_report_zero_and_still_compute(case):
    N, C, K, H, W = case[:5]
    assert not R.k3_covered(0, N, C, K, H, W)
    for what in (0, 1):
        covered = R.k3_covered(what, N, C, K, H, W)
        assert active(what, N, C, K, H, W) == (1 if covered else 0)
        ref, orc = reference(what, N, C, K, H, W)
        name = '%s %s' % (R.case_id(case[:5]), 'fwd' if what == 0 else 'dgrad')
        judge('k_conv2d_k3 reflect' if covered else 'explicit pad', name, R.err(run(what, N, C, K, H, W), ref), orc)
        with k3(on=0):
            assert active(what, N, C, K, H, W) == 0
            judge('explicit pad', name + ' (switch off)', R.err(run(what, N, C, K, H, W), ref), orc)
    assert active(0, N, C, K, H, W) == 0
    assert active(2, N, C, K, H, W) == 0 and L().nc_conv2d_k3_reflect_active(0, 16, 64, 1, 517, 64) == 0     # no such query; H = 1 has no mirror


def test_weight_gradient_pads_explicitly():
    """nc_conv2d_k3_reflect_wgrad = the padded input through nc_conv_wgrad with padding 0: against float64 autograd, with the bias gradient."""
    N, C, K, H, W = 2, 64, 64, 21, 35
    x, w, b, dy = gpu_inputs(N, C, K, H, W)
    xp = R.reflect_pad(x, 1).double()
    ref = torch.einsum('nkuv,ncuvab->kcab', dy.double(), xp.unfold(2, 3, 1).unfold(3, 3, 1))
    nb = int(L().nc_conv2d_k3_reflect_ws_bytes(N, C, H, W, K))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    bw, dw = out_buffer((K, C, 3, 3))
    bb, db = out_buffer((K,))
    ck(L().nc_conv2d_k3_reflect_wgrad(P(x), P(dy), P(dw), P(db), N, C, H, W, K, P(ws), nb, stream()), 'nc_conv2d_k3_reflect_wgrad')
    intact(bw, dw)
    intact(bb, db)
    # yardstick: the one-accumulator fp32 chain over (n, u, v), 1470 terms
    xg = R.reflect_pad(x, 1)
    cw = torch.zeros(K, C, 3, 3, device=DEV)
    cb = torch.zeros(K, device=DEV)
    for n in range(N):
        for u in range(H):
            for v in range(W):
                cw = cw + dy[n, :, u, v].view(K, 1, 1, 1) * xg[n, :, u:u + 3, v:v + 3].reshape(1, C, 3, 3)
                cb = cb + dy[n, :, u, v]
    judge('wgrad, explicit pad', 'dw', R.err(dw, ref), R.err(cw, ref))
    refb = dy.double().sum((0, 2, 3))
    judge('wgrad, explicit pad', 'dbias', R.err(db, refb), R.err(cb, refb))


# ---- the pad kernels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('NC,H,W,p', R.PAD_CASES)
def test_reflect_pad_forward_is_a_copy_and_backward_an_fp32_sum(NC, H, W, p):
    g = torch.Generator().manual_seed(NC * 1000 + H * 10 + W + p)
    x = torch.randn(NC, H, W, generator=g).to(DEV)
    gy = torch.randn(NC, H + 2 * p, W + 2 * p, generator=g).to(DEV)
    by, y = out_buffer((NC, H + 2 * p, W + 2 * p))
    ck(L().nc_reflect_pad2d_fwd(P(x), P(y), NC, H, W, p, stream()), 'nc_reflect_pad2d_fwd')
    intact(by, y)
    assert torch.equal(y, R.reflect_pad(x, p))
    bd, dx = out_buffer((NC, H, W))
    ck(L().nc_reflect_pad2d_bwd(P(gy), P(dx), NC, H, W, p, stream()), 'nc_reflect_pad2d_bwd')
    intact(bd, dx)
    ref = R.reflect_fold(gy.double(), H, W, p)
    lim = (R.fold_terms(H, W, p, DEV) - 1).double() * NR.U * R.reflect_fold(gy.double().abs(), H, W, p)
    s = NR.share((dx.double() - ref).abs(), lim)
    print('reflect_pad2d_bwd %s: of the limit max %.3f rms %.3f' % ((NC, H, W, p), s[0], s[1]))
    assert s[0] <= 1.0
    assert torch.equal(dx, R.reflect_fold(gy, H, W, p)), 'the documented summation order'


def test_pad_kernels_refuse_what_they_do_not_cover():
    x = torch.zeros(64, device=DEV)
    by, y = out_buffer((256,))
    for (H, W, p) in ((3, 3, 3), (4, 1, 1), (4, 4, 2), (4, 4, 0)):
        assert L().nc_reflect_pad2d_fwd(P(x), P(y), 1, H, W, p, stream()) != 0
        assert L().nc_reflect_pad2d_bwd(P(y), P(x), 1, H, W, p, stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(by).all())


# ---- the tail of a block --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('NC,S', [(6, 35), (128, 64 * 128)])
def test_instnorm_res_fwd_against_fp64(NC, S):
    g = torch.Generator().manual_seed(NC * 7 + S)
    x = (torch.randn(NC, S, generator=g) * 2.0 + 0.5).to(DEV)
    skip = torch.randn(NC, S, generator=g).to(DEV)
    ws = torch.empty(max(int(L().nc_instnorm_ws_bytes(NC, S)), 256), dtype=torch.uint8, device=DEV)
    mean, rstd = torch.empty(NC, device=DEV), torch.empty(NC, device=DEV)
    ck(L().nc_instnorm_stats(P(x), NC, S, NR.EPS, P(mean), P(rstd), P(ws), ws.numel(), stream()), 'nc_instnorm_stats')
    by, y = out_buffer((NC, S))
    ck(L().nc_instnorm_res_fwd(P(x), P(mean), P(rstd), P(skip), P(y), NC, S, stream()), 'nc_instnorm_res_fwd')
    intact(by, y)
    xhat, lim = NR.in_fwd(x, mean, rstd, 1.0)
    ref = skip.double() + xhat
    e = (y.double() - ref).abs()
    bare, full = NR.share(e, lim), NR.share(e, lim + NR.U * ref.abs())
    print('instnorm_res_fwd (%d, %d): of the norm bound alone max %.3f rms %.3f; with the half ulp of the sum max %.3f rms %.3f' % (NC, S, *bare, *full))
    assert full[0] <= 1.0
    # slope 1 is the identity activation of the existing kernel, bit for bit (the second norm of a batch-norm block relies on the same form)
    ya = torch.empty_like(x)
    ck(L().nc_instnorm_act_fwd(P(x), P(mean), P(rstd), 1.0, P(ya), NC, S, stream()), 'nc_instnorm_act_fwd')
    torch.cuda.synchronize()
    assert torch.equal(ya, (x - mean[:, None]) * rstd[:, None])


# ---- dropout --------------------------------------------------------------------------------------------------------------------------------
def test_dropout():
    from neuroclear_amd.models import networks
    g = torch.Generator().manual_seed(11)
    x = (1.0 + torch.rand(2, 64, 32, 40, generator=g)).to(DEV)
    dy = (1.0 + torch.rand(2, 64, 32, 40, generator=g)).to(DEV)
    n = x.numel()
    assert n == 163840
    drop = networks.Dropout(0.5)
    drop.eval()
    assert torch.equal(drop(x), x)
    drop.train()
    torch.manual_seed(1234)
    xg = x.clone().requires_grad_(True)
    y = drop(xg)
    mask = y != 0
    zeros = 1.0 - float(mask.double().mean())
    print('dropout: zero fraction %.5f (0.5 +- %.5f)' % (zeros, 5 * 0.5 / math.sqrt(n)))
    assert abs(zeros - 0.5) <= 5 * 0.5 / math.sqrt(n)
    assert torch.equal(y, torch.where(mask, 2.0 * x, torch.zeros_like(x)))
    y.backward(dy)
    assert torch.equal(xg.grad, torch.where(mask, 2.0 * dy, torch.zeros_like(dy)))
    torch.manual_seed(1234)
    assert torch.equal(drop(x), y.detach())
    torch.manual_seed(1235)
    assert not torch.equal(drop(x) != 0, mask)
