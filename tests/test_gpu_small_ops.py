"""The four losses and Adam (csrc/misc.hip) and the spectral norm (csrc/spectral.hip), op level, against float64: every loss mode forward and
backward across the wave, workgroup and cdiv(n, 1024) edges, the cap of k_loss_partial at 256 workgroups and the wrap of the backward grid; one
Adam step on both forms of the lerp, at the boundary between them and past the grid wrap, once with p = 0 and lr = 1 (the stored p IS the
update: an error is not hidden under p's ulp) and once with production values; the spectral norm at K = 1, M < 64, K and M past the 1024
threads, M = 16384, without the power iteration and with norms below eps, and its backward with a random, an orthogonal and a parallel G.

The entry points are called through the C ABI directly; the Python layer (GANLoss, ops.spectral_norm_weight) is held to the same references.
References, limits, cases and the reasoning behind them: tests/small_ops_reference.py (checked on the CPU by
tests/test_small_ops_reference.py).  The limits are derived from the kernels' fp32 rounding points, not measured; the module prints the share of
its limit every result uses and, at its end, the worst share per kernel.  Outputs are pre-filled with NaN between NaN guard words, the loss
workspace with NaN too: an element that is not written, or one written outside the tensor, fails.  No element is left out of any comparison.

Worst share of the limit per kernel on an MI355X (max, rms; 1.0 = at the limit): WORST_MEASURED below; the module takes MODULE_SECONDS of
wall time.  The shares near 1.0 (Adam, the l1 and mean
gradients) are results whose limit is one rounding of the stored value, u |ref|: among two million elements some sit at half an ulp just above a
power of two, which is u |ref| to three digits."""
import ctypes
import math
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_ops_reference as R  # noqa: E402

DEV = 'cuda'
NC_ERR_SHAPE, NC_ERR_WS, NC_ERR_ARG = -1, -2, -4
GUARD = 4
WORST = {}
T0 = [None]

# measured on an MI355X (the table this module prints): kernel, max, rms
MODULE_SECONDS = '2.8 s'
WORST_MEASURED = """
  GANLoss lsgan                      max 0.336  rms 0.240
  GANLoss vanilla                    max 0.556  rms 0.182
  GANLoss wgangp                     max 0.406  rms 0.406
  k_adam m (g - (g - m)(1 - wl))     max 0.999  rms 0.281
  k_adam m (m + wl (g - m))          max 0.998  rms 0.296
  k_adam p, production               max 0.998  rms 0.498
  k_adam p, update                   max 0.449  rms 0.263
  k_adam v                           max 0.997  rms 0.293
  k_l1_bwd                           max 0.992  rms 0.940
  k_logit_bwd bce                    max 0.760  rms 0.278
  k_logit_bwd mean                   max 0.992  rms 0.992
  k_loss_partial + k_loss_final bce  max 0.220  rms 0.220
  k_loss_partial + k_loss_final l1   max 0.238  rms 0.238
  k_loss_partial + k_loss_final mean max 0.488  rms 0.488
  k_loss_partial + k_loss_final mse  max 0.266  rms 0.266
  k_mse_bwd                          max 0.631  rms 0.414
  k_spectral_bwd                     max 0.737  rms 0.089
  k_spectral_fwd sigma               max 0.006  rms 0.006
  k_spectral_fwd u                   max 0.013  rms 0.007
  k_spectral_fwd v                   max 0.095  rms 0.034
  k_spectral_fwd w                   max 0.023  rms 0.016
  ops.spectral_norm_weight           max 0.112  rms 0.041
"""


def L():
    from neuroclear_amd._lib import lib
    return lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(code, what):
    assert code == 0, (what, code, L().nc_last_error())


@pytest.fixture(scope='module', autouse=True)
def _worst_table():
    T0[0] = time.time()
    yield
    torch.cuda.synchronize()
    print('\nworst share of the limit per kernel (max, rms; 1.0 = at the limit)')
    for k in sorted(WORST):
        print('  %-36s max %.3f  rms %.3f' % (k, WORST[k][0], WORST[k][1]))
    print('module wall time %.1f s' % (time.time() - T0[0]))


def judge(kernel, what, out, ref, lim, quiet=False):
    sh = R.share(R.diff(out, ref), lim)
    if not quiet:
        print('%-34s %-62s of the limit: max %.3f rms %.3f' % (kernel, what, sh[0], sh[1]))
    w = WORST.get(kernel, (0.0, 0.0))
    WORST[kernel] = (max(w[0], sh[0]), max(w[1], sh[1]))
    assert sh[0] <= 1.0, (kernel, what, sh)


class Out:
    """n elements between NaN guards.  fill=None: a NaN-filled fp32 output; else an in / out operand holding `fill`"""

    def __init__(self, n, fill=None, dtype=torch.float32):
        self.whole = torch.full((n + 2 * GUARD,), math.nan, device=DEV, dtype=dtype)
        self.t = self.whole[GUARD:GUARD + n]
        self.lo, self.hi = self.whole[:GUARD], self.whole[GUARD + n:]
        if fill is not None:
            self.t.copy_(fill.reshape(-1))

    def intact(self):
        return bool(torch.isnan(self.lo).all()) and bool(torch.isnan(self.hi).all())

    def untouched(self):
        return bool(torch.isnan(self.whole).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------------------------------------
def loss_ws(n):
    nb = int(L().nc_loss_ws_bytes(n))
    assert nb == 256 * 8
    return Out(nb // 8, dtype=torch.float64), nb     # NaN partial sums: one that is read without having been written poisons the loss


def call_loss_fwd(mode, a, b, target, n, out, ws, nb):
    if mode == 'mse':
        return L().nc_mse_const_fwd(P(a), n, target, P(out), P(ws), nb, stream())
    if mode == 'bce':
        return L().nc_bce_logits_const_fwd(P(a), n, target, P(out), P(ws), nb, stream())
    if mode == 'mean':
        return L().nc_mean_fwd(P(a), n, P(out), P(ws), nb, stream())
    return L().nc_l1_fwd(P(a), P(b), n, P(out), P(ws), nb, stream())


def call_loss_bwd(mode, a, b, target, n, gs, dp):
    if mode == 'mse':
        return L().nc_mse_const_bwd(P(a), n, target, P(gs), P(dp), stream())
    if mode == 'bce':
        return L().nc_bce_logits_const_bwd(P(a), n, target, P(gs), P(dp), stream())
    if mode == 'mean':
        return L().nc_mean_bwd(n, P(gs), P(dp), stream())
    return L().nc_l1_bwd(P(a), P(b), n, P(gs), P(dp), stream())


KERNEL_F = {m: 'k_loss_partial + k_loss_final ' + m for m in R.LOSS_MODES}
KERNEL_B = {'mse': 'k_mse_bwd', 'l1': 'k_l1_bwd', 'bce': 'k_logit_bwd bce', 'mean': 'k_logit_bwd mean'}


@pytest.mark.parametrize('n', R.LOSS_SIZES)
@pytest.mark.parametrize('mode', R.LOSS_MODES)
def test_losses_against_fp64(mode, n):
    """every target with every gscale up to n = 1025; above, target k with gscale k.  (l1 and mean take no target: one input, every gscale.)"""
    pairs = [(t, g) for t in R.TARGETS for g in R.GSCALES] if n <= 1025 else list(zip(R.TARGETS, R.GSCALES))
    if mode in ('l1', 'mean'):
        pairs = [(0.0, g) for g in R.GSCALES]
    done_f = set()
    for target, gscale in pairs:
        a, b = (t.to(DEV) if t is not None else None for t in R.loss_inputs(mode, n, target))
        what = 'n %d target %.1f gscale %.2f' % (n, target, gscale)
        if target not in done_f:
            done_f.add(target)
            ws, nb = loss_ws(n)
            out = Out(1)
            ok(call_loss_fwd(mode, a, b, target, n, out.t, ws.t, nb), mode + ' forward')
            ref, lim = R.loss_fwd(mode, a, b, target)
            assert out.intact() and ws.intact()
            judge(KERNEL_F[mode], what, out.t, ref.reshape(1), lim.reshape(1))
            used = min(-(-n // 1024), 256)     # the partials in use are written, the others are not touched
            assert not bool(torch.isnan(ws.t[:used]).any()) and bool(torch.isnan(ws.t[used:]).all())
        gs = torch.tensor([gscale], device=DEV)
        dp = Out(n)
        ok(call_loss_bwd(mode, a, b, target, n, gs, dp.t), mode + ' backward')
        gref, glim = R.loss_bwd(mode, a, b, target, gscale)
        assert dp.intact()
        judge(KERNEL_B[mode], what, dp.t, gref, glim)
        if mode == 'l1' and n >= 20:     # exact zeros where a == b, a gradient where they differ by a denormal
            assert bool((dp.t[::10] == 0).all()) and bool((dp.t[5::20] * gscale > 0).all()) and bool((dp.t[15::20] * gscale < 0).all())


@pytest.mark.parametrize('mode', R.LOSS_MODES)
def test_one_nan_in_the_input_gives_a_nan_loss(mode):
    for n, at in ((1025, 1024), (262145, 262144), (262145, 77)):
        a, b = (t.to(DEV).clone() if t is not None else None for t in R.loss_inputs(mode, n, 0.0))
        a[at] = math.nan
        ws, nb = loss_ws(n)
        out = Out(1)
        ok(call_loss_fwd(mode, a, b, 0.0, n, out.t, ws.t, nb), mode)
        assert out.intact() and math.isnan(float(out.t))
        a[at] = 0.5
        out.t.fill_(math.nan)
        ok(call_loss_fwd(mode, a, b, 0.0, n, out.t, ws.t, nb), mode)
        assert math.isfinite(float(out.t))


def test_losses_refuse_bad_arguments():
    """null pointers: NC_ERR_ARG; n < 1: NC_ERR_SHAPE; a workspace that is missing or one byte short: NC_ERR_WS; nothing is written"""
    n = 257
    a, b = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    gs = torch.ones(1, device=DEV)
    ws, nb = loss_ws(n)
    out, dp = Out(1), Out(n)
    for mode in R.LOSS_MODES:
        assert call_loss_fwd(mode, None, b, 0.0, n, out.t, ws.t, nb) == NC_ERR_ARG, mode
        assert call_loss_fwd(mode, a, b, 0.0, n, None, ws.t, nb) == NC_ERR_ARG, mode
        for bad_n in (0, -5):
            assert call_loss_fwd(mode, a, b, 0.0, bad_n, out.t, ws.t, nb) == NC_ERR_SHAPE, mode
            assert call_loss_bwd(mode, a, b, 0.0, bad_n, gs, dp.t) == NC_ERR_SHAPE, mode
        assert call_loss_fwd(mode, a, b, 0.0, n, out.t, ws.t, nb - 1) == NC_ERR_WS, mode
        assert call_loss_fwd(mode, a, b, 0.0, n, out.t, None, nb) == NC_ERR_WS, mode
        assert call_loss_bwd(mode, a, b, 0.0, n, None, dp.t) == NC_ERR_ARG, mode
        assert call_loss_bwd(mode, a, b, 0.0, n, gs, None) == NC_ERR_ARG, mode
        if mode != 'mean':
            assert call_loss_bwd(mode, None, b, 0.0, n, gs, dp.t) == NC_ERR_ARG, mode
    assert L().nc_l1_fwd(P(a), P(None), n, P(out.t), P(ws.t), nb, stream()) == NC_ERR_ARG
    assert L().nc_l1_bwd(P(a), P(None), n, P(gs), P(dp.t), stream()) == NC_ERR_ARG
    torch.cuda.synchronize()
    assert out.untouched() and dp.untouched() and ws.untouched()


@pytest.mark.parametrize('target_is_real', [True, False])
@pytest.mark.parametrize('gan_mode', ['lsgan', 'vanilla', 'wgangp'])
def test_ganloss_against_fp64(gan_mode, target_is_real):
    """GANLoss with target_real_label = 0.9: the label the mode's kernel receives, and the sign of the wgan mean and of its gradient"""
    from neuroclear_amd.models.networks import GANLoss
    mode = {'lsgan': 'mse', 'vanilla': 'bce', 'wgangp': 'mean'}[gan_mode]
    target = 0.9 if target_is_real else 0.0
    a, _ = R.loss_inputs(mode, 2 * 7 * 9, target)
    pred = a.to(DEV).view(2, 1, 7, 9).requires_grad_(True)
    crit = GANLoss(gan_mode, target_real_label=0.9).to(DEV)
    loss = crit(pred, target_is_real)
    (grad,) = torch.autograd.grad(loss * 0.37, pred)
    sign = -1.0 if (mode == 'mean' and target_is_real) else 1.0
    ref, lim = R.loss_fwd(mode, a, None, target)
    gref, glim = R.loss_bwd(mode, a, None, target, sign * 0.37)
    what = '%s target_is_real %s' % (gan_mode, target_is_real)
    judge('GANLoss ' + gan_mode, what, loss.detach().cpu().reshape(1), sign * ref.reshape(1), lim.reshape(1))
    judge('GANLoss ' + gan_mode, what + ' gradient', grad.reshape(-1).cpu(), gref, glim)
    if mode == 'mean':     # 1000 + noise: the sign is not in doubt
        assert float(loss.detach()) * sign > 900 and bool((grad * sign > 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------------------------
def run_adam(case, p_mode, quiet):
    n, b1, b2, step, eps = case
    p, g, m, v = (t.to(DEV) for t in R.adam_inputs(n))
    lr = R.ADAM_LR
    if p_mode == 'update':
        p, lr = torch.zeros_like(p), 1.0
    po, mo, vo = Out(n, p), Out(n, m), Out(n, v)
    ok(L().nc_adam_step(P(po.t), P(g), P(mo.t), P(vo.t), n, lr, b1, b2, eps, step, stream()), 'nc_adam_step')
    ref = R.adam_ref(p, g, m, v, lr, b1, b2, eps, step)
    assert po.intact() and mo.intact() and vo.intact()
    form = 'm + wl (g - m)' if R.f32(1.0) - R.f32(b1) < 0.5 else 'g - (g - m)(1 - wl)'
    what = 'n %d beta %.1f %.3f step %d eps %.0e %s' % (n, b1, b2, step, eps, p_mode)
    for name, o in (('p', po), ('m', mo), ('v', vo)):
        judge('k_adam %s%s' % (name, ' (' + form + ')' if name == 'm' else ', ' + p_mode if name == 'p' else ''), what, o.t, *ref[name], quiet=quiet)
    if n >= 7 and p_mode == 'update':
        # g = +-1e-30 at v = 0: g^2 underflows, the denominator is eps alone; the all-zero element stays zero
        upd = ref['m'][0][1:3] * (R.f32(lr) / (1.0 - R.f32(b1) ** step)) / R.f32(eps)
        assert float(vo.t[1]) == 0.0 and float(vo.t[2]) == 0.0 and float(po.t[6]) == 0.0
        assert float((po.t[1:3].double() + upd).abs().max()) <= 8 * R.U * float(upd.abs().max()) + R.TINY


@pytest.mark.parametrize('n', R.ADAM_SIZES)
def test_adam_step_against_fp64(n):
    """every (beta1, beta2, step, eps) at n = 1 and 257; at the size that wraps the grid every value of each, once.  Each case twice: p = 0 and
    lr = 1, and p ~ 0.05, lr = 1e-4"""
    cases = [c for c in R.ADAM_SMALL + R.ADAM_LARGE if c[0] == n]
    assert cases
    for case in cases:
        for p_mode in ('update', 'production'):
            run_adam(case, p_mode, quiet=n < R.ADAM_SIZES[-1] and not (case[2] == 0.999 and case[4] == 1e-8 and case[3] in (1, 100000)))


def test_adam_refuses_bad_arguments():
    n = 257
    p, g, m, v = (t.to(DEV) for t in R.adam_inputs(n))
    po, mo, vo = Out(n, p), Out(n, m), Out(n, v)
    args = (n, 1e-4, 0.9, 0.999, 1e-8)
    assert L().nc_adam_step(P(po.t), P(g), P(mo.t), P(vo.t), *args, 0, stream()) == NC_ERR_SHAPE       # step < 1
    assert L().nc_adam_step(P(po.t), P(g), P(mo.t), P(vo.t), *args, -3, stream()) == NC_ERR_SHAPE
    assert L().nc_adam_step(P(po.t), P(g), P(mo.t), P(vo.t), 0, *args[1:], 1, stream()) == NC_ERR_SHAPE   # n < 1
    assert L().nc_adam_step(P(po.t), P(g), P(mo.t), P(vo.t), -1, *args[1:], 1, stream()) == NC_ERR_SHAPE
    for k in range(4):
        ptrs = [P(po.t), P(g), P(mo.t), P(vo.t)]
        ptrs[k] = P(None)
        assert L().nc_adam_step(*ptrs, *args, 1, stream()) == NC_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(po.t, p) and torch.equal(mo.t, m) and torch.equal(vo.t, v) and po.intact() and mo.intact() and vo.intact()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# spectral norm
# ---------------------------------------------------------------------------------------------------------------------------------------------
def run_spectral_fwd(W, u, v, pi):
    K, M = W.shape
    uo, vo = Out(K, u), Out(M, v)
    w, sigma, scratch = Out(K * M), Out(1), Out(K)
    ok(L().nc_spectral_norm_fwd(P(W), P(uo.t), P(vo.t), P(w.t), P(sigma.t), P(scratch.t), K, M, pi, R.SN_EPS, stream()), 'nc_spectral_norm_fwd')
    torch.cuda.synchronize()
    assert all(o.intact() for o in (uo, vo, w, sigma, scratch))
    return uo.t, vo.t, sigma.t, w.t.view(K, M)


SPECTRAL_IDS = ['x'.join(str(v) for v in c) for c in R.SPECTRAL_CASES + [R.SPECTRAL_TINY]]


@pytest.mark.parametrize('pi', [1, 0], ids=['power_iteration', 'no_power_iteration'])
@pytest.mark.parametrize('case', R.SPECTRAL_CASES + [R.SPECTRAL_TINY], ids=SPECTRAL_IDS)
def test_spectral_norm_against_fp64(case, pi):
    K, M = case[:2]
    W, u, v, G = (t.to(DEV) for t in R.spectral_inputs(*case))
    cid = '%s power_iteration %d' % ('x'.join(str(c) for c in case), pi)
    uo, vo, sigma, w = run_spectral_fwd(W, u, v, pi)
    ref, norms = R.spectral_fwd_ref(W, u, v, pi)
    if pi:
        judge('k_spectral_fwd v', cid, vo, *ref['v'])
        judge('k_spectral_fwd u', cid, uo, *ref['u'])
        if len(case) == 3:     # both norms below eps: v = W^T u / eps, u = W v / eps, nowhere near unit length
            assert max(norms) < 0.5 * R.SN_EPS and float(vo.norm()) < 1e-3 and float(uo.norm()) < 1e-3
        else:
            assert abs(float(vo.double().norm()) - 1.0) < 1e-5 and abs(float(uo.double().norm()) - 1.0) < 1e-5
    else:
        assert torch.equal(uo, u) and torch.equal(vo, v)     # bit-equal: not written, or written with themselves
    judge('k_spectral_fwd sigma', cid, sigma, *ref['sigma'])
    judge('k_spectral_fwd w', cid, w, *ref['w'])
    assert not bool(torch.isnan(w).any())
    if len(case) == 3:
        return     # (sigma ~ 1e-40: no backward is asked of it)
    for kind in ('random', 'orthogonal', 'parallel'):
        Gk = R.spectral_G(kind, G, w)
        dw = Out(K * M)
        ok(L().nc_spectral_norm_bwd(P(Gk), P(w), P(uo), P(vo), P(sigma), P(dw.t), K, M, stream()), 'nc_spectral_norm_bwd')
        bref, blim = R.spectral_bwd_ref(Gk, w, uo, vo, sigma)
        assert dw.intact()
        judge('k_spectral_bwd', '%s G %s' % (cid, kind), dw.t.view(K, M), bref, blim)
        c = float((Gk.double() * w.double()).sum())
        if kind == 'orthogonal':
            assert abs(c) <= 1e-5 * float((Gk.double() * w.double()).abs().sum())
        if kind == 'parallel' and K * M > 1:
            assert c > 0


def test_spectral_norm_refuses_bad_arguments():
    K, M = 3, 5
    W, u, v, G = (t.to(DEV) for t in R.spectral_inputs(K, M))
    uo, vo, w, sigma, scratch, dw = Out(K, u), Out(M, v), Out(K * M), Out(1), Out(K), Out(K * M)
    ptrs = [P(W), P(uo.t), P(vo.t), P(w.t), P(sigma.t), P(scratch.t)]
    for k in range(6):
        q = list(ptrs)
        q[k] = P(None)
        assert L().nc_spectral_norm_fwd(*q, K, M, 1, R.SN_EPS, stream()) == NC_ERR_ARG
    assert L().nc_spectral_norm_fwd(*ptrs, 0, M, 1, R.SN_EPS, stream()) == NC_ERR_SHAPE
    assert L().nc_spectral_norm_fwd(*ptrs, K, 0, 1, R.SN_EPS, stream()) == NC_ERR_SHAPE
    one = torch.ones(1, device=DEV)
    bptrs = [P(G), P(W), P(u), P(v), P(one), P(dw.t)]
    for k in range(6):
        q = list(bptrs)
        q[k] = P(None)
        assert L().nc_spectral_norm_bwd(*q, K, M, stream()) == NC_ERR_ARG
    assert L().nc_spectral_norm_bwd(*bptrs, K, -1, stream()) == NC_ERR_SHAPE
    torch.cuda.synchronize()
    assert torch.equal(uo.t, u) and torch.equal(vo.t, v) and all(o.untouched() for o in (w, sigma, scratch, dw))


@pytest.mark.parametrize('kind', ['4-D', '5-D', 'non-contiguous'])
def test_spectral_norm_weight_against_fp64(kind):
    """ops.spectral_norm_weight: forward (u, v updated in place) and autograd.grad.  The op does not hand out its sigma: the gradient is held
    to the reference at the float64 sigma, its limit widened by sigma's own (dW is proportional to 1 / sigma)"""
    from neuroclear_amd import ops
    shape = {'4-D': (8, 4, 3, 3), '5-D': (6, 2, 3, 3, 3), 'non-contiguous': (8, 4, 3, 3)}[kind]
    K = shape[0]
    M = math.prod(shape[1:])
    W, u, v, G = R.spectral_inputs(K, M)
    if kind == 'non-contiguous':
        base = W.view(shape).transpose(0, 1).contiguous().to(DEV)
        w_orig = base.transpose(0, 1).requires_grad_(True)
        assert not w_orig.is_contiguous()
    else:
        w_orig = W.view(shape).to(DEV).requires_grad_(True)
    assert torch.equal(w_orig.detach().cpu().reshape(K, M), W)
    ub, vb = u.to(DEV).clone(), v.to(DEV).clone()
    w = ops.spectral_norm_weight(w_orig, ub, vb, True)
    (dW,) = torch.autograd.grad(w, w_orig, G.view(shape).to(DEV))
    assert w.shape == tuple(shape) and dW.shape == tuple(shape)
    ref, _ = R.spectral_fwd_ref(W, u, v, 1)
    what = 'spectral_norm_weight ' + kind
    judge('ops.spectral_norm_weight', what + ' u', ub.cpu(), *ref['u'])
    judge('ops.spectral_norm_weight', what + ' v', vb.cpu(), *ref['v'])
    judge('ops.spectral_norm_weight', what + ' w', w.detach().cpu().reshape(K, M), *ref['w'])
    sref, slim = ref['sigma']
    bref, blim = R.spectral_bwd_ref(G, w.detach().cpu().reshape(K, M), ub.cpu(), vb.cpu(), sref)
    judge('ops.spectral_norm_weight', what + ' dW', dW.cpu().reshape(K, M), bref, blim + bref.abs() * (slim / sref.abs() + R.U))
