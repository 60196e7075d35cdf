"""CPU: the references and limits of the op-level tests of the losses, Adam and the spectral norm (tests/small_ops_reference.py) are themselves
checked -- the closed forms against torch's float64 operators, autograd, torch.optim.Adam and torch.nn.utils.spectral_norm; the derived limits
against a numpy fp32 restatement of each kernel (met on every case) and against the named wrong variants of it (each missed on at least one
case), so the limits have teeth before any GPU run."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_ops_reference as R  # noqa: E402

SMALL = R.LOSS_SIZES[:8]


def _close(a, r, tol=1e-12):
    a, r = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(r, dtype=torch.float64)
    assert a.shape == r.shape
    assert float((a - r).abs().max()) <= tol * max(float(r.abs().max()), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the closed forms are torch's float64 operators
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('target', R.TARGETS)
@pytest.mark.parametrize('mode', R.LOSS_MODES)
def test_loss_references_are_float64_autograd(mode, target):
    n, gscale = 257, 0.37
    a, b = R.loss_inputs(mode, n, target)
    x = a.double().requires_grad_(True)
    t = torch.full_like(x, R.f32(target))
    if mode == 'mse':
        want = F.mse_loss(x, t)
    elif mode == 'l1':
        want = F.l1_loss(x, b.double())
    elif mode == 'bce':
        want = F.binary_cross_entropy_with_logits(x, t)
    else:
        want = x.mean()
    (gx,) = torch.autograd.grad(want * R.f32(gscale), x)
    ref, lim = R.loss_fwd(mode, a, b, target)
    _close(ref, want.detach())
    assert float(lim) > 0
    gref, glim = R.loss_bwd(mode, a, b, target, gscale)
    _close(gref, gx)
    assert bool((glim > 0).all())
    if mode == 'l1':    # the pairs that are equal get no gradient, the denormal differences do
        assert bool((gref[::10] == 0).all()) and bool((gref[5::20] > 0).all()) and bool((gref[15::20] < 0).all())
        assert float((a[5::20] - b[5::20]).abs().max()) < R.MINN


@pytest.mark.parametrize('b1', R.ADAM_BETA1)
@pytest.mark.parametrize('step', (1, 2, 10))
def test_adam_reference_is_torch_optim_adam_in_float64(b1, step):
    """`step` steps of torch.optim.Adam on a float64 copy; the reference restates the last one from the state before it"""
    b2, eps, lr = 0.999, 1e-8, R.ADAM_LR
    p0, g, _, _ = R.adam_inputs(257)
    w = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([w], lr=R.f32(lr), betas=(R.f32(b1), R.f32(b2)), eps=R.f32(eps))
    gen = torch.Generator().manual_seed(step)
    for k in range(step):
        if k == step - 1:
            st = opt.state[w]
            before = (w.detach().clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone()) if st else (w.detach().clone(), torch.zeros_like(w), torch.zeros_like(w))
            gk = g.double()
        else:
            gk = torch.randn(257, generator=gen, dtype=torch.float64)
        w.grad = gk.clone()
        opt.step()
    # the reference takes fp32 operands: hand it the float64 state through a float64-preserving path
    ref = R.adam_ref(*(_Exact(t) for t in (before[0], g.double(), before[1], before[2])), lr, b1, b2, eps, step)
    _close(ref['p'][0], w.detach(), 1e-11)
    _close(ref['m'][0], opt.state[w]['exp_avg'], 1e-11)
    _close(ref['v'][0], opt.state[w]['exp_avg_sq'], 1e-11)
    assert all(bool((ref[k][1] > 0).all()) for k in 'pmv')


class _Exact:
    """a float64 tensor that answers .double() with itself (adam_ref calls it on its fp32 operands)"""

    def __init__(self, t):
        self.t = t

    def double(self):
        return self.t

    @property
    def shape(self):
        return self.t.shape


@pytest.mark.parametrize('shape', [(6, 5), (4, 3, 2, 2)])
def test_spectral_reference_is_torch_spectral_norm(shape):
    """one power iteration of torch.nn.utils.spectral_norm in float64 from an UNNORMALISED u, and autograd through W / (u^T W v) with u and v
    detached (what torch's forward does)"""
    K = shape[0]
    M = int(torch.tensor(shape[1:]).prod())
    W, u, v, G = (t.double() for t in R.spectral_inputs(K, M))
    lin = torch.nn.Linear(M, K, bias=False).double() if len(shape) == 2 else torch.nn.Conv2d(shape[1], K, shape[2], bias=False).double()
    lin = torch.nn.utils.spectral_norm(lin, n_power_iterations=1, eps=R.f32(R.SN_EPS))
    with torch.no_grad():
        lin.weight_orig.copy_(W.view(shape))
        lin.weight_u.copy_(u)
        lin.weight_v.copy_(v)
    lin.train()
    x = torch.zeros(1, M, dtype=torch.float64) if len(shape) == 2 else torch.zeros(1, shape[1], shape[2], shape[3], dtype=torch.float64)
    lin(x)     # the forward pre-hook runs the power iteration and sets .weight
    (dW,) = torch.autograd.grad(lin.weight, lin.weight_orig, G.view(shape))
    ref, norms = R.spectral_fwd_ref(_Exact(W), _Exact(u), _Exact(v), 1)
    _close(ref['u'][0], lin.weight_u)
    _close(ref['v'][0], lin.weight_v)
    _close(ref['w'][0], lin.weight.detach().reshape(K, M))
    sigma = ref['sigma'][0]
    assert norms[0] > 1 and norms[1] > 1
    bref, blim = R.spectral_bwd_ref(_Exact(G), _Exact(ref['w'][0]), _Exact(ref['u'][0]), _Exact(ref['v'][0]), sigma)
    _close(bref, dW.reshape(K, M))
    assert bool((blim > 0).all())
    # without the power iteration: u, v as they are
    ref0, _ = R.spectral_fwd_ref(_Exact(W), _Exact(u), _Exact(v), 0)
    _close(ref0['sigma'][0], (u @ (W @ v)).reshape(1))
    assert torch.equal(ref0['u'][0], u) and torch.equal(ref0['v'][0], v)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the case tables reach what they name
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_case_tables_cross_the_edges_they_name():
    assert 262144 // 1024 == 256 and -(-262145 // 1024) == 257                   # the cap of 256 workgroups binds from 262145 on
    assert R.LOSS_SIZES[-1] > 8192 * 256 and R.ADAM_SIZES[-1] > 8192 * 256       # the flat grid wraps
    assert R.LOSS_SIZES[-1] * 4 < 8.4e6 and R.LOSS_SIZES[-1] < 1 << 24             # 8 MB; fl(n) == n
    assert len(R.ADAM_SMALL) == 2 * 4 * 2 * 4 * 2
    for col, want in ((1, R.ADAM_BETA1), (2, R.ADAM_BETA2), (3, R.ADAM_STEPS), (4, R.ADAM_EPS)):
        assert {c[col] for c in R.ADAM_LARGE} == set(want)
    a, _ = R.loss_inputs('bce', 1025, 0.9)
    assert all(R.f32(e) in a.tolist() for e in R.LOGIT_EDGES) and a[-11:].tolist() == a[:11].flip(0).tolist()
    for K, M in R.SPECTRAL_CASES + [R.SPECTRAL_TINY[:2]]:
        W, u, v, _ = R.spectral_inputs(K, M)
        _, norms = R.spectral_fwd_ref(W, u, v, 1)
        assert min(norms) > 2 * R.SN_EPS and abs(float(u.norm()) - 1.0) > 0.05      # (u comes in unnormalised)
    K, M, scale = R.SPECTRAL_TINY
    W, u, v, _ = R.spectral_inputs(K, M, scale)
    ref, norms = R.spectral_fwd_ref(W, u, v, 1)
    assert max(norms) < 0.5 * R.SN_EPS and float(ref['sigma'][0]) > 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the fp32 restatements meet the limits; the wrong variants do not
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _loss_shares(variant_f=None, variant_b=None, sizes=R.LOSS_SIZES):
    """worst share over every case, forward and backward, per mode"""
    worst = {}
    for mode in R.LOSS_MODES:
        wf = wb = 0.0
        for n in sizes:
            for target, gscale in zip(R.TARGETS, R.GSCALES):
                if mode in ('l1', 'mean') and target != R.TARGETS[0] and n > 1025:
                    continue
                a, b = R.loss_inputs(mode, n, target)
                ref, lim = R.loss_fwd(mode, a, b, target)
                wf = max(wf, R.share(R.diff(R.emu_loss_fwd(mode, a, b, target, variant_f), ref), lim)[0])
                gref, glim = R.loss_bwd(mode, a, b, target, gscale)
                wb = max(wb, R.share(R.diff(R.emu_loss_bwd(mode, a, b, target, gscale, variant_b), gref), glim)[0])
        worst[mode] = (wf, wb)
    return worst


def test_loss_restatement_meets_the_limits_and_wrong_variants_do_not():
    good = _loss_shares()
    print('numpy fp32 restatement, worst share (forward, backward):', good)
    assert all(f <= 1 and b <= 1 for f, b in good.values())
    assert good['bce'][0] > 0 and good['mse'][1] > 0                                 # (the limits are not met trivially)
    assert _loss_shares(variant_f='no_max', sizes=SMALL)['bce'][0] > 1
    nm1 = _loss_shares(variant_f='n_minus_1', sizes=SMALL)
    assert nm1['mean'][0] > 1 and nm1['mse'][0] > 1
    # ... and at the LARGEST n, where n / (n - 1) is closest to one
    n = R.LOSS_SIZES[-1]
    for mode in ('mean', 'mse'):
        a, b = R.loss_inputs(mode, n, 0.0)
        ref, lim = R.loss_fwd(mode, a, b, 0.0)
        assert R.share(R.diff(R.emu_loss_fwd(mode, a, b, 0.0, 'n_minus_1'), ref), lim)[0] > 1
    assert _loss_shares(variant_b='plus_g_at_equal', sizes=SMALL)['l1'][1] > 1


def _adam_share(case, p_mode, variant=None):
    n, b1, b2, step, eps = case
    p, g, m, v = R.adam_inputs(n)
    lr = R.ADAM_LR
    if p_mode == 'update':
        p, lr = torch.zeros_like(p), 1.0
    ref = R.adam_ref(p, g, m, v, lr, b1, b2, eps, step)
    out = R.emu_adam(p, g, m, v, lr, b1, b2, eps, step, variant)
    return {k: R.share(R.diff(o, ref[k][0]), ref[k][1])[0] for k, o in zip('pmv', out)}


def test_adam_restatement_meets_the_limits_and_wrong_variants_do_not():
    worst = {k: 0.0 for k in 'pmv'}
    hit = {'other_branch': 0, 'no_eps': 0, 'bc2': 0}
    hidden = 0
    for case in R.ADAM_SMALL + R.ADAM_LARGE[:1]:
        for p_mode in ('update', 'production'):
            s = _adam_share(case, p_mode)
            assert max(s.values()) <= 1, (case, p_mode, s)
            worst = {k: max(worst[k], s[k]) for k in 'pmv'}
            if case[0] == 1:
                continue
            for variant in hit:
                w = _adam_share(case, p_mode, variant)
                bad = w['m'] > 1 if variant == 'other_branch' else w['p'] > 1
                hit[variant] += bad
                if variant == 'bc2' and p_mode == 'production' and not bad:
                    hidden += 1
    print('numpy fp32 restatement of k_adam, worst share:', worst, 'cases a wrong variant misses its limit on:', hit)
    assert all(v > 0 for v in hit.values()), hit
    # the other lerp form is caught on BOTH sides of wl < 0.5 (it differs in rounding only: the limit of m is that tight)
    for b1 in (0.1, 0.9):
        assert _adam_share((257, b1, 0.999, 10, 1e-8), 'update', 'other_branch')['m'] > 1, b1
    # a wrong bias correction is always caught with p = 0, lr = 1 (except where bc2 is 1 to fp32, step 100000)
    for case in R.ADAM_SMALL:
        if case[0] > 1 and case[3] < 100000:
            assert _adam_share(case, 'update', 'bc2')['p'] > 1, case


@pytest.mark.parametrize('case', R.SPECTRAL_CASES + [R.SPECTRAL_TINY], ids=lambda c: 'x'.join(str(v) for v in c))
def test_spectral_restatement_meets_the_limits_and_wrong_variants_do_not(case):
    K, M = case[:2]
    W, u, v, G = R.spectral_inputs(*case)
    for pi in (1, 0):
        ref, _ = R.spectral_fwd_ref(W, u, v, pi)
        out = dict(zip(('u', 'v', 'sigma', 'w'), R.emu_spectral_fwd(W, u, v, pi)))
        s = {k: R.share(R.diff(out[k], ref[k][0]), ref[k][1])[0] for k in ref}
        print('%dx%d power_iteration %d: share of the limit %s' % (K, M, pi, s))
        assert max(s.values()) <= 1, s
        if pi == 0:
            assert torch.equal(out['u'], u) and torch.equal(out['v'], v)
            continue
        for variant in ('no_u_update', 'sigma_old_u'):
            bad = dict(zip(('u', 'v', 'sigma', 'w'), R.emu_spectral_fwd(W, u, v, 1, variant=variant)))
            assert R.share(R.diff(bad['sigma'], ref['sigma'][0]), ref['sigma'][1])[0] > 1, variant
            assert R.share(R.diff(bad['w'], ref['w'][0]), ref['w'][1])[0] > 1, variant
        if len(case) == 3:
            continue     # (sigma ~ 1e-40: the backward of the tiny case is not asked for)
        for kind in ('random', 'orthogonal', 'parallel'):
            Gk = R.spectral_G(kind, G, out['w'])
            bref, blim = R.spectral_bwd_ref(Gk, out['w'], out['u'], out['v'], out['sigma'])
            sb = R.share(R.diff(R.emu_spectral_bwd(Gk, out['w'], out['u'], out['v'], out['sigma']), bref), blim)[0]
            print('%dx%d backward, G %s: share of the limit %.3f' % (K, M, kind, sb))
            assert sb <= 1
            if kind != 'orthogonal':     # (there the rank-one term is rounding noise, and leaving it out is no error)
                for variant in ('no_rank_one', 'sigma_twice'):
                    assert R.share(R.diff(R.emu_spectral_bwd(Gk, out['w'], out['u'], out['v'], out['sigma'], variant), bref), blim)[0] > 1, (kind, variant)
