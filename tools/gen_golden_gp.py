"""Golden vectors of the WGAN-GP gradient penalty (cal_gradient_penalty, networks.py:321-359) on the 2-D PatchGAN with instance norm,
from the REFERENCE itself on the CPU, with the helpers of oracle.gen_golden.

    python tools/gen_golden_gp.py            (from the repo root; needs the reference checkout that oracle.gen_golden names)

Writes tests/golden/gradient_penalty.npz.  Weights are not stored: both sides rebuild them with
neuroclear_amd.util.seed.weights_from_seed(patchgan_spec(2, 1, 64, n_layers), seed).  Inputs are rand_input(seed, shape).

Every case also runs the reference module .double() on the same weights, inputs and alpha, and records each output's fp32 error
against it (max |fp32 - fp64| / max |fp64|).  A case is admitted only if every output -- penalty, gradients, every weight gradient, the
first conv's bias gradient, the gradients of real_data / fake_data -- stays within ADMIT.  The head's bias (.grad None) and the biases
in front of an InstanceNorm (analytically zero, fp32 rounding noise) are recorded but are no outputs of that condition."""
import inspect
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oracle import gen_golden as gg  # noqa: E402
from oracle.gen_golden import big_summary, rand_input, ref_modules  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

ADMIT = 1e-4
# (tag, netD, n_layers, type, shape, constant, lambda_gp, weight seed, alpha seed)
CASES = [
    ('real_nl3_b2_32', 'basic', 3, 'real', (2, 1, 32, 32), 1.0, 10.0, 31, 0),
    ('fake_nl2_b3_40', 'n_layers', 2, 'fake', (3, 1, 40, 40), 1.0, 10.0, 32, 0),
    ('mixed_nl3_b2_48', 'basic', 3, 'mixed', (2, 1, 48, 48), 1.0, 10.0, 33, 101),
    ('mixed_nl4_b2_64_c05_l3', 'n_layers', 4, 'mixed', (2, 1, 64, 64), 0.5, 3.0, 34, 102),
    ('mixed_nl2_b4_36_c2_l1', 'n_layers', 2, 'mixed', (4, 1, 36, 36), 2.0, 1.0, 35, 103),
    ('mixed_nl3_b2_108', 'basic', 3, 'mixed', (2, 1, 108, 108), 1.0, 10.0, 36, 104),
    ('real_nl3_b3_108_c07', 'basic', 3, 'real', (3, 1, 108, 108), 0.7, 10.0, 37, 0),
    ('mixed_nl3_b2_108_s2', 'basic', 3, 'mixed', (2, 1, 108, 108), 1.0, 10.0, 39, 105),
    ('fake_nl3_b4_108', 'basic', 3, 'fake', (4, 1, 108, 108), 1.0, 10.0, 40, 0),
]
ZERO_CASE = ('lambda0_nl3_b2_32', 'basic', 3, 'mixed', (2, 1, 32, 32), 1.0, 0.0, 38, 0)
SUMMARY_N = 1024  # arrays above this many elements go in as big_summary(a, SUMMARY_N)


def _store(out, key, a):
    a = np.asarray(a)
    if a.size <= SUMMARY_N:
        out[key] = a.astype(np.float32)
    else:
        out[key + '_sum'] = big_summary(a, SUMMARY_N)


def _run(networks, netD, n_layers, typ, shape, constant, lam, wseed, aseed, i, dtype):
    net = networks.define_D(1, 64, netD, n_layers, 'instance', 'normal', 0.02, False, [], dimension=2)
    net.train()
    sd = S.weights_from_seed(S.patchgan_spec(2, 1, 64, n_layers), wseed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(dtype)
    real = torch.from_numpy(rand_input(800 + i, shape)).to(dtype)
    fake = torch.from_numpy(rand_input(900 + i, shape)).to(dtype)
    if typ == 'mixed':  # leaves that want gradients, like the generator output / a real batch the caller differentiates
        real.requires_grad_(True)
        fake.requires_grad_(True)
    torch.manual_seed(aseed)
    alpha = torch.rand(shape[0], 1)  # what the reference draws below (fp32 in both runs: torch.rand's default dtype)
    torch.manual_seed(aseed)
    pen, grads = networks.cal_gradient_penalty(net, real, fake, 'cpu', typ, constant, lam)
    pen.backward()
    res = dict(penalty=np.array(pen.item()), gradients=grads.detach().numpy().copy())
    pgrads = []
    for k, p in net.named_parameters():
        pgrads.append(None if p.grad is None else p.grad.numpy().copy())
    res['pgrads'] = pgrads
    res['real_grad'] = real.grad.numpy().copy() if real.grad is not None else None
    res['fake_grad'] = fake.grad.numpy().copy() if fake.grad is not None else None
    res['alpha'] = alpha.numpy().astype(np.float32).ravel()
    res['keys'] = [k for k, _ in net.named_parameters()]
    return res


def _err(a32, a64):
    a32, a64 = np.asarray(a32, np.float64), np.asarray(a64, np.float64)
    return float(np.abs(a32 - a64).max() / max(np.abs(a64).max(), 1e-300)), float(np.abs(a64).max())


def gen(networks):
    out = dict(summary_n=SUMMARY_N, admit=ADMIT)
    sig = inspect.signature(networks.cal_gradient_penalty)
    out['sig_names'] = np.array(list(sig.parameters))
    out['sig_defaults'] = np.array([repr(p.default) if p.default is not inspect.Parameter.empty else '<none>' for p in sig.parameters.values()])
    tags, rejected = [], []
    for i, (tag, netD, nl, typ, shape, c, lam, wseed, aseed) in enumerate(CASES):
        r32 = _run(networks, netD, nl, typ, shape, c, lam, wseed, aseed, i, torch.float32)
        r64 = _run(networks, netD, nl, typ, shape, c, lam, wseed, aseed, i, torch.float64)
        assert np.array_equal(r32['alpha'], r64['alpha'])
        pre = tag + '_'
        out[pre + 'netD'], out[pre + 'n_layers'], out[pre + 'type'] = netD, nl, typ
        out[pre + 'shape'] = np.array(shape)
        out[pre + 'constant'], out[pre + 'lambda_gp'], out[pre + 'seed'] = c, lam, wseed
        out[pre + 'real_seed'], out[pre + 'fake_seed'], out[pre + 'alpha_seed'] = 800 + i, 900 + i, aseed
        out[pre + 'alpha'] = r32['alpha']
        out[pre + 'pkeys'] = np.array(r32['keys'])
        names, errs, amax = [], [], []

        def rec(name, a32, a64, admitted=True):
            e, m = _err(a32, a64)
            _store(out, pre + name, a32)
            if admitted:
                names.append(name); errs.append(e); amax.append(m)
            return e

        rec('penalty', r32['penalty'], r64['penalty'])
        rec('gradients', r32['gradients'], r64['gradients'])
        none_flags, in_bias = [], []
        nP = len(r32['pgrads'])
        for j, (g32, g64) in enumerate(zip(r32['pgrads'], r64['pgrads'])):
            none_flags.append(g32 is None)
            if g32 is None:
                continue
            is_bias = r32['keys'][j].endswith('.bias')
            if is_bias and 1 < j < nP - 1:  # a bias in front of an InstanceNorm: analytically zero
                _store(out, pre + 'g%d' % j, g32)
                wmax = float(np.abs(r32['pgrads'][j - 1]).max())
                in_bias.append([j, float(np.abs(g32).max()) / wmax, float(np.abs(g64).max()) / float(np.abs(r64['pgrads'][j - 1]).max())])
            else:
                rec('g%d' % j, g32, g64)
        out[pre + 'grad_none'] = np.array(none_flags)
        out[pre + 'in_bias_ratio'] = np.array(in_bias)  # rows: param index, fp32 max / its weight's max, fp64 likewise
        for side in ('real_grad', 'fake_grad'):
            if r32[side] is not None:
                rec(side, r32[side], r64[side])
        out[pre + 'err_names'] = np.array(names)
        out[pre + 'err32'] = np.array(errs)
        out[pre + 'absmax64'] = np.array(amax)
        worst = max(errs)
        print('%-24s pen %.6g  worst fp32 err %.2e (%s)' % (tag, r32['penalty'], worst, names[int(np.argmax(errs))]))
        if worst > ADMIT:  # not admitted: its keys leave the fixture
            print('%-24s NOT ADMITTED: fp32 error %.3e > %.0e' % (tag, worst, ADMIT))
            for k in [k for k in out if k.startswith(pre)]:
                del out[k]
            rejected.append(tag)
            continue
        tags.append(tag)
    tag, netD, nl, typ, shape, c, lam, wseed, aseed = ZERO_CASE
    net = networks.define_D(1, 64, netD, nl, 'instance', 'normal', 0.02, False, [], dimension=2)
    res = networks.cal_gradient_penalty(net, torch.zeros(shape), torch.zeros(shape), 'cpu', typ, c, lam)
    assert res == (0.0, None)
    out['zero_case'] = np.array([tag, repr(res)])
    out['cases'] = np.array(tags)
    out['rejected'] = np.array(rejected)
    # what the admitted cases must still cover
    adm = [c for c in CASES if c[0] in tags]
    assert {c[3] for c in adm} == {'real', 'fake', 'mixed'} and {2, 3, 4} <= {c[2] for c in adm}
    assert any(c[5] != 1.0 for c in adm) and any(c[6] != 10.0 for c in adm)
    assert any(c[4][0] >= 2 and c[4][2:] == (108, 108) for c in adm)
    np.savez_compressed(os.path.join(gg.OUT, 'gradient_penalty.npz'), **out)


if __name__ == '__main__':
    gen(ref_modules())
