"""CPU tests of the WGAN-GP gradient penalty (networks.cal_gradient_penalty, reference networks.py:321-359): the golden fixture
(tests/golden/gradient_penalty.npz, tools/gen_golden_gp.py) and its admission condition, an fp64 restatement that reproduces it, the
public signature, the lambda_gp = 0 and bad-type paths, and the nc_patchgan_gp_* exports.  The GPU side is
tests/test_gpu_gradient_penalty.py."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from neuroclear_amd import _lib
from neuroclear_amd.models import networks
from neuroclear_amd.util import seed as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gradient_penalty.npz')
ADMIT = 1e-4            # the generator's admission condition: reference fp32 error against fp64, relative to max |fp64|
IN_BIAS = 2.0 ** -20    # an InstanceNorm-fed bias gradient, relative to its layer's weight-gradient max
GP_SYMBOLS = ('nc_patchgan_gp_saved_floats', 'nc_patchgan_gp_ws_bytes', 'nc_patchgan_gp_fwd', 'nc_patchgan_gp_bwd')


def rnd(seed, shape):
    return np.random.default_rng(int(seed)).random(tuple(int(s) for s in shape), dtype=np.float32)


def big_summary(a, n, key=55):
    a = np.asarray(a).ravel()
    idx = np.random.default_rng(key).integers(0, a.size, size=min(n, a.size))
    return np.concatenate([[np.sqrt((a.astype(np.float64) ** 2).sum()), a.astype(np.float64).sum()], a[idx].astype(np.float64)])


def patchgan_fp64(x, weights, n_layers):
    """NLayerDiscriminator (networks.py:1009-1067, instance norm, 2-D) as plain functional torch."""
    ws = list(weights)
    h = x
    for i in range(n_layers + 2):
        w, b = ws[2 * i], ws[2 * i + 1]
        h = F.conv2d(h, w, b, 2 if i < n_layers else 1, 1)
        if i == n_layers + 1:
            return h
        if i > 0:
            h = F.instance_norm(h, eps=1e-5)
        h = F.leaky_relu(h, 0.2)


def gp_fp64(sd, n_layers, real, fake, alpha, typ, constant, lambda_gp):
    """cal_gradient_penalty restated in fp64 on the CPU: penalty, gradients [B, -1], parameter gradients (None where unused), and the
    gradients of real / fake."""
    params = [torch.from_numpy(v).double().requires_grad_(True) for v in sd.values()]
    real = torch.from_numpy(real).double().requires_grad_(typ != 'fake')
    fake = torch.from_numpy(fake).double().requires_grad_(typ != 'real')
    if typ == 'real':
        x = real
    elif typ == 'fake':
        x = fake
    else:
        a = torch.from_numpy(alpha).double().view(-1, 1, 1, 1)
        x = a * real + (1 - a) * fake
    y = patchgan_fp64(x, params, n_layers)
    g, = torch.autograd.grad(y, x, torch.ones_like(y), create_graph=True)
    g = g.view(x.shape[0], -1)
    pen = (((g + 1e-16).norm(2, dim=1) - constant) ** 2).mean() * lambda_gp
    pen.backward()
    return dict(penalty=pen.item(), gradients=g.detach().numpy(),
                pgrads=[p.grad.numpy() if p.grad is not None else None for p in params],
                real_grad=real.grad.numpy() if real.grad is not None else None,
                fake_grad=fake.grad.numpy() if fake.grad is not None else None)


def case_inputs(z, tag):
    pre = tag + '_'
    shape = tuple(int(s) for s in z[pre + 'shape'])
    nl = int(z[pre + 'n_layers'])
    sd = S.weights_from_seed(S.patchgan_spec(2, 1, 64, nl), int(z[pre + 'seed']))
    return (sd, nl, rnd(z[pre + 'real_seed'], shape), rnd(z[pre + 'fake_seed'], shape), z[pre + 'alpha'], str(z[pre + 'type']),
            float(z[pre + 'constant']), float(z[pre + 'lambda_gp']))


def output(res, name):
    if name in ('penalty', 'gradients', 'real_grad', 'fake_grad'):
        return np.asarray(res[name])
    return res['pgrads'][int(name[1:])]


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLDEN)


def test_golden_loads_and_is_admitted(gold):
    z = gold
    cases = [str(c) for c in z['cases']]
    assert len(cases) >= 5
    assert float(z['admit']) == ADMIT
    types, layers, big = set(), set(), False
    for tag in cases:
        errs = z[tag + '_err32']
        names = [str(n) for n in z[tag + '_err_names']]
        assert {'penalty', 'gradients', 'g0', 'g1'} <= set(names), names
        assert len(errs) == len(names) and np.all(np.isfinite(errs))
        assert errs.max() <= ADMIT, (tag, dict(zip(names, errs)))
        types.add(str(z[tag + '_type']))
        layers.add(int(z[tag + '_n_layers']))
        shape = tuple(z[tag + '_shape'])
        big |= shape[0] >= 2 and shape[2:] == (108, 108)
    assert types == {'real', 'fake', 'mixed'} and {2, 3, 4} <= layers and big
    assert any(float(z[t + '_constant']) != 1.0 for t in cases) and any(float(z[t + '_lambda_gp']) != 10.0 for t in cases)
    assert str(z['zero_case'][1]) == '(0.0, None)'


def test_golden_in_fed_bias_grads_are_noise(gold):
    """The biases of the convs in front of an InstanceNorm have an analytically zero gradient: the reference's fp32 values are rounding
    noise below 2^-20 of the same layer's weight-gradient max; its head bias gets no gradient at all."""
    for tag in gold['cases']:
        rows = gold[str(tag) + '_in_bias_ratio']
        assert len(rows) == int(gold[str(tag) + '_n_layers'])
        for j, r32, r64 in rows:
            assert r32 < IN_BIAS, (tag, int(j), r32)
        none = gold[str(tag) + '_grad_none']
        assert none[-1] and not none[:-1].any()


@pytest.mark.parametrize('tag', ['real_nl3_b2_32', 'fake_nl2_b3_40', 'mixed_nl3_b2_48', 'mixed_nl4_b2_64_c05_l3', 'mixed_nl2_b4_36_c2_l1',
                                 'mixed_nl3_b2_108_s2', 'fake_nl3_b4_108'])
def test_fp64_restatement_reproduces_golden(gold, tag):
    """The oracle of the GPU test: the fp64 restatement lands within the recorded fp32 error of every golden output."""
    z = gold
    assert tag in [str(c) for c in z['cases']]
    res = gp_fp64(*case_inputs(z, tag))
    names = [str(n) for n in z[tag + '_err_names']]
    for name, err, amax in zip(names, z[tag + '_err32'], z[tag + '_absmax64']):
        mine = np.asarray(output(res, name), np.float64)
        assert abs(np.abs(mine).max() - amax) <= 1e-9 * amax, (tag, name)
        bound = err * amax * (1 + 1e-6) + 1e-12 * amax
        key = tag + '_' + name
        if key in z:
            ref = z[key].astype(np.float64).reshape(mine.shape)
            assert np.abs(ref - mine).max() <= bound, (tag, name, np.abs(ref - mine).max() / amax, err)
        else:
            summ = z[key + '_sum']
            mine_s = big_summary(mine, int(z['summary_n']))
            assert np.abs(summ[2:] - mine_s[2:]).max() <= bound, (tag, name)
            assert abs(summ[0] - mine_s[0]) <= bound * np.sqrt(mine.size), (tag, name)


def test_signature_matches_reference(gold):
    sig = inspect.signature(networks.cal_gradient_penalty)
    assert list(sig.parameters) == [str(n) for n in gold['sig_names']]
    got = [repr(p.default) if p.default is not inspect.Parameter.empty else '<none>' for p in sig.parameters.values()]
    assert got == [str(d) for d in gold['sig_defaults']]


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError('netD was touched: .%s' % name)

    def __call__(self, *a, **k):
        raise AssertionError('netD was called')


def test_lambda_zero_returns_zero_none():
    real = torch.rand(2, 1, 16, 16)
    assert networks.cal_gradient_penalty(_Untouchable(), real, real, 'cpu', lambda_gp=0.0) == (0.0, None)
    assert networks.cal_gradient_penalty(_Untouchable(), real, real, 'cpu', 'bogus', 1.0, -1.0) == (0.0, None)


def test_bad_type_raises_reference_error():
    net = networks.define_D(1, 64, 'basic', 3, 'instance', 'normal', 0.02, False, [], dimension=2)
    real = torch.rand(2, 1, 16, 16)
    with pytest.raises(NotImplementedError) as e:
        networks.cal_gradient_penalty(net, real, real, 'cpu', type='bogus')
    assert str(e.value) == 'bogus not implemented'


def test_cpu_input_has_no_fallback():
    net = networks.define_D(1, 64, 'basic', 3, 'instance', 'normal', 0.02, False, [], dimension=2)
    real = torch.rand(2, 1, 16, 16)
    with pytest.raises(NotImplementedError, match='no HIP path'):
        networks.cal_gradient_penalty(net, real, real, 'cpu')


def test_gp_symbols_exported():
    syms = _lib.header_symbols()
    for s in GP_SYMBOLS:
        assert s in syms
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(L, s) for s in GP_SYMBOLS)
