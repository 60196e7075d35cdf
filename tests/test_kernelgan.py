"""CPU tests of the KernelGAN patch discriminator (--netD kernelGAN, reference models/networks.py:1113-1145, :243-244): the factory's
module layout against the reference's keys and shapes (tests/golden/kernelgan_ops.npz), seeded weights, init_net, the reference's
input errors, the nc_kgan_* C ABI, and the exact algebra of the collapsed first two convolutions in fp64."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from neuroclear_amd.models import networks
from neuroclear_amd.util import seed as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KGAN_ABI = ['nc_kgan_param_floats', 'nc_kgan_saved_floats', 'nc_kgan_ws_bytes', 'nc_kgan_out_shape', 'nc_kgan_fwd', 'nc_kgan_bwd']


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'kernelgan_ops.npz'), allow_pickle=False)


def _shapes(sd):
    return [','.join(str(s) for s in v.shape) for v in sd.values()]


@pytest.mark.parametrize('nd', [2, 3])
@pytest.mark.parametrize('norm', ['instance', 'batch', 'none', 'spectral'])
def test_define_d_layout(nd, norm):
    net = networks.define_D(1, 64, 'kernelGAN', 3, norm, 'normal', 0.02, False, [], dimension=nd)
    sd = net.state_dict()
    params = [k for k, _ in net.named_parameters()]
    spec = S.kernelgan_spec(nd, 1, 64, 'none' if norm == 'spectral' else norm)
    assert params == [k for k, _ in spec]
    assert [tuple(p.shape) for _, p in net.named_parameters()] == [s for _, s in spec]
    k = (7,) * nd
    assert tuple(sd['first_layer.weight'].shape) == (64, 1) + k
    assert tuple(sd['final_layer.weight'].shape) == (1, 64) + (1,) * nd
    assert ('first_layer.bias' in sd) == (norm == 'instance')
    if norm == 'batch':
        assert all('feature_block.%d.running_mean' % i in sd for i in (1, 4, 7))
    # n_layers_D is ignored: n_layers is fixed at 5
    other = networks.define_D(1, 64, 'kernelGAN', 6, norm, 'normal', 0.02, False, [], dimension=nd)
    assert list(other.state_dict().keys()) == list(sd.keys())


@pytest.mark.parametrize('tag', ['in2_b3_36', 'in3_14x15x16', 'bn2_b2_20', 'none2_b2_20', 'in2_ndf32_b2_20'])
def test_keys_match_reference_and_seeded_weights_load(golden_dir, tag):
    g = _golden(golden_dir)
    nd, norm, ndf = int(g[tag + '_nd']), str(g[tag + '_norm']), int(g[tag + '_ndf'])
    net = networks.define_D(1, ndf, 'kernelGAN', 3, norm, 'normal', 0.02, False, [], dimension=nd)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[tag + '_keys']]
    assert _shapes(sd) == [str(s) for s in g[tag + '_shapes']]
    assert [k for k, _ in net.named_parameters()] == [str(k) for k in g[tag + '_pkeys']]
    w = S.weights_from_seed(S.kernelgan_spec(nd, 1, ndf, norm), int(g[tag + '_seed']))
    res = net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not res.unexpected_keys
    assert all('running' in k or 'num_batches' in k for k in res.missing_keys)
    assert torch.equal(net.first_layer.weight.detach(), torch.from_numpy(w['first_layer.weight']))


@pytest.mark.parametrize('init_type', ['normal', 'kaiming'])
def test_init_net(init_type):
    torch.manual_seed(0)
    net = networks.define_D(1, 64, 'kernelGAN', 3, 'instance', init_type, 0.02, False, [], dimension=2)
    for name, p in net.named_parameters():
        if name.endswith('bias'):
            assert float(p.detach().abs().max()) == 0.0, name
            continue
        fan_in = p[0].numel()
        want = 0.02 if init_type == 'normal' else (2.0 / fan_in) ** 0.5
        if p.numel() >= 1024:
            assert abs(float(p.detach().std()) / want - 1) < 0.1, (name, float(p.std()), want)
            assert abs(float(p.detach().mean())) < 0.1 * want, name


@pytest.mark.parametrize('norm', ['instance', 'batch', 'none'])
def test_small_inputs_raise_value_error(norm):
    net = networks.define_D(1, 64, 'kernelGAN', 3, norm, 'normal', 0.02, False, [], dimension=2)
    with pytest.raises(ValueError):
        net(torch.zeros(2, 1, 6, 20))
    net3 = networks.define_D(1, 64, 'kernelGAN', 3, norm, 'normal', 0.02, False, [], dimension=3)
    with pytest.raises(ValueError):
        net3(torch.zeros(1, 1, 20, 20, 5))


@pytest.mark.parametrize('nd', [2, 3])
def test_one_element_plane_raises_value_error(nd):
    net = networks.define_D(1, 64, 'kernelGAN', 3, 'instance', 'normal', 0.02, False, [], dimension=nd)
    with pytest.raises(ValueError):
        net(torch.zeros((3, 1) + (7,) * nd))


def test_abi_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'nc_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in KGAN_ABI:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
    from neuroclear_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libnc_hip.so is not built')
    L = _lib.lib()
    for name in KGAN_ABI:
        assert hasattr(L, name), name
    I = _lib.I
    assert L.nc_kgan_param_floats(I(64), I(2)) == 64 * 49 + 64 + 3 * (64 * 64 + 64) + 64 + 1
    assert L.nc_kgan_param_floats(I(64), I(3)) == 64 * 343 + 64 + 3 * (64 * 64 + 64) + 64 + 1
    assert L.nc_kgan_ws_bytes(I(1), I(1), I(6), I(20), I(64), I(2)) == 0
    assert L.nc_kgan_saved_floats(I(1), I(1), I(7), I(7), I(64), I(2)) == 0
    assert L.nc_kgan_saved_floats(I(1), I(1), I(8), I(7), I(64), I(2)) > 0


def _layered64(x, prm, nd):
    conv = F.conv2d if nd == 2 else F.conv3d
    w1, b1, w2, b2, w3, b3, w4, b4, w5, b5 = prm
    z1 = conv(x, w1, b1)
    z2 = conv(z1, w2, b2)
    h = F.relu(F.instance_norm(z2, eps=1e-5))
    h = F.relu(F.instance_norm(conv(h, w3, b3), eps=1e-5))
    h = F.relu(F.instance_norm(conv(h, w4, b4), eps=1e-5))
    return conv(h, w5, b5), z2


@pytest.mark.parametrize('nd,shape', [(2, (2, 1, 13, 11)), (3, (1, 1, 9, 10, 8))])
def test_collapse_algebra_fp64(nd, shape):
    """The collapsed forward and every collapsed backward formula (kgan.hip header) against autograd of the layered
    network, in fp64."""
    spec = S.kernelgan_spec(nd)
    w = S.weights_from_seed(spec, 5)
    prm = [torch.from_numpy(w[k]).double().requires_grad_(True) for k, _ in spec]
    x = (torch.from_numpy(np.random.default_rng(3).random(shape)) - 0.5).requires_grad_(True)
    y, z2 = _layered64(x, prm, nd)
    z2.retain_grad()
    r = torch.from_numpy(np.random.default_rng(4).standard_normal(tuple(y.shape)))
    (y * r).sum().backward()
    w1, b1, w2, b2 = [p.detach() for p in prm[:4]]
    C, T = w1.shape[0], w1[0].numel()
    conv = F.conv2d if nd == 2 else F.conv3d
    convT = F.conv_transpose2d if nd == 2 else F.conv_transpose3d
    # forward: z2 = W' * x + b'
    wc = (w2.reshape(C, C) @ w1.reshape(C, T)).reshape(w1.shape)
    bc = w2.reshape(C, C) @ b1 + b2
    assert float((conv(x.detach(), wc, bc) - z2.detach()).abs().max()) < 1e-11 * float(z2.detach().abs().max())
    dz2 = z2.grad.reshape(shape[0], C, -1)                     # [B][C][P]
    if nd == 2:
        patches = F.unfold(x.detach(), 7)                      # [B][T][P]
    else:
        xs = x.detach()[:, 0].unfold(1, 7, 1).unfold(2, 7, 1).unfold(3, 7, 1)   # [B][Do][Ho][Wo][7][7][7]
        patches = xs.reshape(shape[0], -1, T).transpose(1, 2)
    G = torch.einsum('bcp,btp->ct', dz2, patches)
    s = dz2.sum(dim=(0, 2))
    W1, W2 = w1.reshape(C, T), w2.reshape(C, C)

    def close(a, b, scale=None):
        # db1 / db2 are zero up to rounding (the InstanceNorm behind z2 cancels any bias): judged against the weight gradients' scale
        ref = max(float(b.abs().max()), scale or 0.0, 1e-30)
        assert float((a - b).abs().max()) <= 1e-11 * ref, float((a - b).abs().max())
    close((G @ W1.T + torch.outer(s, b1)).reshape(prm[2].shape), prm[2].grad)
    close((W2.T @ G).reshape(prm[0].shape), prm[0].grad)
    close(s, prm[3].grad, float(prm[2].grad.abs().max()))
    close(W2.T @ s, prm[1].grad, float(prm[0].grad.abs().max()))
    close(convT(z2.grad, wc), x.grad)
