"""CPU tests of the 2-D generators (define_G(..., 'unet_deconv' | 'unet_vanilla', dimension=2); reference models/networks.py:361-411, 478-608,
reached through TestModel's opt.image_dimension, models/test_model.py:41-45): construction under every norm, state-dict keys / shapes /
parameter order against the reference's (tests/golden/unet2d_ops.npz) and the seed specs, seeded weights, init_net, the edge checks, no CPU
fallback, the nc_convT2d_* C ABI, and the 3-D nets unchanged."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from neuroclear_amd import _lib
from neuroclear_amd.models import networks
from neuroclear_amd.util import seed as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONVT2D_ABI = ['nc_convT2d_ws_bytes', 'nc_convT2d_k2s2_fwd', 'nc_convT2d_k2s2_dgrad', 'nc_convT2d_k2s2_wgrad']
SPECS = {('unet_deconv', 'instance'): S.unet_deconv_spec, ('unet_deconv', 'batch'): S.unet_deconv_bn_spec, ('unet_deconv', 'none'): S.unet_deconv_spec,
         ('unet_vanilla', 'instance'): S.unet_vanilla_spec, ('unet_vanilla', 'none'): S.unet_vanilla_spec}


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'unet2d_ops.npz'), allow_pickle=False)


def _shapes(sd):
    return [','.join(str(s) for s in v.shape) for v in sd.values()]


def G2(net, norm, init='kaiming'):
    return networks.define_G(1, 1, 64, net, norm, False, init, 0.02, [], dimension=2)


@pytest.mark.parametrize('norm', ['instance', 'batch', 'none'])
@pytest.mark.parametrize('net', ['unet_deconv', 'unet_vanilla'])
def test_both_nets_construct_with_dimension_2(net, norm):
    m = G2(net, norm)
    sd = m.state_dict()
    assert tuple(sd['double_conv1.convolution.0.weight'].shape) == (64, 1, 3, 3)
    assert tuple(sd['t_conv1.weight'].shape) == (128, 64, 2, 2) and tuple(sd['t_conv2.weight'].shape) == (256, 128, 2, 2)
    assert tuple(sd['one_by_one.weight'].shape) == (1, 64, 1, 1)
    if net == 'unet_vanilla':
        assert tuple(sd['t_conv3.weight'].shape) == (512, 256, 2, 2)
    assert ('double_conv1.convolution.1.running_mean' in sd) == (norm == 'batch')
    assert all(v.dim() in (0, 1, 4) for v in sd.values())
    spec = SPECS.get((net, norm))
    if spec is not None:
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in spec(2)]
    # never on a whole-network or 16-bit shortcut
    assert not getattr(m, '_fusable', False)


def test_other_dimensions_raise_what_conv_raises():
    with pytest.raises(Exception) as want:
        networks.conv(4)
    for net in ('unet_deconv', 'unet_vanilla'):
        for nd in (1, 4):
            with pytest.raises(Exception) as e:
                networks.define_G(1, 1, 64, net, 'instance', False, 'kaiming', 0.02, [], dimension=nd)
            assert type(e.value) is type(want.value) and str(e.value) == str(want.value)
    with pytest.raises(Exception) as e:
        networks.ConvTranspose(8, 4, 2, 2, dimension=1)
    assert str(e.value) == str(want.value)
    with pytest.raises(NotImplementedError):
        networks.ConvTranspose(8, 4, 3, 1, dimension=2)


@pytest.mark.parametrize('tag', ['deconv_in_b2_16x24', 'deconv_in_b1_36x20', 'deconv_bn_b2_16', 'vanilla_in_b1_32x48'])
def test_keys_match_reference_and_seeded_weights_load(golden_dir, tag):
    g = _golden(golden_dir)
    assert tag in [str(c) for c in g['cases']]
    net, norm = str(g[tag + '_net']), str(g[tag + '_norm'])
    m = G2(net, norm)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[tag + '_keys']]
    assert _shapes(sd) == [str(s) for s in g[tag + '_shapes']]
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in g[tag + '_pkeys']]
    spec = SPECS[(net, norm)](2)
    assert [k for k, _ in spec] == list(sd.keys())
    w = S.weights_from_seed(spec, int(g[tag + '_seed']))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    assert torch.equal(m.t_conv1.weight.detach(), torch.from_numpy(w['t_conv1.weight']))
    assert torch.equal(m.double_conv1.convolution[3].bias.detach(), torch.from_numpy(w['double_conv1.convolution.3.bias']))
    # y and dx are stored in full, the gradients as (l2, sum, 8 samples) per parameter
    shape = tuple(int(s) for s in g[tag + '_shape'])
    assert g[tag + '_y'].shape == shape and g[tag + '_dx'].shape == shape
    n = len(g[tag + '_pkeys'])
    assert g[tag + '_g_l2'].shape == (n,) and g[tag + '_g_sum'].shape == (n,) and g[tag + '_g_samp'].shape == (n, 8)
    if norm == 'batch':
        assert g[tag + '_y_eval'].shape == shape
        assert int(g[tag + '_buf_double_conv1.convolution.1.num_batches_tracked']) == 1


@pytest.mark.parametrize('init_type', ['normal', 'kaiming'])
@pytest.mark.parametrize('net', ['unet_deconv', 'unet_vanilla'])
def test_init_net(net, init_type):
    torch.manual_seed(0)
    m = G2(net, 'instance', init_type)
    for name, p in m.named_parameters():
        if name.endswith('bias'):
            assert float(p.detach().abs().max()) == 0.0, name
            continue
        fan_in = p[0].numel()   # size(1) * receptive field: for a transposed weight (C, K, 2, 2) that is K * 4, as in torch
        want = 0.02 if init_type == 'normal' else (2.0 / fan_in) ** 0.5
        if p.numel() >= 1024:
            assert abs(float(p.detach().std()) / want - 1) < 0.1, (name, float(p.std()), want)
            assert abs(float(p.detach().mean())) < 0.1 * want, name


@pytest.mark.parametrize('net,bad,good', [('unet_deconv', (18, 16), (20, 16)), ('unet_vanilla', (20, 16), (24, 16))])
def test_edges_raise_value_error_before_any_launch(net, bad, good):
    """Multiples of 4 for unet_deconv, of 8 for unet_vanilla: the reference fails in torch.cat behind a flooring MaxPool2d.  The check comes first:
    on a CPU tensor the bad edge is a ValueError, the good edge gets as far as the first kernel call and raises NcError (there is no CPU path)."""
    m = G2(net, 'instance')
    for sp in (bad, bad[::-1]):
        with pytest.raises(ValueError, match='multiple of %d' % (4 if net == 'unet_deconv' else 8)):
            m(torch.zeros(1, 1, *sp))
    with pytest.raises(ValueError):     # a 3-D volume into the 2-D net
        m(torch.zeros(1, 1, 16, 16, 16))
    with pytest.raises(_lib.NcError):
        m(torch.zeros(1, 1, *good))
    with torch.no_grad(), pytest.raises(_lib.NcError):
        m(torch.zeros(1, 1, *good))


def test_conv_transpose_has_no_cpu_fallback():
    from neuroclear_amd import ops
    ct = networks.ConvTranspose(8, 4, 2, 2, dimension=2)
    assert tuple(ct.weight.shape) == (8, 4, 2, 2) and tuple(ct.bias.shape) == (4,)
    with pytest.raises(_lib.NcError):
        ct(torch.zeros(1, 8, 3, 5))
    with pytest.raises(_lib.NcError):
        ops.conv_transpose_k2s2(torch.zeros(1, 8, 3, 5), torch.zeros(8, 4, 2, 2))
    with pytest.raises(ValueError):
        ct(torch.zeros(1, 8, 3, 5, 5))


def test_abi_is_in_the_header_and_the_library():
    text = open(os.path.join(ROOT, 'include', 'nc_hip.h')).read()
    syms = _lib.header_symbols()
    protos = _lib.prototypes()
    for s in CONVT2D_ABI:
        assert s in syms and s in protos, s
    # the 3-D signatures minus D
    for tail in ('ws_bytes', 'k2s2_fwd', 'k2s2_dgrad', 'k2s2_wgrad'):
        r3, a3 = protos['nc_convT_' + tail]
        r2, a2 = protos['nc_convT2d_' + tail]
        assert r2 is r3 and len(a2) == len(a3) - 1, tail
    # each entry cites the reference's lines
    block = text[text.index('ConvTranspose2d(k=2, s=2)'):text.index('nc_convT2d_k2s2_wgrad')]
    assert 'networks.py:382-390, 500, 503' in block
    for s in CONVT2D_ABI[1:]:
        line = [ln for ln in text.splitlines() if re.search(r'\b%s\(' % s, ln)][0]
        assert 'networks.py:500,503' in line, s
    if os.path.exists(_lib.LIB_PATH):
        L = ctypes.CDLL(_lib.LIB_PATH)
        assert all(hasattr(L, s) for s in CONVT2D_ABI)
    else:
        pytest.fail('libnc_hip.so is not built')


def test_three_dimensional_nets_are_unchanged():
    for net, spec, fus in (('unet_deconv', S.unet_deconv_spec(3), True), ('unet_vanilla', S.unet_vanilla_spec(3), None)):
        m = networks.define_G(1, 1, 64, net, 'instance', False, 'kaiming', 0.02, [])
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in spec]
        assert getattr(m, '_fusable', None) is fus
    assert networks.define_G(1, 1, 64, 'unet_deconv', 'batch', False, 'kaiming', 0.02, [])._fusable is False
    assert tuple(networks.ConvTranspose(8, 4).weight.shape) == (8, 4, 2, 2, 2)
    with pytest.raises(ValueError, match='multiple of 4'):
        networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [])(torch.zeros(1, 1, 16, 16, 18))
