"""CPU tests of the ResNet generators (define_G(..., 'resnet_6blocks' | 'resnet_9blocks', dimension=2); reference models/networks.py:177-180,
724-837, reached through TestModel's opt.image_dimension): state-dict keys / shapes / parameter order against the reference's
(tests/golden/resnet2d_ops.npz) and seed.resnet_spec, the names that still raise, the helpers of tests/resnet2d_reference.py against torch
(pad, fold, the reflect convolution's references, the functional restatement against the goldens), the new C ABI, and no CPU fallback."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet2d_reference as R  # noqa: E402

from neuroclear_amd import _lib, ops  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

CASES = ['r6_in_ngf16_b2_32x40', 'r9_in_ngf8_b1_36x28', 'r6_bn_ngf8_b2_24', 'r6_in_drop_eval_30x22']
ABI = ['nc_conv2d_k3_reflect_ws_bytes', 'nc_conv2d_k3_reflect_active', 'nc_conv2d_k3_reflect_fwd', 'nc_conv2d_k3_reflect_dgrad',
       'nc_conv2d_k3_reflect_wgrad', 'nc_reflect_pad2d_fwd', 'nc_reflect_pad2d_bwd', 'nc_instnorm_res_fwd', 'nc_residual_add', 'nc_dropout_mul']


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'resnet2d_ops.npz'), allow_pickle=False)


def rnd(seed, shape):
    return np.random.default_rng(int(seed)).random(tuple(int(s) for s in shape), dtype=np.float32)


def rel2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def case_spec(g, tag):
    return S.resnet_spec(int(g[tag + '_n_blocks']), int(g[tag + '_ngf']), 1, 1, str(g[tag + '_norm']), bool(g[tag + '_dropout']))


@pytest.mark.parametrize('tag', CASES)
def test_keys_match_reference_and_seeded_weights_load(golden, tag):
    g = golden
    assert tag in [str(c) for c in g['cases']]
    m = networks.define_G(1, 1, int(g[tag + '_ngf']), str(g[tag + '_net']), str(g[tag + '_norm']), bool(g[tag + '_dropout']), 'kaiming', 0.02, [],
                          dimension=2)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[tag + '_keys']]
    assert [','.join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g[tag + '_shapes']]
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in g[tag + '_pkeys']]
    spec = case_spec(g, tag)
    assert [(k, tuple(s)) for k, s in spec] == [(k, tuple(v.shape)) for k, v in sd.items()]
    w = S.weights_from_seed(spec, int(g[tag + '_seed']))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    n = int(g[tag + '_n_blocks'])
    up = m.model[10 + n]
    assert type(up).__name__ == 'ConvTransposeK3S2' and torch.equal(up.weight.detach(), torch.from_numpy(w['model.%d.weight' % (10 + n)]))
    assert tuple(up.weight.shape) == (4 * int(g[tag + '_ngf']), 2 * int(g[tag + '_ngf']), 3, 3)
    # use_bias is true exactly with InstanceNorm; the last convolution always has one
    assert ('model.1.bias' in sd) == (str(g[tag + '_norm']) == 'instance') and 'model.%d.bias' % (17 + n) in sd
    assert ('model.2.running_mean' in sd) == (str(g[tag + '_norm']) == 'batch')
    # what the file holds, and the headroom of the GPU tests' bounds: the reference's own float32 run lies at most a third of each from its float64 run
    assert g[tag + '_y'].shape == tuple(g[tag + '_yshape']) and g[tag + '_dx'].shape == tuple(g[tag + '_shape'])
    assert all(d <= b / 3 for d, b in zip(g[tag + '_d64'], (2e-5, 2e-2, 2e-2))), g[tag + '_d64']
    assert len(g[tag + '_pkeys']) == len(g[tag + '_g_l2']) == len(g[tag + '_g_samp'])


def test_the_output_size_follows_the_reference(golden):
    assert tuple(golden['r6_in_drop_eval_30x22_yshape']) == (1, 1, 32, 24)
    assert tuple(golden['r6_in_ngf16_b2_32x40_yshape']) == (2, 1, 32, 40)


def test_names_that_still_raise():
    with pytest.raises(NotImplementedError, match='2-D only'):
        networks.define_G(1, 1, 8, 'resnet_9blocks', 'instance', False, 'kaiming', 0.02, [], dimension=3)
    with pytest.raises(NotImplementedError, match='2-D only'):
        networks.define_G(1, 1, 8, 'resnet_6blocks', 'instance', False, 'kaiming', 0.02, [])
    for name in ('unet_twoouts', 'VGG'):
        for nd in (2, 3):
            with pytest.raises(NotImplementedError, match='outside the MI355X hot path'):
                networks.define_G(1, 1, 8, name, 'instance', False, 'kaiming', 0.02, [], dimension=nd)
    with pytest.raises(TypeError):      # --norm none: the reference calls None(ngf)
        networks.define_G(1, 1, 8, 'resnet_6blocks', 'none', False, 'kaiming', 0.02, [], dimension=2)


def test_arguments_pass_through_and_init_net():
    torch.manual_seed(0)
    m = networks.define_G(3, 2, 12, 'resnet_6blocks', 'instance', True, 'normal', 0.02, [], dimension=2)
    sd = m.state_dict()
    assert tuple(sd['model.1.weight'].shape) == (12, 3, 7, 7) and tuple(sd['model.23.weight'].shape) == (2, 12, 7, 7)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in S.resnet_spec(6, 12, 3, 2, 'instance', True)]
    assert type(m.model[10].conv_block[4]).__name__ == 'Dropout' and 'model.10.conv_block.6.weight' in sd
    for k, p in m.named_parameters():
        if k.endswith('bias'):
            assert float(p.detach().abs().max()) == 0.0, k
        elif p.numel() >= 1024:
            assert abs(float(p.detach().std()) / 0.02 - 1) < 0.1, k


def test_no_cpu_fallback():
    m = networks.define_G(1, 1, 8, 'resnet_6blocks', 'instance', False, 'kaiming', 0.02, [], dimension=2)
    with pytest.raises(_lib.NcError):
        m(torch.zeros(1, 1, 16, 16))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 1, 16, 16, 16))
    with pytest.raises(_lib.NcError):
        ops.conv_reflect3(torch.zeros(1, 16, 8, 8), torch.zeros(16, 16, 3, 3))
    with pytest.raises(_lib.NcError):
        ops.reflect_pad2d(torch.zeros(1, 1, 8, 8), 3)
    with pytest.raises(_lib.NcError):
        ops.dropout(torch.zeros(1, 1, 8, 8))
    assert ops.dropout(torch.ones(3), 0.5, training=False).sum() == 3


def test_abi_is_in_the_header_and_the_library():
    syms, protos = _lib.header_symbols(), _lib.prototypes()
    for s in ABI:
        assert s in syms and s in protos, s
        assert protos[s][0] is (ctypes.c_size_t if s.endswith('ws_bytes') else ctypes.c_int), s
    text = open(_lib.HEADER_PATH).read()
    block = text[text.index('The ResNet generators'):text.index('nc_dropout_mul')]
    assert 'networks.py:724-837' in block and 'networks.py:808-830' in block
    assert os.path.exists(_lib.LIB_PATH), 'libnc_hip.so is not built'
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(L, s) for s in ABI)


# ---- tests/resnet2d_reference.py against torch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('NC,H,W,p', R.PAD_CASES + [(2, 5, 4, 3), (2, 4, 8, 1)])
def test_pad_and_fold_helpers(NC, H, W, p):
    g = torch.Generator().manual_seed(NC * 100 + H * 10 + W + p)
    x = torch.randn(1, NC, H, W, generator=g)
    assert torch.equal(R.reflect_pad(x, p), F.pad(x, (p, p, p, p), mode='reflect'))
    xd = x.double().requires_grad_(True)
    gy = torch.randn(1, NC, H + 2 * p, W + 2 * p, generator=g, dtype=torch.float64)
    (F.pad(xd, (p, p, p, p), mode='reflect') * gy).sum().backward()
    torch.testing.assert_close(R.reflect_fold(gy, H, W, p), xd.grad, rtol=1e-14, atol=1e-14)
    # the number of folded terms: every padded position lands exactly once
    t = R.fold_terms(H, W, p)
    assert int(t.sum()) == (H + 2 * p) * (W + 2 * p) and int(t.max()) <= 9 and int(t.min()) >= 1
    torch.testing.assert_close(R.reflect_fold(torch.ones(H + 2 * p, W + 2 * p, dtype=torch.float64), H, W, p), t.double())


@pytest.mark.parametrize('N,C,K,H,W', [(2, 4, 6, 5, 7), (1, 3, 2, 2, 2), (1, 2, 3, 3, 9)])
def test_reflect_convolution_references(N, C, K, H, W):
    x, w, b, dy = R.inputs3(N, C, K, H, W)
    xd = x.double().requires_grad_(True)
    y = F.conv2d(F.pad(xd, (1, 1, 1, 1), mode='reflect'), w.double(), b.double())
    torch.testing.assert_close(R.refr_fwd(x, w, b), y.detach(), rtol=1e-13, atol=1e-13)
    (y * dy.double()).sum().backward()
    torch.testing.assert_close(R.refr_dgrad(dy, w), xd.grad, rtol=1e-13, atol=1e-13)
    # the chain oracle in float64 is the reference summed in another order; in float32 it is close to it
    torch.testing.assert_close(R.chainr_fwd(x, w, b, torch.float64), R.refr_fwd(x, w, b), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.chainr_dgrad(dy, w, torch.float64), R.refr_dgrad(dy, w), rtol=1e-12, atol=1e-12)
    assert R.err(R.chainr_fwd(x, w, b), R.refr_fwd(x, w, b))[0] < 1e-5 and R.err(R.chainr_dgrad(dy, w), R.refr_dgrad(dy, w))[0] < 1e-5


def test_the_cases_reach_the_tiled_kernel_and_its_edges():
    for c in R.KR_CASES:
        N, C, K, H, W = c[:5]
        assert R.k3_covered(0, N, C, K, H, W) and R.k3_covered(1, N, C, K, H, W), c
    assert 1 * -(-61 // 4) * -(-97 // 32) * (256 // 64) == 256
    for c in R.KR_OUTSIDE:
        assert not R.k3_covered(0, *c[:5]), c


@pytest.mark.parametrize('tag', CASES)
def test_restatement_reproduces_the_goldens(golden, tag):
    """The functional restatement in float64 lies where the reference's own float64 run lies: at the recorded float32-to-float64 distance from the
    golden y and dx; in float32 it stays inside the GPU tests' bounds."""
    g = golden
    spec = case_spec(g, tag)
    nb, norm, drop, ev = int(g[tag + '_n_blocks']), str(g[tag + '_norm']), bool(g[tag + '_dropout']), bool(g[tag + '_eval'])
    for dtype in (torch.float64, torch.float32):
        sd = {k: (v if v.dtype == torch.int64 else v.to(dtype)) for k, v in S.state_dict_from_seed(spec, int(g[tag + '_seed'])).items()}
        x = torch.from_numpy(rnd(g[tag + '_x_seed'], g[tag + '_shape'])).to(dtype).requires_grad_(True)
        y, stats = R.resnet_forward(sd, x, nb, norm, drop, training=not ev)
        assert tuple(y.shape) == tuple(g[tag + '_yshape'])
        if tuple(y.shape) == tuple(x.shape):
            (y * torch.from_numpy(rnd(g[tag + '_r_seed'], y.shape)).to(dtype)).mean().backward()
        else:
            y.mean().backward()
        ey = float(np.abs(y.detach().numpy() - g[tag + '_y']).max())
        edx = rel2(x.grad.numpy(), g[tag + '_dx'])
        print('%s %s: |y - golden| max %.2e (reference %.2e), dx rel L2 %.2e (reference %.2e)' % (tag, dtype, ey, g[tag + '_d64'][0], edx, g[tag + '_d64'][1]))
        if dtype == torch.float64:
            assert abs(ey - g[tag + '_d64'][0]) <= 0.05 * g[tag + '_d64'][0] + 1e-9
            assert abs(edx - g[tag + '_d64'][1]) <= 0.05 * g[tag + '_d64'][1] + 1e-9
        else:
            assert ey < 2e-5 and edx < 2e-2
        for k, v in stats.items():
            np.testing.assert_allclose(v.numpy(), g[tag + '_buf_' + k], rtol=2e-5, atol=1e-6, err_msg=k)
