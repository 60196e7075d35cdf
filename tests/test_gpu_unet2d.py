"""GPU tests of the 2-D generators (unet_deconv / unet_vanilla with dimension=2) against the reference's own values (tests/golden/unet2d_ops.npz,
written by tools/gen_golden_unet2d.py from the reference's define_G(..., dimension=2) in training mode).

Bounds: the project's own for the 3-D U-Net goldens (tests/test_gpu_nets.py test_unet_deconv) -- |y - golden| max < 2e-5, dx in relative L2 < 2e-2
(a ReLU / max-pool decision that flips on a 1e-7 difference moves isolated pixels), parameter gradients by check_grads' rule with tol 2e-2; the
batch-norm case at test_batch_norm_networks' bounds.  The reference alone stays far inside them: float32 against float64 of its own modules on
the CPU gives y 2.9e-7 .. 3.5e-6, dx 1.3e-6 .. 2.9e-6, worst live parameter gradient 1.3e-5.

A 2-D net runs layer by layer in fp32 under every conv precision, and TestModel reaches it through opt.image_dimension."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neuroclear_amd import ops  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

DEV = 'cuda'
SPECS = {('unet_deconv', 'instance'): S.unet_deconv_spec, ('unet_deconv', 'batch'): S.unet_deconv_bn_spec,
         ('unet_vanilla', 'instance'): S.unet_vanilla_spec}
CASES = ['deconv_in_b2_16x24', 'deconv_in_b1_36x20', 'deconv_bn_b2_16', 'vanilla_in_b1_32x48']


def rnd(seed, shape):
    return np.random.default_rng(int(seed)).random(tuple(int(s) for s in shape), dtype=np.float32)


def rel2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def check_grads(g_l2, g_samp, net, tol):
    """tests/test_gpu_nets.py check_grads' rule."""
    for i, (k, p) in enumerate(net.named_parameters()):
        gr = p.grad.detach().cpu().numpy().ravel()
        l2 = np.sqrt((gr.astype(np.float64) ** 2).sum())
        # biases in front of a norm layer have an exactly-zero true gradient: both sides hold rounding noise there, hence the absolute floor
        assert abs(l2 - g_l2[i]) <= tol * g_l2[i] + 1e-6, (k, l2, g_l2[i])
        idx = np.random.default_rng([77, i]).integers(0, gr.size, size=8)
        np.testing.assert_allclose(gr[idx], g_samp[i], rtol=2e-2, atol=5 * tol * l2 / np.sqrt(gr.size) + 1e-7, err_msg=k)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'unet2d_ops.npz'), allow_pickle=False)


def build(g, tag):
    net_name, norm = str(g[tag + '_net']), str(g[tag + '_norm'])
    net = networks.define_G(1, 1, 64, net_name, norm, False, 'kaiming', 0.02, [0], dimension=2)
    spec = SPECS[(net_name, norm)](2)
    assert list(net.state_dict().keys()) == [k for k, _ in spec] == [str(k) for k in g[tag + '_keys']]
    net.load_state_dict(S.state_dict_from_seed(spec, int(g[tag + '_seed']), DEV))
    net.train()
    return net


@pytest.mark.parametrize('tag', CASES)
def test_against_the_reference(golden, tag):
    g = golden
    net = build(g, tag)
    shape = tuple(int(v) for v in g[tag + '_shape'])
    batch = str(g[tag + '_norm']) == 'batch'
    x = torch.from_numpy(rnd(g[tag + '_x_seed'], shape)).to(DEV).requires_grad_(True)
    y = net(x)
    assert tuple(y.shape) == shape
    ey = float(np.abs(y.detach().cpu().numpy() - g[tag + '_y']).max())
    r = torch.from_numpy(rnd(g[tag + '_r_seed'], y.shape)).to(DEV)
    (y * r).mean().backward()
    edx = rel2(x.grad.cpu().numpy(), g[tag + '_dx'])
    print('%s: |y - golden| max %.2e, dx rel L2 %.2e' % (tag, ey, edx))
    assert ey < 2e-5
    assert edx < 2e-2
    check_grads(g[tag + '_g_l2'], g[tag + '_g_samp'], net, 2e-2)
    if batch:   # tests/test_gpu_nets.py test_batch_norm_networks: the running statistics the step leaves and the eval() forward on them
        sd = net.state_dict()
        pre = tag + '_buf_'
        bufs = [k for k in g.files if k.startswith(pre)]
        assert len(bufs) == 3 * 10         # 10 norm layers: running_mean, running_var, num_batches_tracked
        for k in bufs:
            np.testing.assert_allclose(sd[k[len(pre):]].cpu().numpy(), g[k], rtol=2e-5, atol=1e-6, err_msg=k)
        net.eval()
        with torch.no_grad():
            ye = net(torch.from_numpy(rnd(g[tag + '_xe_seed'], shape)).to(DEV))
        np.testing.assert_allclose(ye.cpu().numpy(), g[tag + '_y_eval'], atol=2e-5, rtol=5e-4)


@pytest.mark.parametrize('tag', ['deconv_in_b1_36x20', 'vanilla_in_b1_32x48'])
def test_no_grad_forward_and_every_precision_give_the_fp32_bits(golden, tag):
    """A 2-D net has no whole-network and no 16-bit shortcut: torch.no_grad(), set_conv_precision('bf16' | 'fp16') and a second run all give the
    bits of the fp32 training-mode forward."""
    g = golden
    net = build(g, tag)
    x = torch.from_numpy(rnd(g[tag + '_x_seed'], g[tag + '_shape'])).to(DEV)
    y = net(x).detach()
    assert torch.equal(net(x).detach(), y)
    with torch.no_grad():
        assert torch.equal(net(x), y)
        prev = ops.conv_precision
        try:
            for name in ('bf16', 'fp16'):
                ops.set_conv_precision(name)
                assert torch.equal(net(x), y), name
        finally:
            ops.set_conv_precision(prev)
    prev = ops.conv_precision
    try:
        ops.set_conv_precision('bf16')
        assert torch.equal(net(x).detach(), y)
    finally:
        ops.set_conv_precision(prev)


def test_edges_raise_before_any_launch():
    net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0], dimension=2)
    van = networks.define_G(1, 1, 64, 'unet_vanilla', 'instance', False, 'kaiming', 0.02, [0], dimension=2)
    with pytest.raises(ValueError, match='multiple of 4'):
        net(torch.zeros(1, 1, 18, 16, device=DEV))
    with pytest.raises(ValueError, match='multiple of 8'):
        van(torch.zeros(1, 1, 20, 16, device=DEV))
    assert tuple(net(torch.zeros(1, 1, 20, 16, device=DEV)).shape) == (1, 1, 20, 16)


def test_testmodel_end_to_end(tmp_path):
    """A seeded checkpoint saved under the reference's file name, loaded by TestModel with --image_dimension 2 (models/test_model.py:41-45):
    create_model -> setup -> set_input -> test(); `fake` is the bare net's output bit for bit."""
    from neuroclear_amd.models import create_model
    from neuroclear_amd.options import TestOptions
    ck = tmp_path / 'ckpt'
    (ck / 'm').mkdir(parents=True)
    (tmp_path / 'data').mkdir()
    spec = S.unet_deconv_spec(2)
    torch.save(S.state_dict_from_seed(spec, 61), str(ck / 'm' / 'iter_3_net_G.pth'))
    topt = TestOptions().parse(['--dataroot', str(tmp_path / 'data'), '--checkpoints_dir', str(ck), '--name', 'm', '--netG', 'unet_deconv',
                                '--norm', 'instance', '--image_dimension', '2', '--load_iter', '3', '--gpu_ids', '0', '--no_dropout'])
    topt.continue_train = False
    assert topt.image_dimension == 2
    tm = create_model(topt)
    tm.setup(topt)
    sd = S.state_dict_from_seed(spec, 61)
    assert list(tm.netG.state_dict().keys()) == list(sd.keys())
    assert torch.equal(tm.netG.t_conv2.weight.detach().cpu(), sd['t_conv2.weight']) and tm.netG.t_conv2.weight.dim() == 4
    a = torch.from_numpy(rnd(62, (1, 1, 36, 20)))
    tm.set_input({'A': a, 'A_paths': 'x'})
    tm.test()
    bare = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'normal', 0.02, [0], dimension=2)
    bare.load_state_dict(S.state_dict_from_seed(spec, 61, DEV))
    with torch.no_grad():
        want = bare(a.to(DEV))
    assert tuple(tm.fake.shape) == (1, 1, 36, 20) and torch.equal(tm.fake, want)
    assert 0.0 < float(tm.fake.min()) and float(tm.fake.max()) < 1.0 and float(tm.fake.std()) > 0.0


# ---- the image-tiled 3 x 3 kernel (csrc/conv2d_k3.hip) against the gather GEMM, through the whole net ----------------------------------------
def _lib():
    from neuroclear_amd._lib import lib
    return lib()


def _forward_with_switch(net, x, on):
    prev = _lib().nc_get_conv2d_k3()
    _lib().nc_set_conv2d_k3(on)
    try:
        with torch.no_grad():
            y = net(x)
        torch.cuda.synchronize()
    finally:
        _lib().nc_set_conv2d_k3(prev)
    return y


def test_switch_on_against_off_on_the_largest_golden_case(golden):
    tag = 'vanilla_in_b1_32x48'
    net = build(golden, tag)
    x = torch.from_numpy(rnd(golden[tag + '_x_seed'], golden[tag + '_shape'])).to(DEV)
    y_on, y_off = _forward_with_switch(net, x, 1), _forward_with_switch(net, x, 0)
    d = float((y_on - y_off).abs().max())
    print('switch on - off, %s: %.2e' % (tag, d))
    assert d < 2e-5
    assert float(np.abs(y_on.cpu().numpy() - golden[tag + '_y']).max()) < 2e-5


def test_switch_on_against_off_where_the_kernel_takes_the_big_layers(golden):
    """1 x 1 x 256 x 320: the 64 -> 64 and 128 -> 64 layers at full size and the 64 -> 128, 128 -> 128, 256 -> 128 layers at half size are on the
    image-tiled kernel (asserted), the one-channel first layer and the quarter-size bottom stay on the gather GEMM."""
    tag = 'deconv_in_b1_36x20'
    net = build(golden, tag)
    L = _lib()
    for (C, K, H, W) in ((64, 64, 256, 320), (128, 64, 256, 320), (64, 128, 128, 160), (128, 128, 128, 160), (256, 128, 128, 160)):
        assert L.nc_conv2d_k3_active(0, 1, C, H, W, K) == 1, (C, K, H, W)
    assert L.nc_conv2d_k3_active(0, 1, 1, 256, 320, 64) == 0 and L.nc_conv2d_k3_active(0, 1, 256, 64, 80, 256) == 0
    x = torch.from_numpy(rnd(63, (1, 1, 256, 320))).to(DEV)
    y_on, y_off = _forward_with_switch(net, x, 1), _forward_with_switch(net, x, 0)
    assert L.nc_conv2d_k3_active(0, 1, 64, 256, 320, 64) == 1
    d = float((y_on - y_off).abs().max())
    print('switch on - off, 256 x 320: %.2e' % d)
    assert d < 2e-5 and float(y_on.std()) > 0.0
    assert torch.equal(_forward_with_switch(net, x, 1), y_on)
    # and through autograd: the data gradient takes the kernel too
    xg = x.clone().requires_grad_(True)
    net(xg).mean().backward()
    g_on = xg.grad.clone()
    prev = L.nc_get_conv2d_k3()
    L.nc_set_conv2d_k3(0)
    try:
        xg.grad = None
        net(xg).mean().backward()
        torch.cuda.synchronize()
    finally:
        L.nc_set_conv2d_k3(prev)
    r = rel2(g_on.cpu().numpy(), xg.grad.cpu().numpy())
    print('dx switch on against off, rel L2 %.2e' % r)
    assert r < 2e-2
