"""GPU tests of the ResNet generators (resnet_6blocks / resnet_9blocks, dimension=2) against the reference's own values
(tests/golden/resnet2d_ops.npz, written by tools/gen_golden_resnet2d.py from the reference's define_G(..., dimension=2)), by the rules of
tests/test_gpu_unet2d.py: |y - golden| max < 2e-5, dx in relative L2 < 2e-2, parameter gradients by check_grads' rule with tol 2e-2 (its
absolute floor absorbs the noise-level gradients of the biases in front of an InstanceNorm), the batch-norm case's running statistics and eval()
forward at that file's bounds.  The reference's own float32 run uses at most a third of each bound against its float64 run (stored per case,
asserted by tests/test_resnet2d.py).

One net is large enough for its blocks to run on the image-tiled kernel (asserted); it is held to the float64 restatement of
tests/resnet2d_reference.py on the GPU, to the same step with nc_set_conv2d_k3(0), and to itself bit for bit.  TestModel reaches the nets
through --netG resnet_9blocks --image_dimension 2."""
import os
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet2d_reference as R  # noqa: E402

from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

DEV = 'cuda'
CASES = ['r6_in_ngf16_b2_32x40', 'r9_in_ngf8_b1_36x28', 'r6_bn_ngf8_b2_24', 'r6_in_drop_eval_30x22']


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
    return np.load(os.path.join(golden_dir, 'resnet2d_ops.npz'), allow_pickle=False)


def lib():
    from neuroclear_amd._lib import lib
    return lib()


def build(g, tag):
    nb, ngf, norm, drop = int(g[tag + '_n_blocks']), int(g[tag + '_ngf']), str(g[tag + '_norm']), bool(g[tag + '_dropout'])
    net = networks.define_G(1, 1, ngf, str(g[tag + '_net']), norm, drop, 'kaiming', 0.02, [0], dimension=2)
    spec = S.resnet_spec(nb, ngf, 1, 1, norm, drop)
    assert list(net.state_dict().keys()) == [k for k, _ in spec] == [str(k) for k in g[tag + '_keys']]
    net.load_state_dict(S.state_dict_from_seed(spec, int(g[tag + '_seed']), DEV))
    return net.eval() if bool(g[tag + '_eval']) else net.train()


def loss(y, x, r_seed):
    if tuple(y.shape) == tuple(x.shape):
        return (y * torch.from_numpy(rnd(r_seed, y.shape)).to(y.device).to(y.dtype)).mean()
    return y.mean()


@pytest.mark.parametrize('tag', CASES)
def test_against_the_reference(golden, tag):
    g = golden
    net = build(g, tag)
    shape = tuple(int(v) for v in g[tag + '_shape'])
    x = torch.from_numpy(rnd(g[tag + '_x_seed'], shape)).to(DEV).requires_grad_(True)
    y = net(x)
    assert tuple(y.shape) == tuple(int(v) for v in g[tag + '_yshape'])
    ey = float(np.abs(y.detach().cpu().numpy() - g[tag + '_y']).max())
    loss(y, x, g[tag + '_r_seed']).backward()
    edx = rel2(x.grad.cpu().numpy(), g[tag + '_dx'])
    print('%s: |y - golden| max %.2e, dx rel L2 %.2e' % (tag, ey, edx))
    assert ey < 2e-5
    assert edx < 2e-2
    check_grads(g[tag + '_g_l2'], g[tag + '_g_samp'], net, 2e-2)
    if str(g[tag + '_norm']) == 'batch':
        sd = net.state_dict()
        pre = tag + '_buf_'
        bufs = [k for k in g.files if k.startswith(pre)]
        assert len(bufs) == 3 * (3 + 2 * int(g[tag + '_n_blocks']) + 2)     # every norm layer: running_mean, running_var, num_batches_tracked
        for k in bufs:
            np.testing.assert_allclose(sd[k[len(pre):]].cpu().numpy(), g[k], rtol=2e-5, atol=1e-6, err_msg=k)
        net.eval()
        with torch.no_grad():
            ye = net(torch.from_numpy(rnd(g[tag + '_xe_seed'], shape)).to(DEV))
        np.testing.assert_allclose(ye.cpu().numpy(), g[tag + '_y_eval'], atol=2e-5, rtol=5e-4)


def test_output_size_and_no_grad_bits(golden):
    """30 x 22 -> 32 x 24 as in the reference; torch.no_grad() (no bias links) and a second run give the training-mode forward's bits."""
    tag = 'r6_in_drop_eval_30x22'
    net = build(golden, tag)
    x = torch.from_numpy(rnd(golden[tag + '_x_seed'], golden[tag + '_shape'])).to(DEV)
    y = net(x).detach()
    assert tuple(y.shape) == (1, 1, 32, 24)
    assert torch.equal(net(x).detach(), y)
    with torch.no_grad():
        assert torch.equal(net(x), y)
    net.train()     # Dropout active: the mask is drawn from torch's generator
    torch.manual_seed(3)
    a = net(x).detach()
    torch.manual_seed(3)
    assert torch.equal(net(x).detach(), a) and not torch.equal(a, y)


def _step(net, x, r_seed):
    xg = x.clone().requires_grad_(True)
    for p in net.parameters():
        p.grad = None
    y = net(xg)
    loss(y, xg, r_seed).backward()
    torch.cuda.synchronize()
    return y.detach(), xg.grad.clone(), [p.grad.clone() for p in net.parameters()]


def test_a_net_that_reaches_the_tiled_kernel():
    """resnet_6blocks, ngf 16, instance norm, x (4, 1, 256, 512): the blocks run at (4, 64, 64, 128) = 256 workgroups of the small tile."""
    L = lib()
    assert L.nc_conv2d_k3_reflect_active(0, 4, 64, 64, 128, 64) == 1 and L.nc_conv2d_k3_reflect_active(1, 4, 64, 64, 128, 64) == 1
    spec = S.resnet_spec(6, 16)
    net = networks.define_G(1, 1, 16, 'resnet_6blocks', 'instance', False, 'kaiming', 0.02, [0], dimension=2)
    net.load_state_dict(S.state_dict_from_seed(spec, 81, DEV))
    net.train()
    x = torch.from_numpy(rnd(82, (4, 1, 256, 512))).to(DEV)
    y, dx, grads = _step(net, x, 83)
    assert tuple(y.shape) == (4, 1, 256, 512) and float(y.std()) > 0.0

    # two runs: the same bits
    y2, dx2, grads2 = _step(net, x, 83)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))

    # the same step on the explicit-pad path
    prev = L.nc_get_conv2d_k3()
    L.nc_set_conv2d_k3(0)
    try:
        assert L.nc_conv2d_k3_reflect_active(0, 4, 64, 64, 128, 64) == 0
        y0, dx0, grads0 = _step(net, x, 83)
    finally:
        L.nc_set_conv2d_k3(prev)
    d = float((y - y0).abs().max())
    print('switch on - off: y %.2e, dx rel L2 %.2e' % (d, rel2(dx.cpu().numpy(), dx0.cpu().numpy())))
    assert d < 2e-5

    # the float64 restatement on the GPU; torch's float32 beside it runs on the CPU (the same modules the reference runs)
    names = [k for k, _ in net.named_parameters()]
    res = {}
    for dtype, dev in ((torch.float64, DEV), (torch.float32, 'cpu')):
        t0 = time.perf_counter()
        sd = {k: v.to(dtype).requires_grad_(True) for k, v in S.state_dict_from_seed(spec, 81, dev).items()}
        xr = x.to(dev).to(dtype).requires_grad_(True)
        yr, _ = R.resnet_forward(sd, xr, 6, 'instance', False, True)
        loss(yr, xr, 83).backward()
        res[dtype] = (yr.detach().to(DEV), xr.grad.to(DEV), [sd[k].grad.to(DEV) for k in names])
        torch.cuda.synchronize()
        print('restatement in %s on %s: %.1f s' % (dtype, dev, time.perf_counter() - t0))
    y64, dx64, g64 = res[torch.float64]
    y32, dx32, g32 = res[torch.float32]

    def rl2(a, b):
        return float(((a.double() - b.double()).pow(2).sum().sqrt() / b.double().pow(2).sum().sqrt().clamp_min(1e-30)))

    ey, ey32 = float((y.double() - y64).abs().max()), float((y32.double() - y64).abs().max())
    edx, edx32 = rl2(dx, dx64), rl2(dx32, dx64)
    print('against float64: y %.2e (torch fp32 %.2e), dx rel L2 %.2e (torch fp32 %.2e)' % (ey, ey32, edx, edx32))
    assert ey < 2e-5 and edx < 2e-2
    for k, a, b, c in zip(names, grads, g64, g32):
        num = float((a.double() - b).pow(2).sum().sqrt())
        den = float(b.pow(2).sum().sqrt())
        print('  %-36s rel L2 %.2e (torch fp32 %.2e), |g64| %.2e' % (k, num / max(den, 1e-30), rl2(c, b), den))
        # check_grads' absolute floor: a bias in front of an InstanceNorm has a zero true gradient, both sides hold rounding noise there
        assert num <= 2e-2 * den + 1e-6, k


def test_testmodel_end_to_end(tmp_path):
    """A seeded checkpoint saved under the reference's file name, loaded by TestModel with --netG resnet_9blocks --image_dimension 2
    (models/test_model.py:41-45): create_model -> setup -> set_input -> test(); `fake` is the bare net's output bit for bit."""
    from neuroclear_amd.models import create_model
    from neuroclear_amd.options import TestOptions
    ck = tmp_path / 'ckpt'
    (ck / 'm').mkdir(parents=True)
    (tmp_path / 'data').mkdir()
    spec = S.resnet_spec(9, 8)
    torch.save(S.state_dict_from_seed(spec, 91), str(ck / 'm' / 'iter_3_net_G.pth'))
    topt = TestOptions().parse(['--dataroot', str(tmp_path / 'data'), '--checkpoints_dir', str(ck), '--name', 'm', '--netG', 'resnet_9blocks',
                                '--ngf', '8', '--norm', 'instance', '--image_dimension', '2', '--load_iter', '3', '--gpu_ids', '0', '--no_dropout'])
    topt.continue_train = False
    tm = create_model(topt)
    tm.setup(topt)
    sd = S.state_dict_from_seed(spec, 91)
    assert list(tm.netG.state_dict().keys()) == list(sd.keys())
    assert torch.equal(tm.netG.model[19].weight.detach().cpu(), sd['model.19.weight']) and tuple(sd['model.19.weight'].shape) == (32, 16, 3, 3)
    a = torch.from_numpy(rnd(92, (1, 1, 36, 28)))
    tm.set_input({'A': a, 'A_paths': 'x'})
    tm.test()
    bare = networks.define_G(1, 1, 8, 'resnet_9blocks', 'instance', False, 'normal', 0.02, [0], dimension=2)
    bare.load_state_dict(S.state_dict_from_seed(spec, 91, DEV))
    with torch.no_grad():
        want = bare(a.to(DEV))
    assert tuple(tm.fake.shape) == (1, 1, 36, 28) and torch.equal(tm.fake, want)
    assert 0.0 < float(tm.fake.min()) and float(tm.fake.max()) < 1.0 and float(tm.fake.std()) > 0.0
