"""GPU tests of the KernelGAN patch discriminator (-m gpu): the fused nc_kgan_fwd / _bwd (csrc/kgan.hip) and the layered modules
against the reference (tests/golden/kernelgan_ops.npz), the fused path against fp64, fused against layered at Apollo's 108^2 planes,
run-to-run and cross-stream bits, the parameter-generation guard, and Apollo / Athena / Dryops steps with --netD kernelGAN against the
reference's own losses.  Tolerances are those of the PatchGAN golden tests (tests/test_gpu_nets.py::test_patchgan)."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from neuroclear_amd import _lib, ops  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

DEV = 'cuda'
CASES = ['in2_b3_36', 'in2_b2_20x27', 'in2_b1_8x7', 'in3_14x15x16', 'bn2_b2_20', 'none2_b2_20', 'in2_ndf32_b2_20']


def rnd(seed, shape):
    return np.random.default_rng(int(seed)).random(tuple(int(s) for s in shape), dtype=np.float32)


def rel2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def relmax(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-30))


def big_summary(a, n, key=55):
    a = np.asarray(a).ravel()
    idx = np.random.default_rng(key).integers(0, a.size, size=min(n, a.size))
    return np.concatenate([[np.sqrt((a.astype(np.float64) ** 2).sum()), a.astype(np.float64).sum()], a[idx].astype(np.float64)])


def make_net(nd, norm='instance', ndf=64, seed=5):
    net = networks.define_D(1, ndf, 'kernelGAN', 3, norm, 'normal', 0.02, False, [0], dimension=nd)
    w = S.weights_from_seed(S.kernelgan_spec(nd, 1, ndf, norm), seed)
    net.load_state_dict({k: torch.from_numpy(v).to(DEV) for k, v in w.items()}, strict=False)
    return net


def run(net, x_np, r_np, want_params=True):
    for p in net.parameters():
        p.grad = None
        p.requires_grad_(want_params)
    x = torch.from_numpy(x_np).to(DEV).requires_grad_(True)
    y = net(x)
    (y * torch.from_numpy(r_np).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = [p.grad.detach().cpu().numpy().copy() if p.grad is not None else None for p in net.parameters()]
    return y.detach().cpu().numpy(), x.grad.cpu().numpy(), grads


def case_inputs(g, tag):
    shape = tuple(int(s) for s in g[tag + '_shape'])
    x = rnd(g[tag + '_x_seed'], shape) - np.float32(0.5)
    nd = int(g[tag + '_nd'])
    oshape = (shape[0], 1) + tuple(s - 6 for s in shape[2:])
    r = np.random.default_rng(int(g[tag + '_r_seed'])).standard_normal(oshape).astype(np.float32)
    return x, r, nd


def _cmp(g, key, got, bound, scale=None):
    n = int(g['summary_n'])
    if key in g:
        ref = g[key]
        if scale is None:
            return rel2(got, ref) < bound, rel2(got, ref)
        err = float(np.abs(got - ref).max()) / scale
        return err < bound, err
    s = g[key + '_sum']
    mine = big_summary(got, n)
    if scale is None:
        err = max(abs(mine[0] - s[0]) / max(abs(s[0]), 1e-30), rel2(mine[2:], s[2:]))
    else:
        err = float(np.abs(mine[2:] - s[2:]).max()) / scale
    return err < bound, err


@pytest.mark.parametrize('tag', CASES)
def test_golden(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, 'kernelgan_ops.npz'), allow_pickle=False)
    x_np, r_np, nd = case_inputs(g, tag)
    norm, ndf = str(g[tag + '_norm']), int(g[tag + '_ndf'])
    net = make_net(nd, norm, ndf, int(g[tag + '_seed']))
    net.train()
    if norm == 'instance' and ndf == 64:
        assert net._fused_on(torch.from_numpy(x_np).to(DEV))
    y, dx, grads = run(net, x_np, r_np)
    ok, err = _cmp(g, tag + '_y', y, 5e-4) if (tag + '_y') not in g else (relmax(y, g[tag + '_y']) < 5e-4, relmax(y, g[tag + '_y']))
    assert ok, ('y', err)
    ok, err = _cmp(g, tag + '_dx', dx, 1e-3)
    assert ok, ('dx', err)
    names = [k for k, _ in net.named_parameters()]
    wscale = max(float(np.abs(gr).max()) for k, gr in zip(names, grads) if k.endswith('weight') and gr.ndim > 1)
    for j, (k, gr) in enumerate(zip(names, grads)):
        cancelled = norm == 'instance' and k.endswith('bias') and not k.startswith('final_layer')
        if cancelled:  # zero up to rounding: the InstanceNorm behind these layers cancels any bias
            ok, err = _cmp(g, tag + '_g%d' % j, gr, 1e-4, scale=wscale)
        else:
            ok, err = _cmp(g, tag + '_g%d' % j, gr, 1e-3)
        assert ok, (k, err)
    if norm == 'batch':
        for j in (1, 4, 7):
            m = net.feature_block[j]
            assert rel2(m.running_mean.cpu().numpy(), g[tag + '_rm%d' % j]) < 1e-3
            assert rel2(m.running_var.cpu().numpy(), g[tag + '_rv%d' % j]) < 1e-3


def ref64(x_np, r_np, net, nd):
    conv = F.conv2d if nd == 2 else F.conv3d
    prm = [p.detach().cpu().double().requires_grad_(True) for p in net.parameters()]
    w1, b1, w2, b2, w3, b3, w4, b4, w5, b5 = prm
    x = torch.from_numpy(x_np).double().requires_grad_(True)
    h = conv(conv(x, w1, b1), w2, b2)
    h = F.relu(F.instance_norm(h, eps=1e-5))
    h = F.relu(F.instance_norm(conv(h, w3, b3), eps=1e-5))
    h = F.relu(F.instance_norm(conv(h, w4, b4), eps=1e-5))
    y = conv(h, w5, b5)
    (y * torch.from_numpy(r_np).double()).sum().backward()
    return y.detach().numpy(), x.grad.numpy(), [p.grad.numpy() for p in prm]


@pytest.mark.parametrize('nd,shape', [(2, (3, 1, 36, 36)), (3, (1, 1, 14, 15, 16)), (2, (2, 1, 13, 15))])
def test_against_fp64(nd, shape, monkeypatch):
    """The fused path's error against fp64 is no worse than twice the layered fp32 path's on the same case (y, dx, every weight and every
    bias gradient; the third shape has P = 63, P % 4 != 0: the scalar instantiation of the 1x1 kernels).  The bias gradients in front of an
    InstanceNorm are zero up to rounding: their error is taken on the weight gradients' scale, as in test_golden."""
    net = make_net(nd)
    x_np = rnd(11, shape) - np.float32(0.5)
    oshape = (shape[0], 1) + tuple(s - 6 for s in shape[2:])
    r_np = np.random.default_rng(12).standard_normal(oshape).astype(np.float32)
    y64, dx64, g64 = ref64(x_np, r_np, net, nd)
    fused = run(net, x_np, r_np)
    monkeypatch.setenv('NC_FUSED_KGAN', '0')
    layered = run(net, x_np, r_np)
    names = [k for k, _ in net.named_parameters()]
    wscale = max(float(np.abs(gr).max()) for k, gr in zip(names, g64) if k.endswith('weight') and gr.ndim > 1)
    pairs = [('y', fused[0], layered[0], y64), ('dx', fused[1], layered[1], dx64)]
    pairs += list(zip(names, fused[2], layered[2], g64))
    for k, a, b, ref in pairs:
        if k.endswith('bias') and not k.startswith('final_layer'):
            ea, eb = float(np.abs(a - ref).max()) / wscale, float(np.abs(b - ref).max()) / wscale
        else:
            ea, eb = rel2(a, ref), rel2(b, ref)
        print(k, ea, eb)
        assert ea <= 2 * eb + 1e-7, (k, ea, eb)


def test_fused_matches_layered_108(monkeypatch):
    """Apollo's discriminator call: B = 108 planes of 108^2."""
    net = make_net(2)
    x_np = rnd(13, (108, 1, 108, 108))
    r_np = np.random.default_rng(14).standard_normal((108, 1, 102, 102)).astype(np.float32)
    yf, dxf, gf = run(net, x_np, r_np)
    monkeypatch.setenv('NC_FUSED_KGAN', '0')
    yl, dxl, gl = run(net, x_np, r_np)
    assert relmax(yf, yl) < 5e-4
    assert rel2(dxf, dxl) < 1e-3
    names = [k for k, _ in net.named_parameters()]
    for k, a, b in zip(names, gf, gl):
        if k.endswith('weight') or k.startswith('final_layer'):
            assert rel2(a, b) < 1e-3, (k, rel2(a, b))


def test_dparams_null_same_dx_and_bits():
    net = make_net(2)
    x_np = rnd(15, (4, 1, 40, 33)) - np.float32(0.5)
    r_np = np.random.default_rng(16).standard_normal((4, 1, 34, 27)).astype(np.float32)
    y1, dx1, g1 = run(net, x_np, r_np)
    y2, dx2, g2 = run(net, x_np, r_np)
    assert np.array_equal(y1, y2) and np.array_equal(dx1, dx2)
    assert all(np.array_equal(a, b) for a, b in zip(g1, g2))
    y3, dx3, g3 = run(net, x_np, r_np, want_params=False)  # dparams = NULL
    assert all(g is None for g in g3)
    assert np.array_equal(y1, y3) and np.array_equal(dx1, dx3)


def test_two_streams_same_bits():
    nets = [make_net(2, seed=31), make_net(2, seed=32)]
    xs = [rnd(17 + i, (8, 1, 60, 60)) for i in range(2)]
    rs = [np.random.default_rng(19 + i).standard_normal((8, 1, 54, 54)).astype(np.float32) for i in range(2)]
    serial = [run(n, x, r) for n, x, r in zip(nets, xs, rs)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = [None, None]
    xt = [torch.from_numpy(x).to(DEV).requires_grad_(True) for x in xs]
    rt = [torch.from_numpy(r).to(DEV) for r in rs]
    for n in nets:
        for p in n.parameters():
            p.grad = None
    torch.cuda.synchronize()
    for i in range(2):
        with torch.cuda.stream(streams[i]):
            y = nets[i](xt[i])
            (y * rt[i]).sum().backward()
            outs[i] = y
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(outs[i].detach().cpu().numpy(), serial[i][0])
        assert np.array_equal(xt[i].grad.cpu().numpy(), serial[i][1])
        for p, g in zip(nets[i].parameters(), serial[i][2]):
            assert np.array_equal(p.grad.cpu().numpy(), g)


def test_parameter_update_between_fwd_and_bwd_raises():
    net = make_net(2)
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    params, off = [], 0
    for p in net.parameters():
        params.append(flat[off:off + p.numel()].view(p.shape).requires_grad_(True))
        off += p.numel()
    x = torch.from_numpy(rnd(21, (2, 1, 20, 20))).to(DEV)
    y = ops.kernelgan(x, params, 2)
    ops.bump_param_generation(flat)
    with pytest.raises(_lib.NcError):
        y.sum().backward()


def test_c_api_rejects_small_inputs():
    L, I = _lib.lib(), _lib.I
    assert L.nc_kgan_out_shape(I(1), I(1), I(7), I(7), I(64), I(2), None, None, None) != 0
    assert 'one element' in L.nc_last_error().decode()
    assert L.nc_kgan_out_shape(I(1), I(1), I(6), I(9), I(64), I(2), None, None, None) != 0
    assert L.nc_kgan_out_shape(I(1), I(1), I(8), I(7), I(64), I(2), None, None, None) == 0


# ---- model steps --------------------------------------------------------------------------------------------------------------
APOLLO_NETS = ['G_A', 'G_B', 'D_A_axial', 'D_A_lateral', 'D_B_axial', 'D_B_lateral']
ATHENA_NETS = ['G_A', 'G_B', 'D_A_yz', 'D_A_xy', 'D_A_xz', 'D_B_yz', 'D_B_xy', 'D_B_xz']
DRYOPS_NETS = ['G_A', 'D_A_axial', 'D_A_lateral']


def _opt(model='axial_to_lateral_gan_apollo'):
    return Namespace(gpu_ids=[0], isTrain=True, image_dimension=3, checkpoints_dir='/tmp/nc_ckpt', name='t',
                     preprocess='none', gan_mode='lsgan', randomize_projection_depth=True, projection_depth=10,
                     min_projection_depth=2, lambda_plane=[1, 1, 1], lambda_A=5.0, input_nc=1, output_nc=1, ngf=64,
                     ndf=64, netG='unet_deconv', netG_B='deep_linear_gen', netD='kernelGAN', n_layers_D=3,
                     norm='instance', no_dropout=True, init_type='kaiming', init_gain=0.02, lr=1e-4, beta1=0.1,
                     direction='AtoB', model=model)


def _load(net, spec, seed):
    net.load_state_dict(S.state_dict_from_seed(spec, seed, DEV))


def _steps(model, nets, specs, g, size, step_seed):
    for i, (n, sp) in enumerate(zip(nets, specs)):
        _load(getattr(model, 'net' + n), sp, int(g['net_seed0']) + i)
    before = {n: [p.detach().clone() for p in getattr(model, 'net' + n).parameters()] for n in nets}
    real = torch.from_numpy(rnd(g['real_seed'], (1, 1, size, size, size)))
    if step_seed is not None:
        np.random.seed(step_seed)
    names = [str(s) for s in g['loss_names']]
    for it in range(2):
        model.set_input({'A': real, 'A_paths': 'x'})
        model.optimize_parameters()
        L = model.get_current_losses()
        got = np.array([L[n] for n in names])
        print(it, dict(zip(names, got)), g['losses'][it])
        np.testing.assert_allclose(got, g['losses'][it], rtol=2e-5 if it == 0 else 5e-3, err_msg='step %d' % it)
        if it == 0 and 'fake0' in g:
            assert float(np.abs(model.fake.detach().cpu().numpy() - g['fake0']).max()) < 2e-5
    for n in nets:
        ps = list(getattr(model, 'net' + n).parameters())
        upd = np.array([float((a.detach() - b).double().norm()) for a, b in zip(ps, before[n])])
        sel = np.array([a.dim() > 1 for a in ps])
        np.testing.assert_allclose(upd[sel], g['upd_' + n][sel], rtol=5e-2, err_msg=n)


@pytest.mark.parametrize('d_streams', [True, False])
def test_apollo_step_kgan(golden_dir, d_streams, monkeypatch):
    from neuroclear_amd.models import create_model
    from neuroclear_amd.models.axial_to_lateral_gan_apollo_model import AxialToLateralGANApolloModel
    monkeypatch.setattr(AxialToLateralGANApolloModel, '_d_streams_on', d_streams)
    g = np.load(os.path.join(golden_dir, 'apollo_step_36_kgan.npz'), allow_pickle=False)
    model = create_model(_opt())
    specs = [S.unet_deconv_spec(), S.deep_linear_spec()] + [S.kernelgan_spec(2)] * 4
    _steps(model, APOLLO_NETS, specs, g, int(g['size']), int(g['step_seed']))


def test_athena_step_kgan(golden_dir):
    from neuroclear_amd.models import create_model
    g = np.load(os.path.join(golden_dir, 'athena_step_36_kgan.npz'), allow_pickle=False)
    opt = _opt('axial_to_lateral_gan_athena')
    opt.conversion_plane = ['yz', 'xy']
    opt.pool_size = 50
    model = create_model(opt)
    specs = [S.unet_deconv_spec(), S.deep_linear_spec()] + [S.kernelgan_spec(2)] * 6
    _steps(model, ATHENA_NETS, specs, g, int(g['size']), None)


def test_dryops_step_kgan(golden_dir):
    from neuroclear_amd.models import create_model
    g = np.load(os.path.join(golden_dir, 'dryops_step_deconv_kgan_36.npz'), allow_pickle=False)
    model = create_model(_opt('axial_to_lateral_gan_dryops'))
    specs = [S.unet_deconv_spec(), S.kernelgan_spec(2), S.kernelgan_spec(2)]
    _steps(model, DRYOPS_NETS, specs, g, int(g['size']), int(g['step_seed']))


def test_apollo_108_kgan():
    """One full-size Apollo step (108^3 crop, its discriminators on side streams) with --netD kernelGAN: finite losses."""
    from neuroclear_amd.models import create_model
    model = create_model(_opt())
    for i, (n, sp) in enumerate(zip(APOLLO_NETS, [S.unet_deconv_spec(), S.deep_linear_spec()] + [S.kernelgan_spec(2)] * 4)):
        _load(getattr(model, 'net' + n), sp, 40 + i)
    np.random.seed(1234)
    model.set_input({'A': torch.from_numpy(rnd(5, (1, 1, 108, 108, 108))), 'A_paths': 'x'})
    model.optimize_parameters()
    L = model.get_current_losses()
    assert all(np.isfinite(v) for v in L.values()), L
