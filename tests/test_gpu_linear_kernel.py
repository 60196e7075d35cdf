"""GPU tests of the learned-PSF generators (-m gpu): nc_lk_fwd / _dgrad / _wgrad (csrc/conv_lk.hip) against fp64, run-to-run bits, the
reference's LinearKernel / LinearKernel_double (tests/golden/linear_kernel_ops.npz), Apollo / Athena steps with --netG_B linearkernel*
against the reference's own losses, a full-size 108^3 Apollo step with linearkernel_LK31, diced inference through TestModel and the
precision switch.

fp64 references are scipy.signal.correlate (FFT) on the CPU.  Bounds: per element |err| <= 2e-6 (|w| * |x|) for the forward and the data
gradient, <= 2e-6 sum |x dy| per tap for the weight gradient, each plus a floor of 1e-12 of the largest |operands| result (the FFT's
own rounding where the exact result is 0)."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch
from scipy import signal

pytestmark = pytest.mark.gpu

from neuroclear_amd import ops  # noqa: E402
from neuroclear_amd._lib import I, P, Z, check, lib  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

DEV = 'cuda'


def G(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def rnd(seed, shape):
    return np.random.default_rng(int(seed)).random(tuple(int(s) for s in shape), dtype=np.float32)


def _p(t):
    return P(t.data_ptr())


def _st():
    return P(torch.cuda.current_stream().cuda_stream)


def lk_fwd(x, w, flip=False):
    N, _, D, H, W = x.shape
    y = torch.empty_like(x)
    fn = lib().nc_lk_dgrad if flip else lib().nc_lk_fwd
    check(fn(_p(x), _p(w), _p(y), I(N), I(D), I(H), I(W), I(w.shape[-1]), P(0), Z(0), _st()), 'nc_lk')
    return y


def lk_wgrad(x, dy, k):
    N, _, D, H, W = x.shape
    nb = lib().nc_lk_ws_bytes(I(N), I(D), I(H), I(W), I(k))
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=x.device)
    dw = torch.empty((1, 1, k, k, k), dtype=torch.float32, device=x.device)
    check(lib().nc_lk_wgrad(_p(x), _p(dy), _p(dw), I(N), I(D), I(H), I(W), I(k), _p(ws), Z(nb), _st()), 'nc_lk_wgrad')
    return dw


def ref_fwd(x, w):
    """fp64 Conv3d(1, 1, k, padding (k - 1) / 2) (a correlation) per batch item."""
    return np.stack([signal.correlate(x[n, 0].astype(np.float64), w[0, 0].astype(np.float64), mode='same', method='fft')[None]
                     for n in range(x.shape[0])])


def ref_wgrad(x, dy, k):
    p = k // 2
    out = 0.0
    for n in range(x.shape[0]):
        xp = np.pad(x[n, 0].astype(np.float64), p)
        out = out + signal.correlate(xp, dy[n, 0].astype(np.float64), mode='valid', method='fft')
    return out[None, None]


def within(got, want, absref):
    """max of |got - want| / (2e-6 absref + 1e-12 max absref); absref = the same operation on |operands| (FFT: ~1e-16 noise around 0)."""
    absref = np.abs(absref)
    bound = 2e-6 * absref + 1e-12 * float(absref.max())
    err = np.abs(got.astype(np.float64) - want)
    return float((err / bound).max())


def case(seed, N, D, H, W, k):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, 1, D, H, W)).astype(np.float32)
    dy = rng.standard_normal((N, 1, D, H, W)).astype(np.float32)
    w = rng.standard_normal((1, 1, k, k, k)).astype(np.float32)
    # zero-filled regions: a slab of the input, a corner of the output gradient
    x[:, :, :, : max(1, H // 5)] = 0
    dy[:, :, : max(1, D // 3), :, W // 2:] = 0
    return x, dy, w


SHAPES = [(1, 37, 29, 45), (2, 9, 14, 21), (1, 8, 40, 12)]


@pytest.mark.parametrize('k', [3, 5, 9, 15, 31])
@pytest.mark.parametrize('shape', SHAPES)
def test_lk_ops_against_fp64(k, shape):
    x, dy, w = case(k * 100 + shape[1], *shape, k)
    X, DY, Wt = (torch.from_numpy(a).to(DEV) for a in (x, dy, w))
    wf = w[:, :, ::-1, ::-1, ::-1].copy()
    y = lk_fwd(X, Wt).cpu().numpy()
    dx = lk_fwd(DY, Wt, flip=True).cpu().numpy()
    dw = lk_wgrad(X, DY, k).cpu().numpy()
    ry, rdx, rdw = ref_fwd(x, w), ref_fwd(dy, wf), ref_wgrad(x, dy, k)
    assert within(y, ry, ref_fwd(np.abs(x), np.abs(w))) <= 1.0
    assert within(dx, rdx, ref_fwd(np.abs(dy), np.abs(wf))) <= 1.0
    assert within(dw, rdw, ref_wgrad(np.abs(x), np.abs(dy), k)) <= 1.0
    if k <= 9 and shape[0] == 1:
        # the generic direct (VALU) path on the same problem: the new path's rms error against fp64 is at most twice its
        rms = lambda a, b: float(np.sqrt(((a.astype(np.float64) - b) ** 2).mean()))  # noqa: E731
        ops.set_force_direct(True)
        try:
            gy = ops.conv_fwd_raw(X, Wt, None, 1, k // 2).cpu().numpy()
            gdx = ops.conv_dgrad_raw(DY, Wt, X.shape, 1, k // 2).cpu().numpy()
            gdw = ops.conv_wgrad_raw(X, DY, Wt.shape, 1, k // 2, False)[0].cpu().numpy()
        finally:
            ops.set_force_direct(False)
        for got, gen, ref in ((y, gy, ry), (dx, gdx, rdx), (dw, gdw, rdw)):
            print('rms lk %.3e direct %.3e' % (rms(got, ref), rms(gen, ref)))
            assert rms(got, ref) <= 2 * rms(gen, ref) + 1e-30


def test_lk_bad_shapes():
    x = torch.zeros(1, 1, 8, 8, 8, device=DEV)
    w = torch.zeros(1, 1, 4, 4, 4, device=DEV)
    for k in (1, 4, 33):
        assert lib().nc_lk_fwd(_p(x), _p(w), _p(x), I(1), I(8), I(8), I(8), I(k), P(0), Z(0), _st()) == -1
    assert lib().nc_lk_fwd(_p(x), _p(w), _p(x), I(1), I(0), I(8), I(8), I(3), P(0), Z(0), _st()) == -1
    assert lib().nc_lk_wgrad(_p(x), _p(x), _p(w), I(1), I(8), I(8), I(8), I(3), P(0), Z(0), _st()) == -2  # no workspace


@pytest.mark.parametrize('k', [9, 31])
def test_lk_deterministic(k):
    x, dy, w = case(7, 1, 40, 36, 52, k)
    X, DY, Wt = (torch.from_numpy(a).to(DEV) for a in (x, dy, w))
    for fn in (lambda: lk_fwd(X, Wt), lambda: lk_fwd(DY, Wt, True), lambda: lk_wgrad(X, DY, k)):
        a, b = fn(), fn()
        assert torch.equal(a, b)


@pytest.mark.parametrize('tag,cls', [('lk9', 'LinearKernel'), ('lk31', 'LinearKernel'), ('lk9double', 'LinearKernel_double')])
def test_modules_match_reference(golden_dir, tag, cls):
    g = G(golden_dir, 'linear_kernel_ops.npz')
    k = int(g[tag + '_k'])
    net = getattr(networks, cls)(1, 1, k).to(DEV)
    net.load_state_dict(S.state_dict_from_seed(S.linear_kernel_spec(k), int(g[tag + '_seed']), DEV))
    shape = tuple(int(s) for s in g['shape'])
    x = (torch.from_numpy(rnd(g['x_seed'], shape)) - 0.5).to(DEV).requires_grad_(True)
    r = torch.from_numpy(np.random.default_rng(int(g['r_seed'])).standard_normal(shape).astype(np.float32)).to(DEV)
    y = net(x)
    (y * r).sum().backward()
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())  # noqa: E731
    assert rel(y.detach().cpu().numpy(), g[tag + '_y']) < 1e-5
    assert rel(x.grad.cpu().numpy(), g[tag + '_dx']) < 1e-5
    dw = net.convlayer.weight.grad.cpu().numpy()
    assert rel(dw, g[tag + '_dw']) < 1e-5
    if cls == 'LinearKernel_double':
        # the shared weight receives BOTH contributions: either one alone is far from the reference
        w = net.convlayer.weight.detach()
        h = ops.linear_kernel(x.detach(), w)
        one = lk_wgrad(h.contiguous(), r, k).cpu().numpy()  # the outer application's term only
        assert rel(one, g[tag + '_dw']) > 1e-2


def _apollo_opt(netG_B):
    return Namespace(gpu_ids=[0], isTrain=True, image_dimension=3, checkpoints_dir='/tmp/nc_ckpt', name='t',
                     preprocess='none', gan_mode='lsgan', randomize_projection_depth=True, projection_depth=10,
                     min_projection_depth=2, lambda_plane=[1, 1, 1], lambda_A=5.0, input_nc=1, output_nc=1, ngf=64,
                     ndf=64, netG='unet_deconv', netG_B=netG_B, netD='basic', n_layers_D=3,
                     norm='instance', no_dropout=True, init_type='kaiming', init_gain=0.02, lr=1e-4, beta1=0.1,
                     direction='AtoB', model='axial_to_lateral_gan_apollo')


APOLLO_NETS = ['G_A', 'G_B', 'D_A_axial', 'D_A_lateral', 'D_B_axial', 'D_B_lateral']
ATHENA_NETS = ['G_A', 'G_B', 'D_A_yz', 'D_A_xy', 'D_A_xz', 'D_B_yz', 'D_B_xy', 'D_B_xz']


def _load(net, spec, seed):
    net.load_state_dict(S.state_dict_from_seed(spec, seed, DEV))


@pytest.mark.parametrize('tag', ['lk9', 'lk9double', 'lk31'])
@pytest.mark.parametrize('d_streams', [True, False])
def test_apollo_step_lk(golden_dir, tag, d_streams, monkeypatch):
    """Same tolerances as tests/test_gpu_nets.py::test_apollo_step."""
    from neuroclear_amd.models import create_model
    from neuroclear_amd.models.axial_to_lateral_gan_apollo_model import AxialToLateralGANApolloModel
    monkeypatch.setattr(AxialToLateralGANApolloModel, '_d_streams_on', d_streams)
    g = G(golden_dir, 'apollo_step_36_%s.npz' % tag)
    size, k = int(g['size']), int(g['k'])
    model = create_model(_apollo_opt(str(g['netG_B'])))
    specs = [S.unet_deconv_spec(), S.linear_kernel_spec(k)] + [S.patchgan_spec(2)] * 4
    for i, (n, sp) in enumerate(zip(APOLLO_NETS, specs)):
        _load(getattr(model, 'net' + n), sp, int(g['net_seed0']) + i)
    before = {n: [p.detach().clone() for p in getattr(model, 'net' + n).parameters()] for n in APOLLO_NETS}
    real = torch.from_numpy(rnd(g['real_seed'], (1, 1, size, size, size)))
    np.random.seed(int(g['step_seed']))
    names = [str(s) for s in g['loss_names']]
    for it in range(2):
        model.set_input({'A': real, 'A_paths': 'x'})
        model.optimize_parameters()
        L = model.get_current_losses()
        got = np.array([L[n] for n in names])
        print(it, dict(zip(names, got)), g['losses'][it])
        np.testing.assert_allclose(got, g['losses'][it], rtol=2e-5 if it == 0 else 5e-3, err_msg='step %d' % it)
        if it == 0:
            assert float(np.abs(model.fake.detach().cpu().numpy() - g['fake0']).max()) < 2e-5
            rec = model.rec.detach().cpu().numpy()
            assert float(np.abs(rec - g['rec0']).max() / np.abs(g['rec0']).max()) < 2e-4
    for n in APOLLO_NETS:
        ps = list(getattr(model, 'net' + n).parameters())
        upd = np.array([float((a.detach() - b).double().norm()) for a, b in zip(ps, before[n])])
        sel = np.array([a.dim() > 1 for a in ps])
        np.testing.assert_allclose(upd[sel], g['upd_' + n][sel], rtol=5e-2, err_msg=n)


def test_athena_step_lk9(golden_dir):
    """Same tolerances as tests/test_gpu_nets.py::test_athena_step."""
    from neuroclear_amd.models import create_model
    g = G(golden_dir, 'athena_step_36_lk9.npz')
    size, k = int(g['size']), int(g['k'])
    opt = _apollo_opt(str(g['netG_B']))
    opt.model = 'axial_to_lateral_gan_athena'
    opt.conversion_plane = ['yz', 'xy']
    opt.pool_size = 50
    model = create_model(opt)
    specs = [S.unet_deconv_spec(), S.linear_kernel_spec(k)] + [S.patchgan_spec(2)] * 6
    for i, (n, sp) in enumerate(zip(ATHENA_NETS, specs)):
        _load(getattr(model, 'net' + n), sp, int(g['net_seed0']) + i)
    before = {n: [p.detach().clone() for p in getattr(model, 'net' + n).parameters()] for n in ATHENA_NETS}
    real = torch.from_numpy(rnd(g['real_seed'], (1, 1, size, size, size)))
    names = [str(s) for s in g['loss_names']]
    for it in range(2):
        model.set_input({'A': real, 'A_paths': 'x'})
        model.optimize_parameters()
        L = model.get_current_losses()
        got = np.array([L[n] for n in names])
        np.testing.assert_allclose(got, g['losses'][it], rtol=2e-5 if it == 0 else 5e-3, err_msg='step %d' % it)
    for n in ATHENA_NETS:
        ps = list(getattr(model, 'net' + n).parameters())
        upd = np.array([float((a.detach() - b).double().norm()) for a, b in zip(ps, before[n])])
        sel = np.array([a.dim() > 1 for a in ps])
        np.testing.assert_allclose(upd[sel], g['upd_' + n][sel], rtol=5e-2, err_msg=n)


def test_apollo_108_lk31():
    """Full size: two Apollo steps at 108^3 with linearkernel_LK31.  rec = G_B(fake) at 4096 sampled voxels and G_B's weight gradient
    at 256 sampled taps against fp64 (numpy; each tap a dot product over the volume), both from the GPU's own tensors."""
    from neuroclear_amd.models import create_model
    size, k, p = 108, 31, 15
    model = create_model(_apollo_opt('linearkernel_LK31'))
    specs = [S.unet_deconv_spec(), S.linear_kernel_spec(k)] + [S.patchgan_spec(2)] * 4
    for i, (n, sp) in enumerate(zip(APOLLO_NETS, specs)):
        _load(getattr(model, 'net' + n), sp, 40 + i)
    np.random.seed(5)
    real = torch.from_numpy(rnd(9, (1, 1, size, size, size)))
    grads = []
    model.netG_B.convlayer.weight.register_hook(lambda g_: grads.append(g_.detach().clone()))
    w0 = model.netG_B.convlayer.weight.detach().clone()
    for it in range(2):
        model.set_input({'A': real, 'A_paths': 'x'})
        model.optimize_parameters()
        L = model.get_current_losses()
        assert all(np.isfinite(v) for v in L.values()), L
        if it == 0:
            fake = model.fake.detach().double().cpu().numpy()[0, 0]
            rec = model.rec.detach().cpu().numpy()[0, 0]
    w = w0.double().cpu().numpy()[0, 0]
    fp = np.pad(fake, p)
    rng = np.random.default_rng(3)
    vox = rng.integers(0, size, size=(4096, 3))
    errs, bnds = [], []
    for z, y, x in vox:
        win = fp[z:z + k, y:y + k, x:x + k]
        errs.append(abs(rec[z, y, x] - (win * w).sum()))
        bnds.append(2e-6 * (np.abs(win) * np.abs(w)).sum())
    errs, bnds = np.array(errs), np.array(bnds)
    assert float((errs / (bnds + 1e-12 * bnds.max())).max()) <= 1.0
    # G_B's weight gradient of the first step: the generator loss's d/dw = sum over voxels of fake(shifted) * d loss / d rec.  The hook
    # saw the gradient arriving at the weight; recompute it from the tensors autograd used: rec's gradient is not kept, so the check is
    # made on a fresh backward of a seeded linear functional of G_B(fake) with the step-0 weight
    fk = model.fake.detach().clone()  # step 1's fake: any fixed input serves
    wt = w0.clone().requires_grad_(True)
    r = torch.from_numpy(np.random.default_rng(4).standard_normal((1, 1, size, size, size)).astype(np.float32)).to(DEV)
    (ops.linear_kernel(fk, wt) * r).sum().backward()
    dw = wt.grad.double().cpu().numpy()[0, 0]
    fkn, rn = np.pad(fk.double().cpu().numpy()[0, 0], p), r.double().cpu().numpy()[0, 0]
    taps = rng.integers(0, k, size=(256, 3))
    for a, b, c in taps:
        prod = fkn[a:a + size, b:b + size, c:c + size] * rn
        want, bnd = prod.sum(), 2e-6 * np.abs(prod).sum()
        assert abs(dw[a, b, c] - want) <= bnd, (a, b, c, dw[a, b, c], want)
    assert len(grads) == 2 and all(bool(torch.isfinite(g_).all()) for g_ in grads)


def test_diced_inference_testmodel(tmp_path):
    """TestModel with --netG linearkernel --model_suffix _B loads a saved G_B and its diced inference (cubes batched: N > 1) equals per-cube
    fp64 convolution to 1 LSB."""
    from neuroclear_amd import test_dice as td
    from neuroclear_amd.models import create_model
    from neuroclear_amd.options import TestOptions
    from oracle import dice as odice
    ck = tmp_path / 'ckpt'
    (ck / 'm').mkdir(parents=True)
    (tmp_path / 'data').mkdir()
    sd = S.state_dict_from_seed(S.linear_kernel_spec(9), 17)
    sd['convlayer.weight'] = sd['convlayer.weight'].abs() / sd['convlayer.weight'].abs().sum()  # a normalised PSF: output in [0, 1]
    torch.save(sd, str(ck / 'm' / 'iter_3_net_G_B.pth'))
    topt = TestOptions().parse(['--dataroot', str(tmp_path / 'data'), '--checkpoints_dir', str(ck), '--name', 'm', '--model_suffix', '_B',
                                '--netG', 'linearkernel', '--load_iter', '3', '--gpu_ids', '0', '--no_dropout'])
    topt.continue_train = False
    tm = create_model(topt)
    tm.setup(topt)
    assert torch.equal(tm.netG.convlayer.weight.detach().cpu(), sd['convlayer.weight'])
    vol = S.random_volume(2, (40, 40, 40))
    opt = Namespace(dice_size=[24, 24, 24], overlap=4, border_cut=4, gpu_ids=[0], skip_real=True, data_type='uint16',
                    histogram_match=False, normalize_intensity=False)
    with torch.no_grad():
        got = td.diced_inference(tm.netG, vol, opt, assemble='reduce')
    padded = odice.pad_for_dicing(vol, 24, 4)
    steps = odice.grid_steps(padded.shape, 24, 4)
    refl = odice.reflect_pad(padded, 4)
    n = int(np.prod(steps))
    w = sd['convlayer.weight'].numpy()
    outs = [ref_fwd(odice.normalize(odice.cut_cube(refl, i, steps, 24, 4, 4))[None, None], w)[0, 0] for i in range(n)]
    want = odice.assemble(outs, padded.shape, vol.shape, 24, 4, 4, 'uint16')
    d = int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max())
    assert d <= 1, d


def test_precision_switch_keeps_fp32():
    net = networks.define_G(1, 1, 64, 'linearkernel', 'instance', False, 'normal', 0.02, [0])
    x = torch.rand(2, 1, 30, 34, 26, device=DEV)
    with torch.no_grad():
        y32 = net(x)
        prev = ops.conv_precision
        try:
            for name in ('bf16', 'fp16'):
                ops.set_conv_precision(name)
                assert torch.equal(net(x), y32), name
        finally:
            ops.set_conv_precision(prev)
