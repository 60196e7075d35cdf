"""Golden vectors of the KernelGAN patch discriminator (--netD kernelGAN), from the REFERENCE itself on the CPU, with the helpers of
oracle.gen_golden.

    python tools/gen_golden_kernelgan.py            (from the repo root; needs the reference checkout that oracle.gen_golden names)

Writes tests/golden/kernelgan_ops.npz, apollo_step_36_kgan.npz, athena_step_36_kgan.npz and dryops_step_deconv_kgan_36.npz.  Weights
are not stored: both sides rebuild them with neuroclear_amd.util.seed.weights_from_seed(kernelgan_spec(...), seed)."""
import contextlib
import io
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oracle import gen_golden as gg  # noqa: E402
from oracle.gen_golden import _opt_train, big_summary, load_sd, rand_input, ref_modules  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

# (tag, nd, norm, ndf, input shape, weight seed, full gradients?)
OPS_CASES = [
    ('in2_b3_36', 2, 'instance', 64, (3, 1, 36, 36), 21, True),
    ('in2_b2_20x27', 2, 'instance', 64, (2, 1, 20, 27), 22, True),
    ('in2_b1_8x7', 2, 'instance', 64, (1, 1, 8, 7), 23, True),
    ('in3_14x15x16', 3, 'instance', 64, (1, 1, 14, 15, 16), 24, False),
    ('bn2_b2_20', 2, 'batch', 64, (2, 1, 20, 20), 25, False),
    ('none2_b2_20', 2, 'none', 64, (2, 1, 20, 20), 26, False),
    ('in2_ndf32_b2_20', 2, 'instance', 32, (2, 1, 20, 20), 27, False),
]
SUMMARY_N = 1024  # arrays above this many elements go in as big_summary(a, SUMMARY_N) unless the case keeps full gradients


def _store(out, key, a, full):
    a = np.asarray(a)
    if full or a.size <= SUMMARY_N:
        out[key] = a.astype(np.float32)
    else:
        out[key + '_sum'] = big_summary(a, SUMMARY_N)


def gen_ops(networks):
    out = dict(cases=np.array([c[0] for c in OPS_CASES]), summary_n=SUMMARY_N)
    for i, (tag, nd, norm, ndf, shape, seed, full) in enumerate(OPS_CASES):
        net = networks.define_D(1, ndf, 'kernelGAN', 3, norm, 'normal', 0.02, False, [], dimension=nd)
        net.train()
        sd = S.weights_from_seed(S.kernelgan_spec(nd, 1, ndf, norm), seed)
        missing, unexpected = net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        assert not unexpected and all('running' in k or 'num_batches' in k for k in missing), (missing, unexpected)
        x_np = rand_input(600 + i, shape) - np.float32(0.5)
        x = torch.from_numpy(x_np).requires_grad_(True)
        y = net(x)
        r_np = np.random.default_rng(700 + i).standard_normal(tuple(y.shape)).astype(np.float32)
        (y * torch.from_numpy(r_np)).sum().backward()
        keys = [k for k, _ in net.named_parameters()]
        pre = tag + '_'
        out[pre + 'nd'], out[pre + 'norm'], out[pre + 'ndf'], out[pre + 'seed'] = nd, norm, ndf, seed
        out[pre + 'shape'] = np.array(shape)
        out[pre + 'x_seed'], out[pre + 'r_seed'] = 600 + i, 700 + i
        out[pre + 'keys'] = np.array(list(net.state_dict().keys()))
        out[pre + 'shapes'] = np.array([','.join(str(s) for s in v.shape) for v in net.state_dict().values()])
        out[pre + 'pkeys'] = np.array(keys)
        _store(out, pre + 'y', y.detach().numpy(), full)
        _store(out, pre + 'dx', x.grad.numpy(), full)
        for j, (k, p) in enumerate(net.named_parameters()):
            _store(out, pre + 'g%d' % j, p.grad.numpy(), full)
        if norm == 'batch':
            for j in (1, 4, 7):
                m = net.feature_block[j]
                out[pre + 'rm%d' % j] = m.running_mean.numpy().copy()
                out[pre + 'rv%d' % j] = m.running_var.numpy().copy()
        print('ops', tag, tuple(y.shape))
    np.savez_compressed(os.path.join(gg.OUT, 'kernelgan_ops.npz'), **out)


def _two_steps(model, nets, real, step_seed):
    before = {n: [p.detach().clone() for p in getattr(model, 'net' + n).parameters()] for n in nets}
    if step_seed is not None:
        np.random.seed(step_seed)
    losses, fake0 = [], None
    for it in range(2):
        model.set_input({'A': real, 'A_paths': 'x'})
        model.optimize_parameters()
        losses.append([model.get_current_losses()[n] for n in model.loss_names])
        if it == 0:
            fake0 = model.fake.detach().numpy().copy()
    upd = {}
    for n in nets:
        after = [p.detach() for p in getattr(model, 'net' + n).parameters()]
        upd[n] = np.array([float((a - b).double().norm()) for a, b in zip(after, before[n])])
    return losses, fake0, upd


def gen_apollo_kgan(size=36, step_seed=1234, real_seed=321):
    from models.axial_to_lateral_gan_apollo_model import AxialToLateralGANApolloModel
    with contextlib.redirect_stdout(io.StringIO()):
        model = AxialToLateralGANApolloModel(_opt_train('axial_to_lateral_gan_apollo', dict(netD='kernelGAN')))
    specs = [S.unet_deconv_spec(), S.deep_linear_spec()] + [S.kernelgan_spec(2)] * 4
    for i, (name, spec) in enumerate(zip(gg.APOLLO_NETS, specs)):
        load_sd(getattr(model, 'net' + name), S.weights_from_seed(spec, 40 + i))
    real = torch.from_numpy(rand_input(real_seed, (1, 1, size, size, size)))
    losses, fake0, upd = _two_steps(model, gg.APOLLO_NETS, real, step_seed)
    np.savez_compressed(os.path.join(gg.OUT, 'apollo_step_36_kgan.npz'), size=size, step_seed=step_seed, real_seed=real_seed, batch=1,
                        net_seed0=40, netD='kernelGAN', loss_names=np.array(model.loss_names), losses=np.array(losses),
                        gan_mode='lsgan', fake0=fake0, **{'upd_' + n: v for n, v in upd.items()})
    print('apollo', dict(zip(model.loss_names, losses[0])))


def gen_athena_kgan():
    from models.axial_to_lateral_gan_athena_model import AxialToLateralGANAthenaModel
    size = 36
    with contextlib.redirect_stdout(io.StringIO()):
        model = AxialToLateralGANAthenaModel(_opt_train('axial_to_lateral_gan_athena',
                                                        dict(conversion_plane=['yz', 'xy'], pool_size=50, netD='kernelGAN')))
    specs = [S.unet_deconv_spec(), S.deep_linear_spec()] + [S.kernelgan_spec(2)] * 6
    for i, (name, spec) in enumerate(zip(gg.ATHENA_NETS, specs)):
        load_sd(getattr(model, 'net' + name), S.weights_from_seed(spec, 60 + i))
    real = torch.from_numpy(rand_input(654, (1, 1, size, size, size)))
    losses, _, upd = _two_steps(model, gg.ATHENA_NETS, real, None)
    np.savez_compressed(os.path.join(gg.OUT, 'athena_step_36_kgan.npz'), size=size, real_seed=654, net_seed0=60, netD='kernelGAN',
                        loss_names=np.array(model.loss_names), losses=np.array(losses), **{'upd_' + n: v for n, v in upd.items()})
    print('athena', dict(zip(model.loss_names, losses[0])))


def gen_dryops_kgan(size=36, step_seed=4321):
    from models.axial_to_lateral_gan_dryops_model import AxialToLateralGANDryopsModel
    with contextlib.redirect_stdout(io.StringIO()):
        model = AxialToLateralGANDryopsModel(_opt_train('axial_to_lateral_gan_dryops', dict(netG='unet_deconv', netD='kernelGAN')))
    specs = [S.unet_deconv_spec(), S.kernelgan_spec(2), S.kernelgan_spec(2)]
    for i, (name, spec) in enumerate(zip(gg.DRYOPS_NETS, specs)):
        load_sd(getattr(model, 'net' + name), S.weights_from_seed(spec, 80 + i))
    real = torch.from_numpy(rand_input(987, (1, 1, size, size, size)))
    losses, fake0, upd = _two_steps(model, gg.DRYOPS_NETS, real, step_seed)
    np.savez_compressed(os.path.join(gg.OUT, 'dryops_step_deconv_kgan_36.npz'), size=size, step_seed=step_seed, real_seed=987, batch=1,
                        net_seed0=80, netG='unet_deconv', netD='kernelGAN', loss_names=np.array(model.loss_names),
                        losses=np.array(losses), fake0=fake0, **{'upd_' + n: v for n, v in upd.items()})
    print('dryops', dict(zip(model.loss_names, losses[0])))


if __name__ == '__main__':
    networks = ref_modules()
    gen_ops(networks)
    gen_apollo_kgan()
    gen_athena_kgan()
    gen_dryops_kgan()
