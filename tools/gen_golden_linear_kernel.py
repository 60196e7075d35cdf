"""Golden vectors of the learned-PSF generators (--netG_B linearkernel / linearkernel_double / linearkernel_LK31), from the REFERENCE
itself on the CPU, with the helpers of oracle.gen_golden.

    python tools/gen_golden_linear_kernel.py            (from the repo root; needs the reference checkout that oracle.gen_golden names)

Writes tests/golden/linear_kernel_ops.npz, apollo_step_36_lk{9,9double,31}.npz and athena_step_36_lk9.npz.  Weights are not stored:
both sides rebuild them with neuroclear_amd.util.seed.weights_from_seed(linear_kernel_spec(k), seed)."""
import contextlib
import io
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oracle import gen_golden as gg  # noqa: E402
from oracle.gen_golden import _opt_train, load_sd, rand_input, ref_modules  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

OPS_SHAPE = (1, 1, 19, 23, 29)
# (tag, reference class, k, weight seed)
OPS_CASES = [('lk9', 'LinearKernel', 9, 11), ('lk31', 'LinearKernel', 31, 12), ('lk9double', 'LinearKernel_double', 9, 13)]
# (file tag, --netG_B, k)
STEP_CASES = [('lk9', 'linearkernel', 9), ('lk9double', 'linearkernel_double', 9), ('lk31', 'linearkernel_LK31', 31)]


def gen_ops(networks):
    out = dict(shape=np.array(OPS_SHAPE), x_seed=501, r_seed=502)
    x_np = rand_input(501, OPS_SHAPE) - np.float32(0.5)
    r_np = np.random.default_rng(502).standard_normal(OPS_SHAPE).astype(np.float32)
    for tag, cls, k, seed in OPS_CASES:
        net = getattr(networks, cls)(1, 1, k, dimension=3)
        sd = S.weights_from_seed(S.linear_kernel_spec(k), seed)
        load_sd(net, sd)
        x = torch.from_numpy(x_np).requires_grad_(True)
        y = net(x)
        (y * torch.from_numpy(r_np)).sum().backward()
        keys = list(net.state_dict().keys())
        out[tag + '_k'] = k
        out[tag + '_seed'] = seed
        out[tag + '_keys'] = np.array(keys)
        out[tag + '_shapes'] = np.array([list(v.shape) for v in net.state_dict().values()])
        out[tag + '_y'] = y.detach().numpy()
        out[tag + '_dx'] = x.grad.numpy()
        out[tag + '_dw'] = net.convlayer.weight.grad.numpy()
    np.savez_compressed(os.path.join(gg.OUT, 'linear_kernel_ops.npz'), **out)
    print('ops', [c[0] for c in OPS_CASES])


def gen_apollo_lk(tag, netG_B, k, size=36, step_seed=1234, real_seed=321):
    """gg.gen_apollo with G_B = the linear kernel (gen_apollo itself loads the deep-linear spec into G_B)."""
    from models.axial_to_lateral_gan_apollo_model import AxialToLateralGANApolloModel
    with contextlib.redirect_stdout(io.StringIO()):
        model = AxialToLateralGANApolloModel(_opt_train('axial_to_lateral_gan_apollo', dict(netG_B=netG_B)))
    specs = [S.unet_deconv_spec(), S.linear_kernel_spec(k)] + [S.patchgan_spec(2)] * 4
    for i, (name, spec) in enumerate(zip(gg.APOLLO_NETS, specs)):
        load_sd(getattr(model, 'net' + name), S.weights_from_seed(spec, 40 + i))
    real = torch.from_numpy(rand_input(real_seed, (1, 1, size, size, size)))
    before = {n: [p.detach().clone() for p in getattr(model, 'net' + n).parameters()] for n in gg.APOLLO_NETS}
    np.random.seed(step_seed)
    draws, losses = [], []
    orig_randint = np.random.randint

    def spy(*a, **kw):
        v = orig_randint(*a, **kw)
        draws.append(int(v))
        return v
    np.random.randint = spy
    try:
        for it in range(2):
            model.set_input({'A': real, 'A_paths': 'x'})
            model.optimize_parameters()
            losses.append([model.get_current_losses()[n] for n in model.loss_names])
            if it == 0:
                fake0 = model.fake.detach().numpy().copy()
                rec0 = model.rec.detach().numpy().copy()
    finally:
        np.random.randint = orig_randint
    upd = {}
    for n in gg.APOLLO_NETS:
        after = [p.detach() for p in getattr(model, 'net' + n).parameters()]
        upd[n] = np.array([float((a - b).double().norm()) for a, b in zip(after, before[n])])
    np.savez_compressed(os.path.join(gg.OUT, 'apollo_step_36_%s.npz' % tag), size=size, step_seed=step_seed, real_seed=real_seed, batch=1,
                        net_seed0=40, netG_B=netG_B, k=k, loss_names=np.array(model.loss_names), losses=np.array(losses),
                        gan_mode='lsgan', draws=np.array(draws), fake0=fake0, rec0=rec0, **{'upd_' + n: v for n, v in upd.items()})
    print('apollo', tag, dict(zip(model.loss_names, losses[0])))


def gen_athena_lk(tag='lk9', netG_B='linearkernel', k=9):
    from models.axial_to_lateral_gan_athena_model import AxialToLateralGANAthenaModel
    size = 36
    with contextlib.redirect_stdout(io.StringIO()):
        model = AxialToLateralGANAthenaModel(_opt_train('axial_to_lateral_gan_athena',
                                                        dict(conversion_plane=['yz', 'xy'], pool_size=50, netG_B=netG_B)))
    specs = [S.unet_deconv_spec(), S.linear_kernel_spec(k)] + [S.patchgan_spec(2)] * 6
    for i, (name, spec) in enumerate(zip(gg.ATHENA_NETS, specs)):
        load_sd(getattr(model, 'net' + name), S.weights_from_seed(spec, 60 + i))
    real = torch.from_numpy(rand_input(654, (1, 1, size, size, size)))
    before = {n: [p.detach().clone() for p in getattr(model, 'net' + n).parameters()] for n in gg.ATHENA_NETS}
    losses = []
    for it in range(2):
        model.set_input({'A': real, 'A_paths': 'x'})
        model.optimize_parameters()
        losses.append([model.get_current_losses()[n] for n in model.loss_names])
    upd = {}
    for n in gg.ATHENA_NETS:
        after = [p.detach() for p in getattr(model, 'net' + n).parameters()]
        upd[n] = np.array([float((a - b).double().norm()) for a, b in zip(after, before[n])])
    np.savez_compressed(os.path.join(gg.OUT, 'athena_step_36_%s.npz' % tag), size=size, real_seed=654, net_seed0=60, netG_B=netG_B, k=k,
                        loss_names=np.array(model.loss_names), losses=np.array(losses), **{'upd_' + n: v for n, v in upd.items()})
    print('athena', tag, dict(zip(model.loss_names, losses[0])))


if __name__ == '__main__':
    networks = ref_modules()
    gen_ops(networks)
    for case in STEP_CASES:
        gen_apollo_lk(*case)
    gen_athena_lk()
