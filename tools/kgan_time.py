"""Timing of the KernelGAN discriminator (--netD kernelGAN; csrc/kgan.hip) in one process:
  1. the fused nc_kgan_fwd / _bwd against the layered modules (NC_FUSED_KGAN=0) at Apollo's discriminator call, B = 108 planes of
     108^2, and once in 3-D at 1 x 64^3; forward alone and forward + backward, the two paths alternating round by round (device events
     around each call);
  2. the Apollo 108^3 training step (optimize_parameters) with --netD kernelGAN against --netD basic, also alternating.
FLOP are the reference's layer-by-layer count (2 per MAC; a backward counted as twice its forward); algorithmic bytes are the three
64-channel fp32 maps the forward saves, written once and read once per direction.  `roof` is the fraction of the fp32 matrix peak
(157.3 TFLOP/s), `hbm_roof` the map bytes' fraction of 8 TB/s.  Prints one JSON line per measurement and, with --out, writes them
all to that file."""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

DEV = 'cuda'
PEAK_FLOP, PEAK_HBM = 157.3e12, 8.0e12


def make_net(nd):
    net = networks.define_D(1, 64, 'kernelGAN', 3, 'instance', 'normal', 0.02, False, [0], dimension=nd)
    net.load_state_dict(S.state_dict_from_seed(S.kernelgan_spec(nd), 5, DEV))
    return net


def time_call(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_ops(rounds, out):
    for nd, shape in ((2, (108, 1, 108, 108)), (3, (1, 1, 64, 64, 64))):
        net = make_net(nd)
        x = torch.rand(shape, device=DEV).requires_grad_(True)
        oshape = shape[:2] + tuple(s - 6 for s in shape[2:])
        r = torch.randn(oshape, device=DEV)
        P = int(np.prod(oshape))
        flop_fwd = 2.0 * P * (64 * 7 ** nd + 3 * 64 * 64 + 64)
        map_bytes = 3 * 64 * P * 4 * 2

        def fwd():
            with torch.no_grad():
                net(x)

        def fwd_bwd():
            x.grad = None
            for p in net.parameters():
                p.grad = None
            (net(x) * r).sum().backward()

        calls = {(mode, what): fn for mode in ('fused', 'layered') for what, fn in (('fwd', fwd), ('fwd_bwd', fwd_bwd))}
        res = {k: [] for k in calls}
        for _ in range(rounds + 1):  # the first round is warm-up
            for (mode, what), fn in calls.items():
                os.environ['NC_FUSED_KGAN'] = '1' if mode == 'fused' else '0'
                res[(mode, what)].append(time_call(fn, 5))
        os.environ.pop('NC_FUSED_KGAN', None)
        for (mode, what), ms in res.items():
            ms = ms[1:]
            med = float(np.median(ms))
            flop = flop_fwd * (1 if what == 'fwd' else 3)
            nbytes = map_bytes * (1 if what == 'fwd' else 2)
            r_ = dict(what='op', nd=nd, shape=list(shape), op=what, path=mode, ms_median=med, ms_min=float(np.min(ms)),
                      gflop=flop / 1e9, tflops=flop / (med * 1e-3) / 1e12, roof=flop / (med * 1e-3) / PEAK_FLOP,
                      map_gbytes=nbytes / 1e9, hbm_roof=nbytes / (med * 1e-3) / PEAK_HBM)
            print(json.dumps(r_), flush=True)
            out.append(r_)


def apollo_opt(netD):
    return Namespace(gpu_ids=[0], isTrain=True, image_dimension=3, checkpoints_dir='/tmp/nc_ckpt', name='t', preprocess='none',
                     gan_mode='lsgan', randomize_projection_depth=True, projection_depth=10, min_projection_depth=2, lambda_plane=[1, 1, 1],
                     lambda_A=5.0, input_nc=1, output_nc=1, ngf=64, ndf=64, netG='unet_deconv', netG_B='deep_linear_gen', netD=netD,
                     n_layers_D=3, norm='instance', no_dropout=True, init_type='kaiming', init_gain=0.02, lr=1e-4, beta1=0.1,
                     direction='AtoB', model='axial_to_lateral_gan_apollo')


def bench_steps(n, steps, rounds, out):
    from neuroclear_amd.models import create_model
    real = torch.from_numpy(np.random.default_rng(9).random((1, 1, n, n, n), dtype=np.float32)).to(DEV)
    models = {}
    for name in ('basic', 'kernelGAN'):
        np.random.seed(1)
        m = create_model(apollo_opt(name))
        for _ in range(3):
            m.set_input({'A': real, 'A_paths': 'x'})
            m.optimize_parameters()
        models[name] = m
    torch.cuda.synchronize()
    res = {name: [] for name in models}
    for _ in range(rounds):
        for name, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                m.set_input({'A': real, 'A_paths': 'x'})
                m.optimize_parameters()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) * 1e3 / steps)
    for name, ms in res.items():
        r = dict(what='apollo_step', n=n, netD=name, ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), rounds=rounds, steps=steps)
        print(json.dumps(r), flush=True)
        out.append(r)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=108)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--skip_steps', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'kgan_time.py measures on the GPU'
    out = []
    bench_ops(a.rounds, out)
    if not a.skip_steps:
        bench_steps(a.n, a.steps, a.rounds, out)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
