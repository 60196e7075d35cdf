"""Timing of the learned-PSF kernels (csrc/conv_lk.hip) at 108^3, N = 1, in one process:
  1. nc_lk_fwd / _dgrad / _wgrad for k = 9 and 31 against the generic nc_conv_fwd / _dgrad / _wgrad on the same Conv3d(1, 1, k), the two
     alternating round by round (device events around each call);
  2. the Apollo 108^3 training step (optimize_parameters) with each --netG_B linear kernel against the default deep_linear_gen, also
     alternating.
Prints one JSON line per measurement and, with --out, writes them all to that file."""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from neuroclear_amd import ops  # noqa: E402
from neuroclear_amd._lib import I, P, Z, check, lib  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

DEV = 'cuda'


def _p(t):
    return P(t.data_ptr())


def op_calls(k, n):
    L = lib()
    st = P(torch.cuda.current_stream().cuda_stream)
    x = torch.rand(1, 1, n, n, n, device=DEV)
    dy = torch.randn(1, 1, n, n, n, device=DEV)
    w = torch.randn(1, 1, k, k, k, device=DEV)
    y, dw = torch.empty_like(x), torch.empty_like(w)
    lws = torch.empty(max(1, L.nc_lk_ws_bytes(I(1), I(n), I(n), I(n), I(k))), dtype=torch.uint8, device=DEV)
    gws = torch.empty(max(1, L.nc_conv_ws_bytes(I(1), I(1), I(n), I(n), I(n), I(1), I(k), I(k), I(k), I(1), I(k // 2))), dtype=torch.uint8,
                      device=DEV)
    g = (I(1), I(1), I(n), I(n), I(n), I(1), I(k), I(k), I(k), I(1), I(k // 2))
    s = (I(1), I(n), I(n), I(n), I(k))
    return {
        ('fwd', 'lk'): lambda: check(L.nc_lk_fwd(_p(x), _p(w), _p(y), *s, _p(lws), Z(lws.numel()), st), 'lk_fwd'),
        ('dgrad', 'lk'): lambda: check(L.nc_lk_dgrad(_p(dy), _p(w), _p(y), *s, _p(lws), Z(lws.numel()), st), 'lk_dgrad'),
        ('wgrad', 'lk'): lambda: check(L.nc_lk_wgrad(_p(x), _p(dy), _p(dw), *s, _p(lws), Z(lws.numel()), st), 'lk_wgrad'),
        ('fwd', 'generic'): lambda: check(L.nc_conv_fwd(_p(x), _p(w), P(0), _p(y), *g, _p(gws), Z(gws.numel()), st), 'conv_fwd'),
        ('dgrad', 'generic'): lambda: check(L.nc_conv_dgrad(_p(dy), _p(w), _p(y), *g, _p(gws), Z(gws.numel()), st), 'conv_dgrad'),
        ('wgrad', 'generic'): lambda: check(L.nc_conv_wgrad(_p(x), _p(dy), _p(dw), P(0), *g, _p(gws), Z(gws.numel()), st), 'conv_wgrad'),
    }


def time_call(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_ops(n, rounds, out):
    for k in (9, 31):
        calls = op_calls(k, n)
        for fn in calls.values():  # warm-up (code objects, first-call set-up)
            fn()
        torch.cuda.synchronize()
        flop = 2.0 * k ** 3 * n ** 3
        res = {key: [] for key in calls}
        for _ in range(rounds):
            for key, fn in calls.items():
                reps = 3 if key[1] == 'generic' and k == 31 else 10
                res[key].append(time_call(fn, reps))
        for (op, path), ms in res.items():
            r = dict(what='op', k=k, n=n, op=op, path=path, ms_median=float(np.median(ms)), ms_min=float(np.min(ms)),
                     tflops=flop / (np.median(ms) * 1e-3) / 1e12)
            print(json.dumps(r), flush=True)
            out.append(r)


def apollo_opt(netG_B):
    return Namespace(gpu_ids=[0], isTrain=True, image_dimension=3, checkpoints_dir='/tmp/nc_ckpt', name='t', preprocess='none',
                     gan_mode='lsgan', randomize_projection_depth=True, projection_depth=10, min_projection_depth=2, lambda_plane=[1, 1, 1],
                     lambda_A=5.0, input_nc=1, output_nc=1, ngf=64, ndf=64, netG='unet_deconv', netG_B=netG_B, netD='basic', n_layers_D=3,
                     norm='instance', no_dropout=True, init_type='kaiming', init_gain=0.02, lr=1e-4, beta1=0.1, direction='AtoB',
                     model='axial_to_lateral_gan_apollo')


def bench_steps(n, steps, rounds, out):
    from neuroclear_amd.models import create_model
    real = torch.from_numpy(np.random.default_rng(9).random((1, 1, n, n, n), dtype=np.float32)).to(DEV)
    models = {}
    for name in ('deep_linear_gen', 'linearkernel', 'linearkernel_double', 'linearkernel_LK31'):
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
        r = dict(what='apollo_step', n=n, netG_B=name, ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), rounds=rounds, steps=steps)
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
    assert torch.cuda.is_available(), 'lk_time.py measures on the GPU'
    out = []
    bench_ops(a.n, a.rounds, out)
    if not a.skip_steps:
        bench_steps(a.n, a.steps, a.rounds, out)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
