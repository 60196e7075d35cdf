"""Timing of the WGAN-GP gradient penalty (networks.cal_gradient_penalty; csrc/patchgan_gp.hip) in one process, at Apollo's discriminator
call: B = 108 planes of 108^2, PatchGAN n_layers 3 (--netD basic), instance norm.  Three legs, alternating round by round, each call
timed with device events (median of the rounds after one warm-up round):
  hip       ops.patchgan_gp forward + penalty.backward()  (nc_patchgan_gp_fwd / _bwd)
  torch     the same penalty through torch's own fp32 double backward: a plain nn.Conv2d / nn.InstanceNorm2d / nn.LeakyReLU restatement
            with the same weights, torch.autograd.grad(create_graph=True), then penalty.backward()
  patchgan  the discriminator's first-order forward + backward (nc_patchgan_fwd / _bwd, y.sum().backward()) at the same shape
Prints one JSON line per leg and a summary line (hip / torch, hip / patchgan); with --out, writes them all to that file."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from neuroclear_amd import ops  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

DEV = 'cuda'


def torch_patchgan(sd, n_layers):
    """NLayerDiscriminator (networks.py:1009-1067) with instance norm as plain torch modules, loaded with the same weights."""
    layers, cin = [], 1
    vals = list(sd.values())  # patchgan_spec order: (weight, bias) per conv
    for i in range(n_layers + 2):
        w, b = torch.from_numpy(vals[2 * i]), torch.from_numpy(vals[2 * i + 1])
        c = nn.Conv2d(cin, w.shape[0], 4, 2 if i < n_layers else 1, 1)
        c.weight.data.copy_(w)
        c.bias.data.copy_(b)
        layers.append(c)
        if i < n_layers + 1:
            if i > 0:
                layers.append(nn.InstanceNorm2d(w.shape[0]))
            layers.append(nn.LeakyReLU(0.2, True))
        cin = w.shape[0]
    return nn.Sequential(*layers).to(DEV)


def time_call(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main(B, n, n_layers, rounds, reps, out):
    sd = S.weights_from_seed(S.patchgan_spec(2, 1, 64, n_layers), 7)
    net = networks.define_D(1, 64, 'n_layers', n_layers, 'instance', 'normal', 0.02, False, [0], dimension=2)
    net.load_state_dict({k: torch.from_numpy(v).to(DEV) for k, v in sd.items()})
    tnet = torch_patchgan(sd, n_layers)
    params = list(net.parameters())
    x = torch.rand(B, 1, n, n, device=DEV).requires_grad_(True)

    def hip():
        for p in params:
            p.grad = None
        x.grad = None
        pen, _ = ops.patchgan_gp(x, params, n_layers, 64, 2, 1.0, 10.0)
        pen.backward()

    def ref():
        for p in tnet.parameters():
            p.grad = None
        x.grad = None
        y = tnet(x)
        g, = torch.autograd.grad(y, x, torch.ones_like(y), create_graph=True)
        pen = (((g.view(B, -1) + 1e-16).norm(2, dim=1) - 1.0) ** 2).mean() * 10.0
        pen.backward()

    def first_order():
        for p in params:
            p.grad = None
        x.grad = None
        net(x).sum().backward()

    legs = dict(hip=hip, torch=ref, patchgan=first_order)
    res = {k: [] for k in legs}
    for r in range(rounds + 1):  # round 0 is warm-up
        for k, fn in legs.items():
            ms = time_call(fn, reps)
            if r:
                res[k].append(ms)
    for k, ms in res.items():
        line = dict(what='gp_time', leg=k, B=B, n=n, n_layers=n_layers, ms_median=float(np.median(ms)), ms_min=float(np.min(ms)),
                    ms_rounds=[float(m) for m in ms], reps=reps)
        print(json.dumps(line), flush=True)
        out.append(line)
    h, t, p = (float(np.median(res[k])) for k in ('hip', 'torch', 'patchgan'))
    line = dict(what='gp_time_summary', hip_over_torch=h / t, hip_over_patchgan_fwd_bwd=h / p, hip_ms=h, torch_ms=t, patchgan_ms=p)
    print(json.dumps(line), flush=True)
    out.append(line)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=108)
    ap.add_argument('--n', type=int, default=108)
    ap.add_argument('--n_layers', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'gp_time.py measures on the GPU'
    out = []
    main(a.B, a.n, a.n_layers, a.rounds, a.reps, out)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
