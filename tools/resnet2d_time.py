"""Timing of the ResNet generator's reflect-padded 3 x 3 convolution in one process (device events around each call, every shape warmed up, the two
sides alternating round by round):
  1. the 256 -> 256 layer of a ResnetBlock (ngf 64) on the 256 x 256 map of a 1024^2 input and on the 64 x 64 map of a 256^2 input, forward and
     data gradient through nc_conv2d_k3_reflect_fwd / _dgrad, with nc_set_conv2d_k3 on (csrc/conv2d_k3.hip where it covers the shape; the data
     gradient includes the fold pass) and off (explicit pad + nc_conv_* with padding 0);
  2. the no_grad forward of resnet_9blocks at 1 x 1 x size x size, switch on and off.
Prints a table with the achieved TFLOP/s and, with --out, writes it to that file (profiles/resnet2d.txt).  'spread' is (max - min) / median over
the rounds of one side; 'verdict' says whether the switch-on side is faster than the switch-off side by more than the larger spread."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from neuroclear_amd._lib import P, check, lib  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

DEV = 'cuda'


def _p(t):
    return P(t.data_ptr()) if t is not None else P(0)


def time_call(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def two_sides(fn, set_side, rounds, reps):
    """fn timed with set_side(1) and set_side(0), alternating round by round -> {1: [ms], 0: [ms]}"""
    for side in (1, 0):
        set_side(side)
        fn()
        fn()
    torch.cuda.synchronize()
    res = {1: [], 0: []}
    for _ in range(rounds):
        for side in (1, 0):
            set_side(side)
            res[side].append(time_call(fn, reps))
    set_side(1)
    return res


def stats(ms):
    return float(np.median(ms)), float((np.max(ms) - np.min(ms)) / np.median(ms))


def conv_rows(size, rounds, lines):
    L = lib()
    st = P(torch.cuda.current_stream().cuda_stream)
    C = K = 256
    H = W = size // 4
    x = torch.randn(1, C, H, W, device=DEV)
    dy = torch.randn(1, K, H, W, device=DEV)
    w = torch.randn(K, C, 3, 3, device=DEV) * (2.0 / (9 * C)) ** 0.5
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    nb = int(L.nc_conv2d_k3_reflect_ws_bytes(1, C, H, W, K))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    g = (1, C, H, W, K)
    calls = {'fwd': lambda: check(L.nc_conv2d_k3_reflect_fwd(_p(x), _p(w), _p(None), _p(y), *g, _p(ws), nb, st), 'reflect_fwd'),
             'dgrad': lambda: check(L.nc_conv2d_k3_reflect_dgrad(_p(dy), _p(w), _p(dx), *g, _p(ws), nb, st), 'reflect_dgrad')}
    flop = 2.0 * 9 * C * K * H * W
    reps = 5 if size >= 1024 else 20
    for what, (op, fn) in enumerate(calls.items()):
        active = int(L.nc_conv2d_k3_reflect_active(what, 1, C, H, W, K))
        res = two_sides(fn, lambda on: L.nc_set_conv2d_k3(on), rounds, reps)
        (m1, s1), (m0, s0) = stats(res[1]), stats(res[0])
        if not active:
            verdict = 'not covered: both sides pad explicitly'
        else:
            verdict = 'kernel faster' if m1 < m0 * (1.0 - max(s1, s0)) else 'NOT faster than the explicit pad beyond the spread'
        lines.append('%4d  reflect %3d->%-3d %4dx%-4d %-5s  k3 %d | on %8.4f ms %6.1f TFLOP/s spread %4.1f%% | off %8.4f ms %6.1f TFLOP/s spread %4.1f%% | %s'
                     % (size, C, K, H, W, op, active, m1, flop / m1 / 1e9, 100 * s1, m0, flop / m0 / 1e9, 100 * s0, verdict))
        print(lines[-1], flush=True)


def net_rows(size, rounds, lines):
    L = lib()
    net = networks.define_G(1, 1, 64, 'resnet_9blocks', 'instance', False, 'kaiming', 0.02, [0], dimension=2)
    net.load_state_dict(S.state_dict_from_seed(S.resnet_spec(9), 5, DEV))
    net.eval()
    x = torch.rand(1, 1, size, size, device=DEV)

    def fwd():
        with torch.no_grad():
            net(x)
    res = two_sides(fwd, lambda on: L.nc_set_conv2d_k3(on), rounds, 3)
    (m1, s1), (m0, s0) = stats(res[1]), stats(res[0])
    verdict = 'faster' if m1 < m0 * (1.0 - max(s1, s0)) else 'not faster beyond the spread'
    lines.append('%4d  resnet_9blocks no_grad forward | on %8.3f ms spread %4.1f%% | off %8.3f ms spread %4.1f%% | %s' % (size, m1, 100 * s1, m0, 100 * s0, verdict))
    print(lines[-1], flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 256])
    ap.add_argument('--net-sizes', type=int, nargs='+', default=[1024])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'resnet2d_time.py measures on the GPU'
    lines = ['# tools/resnet2d_time.py --sizes %s --net-sizes %s --rounds %d on %s' % (' '.join(map(str, a.sizes)), ' '.join(map(str, a.net_sizes)), a.rounds,
                                                                                     torch.cuda.get_device_name(0)),
             '# ReflectionPad2d(1) + Conv2d(256, 256, 3) of a ResnetBlock on the size / 4 map, N = 1: nc_set_conv2d_k3 on / off, median of the rounds;',
             '# k3 = nc_conv2d_k3_reflect_active; the data gradient of the on side includes its fold pass, the off side its explicit pad / fold']
    for size in a.sizes:
        conv_rows(size, a.rounds, lines)
    for size in a.net_sizes:
        net_rows(size, a.rounds, lines)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
