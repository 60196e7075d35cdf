"""Timing of the 2-D generator's kernels in one process (device events around each call, every shape warmed up, the two sides alternating round by
round):
  1. every 3 x 3 convolution shape of unet_deconv(dimension=2) at 1 x 1 x 1024 x 1024 and 1 x 1 x 256 x 256, forward and data gradient, with
     nc_set_conv2d_k3 on (csrc/conv2d_k3.hip where it covers the shape) and off (the gather GEMM: the path these layers had before);
  2. the transposed-convolution forwards (512 -> 256, 256 -> 128, 128 -> 64) on the matrix cores and under nc_set_force_direct(1) (VALU);
  3. the whole no_grad forward at both sizes, switch on and off.
Prints a table with the achieved TFLOP/s and, with --out, writes it to that file (profiles/unet2d_k3.txt).  'spread' is (max - min) / median over
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


def layers(size):
    """(C, K, H, W) of the 3 x 3 layers of Unet_deconv on a size x size image, each shape once."""
    s, h, q = size, size // 2, size // 4
    return [(1, 64, s, s), (64, 64, s, s), (64, 128, h, h), (128, 128, h, h), (128, 256, q, q), (256, 256, q, q), (256, 128, h, h), (128, 64, s, s)]


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
    for (C, K, H, W) in layers(size):
        x = torch.randn(1, C, H, W, device=DEV)
        dy = torch.randn(1, K, H, W, device=DEV)
        w = torch.randn(K, C, 3, 3, device=DEV) * (2.0 / (9 * C)) ** 0.5
        b = torch.randn(K, device=DEV)
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        nb = int(L.nc_conv_ws_bytes(1, C, 1, H, W, K, 1, 3, 3, 1, 1))
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        g = (1, C, 1, H, W, K, 1, 3, 3, 1, 1)
        calls = {'fwd': lambda: check(L.nc_conv_fwd(_p(x), _p(w), _p(b), _p(y), *g, _p(ws), nb, st), 'conv_fwd'),
                 'dgrad': lambda: check(L.nc_conv_dgrad(_p(dy), _p(w), _p(dx), *g, _p(ws), nb, st), 'conv_dgrad')}
        flop = 2.0 * 9 * C * K * H * W
        reps = 3 if size >= 1024 else 10
        for what, (op, fn) in enumerate(calls.items()):
            active = int(L.nc_conv2d_k3_active(what, 1, C, H, W, K))
            res = two_sides(fn, lambda on: L.nc_set_conv2d_k3(on), rounds, reps)
            (m1, s1), (m0, s0) = stats(res[1]), stats(res[0])
            if not active:
                verdict = 'not covered: both sides are the gather GEMM'
            else:
                verdict = 'kernel faster' if m1 < m0 * (1.0 - max(s1, s0)) else 'NOT faster than the gather GEMM beyond the spread'
            lines.append('%4d  %3d->%-3d %4dx%-4d %-5s  k3 %d | on %8.4f ms %6.1f TFLOP/s spread %4.1f%% | off %8.4f ms %6.1f TFLOP/s spread %4.1f%% | %s'
                         % (size, C, K, H, W, op, active, m1, flop / m1 / 1e9, 100 * s1, m0, flop / m0 / 1e9, 100 * s0, verdict))
            print(lines[-1], flush=True)


def convt_rows(size, rounds, lines):
    L = lib()
    st = P(torch.cuda.current_stream().cuda_stream)
    for (C, K, H, W) in ((512, 256, size // 8, size // 8), (256, 128, size // 4, size // 4), (128, 64, size // 2, size // 2)):
        x = torch.randn(1, C, H, W, device=DEV)
        w = torch.randn(C, K, 2, 2, device=DEV) * (2.0 / (4 * C)) ** 0.5
        b = torch.randn(K, device=DEV)
        y = torch.empty(1, K, 2 * H, 2 * W, device=DEV)
        fn = lambda: check(L.nc_convT2d_k2s2_fwd(_p(x), _p(w), _p(b), _p(y), 1, C, H, W, K, st), 'convT2d_fwd')  # noqa: E731
        res = two_sides(fn, lambda mfma: L.nc_set_force_direct(0 if mfma else 1), rounds, 10)
        L.nc_set_force_direct(0)
        (m1, s1), (m0, s0) = stats(res[1]), stats(res[0])
        flop = 2.0 * 4 * C * K * H * W
        lines.append('%4d  convT %3d->%-3d %4dx%-4d fwd | matrix cores %8.4f ms %6.1f TFLOP/s spread %4.1f%% | VALU %8.4f ms %6.1f TFLOP/s spread %4.1f%%'
                     % (size, C, K, H, W, m1, flop / m1 / 1e9, 100 * s1, m0, flop / m0 / 1e9, 100 * s0))
        print(lines[-1], flush=True)


def net_rows(size, rounds, lines):
    L = lib()
    net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0], dimension=2)
    net.load_state_dict(S.state_dict_from_seed(S.unet_deconv_spec(2), 5, DEV))
    x = torch.rand(1, 1, size, size, device=DEV)

    def fwd():
        with torch.no_grad():
            net(x)
    res = two_sides(fwd, lambda on: L.nc_set_conv2d_k3(on), rounds, 3)
    (m1, s1), (m0, s0) = stats(res[1]), stats(res[0])
    lines.append('%4d  unet_deconv 2-D no_grad forward | on %8.3f ms spread %4.1f%% | off %8.3f ms spread %4.1f%%' % (size, m1, 100 * s1, m0, 100 * s0))
    print(lines[-1], flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 256])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'unet2d_time.py measures on the GPU'
    lines = ['# tools/unet2d_time.py --sizes %s --rounds %d on %s' % (' '.join(map(str, a.sizes)), a.rounds, torch.cuda.get_device_name(0)),
             '# 3 x 3 layers of unet_deconv(dimension=2), N = 1: nc_set_conv2d_k3 on / off, median of the rounds; k3 = nc_conv2d_k3_active']
    for size in a.sizes:
        conv_rows(size, a.rounds, lines)
    for size in a.sizes:
        convt_rows(size, a.rounds, lines)
    for size in a.sizes:
        net_rows(size, a.rounds, lines)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
