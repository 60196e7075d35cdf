"""Timing of the 2-D diced inference (neuroclear_amd.infer_dice2d.diced_inference_2d) on one plane:
  python tools/dice2d_time.py --net resnet_9blocks [--size 2048 --roi 120 --overlap 15 --border 10 --nbatch 8 --runs 3] [--out FILE]
times the whole call (upload of the uint16 plane, dicing, the network, overlap-add, finalisation, download) between two device events: one
warm-up, then the median of --runs.  Seeded weights, a random uint16 plane.
  python tools/dice2d_time.py --summarise KERNEL_STATS.csv [--out FILE]
reads the per-kernel statistics of a `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/dice2d_time.py ... --runs 1` run
and prints the share of the three kernels of csrc/dice2d.hip in the summed kernel time, beside the largest kernels of the run."""
import argparse
import csv
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DICE2D = ('k_cut_tiles2d', 'k_scatter_add2d', 'k_finalize2d')


def measure(a):
    import torch
    from argparse import Namespace
    from neuroclear_amd.models import networks
    from neuroclear_amd.infer_dice2d import diced_inference_2d
    from neuroclear_amd.util import seed as S
    assert torch.cuda.is_available(), 'dice2d_time.py measures on the GPU'
    dev = 'cuda'
    if a.net == 'unet_deconv':
        net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0], dimension=2)
        net.load_state_dict(S.state_dict_from_seed(S.unet_deconv_spec(2), 5, dev))
    else:
        blocks = {'resnet_6blocks': 6, 'resnet_9blocks': 9}[a.net]
        net = networks.define_G(1, 1, 64, a.net, 'instance', False, 'kaiming', 0.02, [0], dimension=2)
        net.load_state_dict(S.state_dict_from_seed(S.resnet_spec(blocks), 5, dev))
    img = np.random.default_rng(6).integers(0, 65536, (a.size, a.size), dtype=np.uint16)
    opt = Namespace(dice_size=[a.roi] * 2, overlap=a.overlap, border_cut=a.border, gpu_ids=[0], skip_real=True, data_type='uint16',
                    histogram_match=False, normalize_intensity=False)
    net_ms = []

    def on_batch(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = fn()
        e1.record()
        net_ms.append((e0, e1))
        return y

    ms, inside = [], []
    for run in range(a.runs + 1):     # the first run is the warm-up
        del net_ms[:]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = diced_inference_2d(net, img, opt, nbatch=a.nbatch, on_batch=on_batch)
        e1.record()
        e1.synchronize()
        if run:
            ms.append(e0.elapsed_time(e1))
            inside.append(sum(s.elapsed_time(e) for s, e in net_ms))
    assert out.shape == img.shape and out.dtype == np.uint16
    E = a.roi + 2 * a.border
    lines = ['# tools/dice2d_time.py --net %s --size %d --roi %d --overlap %d --border %d --nbatch %d --runs %d on %s'
             % (a.net, a.size, a.roi, a.overlap, a.border, a.nbatch, a.runs, torch.cuda.get_device_name(0)),
             '%s  %d x %d uint16, %d network calls on [%d, 1, %d, %d]: %.1f ms per image (median of %d after 1 warm-up; runs %s), of which %.1f ms '
             'between the events around the network calls'
             % (a.net, a.size, a.size, len(net_ms), a.nbatch, E, E, float(np.median(ms)), a.runs, ' '.join('%.1f' % m for m in ms),
                float(np.median(inside)))]
    return lines


def summarise(path):
    rows = []
    with open(path, newline='') as f:
        for r in csv.DictReader(f):
            rows.append((r['Name'], int(r['Calls']), float(r['TotalDurationNs'])))
    total = sum(t for _, _, t in rows)
    lines = ['# per-kernel statistics of one kernel-trace run (%s): %d kernels, %.1f ms of kernel time in all' % (os.path.basename(path), len(rows), total / 1e6)]
    mine = 0.0
    for key in DICE2D:
        sel = [(c, t) for n, c, t in rows if key in n]
        calls, t = sum(c for c, _ in sel), sum(t for _, t in sel)
        mine += t
        lines.append('%-18s %6d calls %10.3f ms %6.2f %%' % (key, calls, t / 1e6, 100.0 * t / total))
    lines.append('%-18s %6s       %10.3f ms %6.2f %%' % ('the three together', '', mine / 1e6, 100.0 * mine / total))
    lines.append('# the largest kernels of the run')
    for n, c, t in sorted(rows, key=lambda r: -r[2])[:12]:
        lines.append('%6.2f %% %10.3f ms %6d calls  %s' % (100.0 * t / total, t / 1e6, c, n[:110]))
    return lines


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--net', default='resnet_9blocks', choices=['resnet_6blocks', 'resnet_9blocks', 'unet_deconv'])
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--roi', type=int, default=120)
    ap.add_argument('--overlap', type=int, default=15)
    ap.add_argument('--border', type=int, default=10)
    ap.add_argument('--nbatch', type=int, default=8)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--summarise', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = summarise(a.summarise) if a.summarise else measure(a)
    print('\n'.join(lines), flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
