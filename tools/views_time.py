"""Cost of one display of the training progress views (--display_freq) next to the training step, in one process, with device events:
  step      one Apollo optimize_parameters() on a 108^3 crop (bench.py's options and synthetic crop)
  views     the three nc_progress_views calls of one display (real, fake, rec of that model) into preallocated buffers: device time only
  display   the three ops.progress_views calls as Visualizer.display_current_results issues them: allocation, launch, copy to the host
Median of the rounds after one warm-up round; one JSON line per leg; with --out, written to that file as well."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from neuroclear_amd import _lib, ops  # noqa: E402
from neuroclear_amd.models import create_model  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main(crop, rounds, out):
    with contextlib.redirect_stdout(io.StringIO()):
        model = create_model(bench.apollo_opt(0))
    real = torch.from_numpy((S.random_volume(100, crop).astype(np.float64) / 65535.0).astype(np.float32))[None, None].cuda()
    data = {'A': real, 'A_paths': 'synthetic'}
    L = _lib.lib()
    nv = L.nc_progress_views_bytes(crop, crop, crop)
    bufs = [(torch.empty(nv, dtype=torch.uint8, device='cuda'), torch.empty(256, dtype=torch.int32, device='cuda')) for _ in range(3)]

    def step():
        model.set_input(data)
        model.optimize_parameters()

    def views():
        for (v, h), t in zip(bufs, model.get_current_visuals().values()):
            t = t.detach()
            _lib.check(L.nc_progress_views(t.data_ptr(), t.shape[0], t.shape[1], crop, crop, crop, crop // 2, v.data_ptr(), h.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), 'nc_progress_views')

    def display():
        for t in model.get_current_visuals().values():
            ops.progress_views(t)

    legs = dict(step=step, views=views, display=display)
    res = {k: [] for k in legs}
    for r in range(rounds + 1):
        for k, fn in legs.items():
            ms = timed(fn)
            if r:
                res[k].append(ms)
    for k, ms in res.items():
        line = dict(what='views_time', leg=k, crop=crop, ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_rounds=[float(m) for m in ms])
        print(json.dumps(line), flush=True)
        out.append(line)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--crop', type=int, default=108)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'views_time.py measures on the GPU'
    out = []
    main(a.crop, a.rounds, out)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
