"""CPU: bench.py --dump-outputs -- the files it writes (float32 / float64 .npy, larger arrays as a fixed seeded sample of their flat
indices, the same sample on every run) and the train step's outputs it collects from a model."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_types_and_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_MAX_ELEMS', dict(volume=1000, param=10, inference=64))
    vol = np.random.default_rng(1).integers(0, 65536, (20, 20, 20), dtype=np.uint16)
    arrays = dict(loss_G=np.float64(0.125), fake=np.arange(1000, dtype=np.float32).reshape(10, 10, 10),
                  param_G=np.linspace(0, 1, 11, dtype=np.float32), volume=vol)
    kind = dict(loss_G='volume', fake='volume', param_G='param', volume='inference')
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), arrays, kind)
    got = {n: np.load(str(tmp_path / 'a' / (n + '.npy'))) for n in arrays}
    assert got['loss_G'].dtype == np.float64 and got['loss_G'].tolist() == [0.125]
    assert got['fake'].dtype == np.float32 and np.array_equal(got['fake'], arrays['fake'].reshape(-1))  # at the cap: whole
    assert got['param_G'].dtype == np.float32 and got['param_G'].size == 10
    assert got['volume'].dtype == np.float32 and got['volume'].size == 64
    idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(vol.size, 64, replace=False))
    assert np.array_equal(got['volume'], vol.reshape(-1)[idx].astype(np.float32))
    for n in arrays:  # a second run writes the same files
        assert np.array_equal(got[n], np.load(str(tmp_path / 'b' / (n + '.npy'))))


def test_train_outputs_collects_losses_visuals_and_parameters():
    torch.manual_seed(0)
    nets = dict(netG_A=torch.nn.Conv3d(1, 2, 3), netD_A=torch.nn.Linear(4, 1))
    model = SimpleNamespace(fake=torch.rand(1, 1, 3, 3, 3), rec=torch.rand(1, 1, 3, 3, 3), model_names=['G_A', 'D_A'],
                            get_current_losses=lambda: dict(G_A=1.5, cycle=torch.tensor(0.25)), **nets)
    arrays, kind = bench.train_outputs(model)
    assert sorted(arrays) == ['fake', 'loss_G_A', 'loss_cycle', 'param_D_A', 'param_G_A', 'rec']
    assert float(arrays['loss_cycle']) == 0.25 and kind['param_G_A'] == 'param' and kind['fake'] == 'volume'
    want = torch.cat([p.detach().reshape(-1) for p in nets['netG_A'].parameters()]).numpy()
    assert np.array_equal(arrays['param_G_A'], want) and arrays['fake'].shape == (1, 1, 3, 3, 3)


def test_steps_below_one_is_refused_before_any_gpu_work():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and '--steps must be >= 1' in r.stderr
