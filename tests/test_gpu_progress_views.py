"""GPU: the training progress views (csrc/views.hip: nc_tensor2im, nc_progress_views; ops.tensor2im / ops.progress_views;
util/visualizer.py; train_onecube --display_freq) against the numpy restatement of tests/views_reference.py, which
tests/test_progress_views.py pins to the reference's own outputs (tests/golden/progress_views.npz).  All results are integers and every
comparison is assert_array_equal.  Shapes: one voxel; extents below a wave; a row longer than a wave (70) and one past a 256-lane tile
(257); odd extents over several blocks; the test crop (36^3) and the training crop (108^3); a [2, 3, ...] tensor whose samples and
channels differ, so that taking sample 0, channel 0 is tested."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import views_reference as V  # noqa: E402

from neuroclear_amd import _lib, ops  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402
from neuroclear_amd.util import tiff  # noqa: E402

DEV = 'cuda'
SHAPES = [(1, 1, 1, 1, 1), (1, 1, 3, 2, 5), (1, 1, 9, 7, 70), (1, 1, 5, 3, 257), (1, 1, 33, 17, 19), (1, 1, 36, 36, 36),
          (1, 1, 108, 108, 108), (2, 3, 6, 7, 8)]
LOSS_LINE = re.compile(r'^\(epoch: 1, epoch_progress: \d+%, iter time: \d+\.\d{3}, data load time: \d+\.\d{3}\) (\w+: -?\d+\.\d{3} )+$')


def _same(got, want):
    assert sorted(got) == sorted(want) == sorted(V.KEYS + ('hist',))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_views_and_tensor2im_equal_the_restatement(shape):
    x = V.volume(40 + len(SHAPES) * shape[-1] + shape[-2], shape)
    t = torch.from_numpy(x).to(DEV)
    D, H, W = shape[2:]
    want = V.views(x)
    got = ops.progress_views(t)
    _same(got, want)
    assert got['hist'].dtype == np.int64 and got['hist'].sum() == D * H * W
    np.testing.assert_array_equal(got['hist'], np.bincount(V.tensor2im(x, np.uint8)[0, 0].ravel(), minlength=256))
    if shape[0] > 1:  # the other samples and channels would give other arrays
        assert any(not np.array_equal(V.views(x[n:n + 1, c:c + 1])['mip_xy'], want['mip_xy']) for n in range(shape[0]) for c in range(shape[1])
                   if (n, c) != (0, 0))
    for index in sorted({0, min(D, H, W) - 1}):
        _same(ops.progress_views(t, index), V.views(x, index))
    for ty in (np.uint8, np.uint16):
        got = ops.tensor2im(t, ty)
        assert got.dtype == ty and got.shape == shape
        np.testing.assert_array_equal(got, V.tensor2im(x, ty))
    np.testing.assert_array_equal(ops.tensor2im(t[0], np.uint8), V.tensor2im(x[0], np.uint8))  # save_current_visuals' call


def test_golden_volumes_and_special_values(golden_dir):
    g = np.load(os.path.join(golden_dir, 'progress_views.npz'))
    for i, shape in enumerate(V.GOLDEN_SHAPES):
        t = torch.from_numpy(V.volume(700 + i, shape)).to(DEV)
        got = ops.progress_views(t)
        for key in V.KEYS:
            np.testing.assert_array_equal(got[key], g['v%d_%s' % (i, key)], err_msg=key)
        np.testing.assert_array_equal(got['hist'], np.bincount(g['v%d_u8' % i][0, 0].ravel(), minlength=256))
        np.testing.assert_array_equal(ops.tensor2im(t, np.uint8), g['v%d_u8' % i])
        np.testing.assert_array_equal(ops.tensor2im(t, np.uint16), g['v%d_u16' % i])
    sp = V.special_values()
    t = torch.from_numpy(sp).to(DEV)
    np.testing.assert_array_equal(ops.tensor2im(t, np.uint8), g['special_u8'])
    np.testing.assert_array_equal(ops.tensor2im(t, np.uint16), g['special_u16'])
    # the same values through the view kernels: as one row (the row kernel) and as one column along d and along h (the column kernel)
    n = sp.size
    for shape, keys in (((1, 1, 1, 1, n), ('slice_xy', 'mip_xy', 'mip_xz')), ((1, 1, n, 1, 1), ('slice_yz', 'mip_xz', 'mip_yz')),
                        ((1, 1, 1, n, 1), ('slice_xy', 'mip_xy', 'mip_yz'))):
        got = ops.progress_views(t.reshape(shape), 0)
        for key in keys:
            np.testing.assert_array_equal(got[key].ravel(), g['special_u8'], err_msg='%s %s' % (shape, key))
        np.testing.assert_array_equal(got['hist'], np.bincount(g['special_u8'], minlength=256))


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1027, 256 * 4 * 3 + 2])
def test_tensor2im_tails_and_unaligned_pointers(n):
    x = V.volume(n, (n + 3,))
    x[:min(n, V.special_values().size)] = V.special_values()[:n]
    t = torch.from_numpy(x).to(DEV)
    for off in (0, 1, 3):  # 1, 3: a pointer that is not 16-byte aligned takes the element-wise form
        for ty in (np.uint8, np.uint16):
            np.testing.assert_array_equal(ops.tensor2im(t[off:off + n], ty), V.tensor2im(x[off:off + n], ty))


def _call(L, t, shape, index, views, hist, stream=None):
    N, C, D, H, W = shape
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    return L.nc_progress_views(t.data_ptr() if t is not None else None, N, C, D, H, W, index, views.data_ptr() if views is not None else None,
                               hist.data_ptr() if hist is not None else None, st)


def _buffers(nv):
    return torch.full((nv + 64,), 0xFF, dtype=torch.uint8, device=DEV), torch.full((256 + 16,), -1, dtype=torch.int32, device=DEV)


def _unpack(views, shape):
    D, H, W = shape[2:]
    out, off = {}, 0
    for key, s in zip(V.KEYS, ((H, W), (D, W), (D, H)) * 2):
        out[key] = views[off:off + s[0] * s[1]].reshape(s)
        off += s[0] * s[1]
    return out


@pytest.mark.parametrize('shape', [(1, 1, 9, 7, 70), (2, 3, 6, 7, 8), (1, 1, 36, 36, 36)], ids=lambda s: 'x'.join(map(str, s)))
def test_c_abi_runs_streams_guards_and_null_outputs(shape):
    L = _lib.lib()
    D, H, W = shape[2:]
    nv = L.nc_progress_views_bytes(D, H, W)
    assert nv == 2 * (H * W + D * W + D * H)
    x = V.volume(5, shape)
    t = torch.from_numpy(x).to(DEV)
    index = min(D, H, W) // 2
    want = V.views(x, index)
    runs = []
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for stream in (None, None, side):
        views, hist = _buffers(nv)
        torch.cuda.synchronize()
        assert _call(L, t, shape, index, views, hist, stream) == 0
        torch.cuda.synchronize()
        v, h = views.cpu().numpy(), hist.cpu().numpy()
        assert (v[nv:] == 0xFF).all() and (h[256:] == -1).all()  # guard bytes past both ends
        got = _unpack(v[:nv], shape)
        for key in V.KEYS:
            np.testing.assert_array_equal(got[key], want[key], err_msg=key)
        np.testing.assert_array_equal(h[:256], want['hist'])
        runs.append((v.tobytes(), h.tobytes()))
    assert runs[0] == runs[1] == runs[2]
    # hist256 is zeroed by the call: a second call into the same buffer does not accumulate
    views, hist = _buffers(nv)
    assert _call(L, t, shape, index, views, hist) == 0 and _call(L, t, shape, index, views, hist) == 0
    torch.cuda.synchronize()
    assert (views.cpu().numpy().tobytes(), hist.cpu().numpy().tobytes()) == runs[0]
    # views = NULL / hist256 = NULL: the other output is complete, the buffer not passed is untouched
    views, hist = _buffers(nv)
    assert _call(L, t, shape, index, None, hist) == 0
    torch.cuda.synchronize()
    assert hist.cpu().numpy().tobytes() == runs[0][1] and (views.cpu().numpy() == 0xFF).all()
    views, hist = _buffers(nv)
    assert _call(L, t, shape, index, views, None) == 0
    torch.cuda.synchronize()
    assert views.cpu().numpy().tobytes() == runs[0][0] and (hist.cpu().numpy() == -1).all()
    assert _call(L, t, shape, index, None, None) == 0


def test_refusals_come_before_any_write():
    L = _lib.lib()
    shape = (1, 1, 6, 5, 7)
    t = torch.from_numpy(V.volume(6, shape)).to(DEV)
    views, hist = _buffers(L.nc_progress_views_bytes(6, 5, 7))
    torch.cuda.synchronize()
    ARG, SHAPE = -4, -1
    assert _call(L, None, shape, 2, views, hist) == ARG
    assert b'null' in L.nc_last_error()
    for bad in ((1, 1, 0, 5, 7), (1, 1, 6, 0, 7), (1, 1, 6, 5, 0), (0, 1, 6, 5, 7), (1, 0, 6, 5, 7), (1, 1, -1, 5, 7)):
        assert _call(L, t, bad, 0, views, hist) == SHAPE, bad
    for index in (5, 6, 7, -1):  # min(D, H, W) = 5
        assert _call(L, t, shape, index, views, hist) == SHAPE, index
    assert b'index' in L.nc_last_error()
    assert _call(L, t, shape, 4, views, hist) == 0  # the last index inside
    views, hist = _buffers(L.nc_progress_views_bytes(6, 5, 7))
    torch.cuda.synchronize()
    assert _call(L, t, (1, 1, 2048, 1024, 1024), 0, views, hist) == SHAPE  # D * H * W = 2^31
    assert _call(L, t, (1, 1, 1, 46341, 46341), 0, views, hist) == SHAPE  # ... just above it
    assert L.nc_progress_views_bytes(0, 5, 7) == 0 and L.nc_progress_views_bytes(6, 5, -1) == 0
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((64,), 0xFF, dtype=torch.uint8, device=DEV)
    assert L.nc_tensor2im(None, out.data_ptr(), 0, 6, st) == ARG and L.nc_tensor2im(t.data_ptr(), None, 0, 6, st) == ARG
    assert L.nc_tensor2im(t.data_ptr(), out.data_ptr(), 2, 6, st) == ARG
    assert L.nc_tensor2im(t.data_ptr(), out.data_ptr(), 0, 0, st) == SHAPE and L.nc_tensor2im(t.data_ptr(), out.data_ptr(), 1, -3, st) == SHAPE
    torch.cuda.synchronize()
    assert (views.cpu().numpy() == 0xFF).all() and (hist.cpu().numpy() == -1).all() and (out.cpu().numpy() == 0xFF).all()
    with pytest.raises(IndexError):
        ops.progress_views(torch.zeros(1, 1, 8, 3, 9, device=DEV))
    with pytest.raises(ValueError):
        ops.progress_views(torch.zeros(1, 8, 8, 8, device=DEV))


ARGV = ['--model', 'axial_to_lateral_gan_apollo', '--preprocess', 'randomcrop_randomflip_addColorChannel_addBatchChannel', '--crop_size', '36', '36',
        '36', '--gan_mode', 'lsgan', '--init_type', 'kaiming', '--norm', 'instance', '--lambda_A', '5', '--lambda_plane', '1', '1', '1',
        '--lr_policy', 'constant', '--randomize_projection_depth', '--projection_depth', '10', '--save_by_iter', '--save_latest_freq', '2',
        '--print_freq', '1', '--max_iters', '2', '--gpu_ids', '0']


def _train(tmp_path, name, extra):
    import random
    from neuroclear_amd import train_onecube
    d = tmp_path / 'data'
    if not d.exists():
        d.mkdir()
        np.save(str(d / 'vol.npy'), S.random_volume(21, 48))
    np.random.seed(3)
    random.seed(3)
    return train_onecube.main(['--dataroot', str(d), '--checkpoints_dir', str(tmp_path / 'ckpt'), '--name', name] + ARGV + extra)


def test_train_onecube_writes_the_views_and_the_loss_log(tmp_path, capsys):
    model = _train(tmp_path, 'shown', ['--display_freq', '1', '--display_histogram'])
    run = tmp_path / 'ckpt' / 'shown'
    img = run / 'web' / 'images'
    labels = ('real', 'fake', 'rec')
    names = sorted(os.listdir(str(img)))
    want_names = ['iter_%d_%s_%s.tif' % (it, lb, key) for it in (1, 2) for lb in labels for key in V.KEYS]
    want_names += ['iter_2_%s_hist.npy' % lb for lb in labels] + ['2_%s.tif' % lb for lb in labels]
    assert names == sorted(want_names) and len(names) == 18 + 18 + 3 + 3
    for lb in labels:
        x = getattr(model, lb).detach().cpu().numpy()  # as left by the last step
        assert x.shape == (1, 1, 36, 36, 36)
        want = V.views(x)
        for key in V.KEYS:
            page = tiff.imread(str(img / ('iter_2_%s_%s.tif' % (lb, key))))
            assert page.dtype == np.uint8 and page.shape == (36, 36)
            np.testing.assert_array_equal(page, want[key], err_msg='%s %s' % (lb, key))
        hist = np.load(str(img / ('iter_2_%s_hist.npy' % lb)))
        assert hist.dtype == np.int64 and hist.shape == (256,)
        np.testing.assert_array_equal(hist, want['hist'])
        vol = tiff.imread(str(img / ('2_%s.tif' % lb)))
        assert vol.dtype == np.uint8
        np.testing.assert_array_equal(vol, V.tensor2im(x[0], np.uint8)[0])
    assert len({tiff.imread(str(img / ('iter_2_%s_mip_xy.tif' % lb))).tobytes() for lb in labels}) == 3  # three different visuals
    rows = (run / 'loss_log.txt').read_text().split('\n')
    assert len(rows) == 4 and rows[3] == ''
    assert re.fullmatch(r'================ Training Loss \(.+\) ================', rows[0])
    assert len(model.loss_names) == 11
    printed = capsys.readouterr().out
    for it, row in ((1, rows[1]), (2, rows[2])):
        assert LOSS_LINE.match(row), row
        assert 'epoch_progress: %d%%' % it in row
        assert re.findall(r'(\w+): -?\d+\.\d{3} ', row) == list(model.loss_names)
        assert row + '\n' in printed
    assert os.path.exists(str(run / 'iter_2_net_G_A.pth'))


def test_train_onecube_without_display_freq_is_todays(tmp_path, capsys):
    _train(tmp_path, 'plain', [])
    run = tmp_path / 'ckpt' / 'plain'
    files = sorted(os.listdir(str(run)))
    assert 'web' not in files and 'loss_log.txt' not in files
    assert files and all(re.fullmatch(r'iter_2_net_\w+\.pth', f) for f in files)
    printed = capsys.readouterr().out
    assert len(re.findall(r'^\(iters: \d+, time: \d+\.\d{3}, data: \d+\.\d{3}\) ', printed, flags=re.M)) == 2 and 'epoch_progress' not in printed


def test_cost_of_one_display_at_108_is_reported():
    """Information, not an assertion (DESIGN.md 4.14 holds the figure next to the step time; tools/views_time.py measures both)."""
    L = _lib.lib()
    ts = [torch.rand(1, 1, 108, 108, 108, device=DEV) for _ in range(3)]
    nv = L.nc_progress_views_bytes(108, 108, 108)
    bufs = [_buffers(nv) for _ in ts]
    ms = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t, (v, h) in zip(ts, bufs):
            assert _call(L, t, t.shape, 54, v, h) == 0
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    print('three nc_progress_views calls at 108^3: %s ms' % ', '.join('%.3f' % m for m in ms))
