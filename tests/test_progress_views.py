"""CPU: the option surface and the host side of the training progress views (--display_freq): the reference's README training command
parses, the new flags carry the reference's defaults (except --display_freq: 0 here), --add_date / --suffix rename as
options/base_options.py:144-150 does, the numpy restatement the GPU tests compare against (tests/views_reference.py) equals every array
of the golden file written by the reference's own tensor2im (tools/gen_golden_views.py), ops.progress_views mirrors the reference's
errors before any launch, and the Visualizer's loss log has the reference's format.  The kernels: tests/test_gpu_progress_views.py."""
import os
import re
import sys
from argparse import Namespace
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import views_reference as V  # noqa: E402

from neuroclear_amd import _lib, ops  # noqa: E402
from neuroclear_amd.options import TrainOptions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the training command of the reference's README ("Training a model"), placeholders filled in, --gpu_ids -1
README_ARGV = ('--dataroot DATA --checkpoints_dir CKPT --add_date --name MODEL --dataset_mode singlevolume --print_freq 10 --display_freq 20 '
               '--preprocess random3Drotate_randomcrop_randomflip_addColorChannel_addBatchChannel --model axial_to_lateral_gan_apollo '
               '--netG unet_deconv --netG_B deep_linear_gen --netD basic --gan_mode lsgan --init_type kaiming --norm instance --batch_size 1 '
               '--lambda_A 5 --gpu_ids -1 --crop_size 108 108 108 --display_histogram --lambda_plane 1 1 1 --save_by_iter '
               '--save_latest_freq 500 --server SERVER --lr_policy constant --randomize_projection_depth --projection_depth 10').split()
BASE = ['--dataroot', 'D', '--model', 'axial_to_lateral_gan_apollo', '--gpu_ids', '-1']
LOSS_LINE = re.compile(r'^\(epoch: \d+, epoch_progress: \d+%, iter time: \d+\.\d{3}, data load time: \d+\.\d{3}\) (\w+: -?\d+\.\d{3} )+$')


def test_readme_training_command_parses():
    opt = TrainOptions().parse(README_ARGV)
    assert re.fullmatch(r'\d{8}-\d{4}_MODEL', opt.name), opt.name
    assert (opt.display_freq, opt.print_freq, opt.display_histogram, opt.server, opt.dataset_mode) == (20, 10, True, 'SERVER', 'singlevolume')
    assert opt.gpu_ids == [] and opt.crop_size == [108, 108, 108] and opt.save_by_iter


def test_defaults_are_the_references_except_display_freq():
    opt = TrainOptions().parse(BASE)
    assert opt.display_freq == 0  # the reference: 100.  Nothing is displayed unless asked for
    want = dict(display_histogram=False, update_html_freq=1000, no_html=False, add_date=False, suffix='', save_epoch_freq=10, momentum=0.9,
                display_ncols=4, display_id=1, display_server='http://localhost', display_env='main', display_port=8097,
                display_winsize=256, server='not-specified', num_threads=8, no_pin_memory=False, load_size=286,
                max_dataset_size=float('inf'), debug=False, name='experiment_name')
    for k, v in want.items():
        assert getattr(opt, k) == v and type(getattr(opt, k)) is type(v), (k, getattr(opt, k))
    more = TrainOptions().parse(BASE + ['--display_ncols', '2', '--display_id', '0', '--display_server', 's', '--display_env', 'e',
                                        '--display_port', '1', '--display_winsize', '64', '--num_threads', '2', '--no_pin_memory',
                                        '--load_size', '100', '--max_dataset_size', '5', '--debug', '--no_html', '--update_html_freq', '7',
                                        '--save_epoch_freq', '3', '--momentum', '0.5'])
    assert (more.max_dataset_size, more.debug, more.no_html, more.momentum) == (5, True, True, 0.5)


def test_add_date_and_suffix_rename_as_the_reference_does():
    o = TrainOptions()
    stamp = o.time
    assert re.fullmatch(r'\d{8}-\d{4}', stamp)
    assert o.parse(BASE + ['--name', 'm', '--add_date']).name == stamp + '_m'
    assert TrainOptions().parse(BASE + ['--name', 'm', '--suffix', '{model}_{netG}_x']).name == 'm_axial_to_lateral_gan_apollo_unet_deconv_x'
    o = TrainOptions()
    assert o.parse(BASE + ['--name', 'm', '--add_date', '--suffix', 'lr{lr}']).name == o.time + '_m_lr0.0001'
    assert TrainOptions().parse(BASE + ['--name', 'm']).name == 'm'


def test_continue_train_keeps_the_name():
    assert TrainOptions().parse(BASE + ['--name', 'm', '--add_date', '--continue_train']).name == 'm'
    assert TrainOptions().parse(BASE + ['--name', 'm', '--continue_train']).name == 'm'


def test_restatement_equals_every_array_of_the_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'progress_views.npz'))
    seen = {'shapes', 'seeds', 'special_x'}
    assert [tuple(s) for s in g['shapes']] == V.GOLDEN_SHAPES and list(g['seeds']) == [700 + i for i in range(len(V.GOLDEN_SHAPES))]
    sp = V.special_values()
    assert sp.dtype == np.float32 and np.array_equal(sp.view(np.uint32), g['special_x'].view(np.uint32))  # bit for bit (-0.0, denormals)
    for name, ty in (('u8', np.uint8), ('u16', np.uint16)):
        got = V.tensor2im(sp, ty)
        assert got.dtype == g['special_' + name].dtype == ty
        np.testing.assert_array_equal(got, g['special_' + name])
        seen.add('special_' + name)
    # the special values do reach both ends and both sides of a step
    assert {0, 1, 127, 128, 254, 255} <= set(g['special_u8'].tolist()) and {0, 1, 65534, 65535} <= set(g['special_u16'].tolist())
    for i, shape in enumerate(V.GOLDEN_SHAPES):
        x = V.volume(700 + i, shape)
        assert x.dtype == np.float32
        for name, ty in (('u8', np.uint8), ('u16', np.uint16)):
            got = V.tensor2im(x, ty)
            assert got.dtype == ty and got.shape == shape
            np.testing.assert_array_equal(got, g['v%d_%s' % (i, name)])
            seen.add('v%d_%s' % (i, name))
        v = V.views(x)
        for key in V.KEYS:
            assert v[key].dtype == np.uint8 and v[key].shape == g['v%d_%s' % (i, key)].shape
            np.testing.assert_array_equal(v[key], g['v%d_%s' % (i, key)])
            seen.add('v%d_%s' % (i, key))
        np.testing.assert_array_equal(v['hist'], np.bincount(g['v%d_u8' % i][0, 0].ravel(), minlength=256))
        assert v['hist'].sum() == shape[2] * shape[3] * shape[4]
    assert seen == set(g.files)
    big = V.volume(1, (1, 1, 20, 20, 20))
    assert (big < 0).mean() > 0.1 and (big > 1).mean() > 0.1  # both clips act
    assert os.path.getsize(os.path.join(golden_dir, 'progress_views.npz')) < 64 << 10


def test_progress_views_mirrors_the_references_errors_before_any_launch(monkeypatch):
    def no_lib():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(ops, 'lib', no_lib)
    with pytest.raises(ValueError):
        ops.progress_views(torch.zeros(1, 8, 8, 8))  # b, c, d, h, w = img_shape
    with pytest.raises(ValueError):
        ops.progress_views(torch.zeros(8, 8, 8))
    with pytest.raises(IndexError):
        ops.progress_views(torch.zeros(1, 1, 8, 3, 9))  # int(8 / 2) = 4 >= H
    with pytest.raises(IndexError):
        ops.progress_views(torch.zeros(1, 1, 8, 9, 4))  # ... >= W
    with pytest.raises(IndexError):
        ops.progress_views(torch.zeros(1, 1, 8, 9, 9), index=8)
    with pytest.raises(_lib.NcError):
        ops.progress_views(torch.zeros(1, 1, 8, 9, 9))  # a CPU tensor: there is no CPU fallback
    with pytest.raises(_lib.NcError):
        ops.tensor2im(torch.zeros(4), np.uint8)
    with pytest.raises(ValueError):
        ops.tensor2im(torch.zeros(4), np.float32)


def test_c_abi_header_and_integration_list_name_the_entry_points():
    protos = _lib.prototypes()
    for name in ('nc_tensor2im', 'nc_progress_views', 'nc_progress_views_bytes'):
        assert name in protos
        assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    import ctypes
    assert protos['nc_progress_views_bytes'][0] is ctypes.c_size_t and len(protos['nc_progress_views'][1]) == 10
    assert protos['nc_tensor2im'][1][3] is ctypes.c_long


def _vopt(tmp_path, **kw):
    d = dict(checkpoints_dir=str(tmp_path), name='run', isTrain=True, no_html=False, display_histogram=False)
    d.update(kw)
    return Namespace(**d)


def test_visualizer_loss_log_has_the_references_format(tmp_path, capsys):
    from neuroclear_amd.util.visualizer import Visualizer
    vis = Visualizer(_vopt(tmp_path))
    assert vis.web_dir == os.path.join(str(tmp_path), 'run', 'web') and vis.img_dir == os.path.join(vis.web_dir, 'images')
    assert os.path.isdir(vis.img_dir) and vis.log_name == os.path.join(str(tmp_path), 'run', 'loss_log.txt')
    losses = OrderedDict([('D_A_lateral', 0.25), ('G_A', 1.23456), ('cycle', -0.5)])
    vis.print_current_losses(1, 40, losses, 0.0219, 0.5)
    line = '(epoch: 1, epoch_progress: 40%, iter time: 0.022, data load time: 0.500) D_A_lateral: 0.250 G_A: 1.235 cycle: -0.500 '
    assert capsys.readouterr().out.endswith(line + '\n')
    assert LOSS_LINE.match(line)
    Visualizer(_vopt(tmp_path)).print_current_losses(1, 41, losses, 1, 2)  # a second run appends: header, line
    rows = open(vis.log_name).read().split('\n')
    assert len(rows) == 5 and rows[4] == ''
    for r in (rows[0], rows[2]):
        assert re.fullmatch(r'================ Training Loss \(.+\) ================', r)
    assert rows[1] == line and LOSS_LINE.match(rows[3])
    # tensorboard-only methods of the reference exist and write nothing; without --display_histogram the histogram call neither
    before = sorted(os.listdir(vis.img_dir)), sorted(os.listdir(os.path.dirname(vis.log_name)))
    vis.reset()
    vis.display_model_hyperparameters()
    vis.plot_current_losses(3, losses, is_epoch=False)
    vis.display_current_histogram(OrderedDict(real=torch.zeros(1, 1, 4, 4, 4)), 3)
    assert (sorted(os.listdir(vis.img_dir)), sorted(os.listdir(os.path.dirname(vis.log_name)))) == before == ([], ['loss_log.txt', 'web'])


def test_no_html_keeps_only_the_loss_log(tmp_path):
    from neuroclear_amd.util.visualizer import Visualizer
    vis = Visualizer(_vopt(tmp_path, no_html=True, display_histogram=True))
    visuals = OrderedDict(real=torch.zeros(1, 1, 4, 4, 4))  # CPU tensors: any launch attempt would raise NcError
    vis.display_current_results(visuals, 1)
    vis.display_current_histogram(visuals, 1)
    vis.save_current_visuals(visuals, 1)
    vis.print_current_losses(1, 1, OrderedDict(G_A=1.0), 0.1, 0.2)
    assert os.listdir(os.path.join(str(tmp_path), 'run')) == ['loss_log.txt']
