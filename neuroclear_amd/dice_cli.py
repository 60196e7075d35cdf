"""What the two diced-inference entry scripts, neuroclear_amd.test_dice (3-D) and neuroclear_amd.infer_dice2d (2-D), share around their loops:
the command line, the loading of the first image of a directory, and the tail that writes the results."""
import os

import numpy as np


def build_parser(image_dimension=3, dice_size=(120, 120, 120), description='test_dice.py on MI355X (reference README.md:150-157)'):
    """The reference's command line for the flags that matter on this path; infer_dice2d.main builds it with its own two defaults."""
    import argparse
    p = argparse.ArgumentParser(description=description)
    p.add_argument('--dataroot', required=True)
    p.add_argument('--name', default='experiment_name')
    p.add_argument('--checkpoints_dir', default='./checkpoints')
    p.add_argument('--results_dir', default='./results/')
    p.add_argument('--gpu_ids', default='0')
    p.add_argument('--model', default='test')
    p.add_argument('--model_suffix', default='')
    p.add_argument('--netG', default='unet_deconv')
    p.add_argument('--norm', default='instance')
    p.add_argument('--init_type', default='normal')
    p.add_argument('--init_gain', type=float, default=0.02)
    p.add_argument('--input_nc', type=int, default=1)
    p.add_argument('--output_nc', type=int, default=1)
    p.add_argument('--ngf', type=int, default=64)
    p.add_argument('--image_dimension', type=int, default=image_dimension)
    p.add_argument('--dice_size', type=int, nargs='+', default=list(dice_size))
    p.add_argument('--overlap', type=int, default=15)
    p.add_argument('--border_cut', type=int, default=10)
    p.add_argument('--data_type', default='uint16')
    p.add_argument('--epoch', default='latest')
    p.add_argument('--load_iter', type=int, default=0)
    p.add_argument('--skip_real', action='store_true')
    p.add_argument('--no_dropout', action='store_true')
    p.add_argument('--histogram_match', action='store_true')
    p.add_argument('--normalize_intensity', action='store_true')
    p.add_argument('--sat_level', type=float, nargs='+', default=[0.25, 99.75])
    p.add_argument('--verbose', action='store_true')
    p.add_argument('--phase', default='test')
    p.add_argument('--data_name', default=None)
    p.add_argument('--dataroot_gt', default=None, help='directory with the ground truth: enables the PSNR report')
    p.add_argument('--save_volume', action='store_true')
    p.add_argument('--save_projections', action='store_true')
    p.add_argument('--save_slices', action='store_true')
    return p


def load_first(dataroot):
    """The first .npy / .tif of a directory, or None without a directory."""
    from .data.diceImage_dataset import _load_volume
    if dataroot is None:
        return None
    names = sorted(f for f in os.listdir(dataroot) if f.endswith(('.npy', '.tif', '.tiff')))
    return _load_volume(os.path.join(dataroot, names[0]))


def save_results(opt, out, real, gt):
    """The tail of both entry scripts: web_dir as at test_dice.py:80-88, volumes/output_volume.npy, write_outputs.  Returns its metrics."""
    print('Image volume re-assembled.')
    print('re-merged image shape: {}'.format(out.shape))
    base = opt.name if opt.data_name is None else opt.data_name + '_by_' + opt.name
    web_dir = os.path.join(opt.results_dir, base, '{}_{}'.format(opt.phase, opt.epoch))
    if opt.load_iter > 0:
        web_dir = '{:s}_iter{:d}'.format(web_dir, opt.load_iter)
    os.makedirs(os.path.join(web_dir, 'volumes'), exist_ok=True)
    np.save(os.path.join(web_dir, 'volumes', 'output_volume.npy'), out)
    from .test_dice import write_outputs
    metrics = write_outputs(opt, web_dir, out, real, gt)
    print('----Test done----')
    return metrics
