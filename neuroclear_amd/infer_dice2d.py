"""Diced inference for the 2-D generators (unet_deconv / unet_vanilla dimension=2, resnet_6blocks / resnet_9blocks): the loop of the
reference's test_dice.py:50-157 -- `for data in dataset: set_input; test; addToStack`, then `assemble_all` -- on a plane or a stack of planes
diced on the two in-plane axes (data/diceImage2d_dataset.py, util/assemble_dice2d.py).

`diced_inference_2d` is the loop: a batch of consecutive tiles per network call, on the calling stream, on one rank.
`main()` takes the command line of neuroclear_amd.test_dice with --image_dimension 2 (its default here) and writes the same output layout;
the 3-D entry script neuroclear_amd/test_dice.py is unchanged."""
import copy
import os

import numpy as np
import torch

from .data.diceImage2d_dataset import DiceImage2DDataSet
from .util.assemble_dice2d import Assemble_Dice2D, match_tile


def diced_inference_2d(netG, image, opt, nbatch=8, with_real=False, on_batch=None):
    """image: uint8/uint16 ndarray, one plane (L1, L2) or a stack (L0, L1, L2) that is diced plane by plane.  Per batch of `nbatch`
    consecutive tiles: one cut, one netG call on [nbatch, 1, E, E], one scatter-add -- under torch.no_grad(), on the calling stream only.
    Returns the assembled uint8/uint16 ndarray with the input's dimensionality, or (fake, real) with with_real (the dice -> assemble round
    trip of the input, the input up to 1 LSB of the truncating cast).
    on_batch(fn) -> result: optional wrapper around each batch's network call.
    nbatch=1 is the reference's batch size (test_dice.py:66); a tile's result depends on its batch mates only through fp32 rounding (within
    1 LSB of the one-tile-per-call result, as for the 3-D path)."""
    if getattr(opt, 'normalize_intensity', False):
        raise NotImplementedError('--normalize_intensity is not implemented for --image_dimension 2')
    nbatch = int(nbatch)
    if nbatch < 1:
        raise ValueError('nbatch must be >= 1')
    opt = copy.copy(opt)
    opt.skip_real = not with_real
    ds = DiceImage2DDataSet(opt, image=image)
    asm = Assemble_Dice2D(opt, ds.size_original())
    n = len(ds)
    R, b = opt.dice_size[0], opt.border_cut
    hm = bool(getattr(opt, 'histogram_match', False))
    with torch.no_grad():
        for first in range(0, n, nbatch):
            count = min(nbatch, n - first)
            x = ds.cut(first, count)
            y = netG(x) if on_batch is None else on_batch(lambda: netG(x))
            if tuple(y.shape) != tuple(x.shape):
                raise ValueError('netG returned %s for tiles of %s' % (tuple(y.shape), tuple(x.shape)))
            if hm:  # every output tile's interior matched to its input tile's interior (util/assemble_dice.py:149-151)
                y = torch.stack([match_tile(y[k], x[k], R, b, ds.device) for k in range(count)], 0)
            if with_real:
                asm.add_tiles('real', x, first)
            asm.add_tiles('fake', y, first)
    asm.assemble_all()
    out = asm.getDict()
    fake, real = out['fake'], out.get('real')
    if ds.single_plane:
        fake, real = fake[0], (None if real is None else real[0])
    return (fake, real) if with_real else fake


def main(argv=None):
    """The command line of neuroclear_amd.test_dice for the 2-D generators.  The first .npy / .tif under --dataroot is the input, 2-D or 3-D;
    a single plane goes through write_outputs as a one-plane stack; output layout and file names are those of the 3-D path."""
    import argparse
    from . import models
    from .data.diceImage_dataset import _load_volume
    from .test_dice import write_outputs
    p = argparse.ArgumentParser(description='test_dice.py for the 2-D generators on MI355X (reference README.md:150-157 with --image_dimension 2)')
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
    p.add_argument('--image_dimension', type=int, default=2)
    p.add_argument('--dice_size', type=int, nargs='+', default=[120, 120])
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
    p.add_argument('--dataroot_gt', default=None, help='directory with the ground-truth image: enables the PSNR report')
    p.add_argument('--save_volume', action='store_true')
    p.add_argument('--save_projections', action='store_true')
    p.add_argument('--save_slices', action='store_true')
    p.add_argument('--nbatch', type=int, default=8, help='tiles per network call')
    opt = p.parse_args(argv)
    if opt.image_dimension != 2:
        raise NotImplementedError('this entry script runs the 2-D generators: --image_dimension 3 is neuroclear_amd.test_dice')
    if opt.normalize_intensity:
        raise NotImplementedError('--normalize_intensity is not implemented for --image_dimension 2')
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise NotImplementedError('--image_dimension 2 runs on one rank: the 2-D diced inference is not sharded (WORLD_SIZE > 1)')
    opt.gpu_ids = [int(g) for g in opt.gpu_ids.split(',') if int(g) >= 0]
    opt.isTrain, opt.continue_train, opt.preprocess = False, False, 'addColorChannel'
    model = models.create_model(opt)
    model.setup(opt)
    names = sorted(f for f in os.listdir(opt.dataroot) if f.endswith(('.npy', '.tif', '.tiff')))
    img = _load_volume(os.path.join(opt.dataroot, names[0]))
    gt = None
    if opt.dataroot_gt is not None:
        gnames = sorted(f for f in os.listdir(opt.dataroot_gt) if f.endswith(('.npy', '.tif', '.tiff')))
        gt = _load_volume(os.path.join(opt.dataroot_gt, gnames[0]))
        gt = gt[None] if gt.ndim == 2 else gt
    want_real = not opt.skip_real
    res = diced_inference_2d(model.netG, img, opt, nbatch=opt.nbatch, with_real=want_real)
    out, real = res if want_real else (res, None)
    if img.ndim == 2:  # the output layout is a volume's: a plane is written as a stack of one
        out, real = out[None], (None if real is None else real[None])
    print('Image volume re-assembled.')
    print('re-merged image shape: {}'.format(out.shape))
    # web_dir as at test_dice.py:80-88
    base = opt.name if opt.data_name is None else opt.data_name + '_by_' + opt.name
    web_dir = os.path.join(opt.results_dir, base, '{}_{}'.format(opt.phase, opt.epoch))
    if opt.load_iter > 0:
        web_dir = '{:s}_iter{:d}'.format(web_dir, opt.load_iter)
    os.makedirs(os.path.join(web_dir, 'volumes'), exist_ok=True)
    np.save(os.path.join(web_dir, 'volumes', 'output_volume.npy'), out)
    metrics = write_outputs(opt, web_dir, out, real, gt)
    print('----Test done----')
    return metrics


if __name__ == '__main__':
    main()
