"""Diced inference for the 2-D generators (unet_deconv / unet_vanilla dimension=2, resnet_6blocks / resnet_9blocks): the loop of the
reference's test_dice.py:50-157 -- `for data in dataset: set_input; test; addToStack`, then `assemble_all` -- on a plane or a stack of planes
diced on the two in-plane axes (data/diceImage2d_dataset.py, util/assemble_dice2d.py).

`diced_inference_2d` is the loop: a batch of consecutive tiles per network call, on the calling stream, on one rank.
`main()` takes the command line of neuroclear_amd.test_dice with --image_dimension 2 (its default here) and writes the same output layout:
parser, input loading and the tail are dice_cli.build_parser / load_first / save_results, as for the 3-D script."""
import copy
import os

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


def build_parser():
    """test_dice.py's command line with --image_dimension 2 and a two-axis --dice_size as defaults, plus --nbatch."""
    from .dice_cli import build_parser as base
    p = base(2, (120, 120), 'test_dice.py for the 2-D generators on MI355X (reference README.md:150-157 with --image_dimension 2)')
    p.add_argument('--nbatch', type=int, default=8, help='tiles per network call')
    return p


def main(argv=None):
    """The command line of neuroclear_amd.test_dice for the 2-D generators.  The first .npy / .tif under --dataroot is the input, 2-D or 3-D;
    a single plane goes through write_outputs as a one-plane stack; output layout and file names are those of the 3-D path."""
    from . import models
    from .dice_cli import load_first, save_results
    opt = build_parser().parse_args(argv)
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
    img, gt = load_first(opt.dataroot), load_first(opt.dataroot_gt)
    want_real = not opt.skip_real
    res = diced_inference_2d(model.netG, img, opt, nbatch=opt.nbatch, with_real=want_real)
    out, real = res if want_real else (res, None)
    # the output layout is a volume's: a plane is written as a stack of one
    out, real, gt = (a[None] if a is not None and a.ndim == 2 else a for a in (out, real, gt))
    return save_results(opt, out, real, gt)


if __name__ == '__main__':
    main()
