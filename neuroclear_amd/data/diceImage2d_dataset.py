"""DiceImage2DDataSet: the dicing of data/diceImage_dataset.py:9-123 on the two in-plane axes, for the 2-D generators
(--image_dimension 2: unet_deconv / unet_vanilla dimension=2, resnet_6blocks / resnet_9blocks).

The input is one plane (L1, L2) or a stack (L0, L1, L2) that is diced plane by plane: axis 0 is neither diced, padded nor
reflected, and a plane is held as a stack of one.  The ORIGINAL uint16 / uint8 image is uploaded once and stays resident in
HBM; `cut(first, count)` launches nc_dice2d_cut_tiles ONCE for `count` consecutive tiles -- the zero dicing pad, the reflect
border and v / 65535 (fp64, then rounded to fp32 like numpy does) are index arithmetic on the device, as in the 3-D set."""
import torch

from .._lib import L_, P, check, lib
from ..util import util
from .diceImage_dataset import load_resident


class DiceImage2DDataSet:
    def __init__(self, opt, image=None):
        """opt: dataroot (directory holding one .npy/.tif image) or `image` given directly (numpy / torch, uint8 or uint16,
        2-D or 3-D); dice_size, overlap, border_cut, gpu_ids as in the reference's options."""
        self.opt = opt
        self.roi_size = opt.dice_size[0]
        self.overlap = opt.overlap
        self.border_cut = opt.border_cut
        if self.border_cut < 1:
            raise ValueError('border_cut must be >= 1: the reference crops cube[b:-b], which is empty for b = 0 '
                             '(util/assemble_dice.py:143-145)')
        self.image, self.is_u16, self.device = load_resident(opt, image, 'image')
        if self.image.dim() not in (2, 3):
            raise ValueError('expected one plane (L1, L2) or a stack of planes (L0, L1, L2)')
        self.single_plane = self.image.dim() == 2
        if self.single_plane:
            self.image = self.image.unsqueeze(0)
        self.image_size_original = tuple(int(s) for s in self.image.shape)
        L0 = self.image_size_original[0]
        self.image_size = (L0,) + util.padded_shape(self.image_size_original[1:], self.roi_size, self.overlap)
        self.steps = (L0,) + util.grid_steps(self.image_size[1:], self.roi_size, self.overlap)

    def __len__(self):
        return self.steps[0] * self.steps[1] * self.steps[2]

    def cut(self, first, count):
        """Tiles first .. first + count - 1 as one [count, 1, E, E] tensor, from one launch."""
        if first < 0 or count < 1 or first + count > len(self):
            raise IndexError((first, count))
        E = self.roi_size + 2 * self.border_cut
        tiles = torch.empty((count, 1, E, E), dtype=torch.float32, device=self.device)
        L0, L1, L2 = self.image_size_original
        check(lib().nc_dice2d_cut_tiles(P(self.image.data_ptr()), 1 if self.is_u16 else 0, L0, L1, L2,
                                        self.roi_size, self.overlap, self.border_cut, L_(int(first)), int(count),
                                        P(tiles.data_ptr()), P(torch.cuda.current_stream().cuda_stream)),
              'nc_dice2d_cut_tiles')
        return tiles

    def __getitem__(self, index):
        if index < 0 or index >= len(self):
            raise IndexError(index)
        return {'A': self.cut(int(index), 1)[0], 'A_paths': str(index)}

    def shape(self):
        return self.steps

    def size(self):
        return self.image_size

    def size_original(self):
        return self.image_size_original
