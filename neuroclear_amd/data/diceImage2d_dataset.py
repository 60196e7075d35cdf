"""DiceImage2DDataSet: the dicing of data/diceImage_dataset.py:9-123 on the two in-plane axes, for the 2-D generators
(--image_dimension 2: unet_deconv / unet_vanilla dimension=2, resnet_6blocks / resnet_9blocks).

The input is one plane (L1, L2) or a stack (L0, L1, L2) that is diced plane by plane: axis 0 is neither diced, padded nor
reflected, and a plane is held as a stack of one.  The ORIGINAL uint16 / uint8 image is uploaded once and stays resident in
HBM; `cut(first, count)` launches nc_dice2d_cut_tiles ONCE for `count` consecutive tiles -- the zero dicing pad, the reflect
border and v / 65535 (fp64, then rounded to fp32 like numpy does) are index arithmetic on the device, as in the 3-D set."""
import os

import numpy as np
import torch

from .._lib import L_, P, check, lib
from ..util import util
from .diceImage_dataset import _load_volume


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
        if image is None:
            names = sorted(f for f in os.listdir(opt.dataroot) if not f.startswith('.') and
                           f.endswith(('.npy', '.tif', '.tiff')))
            if not names:
                raise FileNotFoundError('no image (.npy/.tif) under %s' % opt.dataroot)
            image = _load_volume(os.path.join(opt.dataroot, names[0]))
        if isinstance(image, np.ndarray):
            if image.dtype not in (np.uint8, np.uint16):
                raise TypeError('input volume must be uint8 or uint16 (data/base_dataset.py:134-143), got %s'
                                % image.dtype)
            self.is_u16 = image.dtype == np.uint16
            image = np.ascontiguousarray(image) if image.flags.writeable else image.copy()  # (torch takes no read-only array)
            # torch has no uint16 arithmetic; the bytes are only ever read by the HIP kernel
            host = torch.from_numpy(image.view(np.int16) if self.is_u16 else image)
        else:
            if image.dtype not in (torch.uint8, torch.int16, torch.uint16):
                raise TypeError('input volume must be uint8 or uint16 (data/base_dataset.py:134-143), got %s'
                                % image.dtype)
            self.is_u16 = image.dtype != torch.uint8
            host = image
        if host.dim() not in (2, 3):
            raise ValueError('expected one plane (L1, L2) or a stack of planes (L0, L1, L2)')
        self.single_plane = host.dim() == 2
        if self.single_plane:
            host = host.unsqueeze(0)
        self.device = torch.device('cuda', opt.gpu_ids[0]) if getattr(opt, 'gpu_ids', None) else torch.device('cuda')
        self.image = host.contiguous().to(self.device)
        self.image_size_original = tuple(int(s) for s in host.shape)
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
