"""Assemble_Dice2D: the assembler of util/assemble_dice.py:11-213 on the two in-plane axes, for the tiles of
data/diceImage2d_dataset.py (--image_dimension 2).

Same interface as Assemble_Dice -- addToStack(visuals), assemble_all(), getDict() -- plus add_tiles(name, tiles, first) for a
whole batch of consecutive tiles: ONE nc_assemble2d_scatter_add crops their borders and overlap-adds tile / 8 into the padded
fp32 accumulator [L0, P1, P2], every accumulator pixel adding its tiles in ascending index, so the bits are those of adding
the tiles one by one in index order (the reference's summation order, :167-173) however the sequence is cut into batches.
assemble_all runs nc_assemble2d_finalize: (acc / count) * 8 * scale, truncating cast, crop of the dicing pad, with
count = cover(y) * cover(x) computed from the grid.  The / 8 ... * 8 of the 3-D assembler is kept although at most four
tiles overlap: a plane then carries the bits of a z-layer of the 3-D assembler that one layer of cubes covers.
`--histogram_match` (:149-151) matches every output tile's R x R interior to its input tile's interior."""
from collections import OrderedDict

import numpy as np
import torch

from .._lib import L_, P, check, lib
from . import util
from .assemble_dice import match_histograms


def match_tile(fake, real, roi_size, border_cut, device):
    """util/assemble_dice.py:149-151 for one tile: the border-cropped fake tile matched to the border-cropped real tile;
    returns the (R+2b)^2 fake tile with its interior replaced (the border is dropped by add_tiles anyway)."""
    E, b = roi_size + 2 * border_cut, border_cut
    fake = fake.reshape(E, E).to(device, torch.float32)
    real = real.reshape(E, E).to(device, torch.float32)
    out = fake.clone()
    out[b:-b, b:-b] = match_histograms(fake[b:-b, b:-b], real[b:-b, b:-b])
    return out


class Assemble_Dice2D:
    def __init__(self, opt, image_size_original=None):
        """image_size_original: (L1, L2) of one plane or (L0, L1, L2) of a stack, un-padded; when omitted it is taken from
        opt.volume_shape."""
        if image_size_original is None:
            image_size_original = opt.volume_shape
        size = tuple(int(s) for s in image_size_original)
        if len(size) not in (2, 3):
            raise ValueError('expected the size of one plane (L1, L2) or of a stack of planes (L0, L1, L2)')
        self.single_plane = len(size) == 2
        self.image_size_original = ((1,) + size) if self.single_plane else size
        self.border_cut = opt.border_cut
        self.roi_size = opt.dice_size[0]
        self.overlap = opt.overlap
        if self.border_cut < 1:
            raise ValueError('border_cut must be >= 1 (util/assemble_dice.py:143-145 crops cube[b:-b])')
        if self.overlap < 1:
            raise ValueError('overlap must be >= 1: the reference assembler adds nothing for overlap 0 '
                             '(util/assemble_dice.py:170) and returns an all-zero volume')
        if getattr(opt, 'normalize_intensity', False):
            raise NotImplementedError('--normalize_intensity is not implemented for the 2-D assembler')
        self.histogram_match = bool(getattr(opt, 'histogram_match', False))
        self.step = self.roi_size - self.overlap
        L0 = self.image_size_original[0]
        self.image_size = (L0,) + util.padded_shape(self.image_size_original[1:], self.roi_size, self.overlap)
        self.y_steps, self.x_steps = util.grid_steps(self.image_size[1:], self.roi_size, self.overlap)
        self.len_tile_queue = L0 * self.y_steps * self.x_steps
        self.visual_names = ['real', 'fake']
        self.imtype = opt.data_type
        if self.imtype not in ('uint8', 'uint16'):
            raise ValueError('data_type must be uint8 or uint16')
        self.skip_real = opt.skip_real
        self.device = torch.device('cuda', opt.gpu_ids[0]) if getattr(opt, 'gpu_ids', None) else torch.device('cuda')
        self.acc = OrderedDict()
        self.count = OrderedDict()
        self.visual_ret = OrderedDict()
        for name in self.visual_names:
            if self.skip_real and name == 'real':
                continue
            self.acc[name] = torch.zeros(self.image_size, dtype=torch.float32, device=self.device)
            self.count[name] = 0

    def indexTo3DIndex(self, index):
        per = self.x_steps * self.y_steps
        return index // per, (index % per) // self.x_steps, index % self.x_steps

    def indexToCoordinates(self, index):
        z, y, x = self.indexTo3DIndex(index)
        return z, y * self.step, x * self.step

    def add_tiles(self, name, tiles, first):
        """Overlap-add the network outputs [count, E, E] or [count, 1, E, E] of the tiles first .. first + count - 1."""
        E = self.roi_size + 2 * self.border_cut
        if tiles.dim() == 4 and tiles.shape[1] == 1:
            tiles = tiles[:, 0]
        if tiles.dim() != 3 or tuple(tiles.shape[1:]) != (E, E):
            raise AssertionError('the tile dimensions are invalid.')
        count = int(tiles.shape[0])
        if first < 0 or count < 1 or first + count > self.len_tile_queue:
            raise IndexError((first, count))
        if tiles.dtype != torch.float32 or not tiles.is_cuda:
            tiles = tiles.to(self.device, torch.float32)
        tiles = tiles.contiguous()
        L0, P1, P2 = self.image_size
        check(lib().nc_assemble2d_scatter_add(P(tiles.data_ptr()), P(self.acc[name].data_ptr()), L0, P1, P2,
                                              self.roi_size, self.overlap, self.border_cut, L_(int(first)), count,
                                              P(torch.cuda.current_stream().cuda_stream)), 'nc_assemble2d_scatter_add')
        self.count[name] += count  # assemble_all wants every tile exactly once

    def match_tile(self, fake, real):
        return match_tile(fake, real, self.roi_size, self.border_cut, self.device)

    def addToStack(self, tile):
        """tile: OrderedDict {'real': [1,1,E,E], 'fake': ...} as returned by model.get_current_visuals(): one tile per
        call, in index order."""
        E = self.roi_size + 2 * self.border_cut
        if self.histogram_match:
            tile = OrderedDict(tile)
            tile['fake'] = self.match_tile(tile['fake'], tile['real'])
        for name in self.visual_names:
            if self.skip_real and name == 'real':
                continue
            t = tile[name]
            if t.numel() != E * E:
                raise AssertionError('the tile dimensions are invalid.')
            self.add_tiles(name, t.reshape(1, E, E), self.count[name])

    def assemble_all(self):
        L0, L1, L2 = self.image_size_original
        _, P1, P2 = self.image_size
        for name, acc in self.acc.items():
            if self.count[name] != self.len_tile_queue:
                raise Exception('expected %d tiles for %s, got %d' % (self.len_tile_queue, name, self.count[name]))
            u16 = self.imtype == 'uint16'
            out = torch.empty((L0, L1, L2), dtype=torch.int16 if u16 else torch.uint8, device=self.device)
            check(lib().nc_assemble2d_finalize(P(acc.data_ptr()), P(out.data_ptr()), 1 if u16 else 0, L0, P1, P2, L1, L2,
                                               self.roi_size, self.overlap,
                                               P(torch.cuda.current_stream().cuda_stream)), 'nc_assemble2d_finalize')
            host = out.cpu().numpy()
            host = host.view(np.uint16) if u16 else host
            self.visual_ret[name] = host[0] if self.single_plane else host

    def getDict(self):
        return self.visual_ret
