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
import torch

from .._lib import L_, P, check, lib
from .assemble_dice import Assemble_Base, match_interior


def match_tile(fake, real, roi_size, border_cut, device):
    """util/assemble_dice.py:149-151 for one tile: the (R+2b)^2 fake tile with its interior matched to the real tile's interior."""
    return match_interior(fake, real, roi_size, border_cut, device, 2)


class Assemble_Dice2D(Assemble_Base):
    axes, pieces = 2, 'tiles'

    def __init__(self, opt, image_size_original=None):
        """image_size_original: (L1, L2) of one plane or (L0, L1, L2) of a stack, un-padded; when omitted it is taken from
        opt.volume_shape."""
        if image_size_original is None:
            image_size_original = opt.volume_shape
        size = tuple(image_size_original)
        if len(size) not in (2, 3):
            raise ValueError('expected the size of one plane (L1, L2) or of a stack of planes (L0, L1, L2)')
        if getattr(opt, 'normalize_intensity', False):
            raise NotImplementedError('--normalize_intensity is not implemented for the 2-D assembler')
        self.single_plane = len(size) == 2
        super().__init__(opt, ((1,) + size) if self.single_plane else size)
        self.len_tile_queue = self.len_queue

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

    def _add_one(self, name, tile, index):
        E = self.roi_size + 2 * self.border_cut
        if tile.numel() != E * E:
            raise AssertionError('the tile dimensions are invalid.')
        self.add_tiles(name, tile.reshape(1, E, E), index)

    def _finalize(self, acc, out):
        L0, L1, L2 = self.image_size_original
        _, P1, P2 = self.image_size
        check(lib().nc_assemble2d_finalize(P(acc.data_ptr()), P(out.data_ptr()), int(self.imtype == 'uint16'), L0, P1, P2, L1, L2,
                                           self.roi_size, self.overlap,
                                           P(torch.cuda.current_stream().cuda_stream)), 'nc_assemble2d_finalize')

    def assemble_all(self):
        super().assemble_all()
        if self.single_plane:
            for name, host in self.visual_ret.items():
                self.visual_ret[name] = host[0]
