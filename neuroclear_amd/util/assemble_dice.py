"""Assemble_Dice on the device (reference: util/assemble_dice.py:11-213), and Assemble_Base, which it shares with
util/assemble_dice2d.py.

Same interface -- Assemble_Dice(opt), addToStack(visuals), assemble_all(), getDict() -- but the cubes never leave HBM:
addToStack crops the border and overlap-adds cube/8 into a padded fp32 accumulator right away (nc_assemble_scatter_add,
in arrival = index order, exactly the reference's summation order), assemble_all runs nc_assemble_finalize
((acc / count) * 8 * 65535, truncating cast, crop of the dicing pad) with the count computed analytically.
`--normalize_intensity` (:188-192) runs on the device too: exact percentiles of the merged, still padded volume by radix
select (util/percentile.py restates np.percentile of the reference's numpy 1.21.2), then the arithmetic of
skimage.exposure.rescale_intensity (0.18.3) on a float32 image -- third-party arithmetic restated from its source,
parity unpinned (scikit-image is not installed here).  `--histogram_match` (:149-151, skimage match_histograms of every
border-cropped output cube against its input cube) is nc_match_histograms: radix sort of both cubes + np.interp's
arithmetic in float64 on the device, restated from scikit-image 0.18.3, parity unpinned for the same reason."""
from collections import OrderedDict

import numpy as np
import torch

from .._lib import P, check, lib
from . import util


def match_histograms(source, template):
    """skimage.exposure.match_histograms(source, template) on the device (float32 tensors of equal size)."""
    src = source.contiguous().float()
    tm = template.contiguous().float()
    if src.numel() != tm.numel() or not src.is_cuda or not tm.is_cuda:
        raise ValueError('match_histograms: two CUDA tensors of equal size expected')
    n = src.numel()
    out = torch.empty_like(src)
    nb = lib().nc_match_histograms_ws_bytes(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=src.device)
    check(lib().nc_match_histograms(P(src.data_ptr()), P(tm.data_ptr()), P(out.data_ptr()), n, P(ws.data_ptr()), nb,
                                    P(torch.cuda.current_stream().cuda_stream)), 'nc_match_histograms')
    return out


def match_interior(fake, real, roi_size, border_cut, device, axes):
    """util/assemble_dice.py:149-151: the border-cropped fake piece matched to the border-cropped real piece; returns the
    (R+2b)^axes fake piece with its interior replaced (the border is dropped by the overlap-add anyway)."""
    E, b = roi_size + 2 * border_cut, border_cut
    fake = fake.reshape((E,) * axes).to(device, torch.float32)
    real = real.reshape((E,) * axes).to(device, torch.float32)
    inner = (slice(b, -b),) * axes
    out = fake.clone()
    out[inner] = match_histograms(fake[inner], real[inner])
    return out


def match_cube(fake, real, roi_size, border_cut, device):
    return match_interior(fake, real, roi_size, border_cut, device, 3)


class Assemble_Base:
    """What Assemble_Dice and Assemble_Dice2D share: the option checks, the padded fp32 accumulators, the addToStack loop, the host
    conversion and getDict.  The last `axes` axes of the (L0, L1, L2) image are diced; a subclass adds its geometry, `_add_one` (one
    piece of addToStack) and `_finalize(acc, out)`."""
    axes, pieces = 3, 'cubes'

    def __init__(self, opt, image_size_original=None, acc_planes=None):
        """image_size_original: (L0, L1, L2), un-padded; when omitted it is taken from opt.volume_shape.
        acc_planes: the accumulators hold that many planes of axis 0 only."""
        if image_size_original is None:
            image_size_original = opt.volume_shape
        self.image_size_original = tuple(int(s) for s in image_size_original)
        self.border_cut = opt.border_cut
        self.roi_size = opt.dice_size[0]
        self.overlap = opt.overlap
        if self.border_cut < 1:
            raise ValueError('border_cut must be >= 1 (util/assemble_dice.py:143-145 crops cube[b:-b])')
        if self.overlap < 1:
            raise ValueError('overlap must be >= 1: the reference assembler adds nothing for overlap 0 '
                             '(util/assemble_dice.py:170) and returns an all-zero volume')
        self.histogram_match = bool(getattr(opt, 'histogram_match', False))
        self.step = self.roi_size - self.overlap
        k = 3 - self.axes  # the leading axes are neither diced nor padded: one piece per plane
        self.image_size = self.image_size_original[:k] + util.padded_shape(self.image_size_original[k:], self.roi_size, self.overlap)
        self.z_steps, self.y_steps, self.x_steps = self.image_size[:k] + util.grid_steps(self.image_size[k:], self.roi_size, self.overlap)
        self.len_queue = self.z_steps * self.y_steps * self.x_steps
        self.visual_names = ['real', 'fake']
        self.imtype = opt.data_type
        if self.imtype not in ('uint8', 'uint16'):
            raise ValueError('data_type must be uint8 or uint16')
        self.skip_real = opt.skip_real
        self.device = torch.device('cuda', opt.gpu_ids[0]) if getattr(opt, 'gpu_ids', None) else torch.device('cuda')
        self.acc = OrderedDict()
        self.count = OrderedDict()
        self.visual_ret = OrderedDict()
        shape = self.image_size if acc_planes is None else (acc_planes,) + tuple(self.image_size[1:])
        for name in self.visual_names:
            if self.skip_real and name == 'real':
                continue
            self.acc[name] = torch.zeros(shape, dtype=torch.float32, device=self.device)
            self.count[name] = 0

    def indexTo3DIndex(self, index):
        return (index // (self.x_steps * self.y_steps), (index % (self.x_steps * self.y_steps)) // self.x_steps,
                index % self.x_steps)

    def indexToCoordinates(self, index):
        z, y, x = self.indexTo3DIndex(index)
        return z * (self.step if self.axes == 3 else 1), y * self.step, x * self.step

    def addToStack(self, piece):
        """piece: OrderedDict {'real': [1,1,E,..,E], 'fake': ...} as returned by model.get_current_visuals(): one piece per call, in
        index order."""
        if self.histogram_match:
            piece = OrderedDict(piece)
            piece['fake'] = match_interior(piece['fake'], piece['real'], self.roi_size, self.border_cut, self.device, self.axes)
        for name in self.acc:
            self._add_one(name, piece[name], self.count[name])

    def _empty_out(self, shape):
        return torch.empty(shape, dtype=torch.int16 if self.imtype == 'uint16' else torch.uint8, device=self.device)

    def _to_host(self, out):
        host = out.cpu().numpy()  # torch has no uint16 arithmetic: the kernels wrote uint16 bits into an int16 tensor
        return host.view(np.uint16) if self.imtype == 'uint16' else host

    def assemble_all(self):
        for name, acc in self.acc.items():
            if self.count[name] != self.len_queue:
                raise Exception('expected %d %s for %s, got %d' % (self.len_queue, self.pieces, name, self.count[name]))
            out = self._empty_out(self.image_size_original)
            self._finalize(acc, out)
            self.visual_ret[name] = self._to_host(out)

    def getDict(self):
        return self.visual_ret


class Assemble_Dice(Assemble_Base):
    def __init__(self, opt, image_size_original=None, slab=None):
        """image_size_original: (z, y, x) of the un-padded volume; when omitted it is taken from opt.volume_shape.
        slab = (za, zb): the accumulators hold only the padded planes [za, zb) (sharded inference, test_dice.py assemble='slab':
        a rank's cubes touch two or three z-layers); add_cube then accepts only cubes inside that range."""
        self.slab = None if slab is None else (int(slab[0]), int(slab[1]))
        super().__init__(opt, image_size_original, None if slab is None else self.slab[1] - self.slab[0])
        self.normalize_intensity = bool(getattr(opt, 'normalize_intensity', False))
        self.p1, self.p99 = getattr(opt, 'sat_level', [0.25, 99.75])  # options/test_options.py:25
        self.len_cube_queue = self.len_queue

    def add_cube(self, name, cube, index):
        """Overlap-add one (R+2b)^3 network output at cube position `index`."""
        E = self.roi_size + 2 * self.border_cut
        cube = cube.reshape(-1)
        if cube.numel() != E * E * E:
            raise AssertionError('the cube dimensions are invalid.')
        if cube.dtype != torch.float32 or not cube.is_cuda:
            cube = cube.to(self.device, torch.float32)
        cube = cube.contiguous()
        P0, P1, P2 = self.image_size
        base = self.acc[name].data_ptr()
        if self.slab is not None:  # the kernel indexes absolute planes: hand it where plane 0 WOULD be (it only touches the cube's planes)
            z0 = self.indexToCoordinates(int(index))[0]
            if z0 < self.slab[0] or z0 + self.roi_size > self.slab[1]:
                raise AssertionError('cube %d lies outside the planes [%d, %d) of this accumulator' % (index, self.slab[0], self.slab[1]))
            base -= self.slab[0] * P1 * P2 * 4
        check(lib().nc_assemble_scatter_add(P(cube.data_ptr()), P(base), P0, P1, P2,
                                            self.roi_size, self.overlap, self.border_cut, int(index),
                                            P(torch.cuda.current_stream().cuda_stream)), 'nc_assemble_scatter_add')

    def _add_one(self, name, cube, index):
        self.add_cube(name, cube, index)
        self.count[name] += 1

    def finalize_slab(self, own_acc, za, zb):
        """(acc / count) * 8 * scale and the truncating cast for the padded planes [za, zb) held in own_acc (already complete: every
        rank's contributions added): returns the device tensor of the planes [za, zb) & [0, L0) of the un-padded volume."""
        L0, L1, L2 = self.image_size_original
        P0, P1, P2 = self.image_size
        z0, z1 = min(za, L0), min(zb, L0)
        out = self._empty_out((z1 - z0, L1, L2))
        if z1 > z0:
            check(lib().nc_assemble_finalize_slab(P(own_acc.data_ptr()), P(out.data_ptr()), int(self.imtype == 'uint16'), P0, P1, P2, L0,
                                                  L1, L2, self.roi_size, self.overlap, z0, z1 - z0, za,
                                                  P(torch.cuda.current_stream().cuda_stream)), 'nc_assemble_finalize_slab')
        return out

    def assemble_all(self):
        if self.slab is not None:
            raise Exception('a slab accumulator is finalised by its owner ranks (finalize_slab), not by assemble_all')
        super().assemble_all()

    def _finalize(self, acc, out):
        if self.normalize_intensity:
            return self._finalize_normalized(acc, out, self.imtype == 'uint16')
        L0, L1, L2 = self.image_size_original
        P0, P1, P2 = self.image_size
        check(lib().nc_assemble_finalize(P(acc.data_ptr()), P(out.data_ptr()), int(self.imtype == 'uint16'), P0, P1,
                                         P2, L0, L1, L2, self.roi_size, self.overlap,
                                         P(torch.cuda.current_stream().cuda_stream)), 'nc_assemble_finalize')

    def _finalize_normalized(self, acc, out, u16):
        """util/assemble_dice.py:184-203 with --normalize_intensity: percentiles over the merged PADDED volume."""
        from . import percentile as pct
        L0, L1, L2 = self.image_size_original
        stream = P(torch.cuda.current_stream().cuda_stream)
        merged = torch.empty_like(acc)
        check(lib().nc_assemble_merge(P(acc.data_ptr()), P(merged.data_ptr()), L0, L1, L2, self.roi_size,
                                      self.overlap, stream), 'nc_assemble_merge')
        p_lo, p_hi = pct.percentile(merged, (self.p1, self.p99))
        if not p_hi > p_lo:
            raise ValueError('normalize_intensity: empty intensity range (%g, %g)' % (p_lo, p_hi))
        self.last_percentiles = (p_lo, p_hi)
        check(lib().nc_assemble_rescale_finalize(P(merged.data_ptr()), P(out.data_ptr()), 1 if u16 else 0, L0,
                                                 L1, L2, self.roi_size, self.overlap,
                                                 np.float32(p_lo), np.float32(p_hi), np.float32(p_hi - p_lo),
                                                 stream), 'nc_assemble_rescale_finalize')
