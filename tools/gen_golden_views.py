"""Golden vectors of the training progress views, from the REFERENCE itself on the CPU, with the helpers of oracle.gen_golden.

    python tools/gen_golden_views.py            (from the repo root; needs the reference checkout that oracle.gen_golden names)

Writes tests/golden/progress_views.npz: for the tiny volumes of tests/views_reference.py (regenerated from seeds on both sides, not stored)
and its vector of special values, the outputs of the reference's own util.util.tensor2im as uint8 and uint16; for the volumes also the six
arrays Visualizer.display_current_results takes from the uint8 image.  util/visualizer.py itself imports tensorboard, matplotlib and
tifffile at module level and cannot be loaded here, so its indexing lines (:141-144, 171-173) are applied to the reference's tensor2im
output below, as written there."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

from oracle import gen_golden as gg  # noqa: E402
from oracle.gen_golden import ref_modules  # noqa: E402
import views_reference as V  # noqa: E402


def gen():
    ref_modules()  # (the stand-in modules and the reference on sys.path)
    from util import util as rutil
    out = dict(shapes=np.array(V.GOLDEN_SHAPES), seeds=np.array([700 + i for i in range(len(V.GOLDEN_SHAPES))]))
    sp = V.special_values()
    out['special_x'] = sp  # stored as well: a fixture that does not depend on how the test side builds the vector
    out['special_u8'] = rutil.tensor2im(torch.from_numpy(sp), imtype=np.uint8)
    out['special_u16'] = rutil.tensor2im(torch.from_numpy(sp), imtype=np.uint16)
    for i, shape in enumerate(V.GOLDEN_SHAPES):
        image = torch.from_numpy(V.volume(700 + i, shape))
        pre = 'v%d_' % i
        out[pre + 'u16'] = rutil.tensor2im(image, imtype=np.uint16)
        img_np = rutil.tensor2im(image, imtype=np.uint8)
        out[pre + 'u8'] = img_np
        b, c, d, h, w = img_np.shape
        slice_portion = int(d / 2)
        out[pre + 'slice_xy'] = img_np[0, 0, slice_portion, :, :]
        out[pre + 'slice_xz'] = img_np[0, 0, :, slice_portion, :]
        out[pre + 'slice_yz'] = img_np[0, 0, :, :, slice_portion]
        out[pre + 'mip_xy'] = np.amax(img_np[0, 0], 0)
        out[pre + 'mip_xz'] = np.amax(img_np[0, 0], 1)
        out[pre + 'mip_yz'] = np.amax(img_np[0, 0], 2)
        # save_current_visuals (:252): tensor2im of image[0]
        assert np.array_equal(rutil.tensor2im(image[0], imtype=np.uint8), img_np[0])
    for k, v in out.items():
        assert k in ('shapes', 'seeds', 'special_x') or v.dtype in (np.uint8, np.uint16), (k, v.dtype)
    path = os.path.join(gg.OUT, 'progress_views.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
    gen()
