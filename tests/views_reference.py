"""Reference side of the progress-view tests (nc_tensor2im / nc_progress_views, csrc/views.hip): a numpy restatement of the reference's
util.tensor2im (util/util.py:26-39) and of the indexing of Visualizer.display_current_results (util/visualizer.py:141-144, 171-173), the
inputs both sides regenerate from seeds, and the special values.  tests/test_progress_views.py pins the restatement to the reference's own
outputs (tests/golden/progress_views.npz, written by tools/gen_golden_views.py); tests/test_gpu_progress_views.py holds the kernels to it.
Everything is integer: the comparisons are exact."""
import numpy as np

KEYS = ('slice_xy', 'slice_xz', 'slice_yz', 'mip_xy', 'mip_xz', 'mip_yz')
# [N, C, D, H, W] of the volumes the golden file holds (tiny: the file stays a few KB); their seeds are 700 + position
GOLDEN_SHAPES = [(1, 1, 1, 1, 1), (1, 1, 3, 2, 5), (1, 1, 12, 9, 11), (2, 3, 6, 7, 8)]


def volume(seed, shape):
    """rnd * 1.6 - 0.3 in fp32: about a fifth of the values below 0 and a fifth above 1, so both clips act."""
    r = np.random.default_rng(seed).random(shape, dtype=np.float32)
    return r * np.float32(1.6) - np.float32(0.3)


def special_values():
    """-0.0, 0, 1, the fp32 neighbours of 1, denormals, values far outside, and k / 255, k / 65535 with both fp32 neighbours: the places
    where the truncating cast of x * 255.0f (x * 65535.0f) decides between two integers."""
    f = np.float32
    v = [f(-0.0), f(0.0), f(1.0), np.nextafter(f(1), f(0)), np.nextafter(f(1), f(2)), f(1e-45), f(-1e-45), f(1.1754942e-38), f(1e-39),
         f(-5.0), f(7.0), f(0.5), f(0.25), f(3.4e38), f(-3.4e38)]
    for top, ks in ((255, (1, 2, 3, 7, 85, 127, 128, 200, 254, 255)), (65535, (1, 2, 3, 255, 256, 257, 21845, 32767, 32768, 65534, 65535))):
        for k in ks:
            x = f(k) / f(top)
            v += [np.nextafter(x, f(-1)), x, np.nextafter(x, f(2))]
    return np.array(v, dtype=np.float32)


def tensor2im(x, imtype):
    """util/util.py:26-39 on a float32 array: clip, multiply in place (float32), clip, truncating cast."""
    a = np.array(x, dtype=np.float32, copy=True)
    top = 2 ** 8 * 1.0 - 1 if imtype == np.uint8 else 2 ** 16 * 1.0 - 1
    a = np.clip(a, 0, 1)
    a *= top
    a = np.clip(a, 0, int(top))
    return a.astype(imtype)


def views(x, index=None):
    """The six arrays of visualizer.py:141-144, 171-173 of a [N, C, D, H, W] float32 array, and the counts of the uint8 values of [0, 0]."""
    img = tensor2im(x, np.uint8)
    b, c, d, h, w = img.shape
    s = int(d / 2) if index is None else index
    out = dict(slice_xy=img[0, 0, s, :, :], slice_xz=img[0, 0, :, s, :], slice_yz=img[0, 0, :, :, s],
               mip_xy=np.amax(img[0, 0], 0), mip_xz=np.amax(img[0, 0], 1), mip_yz=np.amax(img[0, 0], 2))
    out['hist'] = np.bincount(img[0, 0].ravel(), minlength=256).astype(np.int64)
    return out
