"""References of the ResNet-generator tests (resnet_6blocks / resnet_9blocks; reference models/networks.py:724-837), in torch, in whatever dtype
they are given.  Checked on the CPU by tests/test_resnet2d.py.  Nothing here calls the library.

PAD AND FOLD.  reflect_pad(x, p) is torch.nn.functional.pad(x, (p,) * 4, mode='reflect') by index arithmetic.  reflect_fold(g, H, W, p) is its
adjoint in the gather form and the summation order of csrc/resnet2d.hip: per output pixel ONE accumulator that starts at zero and adds, rows
outermost in the order (own i + p; low mirror p - i for 1 <= i <= p; high mirror 2 (n - 1) - i + p for n - 1 - p <= i <= n - 2), inside each row
the columns in the same order.  In float32 that is the kernel's chain; in float64 it equals autograd of the pad.

REFLECT CONVOLUTION (ReflectionPad2d(1) + Conv2d 3 x 3).  Reference: the float64 valid convolution of the explicitly padded input; its data gradient
the full correlation on the (H + 2) x (W + 2) domain, folded.  Yardstick: the one-accumulator fp32 chain in the kernel's order -- (c, ty, tx)
forward; (k, ty, tx) on the extended domain, then the fold above, backward.  Error measure and limit: tests/convt_reference.py's (FACTOR 3).

THE NETWORK.  resnet_forward restates ResnetGenerator functionally from a state dict: the layers in the reference's order, reflect pads through
reflect_pad, the transposed convolutions through torch's own, instance norm written out, batch norm through torch.nn.functional.batch_norm on
copies of the running statistics."""
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from convt_reference import FACTOR, MAX_FLOOR, RMS_FLOOR, err, ratios, within  # noqa: E402,F401
from conv2d_reference import case_id, k3_covered  # noqa: E402,F401


# ---- pad and fold ---------------------------------------------------------------------------------------------------------------------------
def mirror_index(n, p, device=None):
    i = torch.arange(-p, n + p, device=device).abs()
    return torch.where(i >= n, 2 * (n - 1) - i, i)


def reflect_pad(x, p):
    H, W = x.shape[-2:]
    assert H > p and W > p
    return x[..., mirror_index(H, p, x.device), :][..., mirror_index(W, p, x.device)]


def fold_sources(n, p, device=None):
    """[(padded index per pixel, valid per pixel)] in the kernel's order: own, low mirror, high mirror."""
    i = torch.arange(n, device=device)
    return [(i + p, torch.ones(n, dtype=torch.bool, device=device)),
            ((p - i).clamp(min=0), (i >= 1) & (i <= p)),
            ((2 * (n - 1) - i + p).clamp(max=n + 2 * p - 1), (i >= n - 1 - p) & (i <= n - 2))]


def reflect_fold(g, H, W, p):
    """Adjoint of reflect_pad: g [..., H + 2p, W + 2p] -> [..., H, W], summed in the documented order in g's dtype."""
    assert tuple(g.shape[-2:]) == (H + 2 * p, W + 2 * p)
    acc = torch.zeros(g.shape[:-2] + (H, W), dtype=g.dtype, device=g.device)
    for ri, rv in fold_sources(H, p, g.device):
        rows = g[..., ri, :]
        for ci, cv in fold_sources(W, p, g.device):
            m = rv[:, None] & cv[None, :]
            acc = acc + torch.where(m, rows[..., ci], torch.zeros((), dtype=g.dtype, device=g.device))
    return acc


def fold_terms(H, W, p, device=None):
    """Number of folded terms per pixel [H, W] (1 .. 9)."""
    r = sum(v.long() for _, v in fold_sources(H, p, device))
    c = sum(v.long() for _, v in fold_sources(W, p, device))
    return r[:, None] * c[None, :]


# ---- ReflectionPad2d(1) + Conv2d(k 3): float64 references and the chain oracle ----------------------------------------------------------------
def _taps_fwd(x):
    """[[x_padded[n, c, u + ty, v + tx]]]: the nine shifted views of the reflect-padded input."""
    N, C, H, W = x.shape
    p = reflect_pad(x, 1)
    return [[p[:, :, ty:ty + H, tx:tx + W] for tx in range(3)] for ty in range(3)]


def _taps_ext(dy):
    """[[dy[n, k, e - ty, f - tx]]] on the extended domain e in 0 .. H + 1, f in 0 .. W + 1 (padded-input coordinates), zero outside the image."""
    N, K, H, W = dy.shape
    z = torch.zeros(N, K, H + 4, W + 4, dtype=dy.dtype, device=dy.device)
    z[:, :, 2:H + 2, 2:W + 2] = dy
    return [[z[:, :, 2 - ty:2 - ty + H + 2, 2 - tx:2 - tx + W + 2] for tx in range(3)] for ty in range(3)]


def refr_fwd(x, w, b=None):
    x, w = x.double(), w.double()
    sh = _taps_fwd(x)
    y = sum(torch.einsum('ncuv,kc->nkuv', sh[ty][tx], w[:, :, ty, tx]) for ty in range(3) for tx in range(3))
    return y if b is None else y + b.double().view(1, -1, 1, 1)


def refr_dgrad(dy, w):
    dy, w = dy.double(), w.double()
    H, W = dy.shape[-2:]
    sh = _taps_ext(dy)
    dxe = sum(torch.einsum('nkuv,kc->ncuv', sh[ty][tx], w[:, :, ty, tx]) for ty in range(3) for tx in range(3))
    return reflect_fold(dxe, H, W, 1)


def chainr_fwd(x, w, b=None, dtype=torch.float32):
    x, w = x.to(dtype), w.to(dtype)
    N, C, H, W = x.shape
    K = w.shape[0]
    acc = torch.zeros(N, K, H, W, dtype=dtype, device=x.device)
    sh = _taps_fwd(x)
    for c in range(C):
        for ty in range(3):
            for tx in range(3):
                acc = acc + sh[ty][tx][:, c].reshape(N, 1, H, W) * w[:, c, ty, tx].reshape(1, K, 1, 1)
    return acc if b is None else acc + b.to(dtype).view(1, K, 1, 1)


def chainr_dgrad(dy, w, dtype=torch.float32):
    dy, w = dy.to(dtype), w.to(dtype)
    N, K, H, W = dy.shape
    C = w.shape[1]
    acc = torch.zeros(N, C, H + 2, W + 2, dtype=dtype, device=dy.device)
    sh = _taps_ext(dy)
    for k in range(K):
        for ty in range(3):
            for tx in range(3):
                acc = acc + sh[ty][tx][:, k].reshape(N, 1, H + 2, W + 2) * w[k, :, ty, tx].reshape(1, C, 1, 1)
    return reflect_fold(acc, H, W, 1)


@functools.lru_cache(maxsize=None)
def inputs3(N, C, K, H, W):
    """x, w, b, dy of the reflect convolution on the CPU in float32: seeded randn, the weights scaled by (2 / (9 C))^0.5, a bias of order 1."""
    g = torch.Generator().manual_seed(200000 * N + 1000 * C + 10 * K + H * W + 3)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = (1.0 + 0.25 * torch.randn(K, generator=g)) * (1.0 - 2.0 * (torch.arange(K) % 2))
    dy = torch.randn(N, K, H, W, generator=g)
    return x, w, b, dy


# (N, C, K, H, W, what it reaches): the smallest shapes that reach the tiled kernel (conv2d_reference.k3_covered) and its edges
KR_CASES = [
    (2, 64, 64, 130, 131, 'ragged tile rows and windows'),
    (1, 256, 256, 61, 97, 'the block\'s own width, exactly 256 workgroups'),
    (8, 64, 64, 5, 517, 'the last tile row has one image row, and its reflected neighbour is in another tile'),
    (16, 64, 64, 3, 517, 'both row folds meet on row 1'),
    (16, 64, 64, 2, 517, 'H = 2'),
    (8, 64, 64, 61, 33, 'a window of one column, whose reflected neighbour is in the previous window'),
]
# outside the coverage: _active reports 0, the entry points pad explicitly and still compute
KR_OUTSIDE = [
    (1, 64, 64, 20, 20, 'too few tiles'),
    (1, 256, 256, 16, 16, 'the block\'s width on the 64 x 64 input\'s map: too few tiles'),
    (2, 17, 64, 130, 131, 'an odd reduction side (forward)'),
]
# (NC, H, W, p) of the pad kernels
PAD_CASES = [(3, 2, 2, 1), (3, 3, 3, 1), (5, 4, 4, 3), (2, 7, 9, 3), (64, 37, 131, 1)]


# ---- the network ------------------------------------------------------------------------------------------------------------------------------
def _inorm(x, eps=1e-5):
    m = x.mean((2, 3), keepdim=True)
    v = ((x - m) ** 2).mean((2, 3), keepdim=True)
    return (x - m) / torch.sqrt(v + eps)


def resnet_forward(sd, x, n_blocks, norm='instance', use_dropout=False, training=True):
    """ResnetGenerator.forward from a state dict (tensors of x's dtype and device).  -> (y, {running-statistics key: value after the step}).
    Dropout is the identity (the goldens' dropout case runs in eval())."""
    stats = {}

    def nrm(h, pre):
        if norm == 'instance':
            return _inorm(h)
        rm, rv = sd[pre + '.running_mean'].clone(), sd[pre + '.running_var'].clone()
        h = F.batch_norm(h, rm, rv, sd[pre + '.weight'], sd[pre + '.bias'], training, 0.1, 1e-5)
        stats[pre + '.running_mean'], stats[pre + '.running_var'] = rm, rv
        return h

    def conv(h, pre, stride=1, pad=0):
        return F.conv2d(h, sd[pre + '.weight'], sd.get(pre + '.bias'), stride, pad)

    h = torch.relu(nrm(conv(reflect_pad(x, 3), 'model.1'), 'model.2'))
    h = torch.relu(nrm(conv(h, 'model.4', 2, 1), 'model.5'))
    h = torch.relu(nrm(conv(h, 'model.7', 2, 1), 'model.8'))
    second = 6 if use_dropout else 5
    for b in range(n_blocks):
        pre = 'model.%d.conv_block.' % (10 + b)
        t = torch.relu(nrm(conv(reflect_pad(h, 1), pre + '1'), pre + '2'))
        h = h + nrm(conv(reflect_pad(t, 1), pre + str(second)), pre + str(second + 1))
    for i in (10 + n_blocks, 13 + n_blocks):
        pre = 'model.%d' % i
        h = F.conv_transpose2d(h, sd[pre + '.weight'], sd.get(pre + '.bias'), 2, 1, 1)
        h = torch.relu(nrm(h, 'model.%d' % (i + 1)))
    return torch.sigmoid(conv(reflect_pad(h, 3), 'model.%d' % (17 + n_blocks))), stats
