"""References, yardstick and cases of the op-level tests of the 2-D generator kernels: ConvTranspose2d(kernel 2, stride 2) (csrc/convt2d.hip,
tests/test_gpu_convt2d.py) and Conv2d(kernel 3, stride 1, padding 1).  Checked on the CPU by tests/test_conv2d_reference.py.  Nothing here calls
the library.

REFERENCE: the definitions as float64 einsums (on whatever device the operands live):
    transposed:  y[n,k,2u+a,2v+b] = bias[k] + sum_c x[n,c,u,v] w[c,k,a,b]      dx = sum_(k,a,b) dy w      dw = sum_(n,u,v) x dy      db = sum dy
    3 x 3:       y[n,k,u,v] = bias[k] + sum_(c,ty,tx) x[n,c,u+ty-1,v+tx-1] w[k,c,ty,tx]  (zero outside the image),  dx its adjoint
YARDSTICK ("chain oracle"): NOT torch's fp32 operator but a one-accumulator fp32 chain -- the terms of an output element added one at a time in
a fixed order, every product and every partial sum rounded to fp32.  That is the worst order an fp32 kernel legitimately has (a kernel that keeps
one MFMA accumulator per output element and walks the reduction serially IS this chain); torch's CPU operator sums in blocks and is 2 .. 6 x
closer to float64, so a correct single-chain kernel would fail a factor-3 limit against it.  Orders: transposed forward over c; its data gradient
over (k, a, b); its weight gradient over (n, u, v); its bias gradient over (n, row, column); 3 x 3 forward over (c, ty, tx), data gradient over
(k, ty, tx).
ERROR MEASURE and LIMIT: tests/convt_reference.py's -- maximum and rms of the error over the rms of the reference;
rms <= FACTOR rms_chain + RMS_FLOOR and max <= FACTOR max_chain + MAX_FLOOR with FACTOR = 3, RMS_FLOOR = 2^-23, MAX_FLOOR = 2^-21."""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from convt_reference import FACTOR, MAX_FLOOR, RMS_FLOOR, err, ratios, within  # noqa: E402,F401


# ---- ConvTranspose2d(k 2, s 2): float64 references ------------------------------------------------------------------------------------------
def ref_fwd(x, w, b=None):
    N, C, H, W = x.shape
    K = w.shape[1]
    y = torch.einsum('ncuv,ckab->nkuavb', x.double(), w.double()).reshape(N, K, 2 * H, 2 * W)
    return y if b is None else y + b.double().view(1, K, 1, 1)


def _taps(dy):
    N, K, H2, W2 = dy.shape
    return dy.reshape(N, K, H2 // 2, 2, W2 // 2, 2)


def ref_dgrad(dy, w):
    return torch.einsum('nkuavb,ckab->ncuv', _taps(dy.double()), w.double())


def ref_wgrad(x, dy):
    return torch.einsum('ncuv,nkuavb->ckab', x.double(), _taps(dy.double()))


def ref_dbias(dy):
    return dy.double().sum((0, 2, 3))


# ---- ConvTranspose2d(k 2, s 2): the chain oracle (dtype=torch.float64 turns each into the reference, summed in the same order) --------------
def chain_fwd(x, w, b=None, dtype=torch.float32):
    N, C, H, W = x.shape
    K = w.shape[1]
    x, w = x.to(dtype), w.to(dtype)
    acc = torch.zeros(N, K, H, 2, W, 2, dtype=dtype, device=x.device)
    for c in range(C):
        acc = acc + x[:, c].reshape(N, 1, H, 1, W, 1) * w[c][None, :, None, :, None, :]
    y = acc.reshape(N, K, 2 * H, 2 * W)
    return y if b is None else y + b.to(dtype).view(1, K, 1, 1)


def chain_dgrad(dy, w, dtype=torch.float32):
    g = _taps(dy.to(dtype))                       # [N, K, H, 2, W, 2]
    w = w.to(dtype)
    N, K, H, _, W, _ = g.shape
    C = w.shape[0]
    acc = torch.zeros(N, C, H, W, dtype=dtype, device=dy.device)
    for k in range(K):
        for a in range(2):
            for b in range(2):
                acc = acc + g[:, k, :, a, :, b].reshape(N, 1, H, W) * w[:, k, a, b].reshape(1, C, 1, 1)
    return acc


def chain_wgrad(x, dy, dtype=torch.float32):
    g = _taps(dy.to(dtype))
    x = x.to(dtype)
    N, C, H, W = x.shape
    K = g.shape[1]
    acc = torch.zeros(C, K, 2, 2, dtype=dtype, device=x.device)
    for n in range(N):
        for u in range(H):
            for v in range(W):
                acc = acc + x[n, :, u, v].reshape(C, 1, 1, 1) * g[n, :, u, :, v, :].reshape(1, K, 2, 2)
    return acc


def chain_dbias(dy, dtype=torch.float32):
    N, K, H2, W2 = dy.shape
    d = dy.to(dtype).permute(0, 2, 3, 1).reshape(-1, K)
    acc = torch.zeros(K, dtype=dtype, device=dy.device)
    for i in range(d.shape[0]):
        acc = acc + d[i]
    return acc


# ---- Conv2d(k 3, s 1, p 1): float64 references and the chain oracle -----------------------------------------------------------------------
def _shifted(x, ty, tx):
    """x[n, c, u + ty - 1, v + tx - 1] with zeros outside the image."""
    N, C, H, W = x.shape
    p = torch.zeros(N, C, H + 2, W + 2, dtype=x.dtype, device=x.device)
    p[:, :, 1:H + 1, 1:W + 1] = x
    return p[:, :, ty:ty + H, tx:tx + W]


def ref3_fwd(x, w, b=None):
    x, w = x.double(), w.double()
    y = sum(torch.einsum('ncuv,kc->nkuv', _shifted(x, ty, tx), w[:, :, ty, tx]) for ty in range(3) for tx in range(3))
    return y if b is None else y + b.double().view(1, -1, 1, 1)


def ref3_dgrad(dy, w):
    """dx[n,c,i,j] = sum_(k,ty,tx) dy[n,k,i-ty+1,j-tx+1] w[k,c,ty,tx]."""
    dy, w = dy.double(), w.double()
    return sum(torch.einsum('nkuv,kc->ncuv', _shifted(dy, 2 - ty, 2 - tx), w[:, :, ty, tx]) for ty in range(3) for tx in range(3))


def chain3_fwd(x, w, b=None, dtype=torch.float32):
    x, w = x.to(dtype), w.to(dtype)
    N, C, H, W = x.shape
    K = w.shape[0]
    acc = torch.zeros(N, K, H, W, dtype=dtype, device=x.device)
    sh = [[_shifted(x, ty, tx) for tx in range(3)] for ty in range(3)]
    for c in range(C):
        for ty in range(3):
            for tx in range(3):
                acc = acc + sh[ty][tx][:, c].reshape(N, 1, H, W) * w[:, c, ty, tx].reshape(1, K, 1, 1)
    return acc if b is None else acc + b.to(dtype).view(1, K, 1, 1)


def chain3_dgrad(dy, w, dtype=torch.float32):
    dy, w = dy.to(dtype), w.to(dtype)
    N, K, H, W = dy.shape
    C = w.shape[1]
    acc = torch.zeros(N, C, H, W, dtype=dtype, device=dy.device)
    sh = [[_shifted(dy, 2 - ty, 2 - tx) for tx in range(3)] for ty in range(3)]
    for k in range(K):
        for ty in range(3):
            for tx in range(3):
                acc = acc + sh[ty][tx][:, k].reshape(N, 1, H, W) * w[k, :, ty, tx].reshape(1, C, 1, 1)
    return acc


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(N, C, K, n):
    """x, w, b, dy of the transposed convolution on the CPU in float32: seeded randn, the weights scaled by (2 / (4 C))^0.5, a bias of order 1
    that is nowhere near zero (a dropped or doubled bias shows in every channel).  Computed once per shape; the tests only read them."""
    g = torch.Generator().manual_seed(1000 * C + 10 * K + N + 7 * n[0] * n[1])
    x = torch.randn(N, C, *n, generator=g)
    w = torch.randn(C, K, 2, 2, generator=g) * (2.0 / (4 * C)) ** 0.5
    b = (1.0 + 0.25 * torch.randn(K, generator=g)) * (1.0 - 2.0 * (torch.arange(K) % 2))
    dy = torch.randn(N, K, 2 * n[0], 2 * n[1], generator=g)
    return x, w, b, dy


# ---- the cases of tests/test_gpu_convt2d.py: the smallest shapes that reach each branch of csrc/convt2d.hip's dispatch (the branch is named per
# case; the conditions are restated in the test beside the calls).  The matrix-core forward walks tiles of 32 pixels, 4 per workgroup: (5, 13) =
# 65 pixels is one workgroup with a ragged third tile (and, at N = 2, a second ragged workgroup whose tiles belong to the second sample), (1, 3)
# one tile of 3 valid lanes.  Its grid is not capped (one tile per wave, no sweep loop), so there is no second-sweep case.  The VALU kernels walk
# blocks of 256 pixels: (20, 13) = 260 is a second, ragged block.
P65, P3, P260 = (5, 13), (1, 3), (20, 13)
DIRECT, NO_WS = 'force-direct', 'no-workspace'
UNET_PAIRS = [(512, 256), (256, 128), (128, 64)]   # t_conv3 / t_conv2 / t_conv1 of the two U-Nets (networks.py:500,503,566-572)

# (N, C, K, n, mode, branch); mode: None = the default dispatch, DIRECT = under nc_set_force_direct(1)
FWD_CASES = (
    # k_convT2d_fwd_mfma: K % 32 == 0, C % 16 == 0, C >= 128, not forced direct
    [(N, C, K, n, None, 'mfma') for (C, K) in UNET_PAIRS for n in (P65, P3) for N in (1, 2)] +
    [(1, 144, 32, P65, None, 'mfma'),           # C / 2 = 72 k-steps: 9 groups of 8, none of the U-Nets' counts
     # k_convT2d_fwd<4>: K % 4 == 0 and not the matrix-core shape, or forced direct
     (2, 128, 64, P260, DIRECT, 'fwd<4>'),
     (2, 128, 48, P260, None, 'fwd<4>'),        # K % 32 != 0
     (2, 136, 32, P260, None, 'fwd<4>'),        # C % 16 != 0
     (2, 64, 32, P260, None, 'fwd<4>'),         # C < 128
     # k_convT2d_fwd<2>: K % 4 != 0, K % 2 == 0;  <1>: K odd
     (2, 10, 6, P260, None, 'fwd<2>'),
     (2, 3, 5, P260, None, 'fwd<1>'),
     (1, 3, 1, P3, None, 'fwd<1>')])

# (N, C, K, n, mode, branch); NO_WS: ws = NULL, ws_bytes = 0
DGRAD_CASES = (
    # the gather GEMM: C >= 64, not forced direct, and the workspace covers the GEMM's split reduction
    [(2, C, K, P65, None, 'gemm') for (C, K) in UNET_PAIRS] +
    [(2, 128, 64, P260, None, 'gemm'),
     # k_convT2d_dgrad<8> at C >= 64: forced direct, or no workspace where the GEMM needs one
     (2, 128, 64, P260, DIRECT, 'dgrad<8>'),
     (2, 512, 256, P65, DIRECT, 'dgrad<8>'),
     (2, 128, 64, P260, NO_WS, 'dgrad<8>'),
     (2, 512, 256, P65, NO_WS, 'dgrad<8>'),
     # C < 64: always the VALU kernels
     (2, 16, 8, P260, None, 'dgrad<8>'),
     (2, 12, 6, P260, None, 'dgrad<4>'),
     (2, 10, 6, P260, None, 'dgrad<1>'),
     (2, 3, 5, P260, None, 'dgrad<1>')])

# (N, C, K, n, mode, branch).  The GEMM is taken whenever a sufficient workspace is passed and gemm_wgrad_supported holds: C >= 16, or a reduction
# N * H * W >= 256 (conv_gemm.hip padded_ok) -- so at 260 pixels even C = 10 and C = 3 go to the GEMM by default, with padded rows.
WGRAD_CASES = (
    [(2, C, K, P65, None, 'gemm') for (C, K) in UNET_PAIRS] +
    [(2, 128, 64, P260, None, 'gemm'),
     (2, 128, 64, P260, DIRECT, 'wgrad<4,4>'),
     (2, 512, 256, P65, DIRECT, 'wgrad<4,4>'),
     (2, 128, 64, P260, NO_WS, 'wgrad<4,4>'),
     (2, 512, 256, P65, NO_WS, 'wgrad<4,4>'),
     (2, 10, 6, P260, None, 'gemm, 10 rows'),
     (2, 10, 6, P260, DIRECT, 'wgrad<1,1>'),
     (1, 12, 8, (15, 13), None, 'wgrad<4,4>'),  # 195 pixels < 256 and C < 16: the default dispatch leaves the GEMM
     (2, 3, 5, P260, None, 'gemm, 3 rows'),
     (2, 3, 5, P260, DIRECT, 'wgrad<1,1>'),
     (1, 3, 5, (15, 13), None, 'wgrad<1,1>')])


# ---- Conv2d(k 3, s 1, p 1): inputs and the cases of tests/test_gpu_conv2d_k3.py -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs3(N, C, K, H, W):
    """x, w, b, dy of the 3 x 3 convolution on the CPU in float32: seeded randn, the weights scaled by (2 / (9 C))^0.5, a bias of order 1."""
    g = torch.Generator().manual_seed(100000 * N + 1000 * C + 10 * K + H * W)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = (1.0 + 0.25 * torch.randn(K, generator=g)) * (1.0 - 2.0 * (torch.arange(K) % 2))
    dy = torch.randn(N, K, H, W, generator=g)
    return x, w, b, dy


# csrc/conv2d_k3.hip takes a layer when the reduction side (C forward, K backward) is even and >= 16, the output side (K forward, C backward) a
# multiple of 64, and the smallest tile -- 4 rows x 32 columns x 64 output channels -- gives at least 256 workgroups:
#     N * ceil(H / 4) * ceil(W / 32) * (output side / 64) >= 256.
# The launcher's two tiles are 8 x 32 (taken when IT gives >= 512 workgroups) and 4 x 32 pixels; a tile never spans two images (at N = 2 the second
# image starts a new tile).  These are the smallest shapes that reach it.
def k3_covered(what, N, C, K, H, W):
    red, out = (C, K) if what == 0 else (K, C)
    return red % 2 == 0 and red >= 16 and out % 64 == 0 and N * -(-H // 4) * -(-W // 32) * (out // 64) >= 256


def k3_auto_cfg(what, N, C, K, H, W):
    out = K if what == 0 else C
    return 0 if N * -(-H // 8) * -(-W // 32) * (out // 64) >= 512 else 1


# (N, C, K, H, W, note)
K3_CASES = [
    (2, 64, 64, 130, 131, 'N = 2; W = 131 is no multiple of 4 nor of the 32-column window, H = 130 none of the tile rows'),
    (1, 256, 128, 131, 97, 'bottom-to-expanding widths; 33 tile rows x 4 windows'),
    (1, 128, 64, 130, 250, 'the concat layer'),
    (1, 16, 64, 132, 256, 'the shortest reduction; W = 256: the last window ends on the image edge.  Backward: C = 16 is no multiple of 64'),
    (2, 18, 64, 130, 131, 'C = 18: chunks of 2 channels'),
    (8, 64, 64, 5, 517, 'a 5 x 517 strip: H below the 8-row tile, a ragged second row of the 4-row tile, 17 windows'),
    (16, 64, 64, 3, 517, 'H = 3: below one tile\'s rows for both tiles'),
    (4, 16, 256, 67, 97, 'forward gives the 8 x 32 tile 576 workgroups: the launcher picks it'),
]
# shapes outside the coverage: they report 0 and still compute (on the gather GEMM)
K3_OUTSIDE = [
    (1, 64, 64, 20, 20, 'too few tiles'),
    (1, 1, 64, 130, 131, 'the one-channel first layer'),
    (2, 64, 96, 130, 131, 'K = 96: no multiple of 64 (forward); backward K = 96 is an even reduction side: covered'),
    (2, 17, 64, 130, 131, 'an odd reduction side (forward)'),
]


def case_id(c):
    return '-'.join('x'.join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c if v is not None).replace(' ', '')
