"""Reference, yardstick and cases of the op-level ConvTranspose3d(kernel 2, stride 2) tests (tests/test_gpu_convt.py; checked on the CPU by
tests/test_convt_reference.py).  Nothing here calls the library.

REFERENCE: the definition in the header comment of csrc/convt.hip as a float64 einsum (on whatever device the operands live):
    y[n,k,2z+a,2y+b,2x+c] = bias[k] + sum_ci x[n,ci,z,y,x] w[ci,k,a,b,c]
    dx = sum_(k,abc) dy w        dw = sum_(n,pos) x dy        db = sum dy
YARDSTICK ("fp32 oracle", as in tests/test_gpu_grad_fp64.py): torch's float32 F.conv_transpose3d and autograd on the CPU -- the reference
project's arithmetic -- measured against the same float64 reference.
ERROR MEASURE: maximum and rms of the error, each divided by the rms of the reference tensor (tests/test_gpu_convt_split.py's).
LIMIT: rms <= 3 rms_oracle + 2^-23 and max <= 3 max_oracle + 2^-21.  Factor 3: the summation order differs (the matrix-core kernels sum in
blocks, the GEMM weight gradient splits its reduction, the oracle sums serially).  The floors are one and four ulps of an fp32 store; they
only matter where the sum is so short that the oracle is nearly exact."""
import functools

import torch
import torch.nn.functional as F

FACTOR = 3.0
RMS_FLOOR = 2.0 ** -23
MAX_FLOOR = 2.0 ** -21
# the limits the project already had for the split-operand (three-term) forward (tests/test_gpu_convt_split.py)
SPLIT_RMS, SPLIT_MAX, SPLIT_FACTOR, SPLIT_FLOOR = 3e-7, 3e-6, 1.5, 5e-8


def ref_fwd(x, w, b=None):
    N, C, D, H, W = x.shape
    K = w.shape[1]
    y = torch.einsum('nczyx,ckabd->nkzaybxd', x.double(), w.double()).reshape(N, K, 2 * D, 2 * H, 2 * W)
    return y if b is None else y + b.double().view(1, K, 1, 1, 1)


def _taps(dy):
    N, K, D2, H2, W2 = dy.shape
    return dy.double().reshape(N, K, D2 // 2, 2, H2 // 2, 2, W2 // 2, 2)


def ref_dgrad(dy, w):
    return torch.einsum('nkzaybxd,ckabd->nczyx', _taps(dy), w.double())


def ref_wgrad(x, dy):
    return torch.einsum('nczyx,nkzaybxd->ckabd', x.double(), _taps(dy))


def ref_dbias(dy):
    return dy.double().sum((0, 2, 3, 4))


def err(t, ref):
    """(max, rms) of t - ref, each over the rms of ref; t and ref on any devices (compared where ref lives)."""
    e = t.to(ref.device).double().reshape(ref.shape) - ref
    s = ref.pow(2).mean().sqrt().item()
    return e.abs().max().item() / s, e.pow(2).mean().sqrt().item() / s


def within(got, oracle):
    """got, oracle: (max, rms) pairs from err()."""
    return got[1] <= FACTOR * oracle[1] + RMS_FLOOR and got[0] <= FACTOR * oracle[0] + MAX_FLOOR


def ratios(got, oracle):
    """How much of the limit a result uses: (max, rms), each 1.0 at the limit."""
    return got[0] / (FACTOR * oracle[0] + MAX_FLOOR), got[1] / (FACTOR * oracle[1] + RMS_FLOOR)


@functools.lru_cache(maxsize=None)
def inputs(N, C, K, n):
    """x, w, b, dy on the CPU in float32: seeded randn, the weights scaled by (2 / (8 C))^0.5, a bias of order 1 that is nowhere near zero (a
    dropped or doubled bias shows in every channel).  Computed once per shape; the tests only read them."""
    g = torch.Generator().manual_seed(1000 * C + 10 * K + N + n[0] * n[1] * n[2])
    x = torch.randn(N, C, *n, generator=g)
    w = torch.randn(C, K, 2, 2, 2, generator=g) * (2.0 / (8 * C)) ** 0.5
    b = (1.0 + 0.25 * torch.randn(K, generator=g)) * (1.0 - 2.0 * (torch.arange(K) % 2))
    dy = torch.randn(N, K, 2 * n[0], 2 * n[1], 2 * n[2], generator=g) if N * K * 8 * n[0] * n[1] * n[2] <= 1 << 24 else None
    return x, w, b, dy


@functools.lru_cache(maxsize=2)
def oracle_fwd(N, C, K, n, with_bias):
    x, w, b, _ = inputs(N, C, K, n)
    return F.conv_transpose3d(x, w, b if with_bias else None, stride=2)


@functools.lru_cache(maxsize=None)
def oracle_bwd(N, C, K, n):
    """dx, dw, db of the fp32 oracle for the gradient dy at its output."""
    x, w, b, dy = inputs(N, C, K, n)
    x, w, b = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    return tuple(t.detach() for t in torch.autograd.grad(F.conv_transpose3d(x, w, b, stride=2), (x, w, b), dy))


# ---- the cases: the smallest shapes that reach each branch of csrc/convt.hip's dispatch (the branch is named per case; the conditions are
# restated in tests/test_gpu_convt.py beside the calls).  S = 260 = (4, 5, 13): a second, ragged block of the 256-position grids.
P260 = (4, 5, 13)
DIRECT, NO_WS = 'force-direct', 'no-workspace'

# (N, C, K, n, mode, branch); mode: None = the default dispatch, DIRECT = under nc_set_force_direct(1)
FWD_CASES = [
    # k_convT_fwd_mfma: C == 128, K % 32 == 0, not forced direct.  Tiles of 32 positions, 4 per workgroup and sweep.
    (1, 128, 32, (1, 2, 3), None, 'mfma'),      # S = 6 < 32: one tile, mostly invalid lanes
    (2, 128, 128, (1, 2, 3), None, 'mfma'),     # the same, a second sample
    (1, 128, 64, (3, 5, 7), None, 'mfma'),      # S = 105, S % 32 != 0
    (2, 128, 32, (3, 5, 7), None, 'mfma'),      # N = 2, S % 32 != 0: the second sample's first tile starts at position 128 of the tile grid, 105 of x
    (2, 128, 96, (3, 5, 7), None, 'mfma'),
    (2, 128, 64, (2, 4, 4), None, 'mfma'),      # S = 32: whole tiles
    # the capped grid: 2 * cdiv(17391, 32) = 1088 tiles, cdiv(1088, 4) = 272 > cap cdiv(2048, 2 * 4) = 256 workgroups -> 1024 tiles per sweep, a
    # second sweep of 64 tiles taken by the first 16 workgroups only.  Output 142 MB; the fp64 reference is taken on the GPU.
    (2, 128, 128, (17, 31, 33), None, 'mfma-capped'),
    # k_convT_fwd<4>: K % 4 == 0 and not (C == 128 and K % 32 == 0), or forced direct
    (1, 256, 128, (3, 4, 5), None, 'fwd<4>'),   # the training layer (gen_nets.hip), one block of positions
    (2, 256, 128, P260, None, 'fwd<4>'),
    (2, 128, 48, P260, None, 'fwd<4>'),         # C == 128 but K % 32 != 0
    (2, 64, 32, P260, None, 'fwd<4>'),
    (2, 128, 64, P260, DIRECT, 'fwd<4>'),
    # k_convT_fwd<2>: K % 4 != 0, K % 2 == 0
    (2, 10, 6, P260, None, 'fwd<2>'),
    # k_convT_fwd<1>: K odd
    (2, 3, 5, P260, None, 'fwd<1>'),
    (2, 3, 1, P260, None, 'fwd<1>'),
]

# (N, C, K, n, mode, branch); NO_WS: ws = NULL, ws_bytes = 0
DGRAD_CASES = [
    # the gather GEMM: C >= 64, not forced direct, and the workspace covers the GEMM's split reduction
    (2, 128, 64, P260, None, 'gemm'),
    (2, 256, 128, P260, None, 'gemm'),
    # k_convT_dgrad<8> at C >= 64: forced direct, or no workspace where the GEMM needs one (it does at both shapes: its reduction is split)
    (2, 128, 64, P260, DIRECT, 'dgrad<8>'),
    (2, 256, 128, P260, DIRECT, 'dgrad<8>'),
    (2, 128, 64, P260, NO_WS, 'dgrad<8>'),
    (2, 256, 128, P260, NO_WS, 'dgrad<8>'),
    # C < 64: always the VALU kernels
    (2, 16, 8, P260, None, 'dgrad<8>'),
    (2, 12, 6, P260, None, 'dgrad<4>'),
    (2, 5, 3, P260, None, 'dgrad<1>'),
    (2, 1, 1, P260, None, 'dgrad<1>'),
]

# (N, C, K, n, mode, branch).  The GEMM is taken whenever a sufficient workspace is passed and gemm_wgrad_supported holds: C >= 16, or a
# reduction N * S >= 256 (conv_gemm.hip padded_ok) -- so at S = 260 even C = 12 and C = 5 go to the GEMM by default, with padded rows, and
# the VALU kernels are reached under force-direct, without a workspace, or by default at N * S < 256 (where no lane strides).
WGRAD_CASES = [
    (1, 128, 64, P260, None, 'gemm'),
    (2, 128, 64, P260, None, 'gemm'),
    (1, 256, 128, P260, None, 'gemm'),
    (2, 256, 128, P260, None, 'gemm'),
    (1, 128, 64, P260, DIRECT, 'wgrad<4,4>'),
    (2, 128, 64, P260, DIRECT, 'wgrad<4,4>'),
    (1, 256, 128, P260, DIRECT, 'wgrad<4,4>'),
    (2, 256, 128, P260, DIRECT, 'wgrad<4,4>'),
    (2, 12, 8, P260, None, 'gemm, 12 rows'),
    (2, 12, 8, P260, DIRECT, 'wgrad<4,4>'),
    (2, 12, 8, P260, NO_WS, 'wgrad<4,4>'),
    (1, 12, 8, (3, 5, 13), None, 'wgrad<4,4>'),  # S = 195 < 256 and C < 16: the default dispatch leaves the GEMM
    (2, 5, 6, P260, None, 'gemm, 5 rows'),
    (2, 5, 6, P260, DIRECT, 'wgrad<1,1>'),
    (2, 5, 6, P260, NO_WS, 'wgrad<1,1>'),
    (1, 5, 6, (3, 5, 13), None, 'wgrad<1,1>'),
]

# (N, C, K, n, QN): nc_convT_k2s2_fwd_split (csrc/convt_s3.hip k_convT_s3<QN, 3>).  QN = 8 while (C / 32) * 8 * 3 KiB <= 128 KiB, i.e. C <= 160.
# Tiles of 512 positions: S = 585 = (5, 9, 13) gives a whole and a ragged tile per sample, the ragged one with empty waves.
P585 = (5, 9, 13)
SPLIT_CASES = [
    (2, 32, 16, P585, 8),
    (2, 96, 48, P585, 8),
    (2, 160, 16, P585, 8),
    (2, 192, 48, P585, 4),
    (2, 224, 16, P585, 4),
    # more tiles than slots: C = 128 -> QN = 8, ngroups = K / 16 = 4, per_xcd = 32 / 4 = 8, grid 8 * 4 * 8 = 256 workgroups = 64 tile slots;
    # S = 33759 -> cdiv(S, 512) = 66 tiles: slots 0 and 1 take a second tile, the last one ragged
    (1, 128, 64, (33, 33, 31), 8),
]

# nc_convT_k2s2_fwd_s3_debug (csrc/convt.hip convT_fwd_s3: the matrix-core kernel's own three-term output)
S3_CASES = [(2, 128, 32, (3, 5, 7)), (2, 128, 64, (3, 5, 7))]


def case_id(c):
    return '-'.join('x'.join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c if v is not None).replace(' ', '')
