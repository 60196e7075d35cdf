"""Every WRITER of the two-term fp16 operand form ("H2": csrc/s3_common.hpp, csrc/h2.hip), operator by operator, against fp64.

An H2 tensor holds two fp16 terms of t * 2^k per element, k from one cell per tensor (per half of a concatenation): [N][C/8][2][S] 16-byte
units, the cells nc_h2_cells_offset(N * C * S) bytes behind the start.  The consumers (the convolutions) have tests/test_gpu_h2.py; here the
tensors themselves are DECODED on the host and held to the

REPRESENTATION CRITERION (R), element by element against the fp32 value t the writer split:
  * every term is finite;
  * max|t| * 2^k < 2^15;
  * |decoded - t| <= max(2^-22 |t|, 2^-25 * 2^-k)
(two round-to-nearest fp16 roundings, 11 significant bits each; a second term below fp16's normal range is rounded to a multiple of 2^-24,
i.e. to 2^-25 absolute -- s3_common.hpp's statement of the form, no margin added).  Where a writer also stores the fp32 tensor, t is that
tensor bit for bit.

The writers are reached through the debug exports of csrc/h2_debug.hip, which forward to the internal functions unchanged:
  nc_to_h2_debug                      h2_zero_cells + h2_absmax | h2_set_cell, split2h_into          (k_absmax, k_split2h)
  nc_act_split2h_debug                act_split2h                                                     (k_act_split2h)
  nc_act_split2h_pool_debug           act_split2h_pool                                                (k_act_split2h_pool)
  nc_maxpool2_h2_debug                maxpool2_h2                                                     (k_maxpool2_h2)
  nc_h2_to_s3_if_debug                h2_to_s3_if                                                     (k_h2_to_s3_if)
  nc_instnorm_act_bwd_dbias_h2_debug  instnorm_act_bwd_dbias_h2 | _rank1                              (k_in_bwd_*_h2<false | true>)
  nc_convT_k2s2_fwd_split_h2_debug    convT_h2_bound + convT_fwd_split_h2                             (k_convT_bound, k_convT_s3<QN, 2>)
"""
import ctypes
import functools
import math
import os
import struct
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENT = 0xA5           # sentinel byte of every output buffer (0xA5A5 is a finite fp16 / bf16)
GUARD_LOW, GUARD_ALL, GUARD_FLAG = 0, 1, 2   # common.hpp kGuardLow / kGuardAll / kGuardFlag
GUARD_DROP = 17 << 23                        # common.hpp kGuardDrop: float bits, 2^-17 below the cell
SPLIT2H_GRID_CAP = 4096                      # h2.hip split2h_into: with a guard, at most this many workgroups (gridDim.x * gridDim.y)


def L():
    from neuroclear_amd._lib import lib
    return lib()


@pytest.fixture(autouse=True)
def _restore():
    gd = L().nc_get_h2_guard()
    yield
    L().nc_set_h2_guard(gd)


def ck(code, what):
    from neuroclear_amd._lib import check
    check(code, what)


def P(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset) if t is not None else ctypes.c_void_p(0)


def I(v):
    return ctypes.c_int(v)


def LG(v):
    return ctypes.c_long(v)


def FL(v):
    return ctypes.c_float(v)


def Z(v):
    return ctypes.c_size_t(v)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32_bits(v):
    return struct.unpack('<I', struct.pack('<f', v))[0]


def h2_exp(bits):
    """s3_common.hpp h2_exp: the power of two of a cell (float bits of a magnitude that bounds the tensor)."""
    e = (bits >> 23) & 0x1FF
    k = 14 - (e - 127) if e else 0
    return min(k, 126)


def h2_alloc(N, ctot, S, capacity=None):
    """A sentinel-filled buffer for an H2 tensor (capacity: more bytes, the norm backward's S3 capacity) and the byte offset of its cells."""
    off = L().nc_h2_cells_offset(Z(N * ctot * S))
    nb = L().nc_h2_bytes(I(N), I(ctot), LG(S))
    assert off == (N * ctot * S * 4 + 255) // 256 * 256 and nb == off + 256
    buf = torch.full((max(nb, capacity or 0),), SENT, dtype=torch.uint8, device=DEV)
    return buf, off


def cells_of(buf, off):
    torch.cuda.synchronize()
    return [int(v) & 0xFFFFFFFF for v in buf[off:off + 256].view(torch.int32).tolist()]


def h2_terms(buf, N, ctot, S):
    """The raw terms as [N][ctot][S] fp16 tensors (a0, a1)."""
    t = buf[:N * ctot * S * 4].view(torch.float16).view(N, ctot // 8, 2, S, 8)
    a0 = t[:, :, 0].permute(0, 1, 3, 2).reshape(N, ctot, S)
    a1 = t[:, :, 1].permute(0, 1, 3, 2).reshape(N, ctot, S)
    return a0, a1


def h2_decode(buf, N, ctot, S, k):
    """THE decoder: (a0 + a1) * 2^-k in fp64 as [N][ctot][S], and the raw terms.  k: one int, or one per channel (a tensor converted in two halves)."""
    a0, a1 = h2_terms(buf, N, ctot, S)
    if isinstance(k, int):
        inv = 2.0 ** -k
    else:
        inv = torch.tensor([2.0 ** -kk for kk in k], dtype=torch.float64, device=DEV).view(1, ctot, 1)
    return (a0.double() + a1.double()) * inv, a0, a1


def block_bytes(buf, N, ctot, S, c_lo, c_hi):
    """The bytes of channels [c_lo, c_hi) of every sample."""
    return buf[:N * ctot * S * 4].view(N, ctot // 8, 2 * S * 16)[:, c_lo // 8:c_hi // 8]


def assert_R(dec, a0, a1, t, k, what, keep=None):
    """Criterion R (module docstring).  keep: a mask of the elements it applies to (non-finite inputs have a rule of their own)."""
    td = t.double()
    if keep is not None:
        dec, a0, a1, td = dec[keep], a0[keep], a1[keep], td[keep]
    assert bool(torch.isfinite(a0).all()) and bool(torch.isfinite(a1).all()), what
    top = float(td.abs().max()) if td.numel() else 0.0
    assert top * 2.0 ** k < 2.0 ** 15, (what, top, k)
    lim = torch.maximum(td.abs() * 2.0 ** -22, torch.full_like(td, 2.0 ** -25 * 2.0 ** -k))
    ratio = ((dec - td).abs() / lim)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print('%s: k %d, worst |decoded - t| / limit %.3f' % (what, k, worst))
    assert bool(((dec - td).abs() <= lim).all()), (what, worst)


def err(a, r):
    s = r.pow(2).mean().sqrt().item()
    e = a.double() - r
    return e.abs().max().item() / s, e.pow(2).mean().sqrt().item() / s


# ---------------------------------------------------------------------------------------------------------------------------------------------
# nc_to_h2_debug: k_absmax + k_split2h
# ---------------------------------------------------------------------------------------------------------------------------------------------
def to_h2(x, N, C, S, xstride, ctot, c0, bound=0.0, guard=False, cell_index=0):
    buf, off = h2_alloc(N, ctot, S)
    g = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) if guard else None
    ck(L().nc_to_h2_debug(P(x), LG(xstride), P(buf), I(N), I(C), LG(S), I(ctot), I(c0), P(buf, off + 4 * cell_index), FL(bound), P(g), stream()),
       'nc_to_h2_debug')
    torch.cuda.synchronize()
    return buf, off, ([int(v) & 0xFFFFFFFF for v in g.tolist()] if guard else None)


def strided_input(N, C, S, xstride, g, fill=1.0e30):
    """[N][C][S] values inside a buffer whose samples are xstride floats apart; the gaps hold a magnitude that would wreck a cell that read them."""
    flat = torch.full((N * xstride,), fill, device=DEV)
    x = torch.randn(N, C, S, device=DEV, generator=g) * torch.exp2(torch.empty(N, C, S, device=DEV).uniform_(-30.0, 1.0, generator=g))
    for n in range(N):
        flat[n * xstride:n * xstride + C * S] = x[n].reshape(-1)
    return flat, x


def finite_max_bits(x):
    b = x.abs().view(torch.int32)
    return int(torch.where(b < 0x7F800000, b, torch.zeros_like(b)).max())


@pytest.mark.parametrize('S', [1, 63, 64, 65, 257, 4099])
def test_split2h_meets_the_representation_criterion(S):
    """N = 2 with the samples further apart than C * S (and the second one only 4-byte aligned), C = 8 written as channels [8, 16) of a 24-channel
    tensor: criterion R, the other two channel blocks and the other cells keep the sentinel, the measured cell is the float bits of the largest
    finite |x| (which sits in the LAST element of the second sample: the ragged tail of both kernels), and a cell given as a bound."""
    N, C, ctot, c0 = 2, 8, 24, 8
    xstride = C * S + 5
    g = torch.Generator(device=DEV).manual_seed(100 + S)
    flat, x = strided_input(N, C, S, xstride, g)
    x[1, C - 1, S - 1] = -13.25
    x[0, 0, 0] = 0.0
    flat[xstride + C * S - 1] = -13.25
    flat[0] = 0.0
    buf, off, _ = to_h2(flat, N, C, S, xstride, ctot, c0)
    cells = cells_of(buf, off)
    assert cells[0] == f32_bits(13.25) == finite_max_bits(x)
    assert all(c == 0xA5A5A5A5 for c in cells[1:])
    k = h2_exp(cells[0])
    dec, a0, a1 = h2_decode(buf, N, ctot, S, k)
    assert_R(dec[:, c0:c0 + C], a0[:, c0:c0 + C], a1[:, c0:c0 + C], x, k, 'split2h S=%d measured' % S)
    assert bool((block_bytes(buf, N, ctot, S, 0, c0) == SENT).all()) and bool((block_bytes(buf, N, ctot, S, c0 + C, ctot) == SENT).all())
    # the cell as a bound the caller knows (h2_set_cell): 100 > 13.25, three bits of head-room given away, the same criterion
    buf2, off2, _ = to_h2(flat, N, C, S, xstride, ctot, c0, bound=100.0)
    assert cells_of(buf2, off2)[0] == f32_bits(100.0)
    k2 = h2_exp(f32_bits(100.0))
    assert k2 == k - 3
    dec2, b0, b1 = h2_decode(buf2, N, ctot, S, k2)
    assert_R(dec2[:, c0:c0 + C], b0[:, c0:c0 + C], b1[:, c0:c0 + C], x, k2, 'split2h S=%d bound' % S)
    assert bool((block_bytes(buf2, N, ctot, S, 0, c0) == SENT).all()) and bool((block_bytes(buf2, N, ctot, S, c0 + C, ctot) == SENT).all())


def test_split2h_of_zeros_and_of_non_finite_elements():
    """An all-zero tensor: cell 0, k = 0, all-zero bytes.  One +inf, one -inf and one NaN element: a0 = the element, a1 = NaN (s3_common.hpp: every
    output they touch becomes NaN), they are left out of the cell, and every other element meets criterion R."""
    N, C, S = 2, 16, 300
    z = torch.zeros(N, C, S, device=DEV)
    buf, off, _ = to_h2(z, N, C, S, C * S, C, 0)
    assert cells_of(buf, off)[0] == 0 and h2_exp(0) == 0
    assert int(buf[:N * C * S * 4].max()) == 0
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(N, C, S, device=DEV, generator=g)
    x[0, 3, 17] = float('inf')
    x[1, 9, 299] = float('-inf')
    x[1, 15, 256] = float('nan')
    buf, off, _ = to_h2(x, N, C, S, C * S, C, 0)
    cell = cells_of(buf, off)[0]
    assert cell == finite_max_bits(x) and cell < 0x7F800000
    k = h2_exp(cell)
    dec, a0, a1 = h2_decode(buf, N, C, S, k)
    assert float(a0[0, 3, 17]) == float('inf') and float(a0[1, 9, 299]) == float('-inf') and bool(torch.isnan(a0[1, 15, 256]))
    assert bool(torch.isnan(a1[0, 3, 17])) and bool(torch.isnan(a1[1, 9, 299])) and bool(torch.isnan(a1[1, 15, 256]))
    assert_R(dec, a0, a1, x, k, 'split2h beside non-finite elements', keep=torch.isfinite(x))


def guard_counts(x, cell_bits):
    """The range guard's counts in Python.  A chunk = a wave's 64 voxels x 8 channels of a 256-voxel tile, i.e. voxels [64 j, 64 j + 64) of one
    8-channel block; `all` = chunks with a finite non-zero element, `low` = those whose largest finite magnitude has float bits below
    cell bits - kGuardDrop (integer comparison, as the kernel's)."""
    N, C, S = x.shape
    b = x.abs().view(torch.int32)
    b = torch.where(b < 0x7F800000, b, torch.zeros_like(b))
    pad = (-S) % 64
    b = torch.nn.functional.pad(b, (0, pad))
    m = b.view(N, C // 8, 8, (S + pad) // 64, 64).amax(dim=(2, 4))
    thr = cell_bits - GUARD_DROP if cell_bits > GUARD_DROP else 0
    return int(((m > 0) & (m < thr)).sum()), int((m > 0).sum())


def test_split2h_guard_counts():
    """guard[kGuardLow] / [kGuardAll] against the Python count: one dark half (2^-21 of the rest; the chunk that straddles the border is not low),
    a few isolated all-zero chunks, a chunk whose only non-zero element is a NaN's neighbour, the ragged last chunk."""
    N, C, S = 2, 16, 4099
    L().nc_set_h2_guard(1)
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(N, C, S, device=DEV, generator=g)
    x[:, :, :S // 2] *= 2.0 ** -21
    x[0, 0:8, 128:192] = 0.0
    x[1, 8:16, 64 * 40:64 * 41] = 0.0
    x[1, 0:8, 4096:] = 0.0          # the ragged chunk of one block: all zero
    x[0, 8:16, 64 * 50:64 * 51] = 0.0
    x[0, 9, 64 * 50 + 5] = float('nan')   # a chunk with nothing finite but zeros: not counted at all
    buf, off, gw = to_h2(x, N, C, S, C * S, C, 0, guard=True)
    cell = cells_of(buf, off)[0]
    low, al = guard_counts(x, cell)
    print('guard counts: low %d all %d (kernel %d %d)' % (low, al, gw[GUARD_LOW], gw[GUARD_ALL]))
    assert al == N * (C // 8) * 65 - 4 and 0 < low < al
    assert gw[GUARD_LOW] == low and gw[GUARD_ALL] == al
    assert all(v == 0 for v in gw[3:])   # (zeroed by the entry point, never written)


def test_split2h_beyond_the_grid_cap():
    """With a guard the launch has at most 4096 workgroups (split2h_into), each walking several 256-voxel tiles and adding its chunk counts once:
    S = 4096 * 256 + 77 voxels of one 8-channel block (33.6 MB of input, 33.6 MB of output -- the smallest tensor above the cap, whatever N and C)
    takes every workgroup through a second tile only for the first one: criterion R over the whole tensor, the ragged tail included, and the counts."""
    N, C = 1, 8
    S = SPLIT2H_GRID_CAP * 256 + 77
    L().nc_set_h2_guard(1)
    g = torch.Generator(device=DEV).manual_seed(12)
    x = torch.randn(N, C, S, device=DEV, generator=g)
    x[:, :, 256 * 1000:256 * 3000] *= 2.0 ** -21
    x[0, :, 64 * 7:64 * 9] = 0.0
    x[0, 5, S - 1] = 77.0
    buf, off, gw = to_h2(x, N, C, S, C * S, C, 0, guard=True)
    cell = cells_of(buf, off)[0]
    assert cell == f32_bits(77.0)
    k = h2_exp(cell)
    dec, a0, a1 = h2_decode(buf, N, C, S, k)
    assert_R(dec, a0, a1, x, k, 'split2h beyond the grid cap')
    low, al = guard_counts(x, cell)
    assert low > 0 and (gw[GUARD_LOW], gw[GUARD_ALL]) == (low, al), (gw, low, al)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# nc_act_split2h_debug, nc_act_split2h_pool_debug, nc_maxpool2_h2_debug
# ---------------------------------------------------------------------------------------------------------------------------------------------
def stats(x, NC, S):
    nb = max(int(L().nc_instnorm_ws_bytes(I(NC), LG(S))), 256)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    mean, rstd = torch.empty(NC, device=DEV), torch.empty(NC, device=DEV)
    ck(L().nc_instnorm_stats(P(x), I(NC), LG(S), FL(1e-5), P(mean), P(rstd), P(ws), Z(nb), stream()), 'nc_instnorm_stats')
    return mean, rstd


def act_ref(x, mean, rstd, slope):
    """(x - mean) * rstd and the activation in fp64 from the SAME fp32 statistics (slope as the fp32 number the kernel receives)."""
    N, C, S = x.shape
    xh = (x.double() - mean.double().view(N, C, 1)) * rstd.double().view(N, C, 1)
    sl = float(torch.tensor(slope, dtype=torch.float32))
    return torch.where(xh > 0, xh, xh * sl), xh > 0


def act_split2h(x, mean, rstd, slope, N, C, S, ctot, c0, want_y=True, cell_index=0):
    buf, off = h2_alloc(N, ctot, S)
    ystride = C * S + 3
    y = torch.full((N * ystride,), float('nan'), device=DEV) if want_y else None
    bound = math.sqrt(S)
    ck(L().nc_act_split2h_debug(P(x), P(mean), P(rstd), FL(slope), P(y), LG(ystride), P(buf), I(N), I(C), LG(S), I(ctot), I(c0), FL(bound),
                                P(buf, off + 4 * cell_index), P(buf, off + 4 * (1 - cell_index)), stream()), 'nc_act_split2h_debug')
    torch.cuda.synchronize()
    return buf, off, y, ystride


def check_act(x, slope, what):
    N, C, S = x.shape
    ctot, c0 = C + 8, 8
    mean, rstd = stats(x, N * C, S)
    ref, pos = act_ref(x, mean, rstd, slope)
    buf, off, yflat, ystride = act_split2h(x, mean, rstd, slope, N, C, S, ctot, c0)
    y = torch.stack([yflat[n * ystride:n * ystride + C * S].view(C, S) for n in range(N)])
    gaps = torch.stack([yflat[n * ystride + C * S:(n + 1) * ystride] for n in range(N)])
    assert bool(torch.isnan(gaps).all())                                        # nothing written between the samples
    d = (y.double() - ref).abs()
    worst = float((d / (ref.abs() * 2.0 ** -22).clamp_min(1e-300)).max())
    print('%s: worst |y - fp64| / (2^-22 |fp64|) %.3f' % (what, worst))
    assert bool((d <= ref.abs() * 2.0 ** -22).all()), worst                    # three fp32 roundings at most: subtract, scale, slope
    assert torch.equal(y > 0, pos)                                              # the ReLU mask is exact
    if slope == 0.0:
        assert bool((y[~pos] == 0).all())
    cells = cells_of(buf, off)
    bits = f32_bits(math.sqrt(S))
    assert cells[0] == bits and cells[1] == bits and all(c == 0xA5A5A5A5 for c in cells[2:])
    k = h2_exp(bits)
    dec, a0, a1 = h2_decode(buf, N, ctot, S, k)
    assert_R(dec[:, c0:], a0[:, c0:], a1[:, c0:], y, k, what)
    assert bool((block_bytes(buf, N, ctot, S, 0, c0) == SENT).all())
    buf2, _, _, _ = act_split2h(x, mean, rstd, slope, N, C, S, ctot, c0, want_y=False)
    assert torch.equal(buf, buf2)                                               # y = NULL: the same H2 bytes
    return y


@pytest.mark.parametrize('slope', [0.0, 0.2])
@pytest.mark.parametrize('N,C,S', [(1, 64, 4096), (2, 16, 2500), (3, 8, 65)])
def test_act_split2h_against_fp64(N, C, S, slope):
    g = torch.Generator(device=DEV).manual_seed(N * 1000 + S)
    x = torch.randn(N, C, S, device=DEV, generator=g) * 2 + 0.5
    check_act(x, slope, 'act_split2h %s slope %g' % ((N, C, S), slope))


@pytest.mark.parametrize('N,C,S', [(1, 64, 4096), (2, 16, 2500)])
def test_act_split2h_input_at_the_bound(N, C, S):
    """|InstanceNorm output| <= sqrt(S - 1) < the bound sqrt(S) the cell is set from, reached by ONE spike in an otherwise constant instance: the
    element stays finite in fp16 and everything meets criterion R (the constant voxels sit at -1 / sqrt(S - 1), 2^-11 of the spike)."""
    g = torch.Generator(device=DEV).manual_seed(S)
    x = torch.randn(N, C, S, device=DEV, generator=g) * 2 + 0.5
    x[N - 1, 3] = 0.25
    x[N - 1, 3, S - 1] = 1000.25
    x[0, 8] = -3.0
    x[0, 8, 100] = -2003.0      # a negative spike: the instance's other voxels are the positive ones
    y = check_act(x, 0.2, 'act_split2h at the bound %s' % ((N, C, S),))
    top = float(y[N - 1, 3, S - 1])
    print('spike: %.4f of sqrt(S - 1) = %.4f' % (top, math.sqrt(S - 1)))
    assert 0.999 * math.sqrt(S - 1) <= top <= math.sqrt(S)
    assert float(y.abs().max()) == top


def first_max_units(a0, a1, D, H, W):
    """MaxPool3d(2) on the terms [N][C][S]: per window the terms of the FIRST maximum of a0 + a1 in scan order (z, y, x)."""
    N, C = a0.shape[:2]
    def win(t):
        return t.view(N, C, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(N, C, D // 2, H // 2, W // 2, 8)
    w0, w1 = win(a0), win(a1)
    val = w0.double() + w1.double()
    top = val.amax(dim=-1, keepdim=True)
    pos = torch.arange(8, device=DEV).view(1, 1, 1, 1, 1, 8).expand_as(val)
    first = torch.where(val == top, pos, torch.full_like(pos, 8)).amin(dim=-1, keepdim=True)
    So = (D // 2) * (H // 2) * (W // 2)
    return torch.gather(w0, -1, first).reshape(N, C, So), torch.gather(w1, -1, first).reshape(N, C, So), first


@pytest.mark.parametrize('C', [8, 16])
@pytest.mark.parametrize('D,H,W', [(2, 2, 2), (4, 6, 10), (6, 4, 34)])
def test_act_split2h_pool_and_maxpool2_h2(D, H, W, C):
    """The fused normalise + convert + pool pass and the pool on the H2 tensor: the full-resolution bytes (written as channels [C, 2C) of a
    2C-channel tensor) are nc_act_split2h_debug's; every pooled unit is byte-equal to the unit of the first maximum of a0 + a1 in scan order.
    Ties: windows of equal values, two equal maxima in one window, and the zeros (+0 and -0 first terms) behind a ReLU.  The pooled tensor is
    DENSE by the functions' contract; it lies in the middle of a larger sentinel buffer, and maxpool2_h2 reads its input at channel offset C."""
    N, S = 2, D * H * W
    So = S // 8
    ctot, c0 = 2 * C, C
    g = torch.Generator(device=DEV).manual_seed(D * 100 + W + C)
    x = torch.randn(N, C, D, H, W, device=DEV, generator=g) * 2 + 0.5
    x[0, :, 0:2, 0:2, 0:2] = x[0, :, 0:1, 0:1, 0:1].clone()                # a window of equal values (the whole instance at 2 x 2 x 2)
    if W > 2:
        x[1, :, 0, 1, 3] = 9.0                                      # two equal maxima in one window: positions 3 and 6 of the scan
        x[1, :, 1, 1, 2] = 9.0
        x[1, 1, :, :, 4:6] = -5.0                                   # windows that are negative throughout
    x = x.reshape(N, C, S).contiguous()
    mean, rstd = stats(x, N * C, S)
    for slope in (0.0, 0.2):
        full, off, _, _ = act_split2h(x, mean, rstd, slope, N, C, S, ctot, c0, want_y=False, cell_index=1)
        pad = 4096
        nbp = N * C * So * 4
        outs = []
        for fused in (True, False):
            pooled = torch.full((pad + nbp + pad,), SENT, dtype=torch.uint8, device=DEV)
            if fused:
                buf, off2 = h2_alloc(N, ctot, S)
                ck(L().nc_act_split2h_pool_debug(P(x), P(mean), P(rstd), FL(slope), P(buf), P(pooled, pad), I(N), I(C), I(D), I(H), I(W), I(ctot),
                                                 I(c0), FL(math.sqrt(S)), P(buf, off2 + 4), stream()), 'nc_act_split2h_pool_debug')
                torch.cuda.synchronize()
                # the cell block: act_split2h was given both cells, the fused pass the second one only
                assert cells_of(buf, off2)[1] == f32_bits(math.sqrt(S)) and cells_of(buf, off2)[0] == 0xA5A5A5A5
                assert torch.equal(buf[:off], full[:off])            # the full-resolution tensor: the same bytes, the first half untouched
            else:
                ck(L().nc_maxpool2_h2_debug(P(full, (c0 // 8) * 2 * S * 16), P(pooled, pad), I(N), I(C), I(ctot), I(D), I(H), I(W), stream()),
                   'nc_maxpool2_h2_debug')
                torch.cuda.synchronize()
            assert bool((pooled[:pad] == SENT).all()) and bool((pooled[pad + nbp:] == SENT).all())
            outs.append(pooled[pad:pad + nbp].clone())
        assert bool((block_bytes(full, N, ctot, S, 0, c0) == SENT).all())
        a0, a1 = h2_terms(full, N, ctot, S)
        e0, e1, first = first_max_units(a0[:, c0:], a1[:, c0:], D, H, W)
        if slope == 0.0:
            assert int((first > 0).sum()) > 0 and bool(((a0[:, c0:] == 0) & (a0[:, c0:].view(torch.int16) < 0)).any())   # (-0 terms exist)
        for name, out in zip(('act_split2h_pool', 'maxpool2_h2'), outs):
            p0, p1 = h2_terms(out, N, C, So)
            assert torch.equal(p0.view(torch.int16), e0.view(torch.int16)), (name, slope)
            assert torch.equal(p1.view(torch.int16), e1.view(torch.int16)), (name, slope)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# nc_h2_to_s3_if_debug
# ---------------------------------------------------------------------------------------------------------------------------------------------
def from_s3(raw, N, C, S):
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    from test_gpu_convt_split import _from_s3
    return _from_s3(raw, N, C, S)


def convt_reference():
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import convt_reference as R
    return R


def test_h2_to_s3_if_is_exact_and_conditional():
    """An H2 tensor converted in two halves with different powers of two (cells [0] and [1]): with the flag set (or no guard words at all) the
    S3 output decodes to exactly the H2 decode; with the flag clear the output buffer keeps its sentinel."""
    N, C, S = 2, 32, 300
    g = torch.Generator(device=DEV).manual_seed(21)
    x = torch.randn(N, C, S, device=DEV, generator=g)
    x[:, C // 2:] *= 2.0 ** -9
    buf, off = h2_alloc(N, C, S)
    for half in (0, 1):
        xa = x[:, half * C // 2:(half + 1) * C // 2].contiguous()
        ck(L().nc_to_h2_debug(P(xa), LG(C // 2 * S), P(buf), I(N), I(C // 2), LG(S), I(C), I(half * C // 2), P(buf, off + 4 * half), FL(0.0),
                              P(None), stream()), 'nc_to_h2_debug')
    cells = cells_of(buf, off)
    ks = [h2_exp(cells[0])] * (C // 2) + [h2_exp(cells[1])] * (C // 2)
    assert ks[-1] >= ks[0] + 8
    dec, a0, a1 = h2_decode(buf, N, C, S, ks)
    for half in (0, 1):
        sl = slice(half * C // 2, (half + 1) * C // 2)
        assert_R(dec[:, sl], a0[:, sl], a1[:, sl], x[:, sl], ks[half * C // 2], 'h2_to_s3_if input half %d' % half)
    nb3 = int(L().nc_s3_bytes(I(N), I(C), LG(S)))
    for flag, guard in ((1, True), (0, True), (None, False)):
        out = torch.full((nb3,), SENT, dtype=torch.uint8, device=DEV)
        gw = torch.tensor([0, 0, flag or 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV) if guard else None
        ck(L().nc_h2_to_s3_if_debug(P(buf), P(out), I(N), I(C), LG(S), P(buf, off), P(gw), stream()), 'nc_h2_to_s3_if_debug')
        torch.cuda.synchronize()
        if flag == 0:
            assert bool((out == SENT).all())
        else:
            assert torch.equal(from_s3(out, N, C, S).double(), dec)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# nc_instnorm_act_bwd_dbias_h2_debug
# ---------------------------------------------------------------------------------------------------------------------------------------------
def in_bwd_fp64(x, dy, slope):
    """The autograd backward of the fp64 normalisation + activation (dy: the fp32 gradient at its output, as fp64)."""
    xd = x.double().requires_grad_(True)
    mean = xd.mean(2, keepdim=True)
    var = xd.var(2, unbiased=False, keepdim=True)
    y = torch.nn.functional.leaky_relu((xd - mean) / (var + 1e-5).sqrt(), float(torch.tensor(slope, dtype=torch.float32)))
    (gx,) = torch.autograd.grad((y * dy.double()).sum(), xd)
    return gx.detach()


def in_bwd_fp32(x, dy, mean, rstd, slope):
    N, C, S = x.shape
    nb = int(L().nc_instnorm_ws_bytes(I(N * C), LG(S)))
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=DEV)
    dx = torch.empty_like(x)
    ck(L().nc_instnorm_act_bwd(P(dy), P(x), P(mean), P(rstd), FL(slope), P(dx), I(N * C), LG(S), P(ws), Z(nb), stream()), 'nc_instnorm_act_bwd')
    return dx


def in_bwd_h2(x, dy, w1, mean, rstd, slope, guard=False):
    """-> the raw dxs buffer (S3 capacity), the byte offset of its cells, dbias, the guard words."""
    N, C, S = x.shape
    buf, off = h2_alloc(N, C, S, capacity=int(L().nc_s3_bytes(I(N), I(C), LG(S))))
    nb = int(L().nc_instnorm_bwd_dbias_ws_bytes(I(N * C), LG(S)))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    db = torch.full((C,), float('nan'), device=DEV)
    gw = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) if guard else None
    ck(L().nc_instnorm_act_bwd_dbias_h2_debug(P(dy), P(w1), P(x), P(mean), P(rstd), FL(slope), P(buf), P(db), I(N), I(C), LG(S), P(ws), Z(nb),
                                              P(gw), stream()), 'nc_instnorm_act_bwd_dbias_h2_debug')
    torch.cuda.synchronize()
    return buf, off, db, ([int(v) & 0xFFFFFFFF for v in gw.tolist()] if guard else None)


def check_in_bwd(x, dy_full, dy_arg, w1, slope, what):
    """dy_full: the C-channel gradient the reference and the fp32 kernel see; dy_arg / w1: what the entry point under test receives."""
    N, C, S = x.shape
    mean, rstd = stats(x, N * C, S)
    ref = in_bwd_fp64(x, dy_full, slope)
    dx32 = in_bwd_fp32(x, dy_full, mean, rstd, slope)
    buf, off, db, _ = in_bwd_h2(x, dy_arg, w1, mean, rstd, slope)
    cells = cells_of(buf, off)
    assert cells[0] == cells[1] and 0 < cells[0] < 0x7F800000
    k = h2_exp(cells[0])
    dec, a0, a1 = h2_decode(buf, N, C, S, k)
    assert bool(torch.isfinite(a0).all()) and bool(torch.isfinite(a1).all())           # no fp16 inf anywhere
    cell_val = struct.unpack('<f', struct.pack('<I', cells[0]))[0]
    top = max(float(dec.abs().max()), float(dx32.abs().max()))
    print('%s: cell %.4g, max|dx| %.4g' % (what, cell_val, top))
    assert cell_val >= top                                                              # the cell bounds the tensor from above
    e, e32 = dec - ref, dx32.double() - ref
    rms = lambda t: float(t.pow(2).mean().sqrt())
    print('%s: rms(e) %.3e rms(e32) %.3e rms(ref) %.3e | max|e| %.3e max|e32| %.3e max|ref| %.3e'
          % (what, rms(e), rms(e32), rms(ref), float(e.abs().max()), float(e32.abs().max()), float(ref.abs().max())))
    assert rms(e) <= 1.3 * rms(e32) + 2.0 ** -22 * rms(ref)
    assert float(e.abs().max()) <= 2.0 * float(e32.abs().max()) + 2.0 ** -21 * float(ref.abs().max())
    # the values split are k_in_bwd_apply's bit for bit (norm_act.hip in_bwd_value: one definition, the same partial sums in the same order):
    # criterion R against the fp32 kernel's tensor
    assert_R(dec, a0, a1, dx32, k, what)
    return mean, rstd


IN_BWD_CASES = [(1, 64, 4096, 0.0), (2, 16, 2500, 0.2), (1, 128, 19683, 0.0)]


@pytest.mark.parametrize('N,C,S,slope', IN_BWD_CASES)
def test_instnorm_backward_in_h2_form_against_fp64(N, C, S, slope):
    """dx of InstanceNorm + (Leaky)ReLU written in H2 form only: no worse against the fp64 autograd backward than the fp32 kernel
    nc_instnorm_act_bwd (the factors 1.3 / 2 of tests/test_gpu_split.py and test_gpu_h2.py) beyond what criterion R allows, the cell an upper
    bound, no fp16 infinity; and the bias gradient = the fp64 channel sum of the decoded tensor under deliberately wrong statistics, where the
    sums are O(1) (tests/test_gpu_ops.py: 1e-6 of sum|dx|)."""
    g = torch.Generator(device=DEV).manual_seed(6 + S)
    x = torch.randn(N, C, S, device=DEV, generator=g) * 2 + 0.5
    dy = torch.randn(N, C, S, device=DEV, generator=g)
    what = 'in_bwd_h2 %s' % ((N, C, S, slope),)
    mean, rstd = check_in_bwd(x, dy, dy, None, slope, what)
    mw = mean + 0.3 * torch.randn(N * C, device=DEV, generator=g)
    rw = rstd * 1.2
    buf, off, db, _ = in_bwd_h2(x, dy, None, mw, rw, slope)
    cells = cells_of(buf, off)
    dec, a0, a1 = h2_decode(buf, N, C, S, h2_exp(cells[0]))
    assert bool(torch.isfinite(a0).all()) and bool(torch.isfinite(a1).all())
    want = dec.sum((0, 2))
    assert float(want.abs().max()) > 1.0                           # the sums are O(1), not rounding noise, in this set-up
    d = float((db.double() - want).abs().max())
    print('%s: dbias off by %.3e, limit %.3e' % (what, d, 1e-6 * float(dec.abs().sum((0, 2)).max())))
    assert d <= 1e-6 * float(dec.abs().sum((0, 2)).max())


@pytest.mark.parametrize('S', [4096, 2500])
def test_instnorm_backward_rank_one_form_against_fp64(S):
    """The rank-one form (k_in_bwd_*_h2<true>): the gradient at the norm's output is w1[c] * dy1[v] from a ONE-channel dy1, never expanded; w1 of
    mixed sign with one tiny entry.  Reference and fp32 kernel run on the expanded tensor (the fp32 product, which is what the kernel forms)."""
    N, C, slope = 1, 64, 0.0
    g = torch.Generator(device=DEV).manual_seed(60 + S)
    x = torch.randn(N, C, S, device=DEV, generator=g) * 2 + 0.5
    dy1 = torch.randn(1, 1, S, device=DEV, generator=g)
    w1 = torch.randn(C, device=DEV, generator=g)
    w1[5] = 3.0e-12
    assert bool((w1 > 0).any()) and bool((w1 < 0).any())
    dy_full = (w1.view(1, C, 1) * dy1).contiguous()
    check_in_bwd(x, dy_full, dy1, w1, slope, 'in_bwd_h2 rank one S=%d' % S)


def test_instnorm_backward_flagged_by_the_guard_leaves_the_s3_form():
    """nc_set_h2_guard(2) and a gradient whose first 8-channel block is 2^-22 of the rest ('dark_channels' of tests/test_gpu_h2.py, a whole block
    of the 16 channels here): half of the chunks lie below 2^-17 of the cell, the call is flagged on the device, and the buffer then holds the S3 form of the SAME
    values -- the fp32 kernel's tensor -- so its decode is held to the same limits against fp64 (and to equality with that tensor)."""
    N, C, S, slope = 2, 16, 2500, 0.2
    L().nc_set_h2_guard(2)
    g = torch.Generator(device=DEV).manual_seed(31)
    x = torch.randn(N, C, S, device=DEV, generator=g) * 2 + 0.5
    dy = torch.randn(N, C, S, device=DEV, generator=g)
    dy[:, :8] *= 2.0 ** -22
    mean, rstd = stats(x, N * C, S)
    ref = in_bwd_fp64(x, dy, slope)
    dx32 = in_bwd_fp32(x, dy, mean, rstd, slope)
    buf, off, db, gw = in_bwd_h2(x, dy, None, mean, rstd, slope, guard=True)
    total = N * C // 8 * ((S + 63) // 64)
    print('guard words', gw[:3], 'of', total, 'chunks')
    assert gw[GUARD_FLAG] == 1 and gw[GUARD_LOW] * 64 > total - gw[GUARD_ALL]
    dec = from_s3(buf[:N * C * S * 6], N, C, S)
    e, e32 = dec.double() - ref, dx32.double() - ref
    rms = lambda t: float(t.pow(2).mean().sqrt())
    assert rms(e) <= 1.3 * rms(e32) + 2.0 ** -22 * rms(ref)
    assert float(e.abs().max()) <= 2.0 * float(e32.abs().max()) + 2.0 ** -21 * float(ref.abs().max())
    assert torch.equal(dec, dx32)
    # the same input unflagged (mode 1 decides the same way outside a whole-network call; guard = NULL: nothing is counted, the H2 form stays)
    buf2, off2, _, _ = in_bwd_h2(x, dy, None, mean, rstd, slope)
    k = h2_exp(cells_of(buf2, off2)[0])
    dec2, a0, a1 = h2_decode(buf2, N, C, S, k)
    assert_R(dec2, a0, a1, dx32, k, 'in_bwd_h2 dark channels, no guard words')


# ---------------------------------------------------------------------------------------------------------------------------------------------
# nc_convT_k2s2_fwd_split_h2_debug
# ---------------------------------------------------------------------------------------------------------------------------------------------
CONVT_CASES = [(1, 128, 64, (3, 5, 7)), (2, 128, 64, (9, 10, 13)), (1, 256, 128, (5, 6, 7)), (2, 256, 128, (3, 35, 5))]


@functools.lru_cache(maxsize=None)
def convt_case(case, with_bias=True):
    """Inputs of a case and its fp64 reference, computed once (the tests only read them)."""
    N, C, K, n = case
    g = torch.Generator(device=DEV).manual_seed(5 + C + n[1])
    x = torch.randn(N, C, *n, device=DEV, generator=g).clamp_min(0)          # a ReLU output, as the layer sees
    w = torch.randn(C, K, 2, 2, 2, device=DEV, generator=g) * 0.05
    b = torch.randn(K, device=DEV, generator=g) if with_bias else None
    return x, w, b, convt_fp64(x, w, b)


def convt_fp64(x, w, b):
    return torch.nn.functional.conv_transpose3d(x.double().cpu(), w.double().cpu(), b.double().cpu() if b is not None else None, stride=2).to(DEV)


def convt_h2(x, w, b, want_y=True):
    """-> y [N][K][8 S] (or None), the 2K-channel H2 buffer whose channels [K, 2K) the call writes, the byte offset of its cells."""
    N, C, D, H, W = x.shape
    K = w.shape[1]
    S2 = 8 * D * H * W
    nb = int(L().nc_convT_k2s2_split_h2_ws_bytes(I(N), I(C), I(D), I(H), I(W), I(K)))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    y = torch.full((N, K, S2), float('nan'), device=DEV) if want_y else None
    buf, off = h2_alloc(N, 2 * K, S2)
    ck(L().nc_convT_k2s2_fwd_split_h2_debug(P(x), P(w), P(b), P(y), P(buf), I(2 * K), I(K), I(N), I(C), I(D), I(H), I(W), I(K), P(buf, off + 4),
                                            P(ws), Z(nb), stream()), 'nc_convT_k2s2_fwd_split_h2_debug')
    torch.cuda.synchronize()
    return y, buf, off


def convt_bound_fp64(w, b, in_bound):
    col = w.double().abs().sum(0).reshape(w.shape[1], 8) * in_bound          # [k][q]
    if b is not None:
        col = col + b.double().abs().view(-1, 1)
    return col


def check_convt_h2_output(x, w, b, ref, what):
    N, C, D, H, W = x.shape
    K = w.shape[1]
    S2 = 8 * D * H * W
    y, buf, off = convt_h2(x, w, b)
    cells = cells_of(buf, off)
    assert cells[0] == 0xA5A5A5A5 and all(c == 0xA5A5A5A5 for c in cells[2:])
    cell_val = struct.unpack('<f', struct.pack('<I', cells[1]))[0]
    in_bound = struct.unpack('<f', struct.pack('<f', math.sqrt(D * H * W)))[0]
    assert float(x.abs().max()) <= in_bound
    bound = float(convt_bound_fp64(w, b, in_bound).max())
    print('%s: cell %.5g, max|ref| %.5g, bound %.5g' % (what, cell_val, float(ref.abs().max()), bound))
    assert cell_val >= float(ref.abs().max()) and cell_val <= 1.01 * bound
    k = h2_exp(cells[1])
    dec, a0, a1 = h2_decode(buf, N, 2 * K, S2, k)
    assert_R(dec[:, K:], a0[:, K:], a1[:, K:], y, k, what)
    assert bool((block_bytes(buf, N, 2 * K, S2, 0, K) == SENT).all())        # the other half of the concatenation is untouched
    _, buf2, _ = convt_h2(x, w, b, want_y=False)
    assert torch.equal(buf, buf2)                                             # y = NULL: the same H2 bytes
    return y, cell_val, bound


@pytest.mark.parametrize('case', CONVT_CASES, ids=[str(c) for c in CONVT_CASES])
def test_conv_transpose_two_term_against_fp64(case):
    """ConvTranspose3d(k 2, s 2) in the two-term form (k_convT_s3<8, 2> at 128 -> 64, <4, 2> at 256 -> 128; 512-voxel tiles with ragged tails, the
    second sample) from a fp32 input, fp32 output and the H2 form of it into channels [K, 2K) of a 2K-channel tensor.  The fp32 output against
    fp64 next to the fp32 kernel nc_convT_k2s2_fwd and the three-term nc_convT_k2s2_fwd_split: the limits tests/test_gpu_h2.py sets for layers
    without a running accumulator (the K-dimension is at most 256: no accumulator restarts), held against the fp32 kernel; the three-term figures
    are printed beside them (with so short a sum the three-term form is nearly exact, a yardstick of its own kind)."""
    N, C, K, n = case
    x, w, b, ref = convt_case(case)
    D, H, W = n
    S2 = 8 * D * H * W
    y, cell_val, bound = check_convt_h2_output(x, w, b, ref, 'convT two-term %s' % (case,))
    y32 = torch.full((N, K, S2), float('nan'), device=DEV)
    ck(L().nc_convT_k2s2_fwd(P(x), P(w), P(b), P(y32), I(N), I(C), I(D), I(H), I(W), I(K), stream()), 'nc_convT_k2s2_fwd')
    nb = int(L().nc_convT_k2s2_split_ws_bytes(I(N), I(C), I(D), I(H), I(W), I(K)))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    y3 = torch.full((N, K, S2), float('nan'), device=DEV)
    ck(L().nc_convT_k2s2_fwd_split(P(x), P(None), P(w), P(b), P(y3), P(None), I(8), I(0), I(N), I(C), I(D), I(H), I(W), I(K), P(ws), Z(nb), stream()),
       'nc_convT_k2s2_fwd_split')
    r = ref.reshape(N, K, S2)
    (m2, r2), (m32, r32), (m3, r3) = err(y, r), err(y32, r), err(y3, r)
    print('%s: max / rms of the output rms: fp32 %.2e/%.2e  three-term %.2e/%.2e  two-term %.2e/%.2e' % (case, m32, r32, m3, r3, m2, r2))
    # the yardsticks are held to fp64 themselves before they measure anything (tests/convt_reference.py: the fp32 kernel within 3 x the distance
    # of torch's fp32 operator on the CPU, the three-term kernel within its own limits of tests/test_gpu_convt_split.py)
    mo, ro = err(torch.nn.functional.conv_transpose3d(x.cpu(), w.cpu(), b.cpu(), stride=2).to(DEV).reshape(N, K, S2), r)
    print('%s: fp32 oracle (CPU) %.2e/%.2e' % (case, mo, ro))
    assert not bool(torch.isnan(y32).any()) and not bool(torch.isnan(y3).any())
    assert convt_reference().within((m32, r32), (mo, ro)), (m32, r32, mo, ro)
    assert r3 < 3e-7 and m3 < 3e-6 and r3 <= 1.5 * ro + 5e-8, (m3, r3, ro)
    assert r2 <= 1.3 * r32 + 2e-8 and m2 <= 2.0 * m32 + 2e-7, (m2, r2, m32, r32)


@pytest.mark.parametrize('with_bias', [True, False])
@pytest.mark.parametrize('case', [CONVT_CASES[0], CONVT_CASES[2]], ids=[str(CONVT_CASES[0]), str(CONVT_CASES[2])])
def test_conv_transpose_output_that_reaches_its_bound(case, with_bias):
    """The cell of the output is a bound from the weights alone: in_bound * sum_ci |w[ci][k][q]| + |bias[k]|, largest column.  At one voxel the input
    is in_bound * sign(w[ci][k*][q*]) (times the sign of the bias) for that column, so one output element REACHES the uninflated bound: it must stay
    finite in fp16 and the whole tensor must meet criterion R."""
    N, C, K, n = case
    x0, w, b, _ = convt_case(case, with_bias)
    D, H, W = n
    in_bound = struct.unpack('<f', struct.pack('<f', math.sqrt(D * H * W)))[0]
    col = convt_bound_fp64(w, b, in_bound)
    kq = int(col.argmax())
    ks, qs = kq // 8, kq % 8
    sgn = torch.sign(w.reshape(C, K, 8)[:, ks, qs])
    if with_bias:
        sgn = sgn * (1.0 if float(b[ks]) >= 0 else -1.0)
    x = x0.clone()
    vz, vy, vx = D - 1, H // 2, W - 1
    x[N - 1, :, vz, vy, vx] = in_bound * sgn
    ref = convt_fp64(x, w, b)
    y, cell_val, bound = check_convt_h2_output(x, w, b, ref, 'convT at its bound %s bias %s' % (case, with_bias))
    o = ((2 * vz + (qs >> 2)) * 2 * H + 2 * vy + ((qs >> 1) & 1)) * 2 * W + 2 * vx + (qs & 1)
    got = abs(float(y[N - 1, ks, o]))
    print('the element: %.6g of the bound %.6g (cell %.6g)' % (got, bound, cell_val))
    assert got >= bound * (1 - 1e-6) and got == float(y.abs().max())
    assert abs(float(ref.reshape(N, K, -1)[N - 1, ks, o])) == pytest.approx(bound, rel=1e-12)
