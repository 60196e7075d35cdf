"""The two kernels that add up FIXED-ORDER partial sums, bit for bit: k_wgrad_s3_reduce (csrc/conv_split.hip, behind every 3^3 / 5^3 weight-gradient
kernel) and k_gemm_split_reduce (csrc/conv_gemm.hip, behind every split gather GEMM), through nc_wgrad_s3_reduce_debug / nc_gemm_split_reduce_debug
(include/nc_hip.h documents the layouts and the orders; both run the launch the library's own paths make).

The reference is a numpy float32 restatement of the documented order -- np.add on float32 arrays, one add per documented add, no np.sum -- and
the comparison is np.array_equal on the uint32 views.  The inputs are randn * 2^randint(-8, 8): magnitudes 2^16 apart, so that another order of
the same adds changes bits.  test_the_emulation_* (no GPU) shows both halves of that for every input set: the emulation is within fp32 rounding
of an fp64 sum, and numpy's pairwise np.sum of the same slots differs from it in at least one bit.  One input set is too short for np.sum to BE
another order -- (64, 64, 27, 3, 1): three slots, which np.sum adds one after the other exactly as the documented order does (its pairwise blocks
start at eight) -- there the other order is the same three slots added last to first.

The whole-path tests at the end guard the plumbing of the callers (nc_conv_wgrad two-term, three-term and bf16; nc_convT_k2s2_wgrad) against
fp64 at the tolerances the existing tests of those entry points use (tests/test_gpu_h2.py, test_gpu_split.py, test_gpu_lp.py, test_gpu_convt.py).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

F32 = np.float32
U = 2.0 ** -24  # unit roundoff of fp32

# (K, C, T3, nwp, NF)
WCASES = [(64, 64, 27, 128, 1),    # per = 16: block 1 at 108^3
          (256, 256, 27, 8, 1),    # per = 1: blocks 5 / 6 at 108^3; 56 MB of partials
          (64, 128, 27, 64, 1),    # block 9: with cells the scale differs between the halves of c
          (64, 64, 27, 5, 3),      # nslots = 15: seven segments of two, one of one
          (64, 64, 27, 3, 1),      # five empty segments
          (64, 64, 125, 4, 2),     # 5^3: TW = 25, five dz groups
          (64, 64, 27, 20, 1),     # per = 3: the looping kernel one step at a time, the last segment empty (per 1 and 2 have kernels of their own)
          (64, 64, 27, 36, 1)]     # per = 5: its four-step group with a slot past the end, then a single step
# (n, splits, bias, inner, K)
SCASES = [(3 * 121 * 4, 7, True, 121, 3),   # a group of four spans two channels
          (1001, 9, False, 1, 1),           # misaligned rows and a tail
          (4096, 2, True, 1024, 4),
          (4096, 256, False, 1, 1),
          (8, 8, True, 2, 4)]
# cells: float bits of the magnitudes the two-term operands were converted with; xcells[0] != xcells[1]
XCELLS, YCELL = (3.0, 100.0), 0.01


def mixed(rng, shape):
    return (rng.standard_normal(shape, dtype=F32) * np.exp2(rng.integers(-8, 9, shape)).astype(F32)).astype(F32)


def geometry(K, C, T3):
    TW = 27 if T3 == 27 else 25
    ndg = T3 // TW
    return TW, ndg, (K // 64) * (C // 32) * ndg


@functools.lru_cache(maxsize=None)
def wpart(case):
    """part in the header's layout, [nwp][npairs][NF][TW][64][32]; computed once per case, read only."""
    K, C, T3, nwp, NF = case
    TW, _, npairs = geometry(K, C, T3)
    p = mixed(np.random.default_rng(1000 + WCASES.index(case)), (nwp, npairs, NF, TW, 64, 32))
    p.setflags(write=False)
    return p


def wslots(case):
    """[nslots][npairs][TW][64][32]: slot sl = w * NF + f (a view)."""
    K, C, T3, nwp, NF = case
    p = wpart(case)
    return p.transpose(0, 2, 1, 3, 4, 5).reshape((nwp * NF,) + p.shape[1:2] + p.shape[3:])


def segments(nslots):
    per = -(-nslots // 8)
    return [range(min(j * per, nslots), min((j + 1) * per, nslots)) for j in range(8)]


@functools.lru_cache(maxsize=None)
def wsum(case):
    """The documented order, unscaled: [npairs][TW][64][32] float32."""
    sl = wslots(case)
    segs = []
    for seg in segments(sl.shape[0]):
        acc = np.zeros(sl.shape[1:], F32)
        for s in seg:
            acc = np.add(acc, sl[s], dtype=F32)
        segs.append(acc)
    r = segs[0]
    for j in range(1, 8):
        r = np.add(r, segs[j], dtype=F32)
    r.setflags(write=False)
    return r


def h2_exp(cell):
    e = int(np.array(cell, F32).view(np.uint32)) >> 23
    return min(14 - (e - 127) if e else 0, 126)


def unscale2(cell_a, cell_b):
    """s3_common.hpp h2_unscale2: 2^-(ka + kb) as two factors, the division truncating as C's does."""
    e = -(h2_exp(cell_a) + h2_exp(cell_b))
    e1 = int(e / 2)
    e2 = e - e1
    return F32(2.0 ** max(e1, -126)), F32(2.0 ** max(e2, -126))


def wexpected(case, cells):
    """dw [K][C][T3] of the documented order; cells: r * f.x * f.y, f by the half of c."""
    K, C, T3, nwp, NF = case
    TW, ndg, npairs = geometry(K, C, T3)
    r = wsum(case).reshape(K // 64, C // 32, ndg, TW, 64, 32).transpose(0, 4, 1, 5, 2, 3).reshape(K, C, T3)
    if not cells:
        return r
    out = np.empty_like(r)
    for half, c in ((0, slice(0, C // 2)), (1, slice(C // 2, C))):
        fx, fy = unscale2(XCELLS[half], YCELL)
        out[:, c] = np.multiply(np.multiply(r[:, c], fx, dtype=F32), fy, dtype=F32)
    return out


@functools.lru_cache(maxsize=None)
def sdata(case):
    n, splits, has_bias, inner, K = case
    rng = np.random.default_rng(2000 + SCASES.index(case))
    slab = mixed(rng, (splits, n))
    bias = mixed(rng, (K,)) if has_bias else None
    slab.setflags(write=False)
    return slab, bias


def sbias(case):
    n, splits, has_bias, inner, K = case
    bias = sdata(case)[1]
    return bias[(np.arange(n) // inner) % K] if has_bias else np.zeros(n, F32)


def sexpected(case):
    slab = sdata(case)[0]
    s = sbias(case)
    for k in range(slab.shape[0]):
        s = np.add(s, slab[k], dtype=F32)
    return s


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# without a GPU: the emulation is a sum, and its order shows in the bits
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', WCASES, ids=[str(c) for c in WCASES])
def test_the_emulation_of_the_weight_gradient_sums(case):
    sl = wslots(case)
    nslots = sl.shape[0]
    emu = wsum(case)
    exact = sl.astype(np.float64).sum(0)
    # a chain of at most per adds inside a segment and 7 across them, every add within u of its own result: (per + 7) u sum |slot| to first order
    per = -(-nslots // 8)
    bound = (per + 7) * U * 1.01 * np.abs(sl).astype(np.float64).sum(0)
    assert np.all(np.abs(emu.astype(np.float64) - exact) <= bound)
    last = np.ascontiguousarray(np.moveaxis(sl, 0, -1))  # the slots along the contiguous axis: np.sum adds THAT axis pairwise
    if nslots >= 8:
        other = np.sum(last, axis=-1, dtype=F32)
    else:  # np.sum of fewer than eight elements is the documented order itself: the same slots last to first instead
        other = np.zeros(sl.shape[1:], F32)
        for s in reversed(range(nslots)):
            other = np.add(other, sl[s], dtype=F32)
    assert not np.array_equal(bits(other), bits(emu))
    assert np.all(np.abs(other.astype(np.float64) - exact) <= nslots * U * 1.01 * np.abs(sl).astype(np.float64).sum(0))  # (it IS a sum of them)


@pytest.mark.parametrize('case', SCASES, ids=[str(c) for c in SCASES])
def test_the_emulation_of_the_split_sums(case):
    slab = sdata(case)[0]
    b = sbias(case)
    emu = sexpected(case)
    exact = slab.astype(np.float64).sum(0) + b
    mag = np.abs(slab).astype(np.float64).sum(0) + np.abs(b)
    assert np.all(np.abs(emu.astype(np.float64) - exact) <= slab.shape[0] * U * 1.01 * mag)
    other = np.add(np.sum(np.ascontiguousarray(slab.T), axis=-1, dtype=F32), b, dtype=F32)  # pairwise, the bias last
    assert not np.array_equal(bits(other), bits(emu))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# on the GPU: the kernels, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def L():
    from neuroclear_amd._lib import lib
    return lib()


def ck(code, what):
    from neuroclear_amd._lib import check
    check(code, what)


def P(t):
    from neuroclear_amd import ops
    return ops._ptr(t)


def stream():
    from neuroclear_amd import ops
    return ops._stream()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def cell_words():
    import torch
    xc = torch.from_numpy(np.array(XCELLS, F32).view(np.int32)).cuda()
    yc = torch.from_numpy(np.array([YCELL], F32).view(np.int32)).cuda()
    return xc, yc


def run_wreduce(case, cells, guard=None):
    import torch
    K, C, T3, nwp, NF = case
    part = dev(wpart(case))
    dw = torch.full((K, C, T3), float('nan'), device='cuda')
    xc, yc = cell_words() if cells else (None, None)
    ck(L().nc_wgrad_s3_reduce_debug(P(part), P(dw), K, C, T3, nwp, NF, P(xc), P(yc), P(guard), stream()), 'nc_wgrad_s3_reduce_debug')
    torch.cuda.synchronize()
    return dw.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('cells', [False, True], ids=['no cells', 'cells'])
@pytest.mark.parametrize('case', WCASES, ids=[str(c) for c in WCASES])
def test_wgrad_s3_reduce_bit_for_bit(case, cells):
    got = run_wreduce(case, cells)
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(wexpected(case, cells)))


@pytest.mark.gpu
@pytest.mark.parametrize('cells', [False, True], ids=['no cells', 'cells'])
def test_wgrad_s3_reduce_leaves_when_it_is_not_its_turn(cells):
    """guard word [2] set = the call was flagged: the form with cells (two-term) leaves; clear: the form without leaves.  dw keeps its NaN.  The
    other setting of the same word runs."""
    import torch
    case = WCASES[4]
    guard = torch.zeros(8, dtype=torch.int32, device='cuda')
    guard[2] = 1 if cells else 0
    assert np.isnan(run_wreduce(case, cells, guard)).all()
    guard[2] = 0 if cells else 1
    assert np.array_equal(bits(run_wreduce(case, cells, guard)), bits(wexpected(case, cells)))


@pytest.mark.gpu
@pytest.mark.parametrize('case', SCASES, ids=[str(c) for c in SCASES])
def test_gemm_split_reduce_bit_for_bit(case):
    import torch
    n, splits, has_bias, inner, K = case
    slab_np, bias_np = sdata(case)
    slab = dev(slab_np)
    bias = dev(bias_np) if has_bias else None
    out = torch.full((n,), float('nan'), device='cuda')
    ck(L().nc_gemm_split_reduce_debug(P(slab), P(out), n, splits, P(bias), inner, K, stream()), 'nc_gemm_split_reduce_debug')
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(sexpected(case)))


@pytest.mark.gpu
def test_gemm_split_reduce_scalar_form_of_a_row_that_is_not_16_byte_aligned():
    """n % 4 == 0 but `out` four bytes off a 16-byte boundary: the one-element form, the same bits."""
    import torch
    case = SCASES[2]
    n, splits, has_bias, inner, K = case
    slab_np, bias_np = sdata(case)
    slab, bias = dev(slab_np), dev(bias_np)
    buf = torch.full((n + 1,), float('nan'), device='cuda')
    out = buf[1:]
    ck(L().nc_gemm_split_reduce_debug(P(slab), P(out), n, splits, P(bias), inner, K, stream()), 'nc_gemm_split_reduce_debug')
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(sexpected(case))) and bool(torch.isnan(buf[0]))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# on the GPU: the callers' plumbing, against fp64
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def _restore():
    from neuroclear_amd import ops
    prev = ops.set_conv_split(True)
    t = L().nc_get_split_terms()
    prec = ops.conv_precision
    yield
    ops.set_conv_precision(prec)
    L().nc_set_split_terms(t)
    ops.set_conv_split(prev)


def rel_err(a, r):
    s = r.pow(2).mean().sqrt().item()
    e = a.double() - r
    return e.abs().max().item() / s, e.pow(2).mean().sqrt().item() / s


@pytest.mark.gpu
def test_conv_wgrad_two_term_three_term_and_bf16_against_fp64(_restore):
    """nc_conv_wgrad, 64 -> 64 channels, 16^3, 3^3.  Two-term and three-term: tests/test_gpu_h2.py test_h2_wgrad_against_fp64 and
    tests/test_gpu_split.py (rms <= 1.3 x, max <= 2 x the fp32 MFMA kernel's error against fp64, plus their floors; three-term rms < 6e-7).
    bf16: tests/test_gpu_lp.py / test_gpu_c8.py (1e-4 of the largest magnitude, against fp64 on the rounded operands)."""
    import torch
    from neuroclear_amd import ops
    N, C, K, E, ks = 1, 64, 64, 16, 3
    g = torch.Generator(device='cuda').manual_seed(9)
    x = torch.randn((N, C, E, E, E), device='cuda', generator=g).clamp_min(0)
    dy = torch.randn((N, K, E, E, E), device='cuda', generator=g)
    shape = (K, C, ks, ks, ks)
    ref = torch.nn.grad.conv3d_weight(x.double(), shape, dy.double(), padding=1)
    res = {}
    for name, split, terms in (('fp32', False, 3), ('t3', True, 3), ('t2', True, 2)):
        ops.set_conv_split(split)
        L().nc_set_split_terms(terms)
        dw = ops.conv_wgrad_raw(x, dy, shape, 1, 1, False)[0]
        assert torch.equal(dw, ops.conv_wgrad_raw(x, dy, shape, 1, 1, False)[0])
        res[name] = rel_err(dw, ref)
    (m32, r32), (m3, r3), (m2, r2) = res['fp32'], res['t3'], res['t2']
    print('wgrad fp32 %.2e/%.2e  three-term %.2e/%.2e  two-term %.2e/%.2e' % (m32, r32, m3, r3, m2, r2))
    assert r2 <= 1.3 * r32 + 2e-8 and m2 <= 2.0 * m32 + 2e-7, (m2, r2, m32, r32)
    assert r2 <= 1.3 * r3 + 2e-8, (r2, r3)
    assert r3 <= 1.3 * r32 + 2e-8 and r3 < 6e-7 and m3 <= 2.0 * m32 + 3e-7, (m3, r3, m32, r32)
    xr, dyr = x.to(torch.bfloat16).float(), dy.to(torch.bfloat16).float()
    refb = torch.nn.grad.conv3d_weight(xr.double(), shape, dyr.double(), padding=1)
    ops.set_conv_split(True)
    L().nc_set_split_terms(2)
    ops.set_conv_precision('bf16')
    dwb = ops.conv_wgrad_raw(x, dy, shape, 1, 1, False)[0]
    ops.set_conv_precision('fp32')
    eb = float((dwb.double() - refb).abs().max())
    print('wgrad bf16 %.2e of the largest' % (eb / float(refb.abs().max())))
    assert eb <= 1e-4 * float(refb.abs().max())


@pytest.mark.gpu
def test_convT_k2s2_wgrad_against_fp64():
    """nc_convT_k2s2_wgrad, 128 -> 64 channels, 8^3: the gather GEMM with its split sums; reference, yardstick and limit of tests/test_gpu_convt.py
    (tests/convt_reference.py)."""
    import torch
    import convt_reference as R
    N, C, K, n = 1, 128, 64, (8, 8, 8)
    x, w, b, dy = (t.cuda() for t in R.inputs(N, C, K, n))
    ref = R.ref_wgrad(x, dy)
    _, odw, odb = R.oracle_bwd(N, C, K, n)
    nb = int(L().nc_convT_ws_bytes(N, C, *n, K))
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    dw = torch.full((C, K, 2, 2, 2), float('nan'), device='cuda')
    db = torch.full((K,), float('nan'), device='cuda')
    ck(L().nc_convT_k2s2_wgrad(P(x), P(dy), P(dw), P(db), N, C, *n, K, P(ws), nb, stream()), 'nc_convT_k2s2_wgrad')
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dw).any()) and not bool(torch.isnan(db).any())
    got, orc = R.err(dw, ref), R.err(odw, ref)
    print('convT wgrad max %.2e rms %.2e | oracle max %.2e rms %.2e' % (got + orc))
    assert R.within(got, orc), (got, orc)
    rdb = R.ref_dbias(dy)
    assert R.within(R.err(db, rdb), R.err(odb, rdb))
