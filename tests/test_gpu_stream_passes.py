"""The streaming passes of the U-Net training step (nc_set_stream_passes; csrc/norm_act.hip, csrc/w_prep.hip, csrc/w_prep.hpp):

  * the folded rank-one apply pass of the last block issues the nine loads of an iteration before it uses the first;
  * the fp32 norm backward keeps the loads of eight iterations in flight in its sums pass and of four in its apply pass, which also issues its
    first loads before it adds up the partial sums (loaded eight at a time, added in the same order);
  * the rank-one form's sums pass keeps eight iterations in flight instead of four;
  * the batched weight preparation takes its cells by rows and writes whole 16-byte fragments, both terms from one read of the eight weights.

No stored value and no order of summation changes, so every comparison is of bytes, switch on against off (off launches the kernels as they
were): the H2 units with their cells, the bias gradient, the guard words, and the workspace, which holds the fp64 partial sums of the sums pass
and the fp64 row sums of the apply pass.

The two-term norm backward exists for instances of more than 2048 voxels only (tests/test_gpu_in_bwd_fold.py), so 8 x 14 x 20 = 2240 voxels is the
smallest instance: one chunk of 8.75 x 256 elements -- a sums thread runs one round of eight and, three quarters of them, one plain iteration;
the fp32 apply pass (three workgroups, 2.9 iterations per thread) runs its plain loop only.  17 x 18 x 20 = 6120 voxels: 23.9 iterations per sums
thread (two rounds of eight and a tail of seven or eight), and six workgroups of the apply pass with 3.98 iterations per thread -- threads
below 1512 run one round of four, the others three plain iterations.  The apply pass's rounds of eight partial sums and its second round of
loads need far longer instances: they have a test of their own below.  The first layer's 7^3 forward (k_build_x8_h2) has no test here: the pull
request that added this file left that kernel as it was."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neuroclear_amd import ops  # noqa: E402
from neuroclear_amd._lib import lib  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402
from test_gpu_h2_writers import FL, LG, I, P, Z, ck, h2_alloc, stats, stream  # noqa: E402
from test_gpu_in_bwd_fold import pool_case, pool_fwd  # noqa: E402
from test_gpu_wprep import BLOCKS, WPREP_BIT  # noqa: E402

DEV = 'cuda'
WS_SENT = 0x3C  # the workspace starts as this byte: what a pass does not write compares equal


@pytest.fixture
def switches():
    L = lib()
    prev = (L.nc_get_split_terms(), L.nc_get_unet_lean(), L.nc_get_h2_guard(), ops.set_conv_split(True), L.nc_get_unet_wprep(),
            L.nc_get_in_bwd_fold(), L.nc_get_stream_passes())
    L.nc_set_split_terms(2)
    L.nc_set_in_bwd_fold(1)
    yield L
    L.nc_set_split_terms(prev[0])
    L.nc_set_unet_lean(prev[1])
    L.nc_set_h2_guard(prev[2])
    ops.set_conv_split(prev[3])
    L.nc_set_unet_wprep(prev[4])
    L.nc_set_in_bwd_fold(prev[5])
    L.nc_set_stream_passes(prev[6])


def raw(t):
    return t.contiguous().view(torch.uint8)


def same_bytes(a, b, what):
    assert len(a) == len(b), what
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(raw(u), raw(v)), '%s: output %d differs' % (what, k)


def test_switch_round_trip(switches):
    before = switches.nc_get_stream_passes()
    assert before == 1  # default on
    assert switches.nc_set_stream_passes(0) == before and switches.nc_get_stream_passes() == 0
    assert switches.nc_set_stream_passes(1) == 0 and switches.nc_get_stream_passes() == 1
    assert switches.nc_set_stream_passes(5) == 1 and switches.nc_get_stream_passes() == 1


# ---------------------------------------------------------------------------------------------------------------------------------------------
# whole network
# ---------------------------------------------------------------------------------------------------------------------------------------------
def guard_stats(L):
    out4 = (ctypes.c_ulonglong * 4)()
    torch.cuda.synchronize()
    assert L.nc_h2_guard_stats(out4, 0) == 0
    return [int(v) for v in out4]


def run_net(sd, x, r, L, on):
    L.nc_set_stream_passes(on)
    before = guard_stats(L)
    net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0])
    net.load_state_dict(sd)
    xi = x.clone().requires_grad_(True)
    y = net(xi)
    kept = int(y.grad_fn.kept)
    (y * r).mean().backward()
    after = guard_stats(L)
    return [y.detach().clone(), xi.grad.detach().clone()] + [p.grad.detach().clone() for p in net.parameters()], kept, \
        [a - b for a, b in zip(after, before)]


def net_data(shape, n):
    sd = S.state_dict_from_seed(S.unet_deconv_spec(), 5, DEV)
    x = torch.from_numpy(np.random.default_rng(31).random((n, 1) + shape, dtype=np.float32)).to(DEV)
    r = torch.from_numpy(np.random.default_rng(32).standard_normal((n, 1) + shape).astype(np.float32)).to(DEV)
    return sd, x, r


@pytest.mark.parametrize('lean,wprep', [(1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('shape', [(24, 24, 24), (40, 24, 32), (20, 24, 28)])
def test_whole_network_on_against_off(shape, n, lean, wprep, switches):
    """y, dx and every parameter gradient of nc_unet_deconv_train_fwd + nc_unet_deconv_bwd: torch.equal, and the range guard counted the same.
    20 x 24 x 28: 13 440 voxels at level 0, no multiple of 256 -- every prefetch loop meets its tail."""
    assert networks._FUSED_GEN
    sd, x, r = net_data(shape, n)
    switches.nc_set_unet_lean(lean)
    switches.nc_set_unet_wprep(wprep)
    off, kept_off, g_off = run_net(sd, x, r, switches, 0)
    on, kept_on, g_on = run_net(sd, x, r, switches, 1)
    print(shape, n, lean, wprep, 'kept %#x / %#x, guard counts %s / %s' % (kept_off, kept_on, g_off, g_on))
    assert kept_on == kept_off and bool(kept_on & WPREP_BIT) == bool(wprep)
    assert g_on == g_off
    for k, (a, b) in enumerate(zip(off, on)):
        assert bool(torch.isfinite(b).all()), k
        assert torch.equal(a, b), k


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the two-term norm backward, per form
# ---------------------------------------------------------------------------------------------------------------------------------------------
INSTANCES = [(8, 14, 20), (17, 18, 20)]


def poison(t, flat_nan, flat_inf):
    v = t.view(-1)
    v[flat_nan] = float('nan')
    v[flat_inf] = float('-inf')


def h2_form(L, x, dy, w1, mean, rstd, slope, dims, dy_stride=None, gp=None, arg=None, guard=True):
    """-> [the dxs buffer up to and including its cells, dbias, guard words, workspace] of one two-term norm backward.  w1: the rank-one form
    (nc_instnorm_act_bwd_dbias_h2_debug, no guard words: with them that entry point may switch kernels and launches the unfolded path);
    otherwise the plain or the POOL form inside a whole-network scope (nc_instnorm_act_bwd_dbias_h2_pool_debug)."""
    N, C, Sv = x.shape
    buf, off = h2_alloc(N, C, Sv, capacity=int(L.nc_s3_bytes(I(N), I(C), LG(Sv))))
    nb = int(L.nc_instnorm_bwd_dbias_ws_bytes(I(N * C), LG(Sv)))
    ws = torch.full((nb,), WS_SENT, dtype=torch.uint8, device=DEV)
    db = torch.full((C,), float('nan'), device=DEV)
    gw = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    if w1 is not None:
        ck(L.nc_instnorm_act_bwd_dbias_h2_debug(P(dy), P(w1), P(x), P(mean), P(rstd), FL(slope), P(buf), P(db), I(N), I(C), LG(Sv), P(ws), Z(nb),
                                                P(None), stream()), 'nc_instnorm_act_bwd_dbias_h2_debug')
    else:
        ck(L.nc_instnorm_act_bwd_dbias_h2_pool_debug(P(dy), LG(dy_stride if dy_stride else C * Sv), P(gp), P(arg), P(x), P(mean), P(rstd), FL(slope),
                                                     P(buf), P(db), I(N), I(C), I(dims[0]), I(dims[1]), I(dims[2]), P(ws), Z(nb),
                                                     P(gw if guard else None), stream()), 'nc_instnorm_act_bwd_dbias_h2_pool_debug')
    torch.cuda.synchronize()
    return [buf[:off + 256].clone(), db, gw, ws]


def on_off(L, fn):
    res = {}
    for on in (0, 1):
        L.nc_set_stream_passes(on)
        res[on] = fn()
    return res[0], res[1]


@pytest.mark.parametrize('bad', [False, True])
@pytest.mark.parametrize('dims', INSTANCES)
def test_rank_one_form(dims, bad, switches):
    """k_in_bwd_sums_h2<true> + the staged k_in_bwd_apply_h2 against the instance as it was.  bad: a NaN in one raw channel and an infinity in
    another (the statistics are those of the clean tensor), the other channels stay finite."""
    C, Sv = 16, dims[0] * dims[1] * dims[2]
    g = torch.Generator(device=DEV).manual_seed(77)
    x = torch.randn(1, C, Sv, device=DEV, generator=g) * 2 + 0.5
    dy1 = torch.randn(1, 1, Sv, device=DEV, generator=g)
    w1 = torch.randn(C, device=DEV, generator=g)
    mean, rstd = stats(x, C, Sv)
    if bad:
        poison(x, 2 * Sv + 700, 9 * Sv + Sv - 1)
    off, on = on_off(switches, lambda: h2_form(switches, x, dy1, w1, mean, rstd, 0.0, dims))
    print('rank one', dims, bad, 'dbias[0] %.6g' % float(on[1][0]))
    same_bytes(off, on, 'rank-one form %s' % (dims,))
    assert bool(torch.isfinite(on[1]).all()) == (not bad) and bool(torch.isfinite(on[1][:2]).all())


@pytest.mark.parametrize('bad', [False, True])
@pytest.mark.parametrize('N,dims,slope', [(1, INSTANCES[0], 0.0), (2, INSTANCES[1], 0.2)])
def test_plain_form(N, dims, slope, bad, switches):
    C, Sv = 16, dims[0] * dims[1] * dims[2]
    g = torch.Generator(device=DEV).manual_seed(78)
    x = torch.randn(N, C, Sv, device=DEV, generator=g) * 2 + 0.5
    dy = torch.randn(N, C, Sv, device=DEV, generator=g)
    dy[:, :8] *= 2.0 ** -22  # (the first block of channels far below the rest: the range guard counts its chunks as low)
    mean, rstd = stats(x, N * C, Sv)
    if bad:
        poison(x, 2 * Sv + 700, 9 * Sv + Sv - 1)
        poison(dy, 11 * Sv + 3, 12 * Sv + 257)
    off, on = on_off(switches, lambda: h2_form(switches, x, dy, None, mean, rstd, slope, dims))
    print('plain', N, dims, bad, 'guard words', on[2][:3].tolist())
    same_bytes(off, on, 'plain form %s' % (dims,))
    assert int(on[2][0]) > 0  # low chunks were counted


@pytest.mark.parametrize('bad', [False, True])
def test_pool_form(bad, switches):
    """8 x 14 x 20 pooled from 16 x 28 x 40: the instance of the norm backward is the UNPOOLED 16 x 28 x 40 block, its pooled gradient 8 x 14 x 20."""
    N, C, dims = 1, 16, (16, 28, 40)
    Sv = dims[0] * dims[1] * dims[2]
    x, act, dcat, gp = pool_case(N, C, *dims, 13, dark=True)
    _, arg = pool_fwd(act)
    mean, rstd = stats(x, N * C, Sv)
    if bad:
        poison(x, 2 * Sv + 700, 9 * Sv + Sv - 1)
        poison(gp, 3 * (Sv // 8) + 5, 12 * (Sv // 8) + 257)
    off, on = on_off(switches, lambda: h2_form(switches, x, dcat, None, mean, rstd, 0.0, dims, dy_stride=2 * C * Sv, gp=gp, arg=arg))
    print('pool', bad, 'guard words', on[2][:3].tolist())
    same_bytes(off, on, 'POOL form')
    assert int(on[2][0]) > 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the fp32 norm backward (block 0 of the step): nc_instnorm_act_bwd_dbias
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [False, True])
@pytest.mark.parametrize('slope', [0.0, 0.2])
@pytest.mark.parametrize('N,dims', [(1, INSTANCES[0]), (2, INSTANCES[1])])
def test_fp32_backward_with_bias_gradient(N, dims, slope, bad, switches):
    L = switches
    C, Sv = 8, dims[0] * dims[1] * dims[2]
    g = torch.Generator(device=DEV).manual_seed(79)
    x = torch.randn(N, C, Sv, device=DEV, generator=g) * 2 + 0.5
    dy = torch.randn(N, C, Sv, device=DEV, generator=g)
    mean, rstd = stats(x, N * C, Sv)
    if bad:
        poison(x, 2 * Sv + 700, 5 * Sv + Sv - 1)
        poison(dy, 3 * Sv + 3, 6 * Sv + 257)
    nb = int(L.nc_instnorm_bwd_dbias_ws_bytes(I(N * C), LG(Sv)))

    def one():
        ws = torch.full((nb,), WS_SENT, dtype=torch.uint8, device=DEV)
        dx = torch.full_like(x, 7.0)
        db = torch.full((C,), float('nan'), device=DEV)
        ck(L.nc_instnorm_act_bwd_dbias(P(dy), P(x), P(mean), P(rstd), FL(slope), P(dx), P(db), I(N), I(C), LG(Sv), P(ws), Z(nb), stream()),
           'nc_instnorm_act_bwd_dbias')
        dx2 = torch.full_like(x, 7.0)  # (the entry point without the bias gradient: the same two kernels, no row sums)
        ck(L.nc_instnorm_act_bwd(P(dy), P(x), P(mean), P(rstd), FL(slope), P(dx2), I(N * C), LG(Sv), P(ws), Z(nb), stream()), 'nc_instnorm_act_bwd')
        torch.cuda.synchronize()
        return [dx, db, ws, dx2]
    off, on = on_off(L, one)
    print('fp32', N, dims, slope, bad, 'dbias', on[1][:2].tolist())
    same_bytes(off, on, 'nc_instnorm_act_bwd_dbias %s' % (dims,))
    assert torch.equal(raw(on[0]), raw(on[3]))
    if not bad:
        assert bool(torch.isfinite(on[0]).all()) and bool(torch.isfinite(on[1]).all())
        # dx sums to zero over an instance up to rounding: a bias gradient of a few ulps of the summed magnitudes
        assert float(on[1].abs().max()) <= 1e-3 * float(on[0].abs().sum(dim=(0, 2)).max())


def pick_splits(NC, S):
    """norm_act.hip pick_splits: partial sums per instance."""
    return max(1, min(-(-2048 // NC), -(-S // 8192), 64))


@pytest.mark.parametrize('N,C,Sv,splits,rounds', [(1, 8, 40 * 40 * 40, 8, 0), (1, 8, 100003, 13, 0), (1, 1, 2200003, 64, 2)])
def test_fp32_backward_partial_sums_in_rounds_of_eight(N, C, Sv, splits, rounds, switches):
    """The apply pass loads the sums pass's partials eight at a time and adds them in the order 0 .. splits - 1: that loop runs from eight partials
    on, i.e. from 57 345 voxels.  40^3: exactly one round of eight.  100 003 voxels (odd: the plain statistics kernel too): 13 partials, one round
    and a plain remainder of five.  2 200 003 voxels in one instance: 64 partials, and the only shape here at which a thread of the apply pass
    (grid capped at 1024 workgroups, 8.4 iterations per thread) REFILLS its four loads for a second round.  dx, the bias gradient and the
    workspace with its fp64 partial and row sums: the same bytes with the switch on and off."""
    L = switches
    assert pick_splits(N * C, Sv) == splits
    bx = min(-(-Sv // 1024), 1024)
    assert Sv // (4 * bx * 256) == rounds  # full rounds of four iterations that every thread of the apply pass runs
    g = torch.Generator(device=DEV).manual_seed(80)
    x = torch.randn(N, C, Sv, device=DEV, generator=g) * 2 + 0.5
    dy = torch.randn(N, C, Sv, device=DEV, generator=g)
    mean, rstd = stats(x, N * C, Sv)
    nb = int(L.nc_instnorm_bwd_dbias_ws_bytes(I(N * C), LG(Sv)))

    def one():
        ws = torch.full((nb,), WS_SENT, dtype=torch.uint8, device=DEV)
        dx = torch.full_like(x, 7.0)
        db = torch.full((C,), float('nan'), device=DEV)
        ck(L.nc_instnorm_act_bwd_dbias(P(dy), P(x), P(mean), P(rstd), FL(0.2), P(dx), P(db), I(N), I(C), LG(Sv), P(ws), Z(nb), stream()),
           'nc_instnorm_act_bwd_dbias')
        torch.cuda.synchronize()
        return [dx, db, ws]
    off, on = on_off(L, one)
    print('fp32', N, C, Sv, 'splits', splits, 'dbias[0] %.6g' % float(on[1][0]))
    same_bytes(off, on, 'nc_instnorm_act_bwd_dbias S = %d' % Sv)
    assert bool(torch.isfinite(on[0]).all()) and bool(torch.isfinite(on[1]).all())
    # the means the apply pass took from the partials are those of the tensor: dx against the formula in fp64, to fp32 rounding of its terms
    xh = (x.double() - mean.double().view(N, C, 1)) * rstd.double().view(N, C, 1)
    gg = torch.where(xh > 0, dy.double(), dy.double() * float(torch.tensor(0.2, dtype=torch.float32)))
    ref = rstd.double().view(N, C, 1) * (gg - gg.mean(2, keepdim=True) - xh * (gg * xh).mean(2, keepdim=True))
    scale = float(ref.abs().max())
    # (three fp32 roundings of terms up to |g| + |xhat mean(g xhat)| <= a few times max|dx| / rstd: 1e-5 of the largest element is an order above that)
    assert float((on[0].double() - ref).abs().max()) <= 1e-5 * scale


@pytest.mark.parametrize('form', ['c8', 's3'])
def test_sums_pass_of_the_16_bit_and_three_term_forms(form, switches):
    """nc_instnorm_act_bwd_c8 and nc_instnorm_act_bwd_dbias_s3 share the fp32 sums pass (k_in_bwd_sums, eight iterations in flight with the
    switch on); their apply passes are not changed.  2 x 16 instances of 17 x 18 x 20: every output and the workspace, on against off."""
    L = switches
    N, C, Sv = 2, 16, 17 * 18 * 20
    g = torch.Generator(device=DEV).manual_seed(81)
    x = torch.randn(N, C, Sv, device=DEV, generator=g) * 2 + 0.5
    dy = torch.randn(N, C, Sv, device=DEV, generator=g)
    mean, rstd = stats(x, N * C, Sv)
    nb = int(L.nc_instnorm_bwd_dbias_ws_bytes(I(N * C), LG(Sv)))

    def one():
        ws = torch.full((nb,), WS_SENT, dtype=torch.uint8, device=DEV)
        db = torch.full((C,), float('nan'), device=DEV)
        if form == 'c8':
            dx = torch.full_like(x, 7.0)
            dxh = torch.full((N * C * Sv * 2,), 0xA5, dtype=torch.uint8, device=DEV)
            ck(L.nc_instnorm_act_bwd_c8(P(dy), P(x), P(mean), P(rstd), FL(0.2), P(dx), P(dxh), P(db), I(N), I(C), LG(Sv), I(1), P(ws), Z(nb),
                                        stream()), 'nc_instnorm_act_bwd_c8')  # (1: NC_DT_F16)
            outs = [dx, dxh, db, ws]
        else:
            dxs = torch.full((int(L.nc_s3_bytes(I(N), I(C), LG(Sv))),), 0xA5, dtype=torch.uint8, device=DEV)
            ck(L.nc_instnorm_act_bwd_dbias_s3(P(dy), P(x), P(mean), P(rstd), FL(0.2), P(dxs), P(db), I(N), I(C), LG(Sv), P(ws), Z(nb), stream()),
               'nc_instnorm_act_bwd_dbias_s3')
            outs = [dxs, db, ws]
        torch.cuda.synchronize()
        return outs
    off, on = on_off(L, one)
    same_bytes(off, on, form)
    assert bool(torch.isfinite(on[-2]).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the batched weight preparation
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [False, True])
def test_batched_pack_and_cells(bad, switches):
    """Block 2 (64 -> 128) and block 9 (128 -> 64, a concatenation whose halves have different powers of two), forward and data-gradient form: the
    pack and the weight cell the batched pass left in `saved` with the switch on equal those with it off, and both equal what the per-layer
    preparation (nc_s3x_pack_h2_debug: k_absmax_w + k_pack_w_s3x<2>) writes from the same weights and input cells.  bad: a NaN and an infinity
    among the weights of both blocks (a cell ignores them, the pack stores what the split makes of them)."""
    L = switches
    shape = (24, 24, 24)
    sd, x, r = net_data(shape, 1)
    sd['t_conv1.weight'] = sd['t_conv1.weight'] * 16.0  # (a bound well away from the InstanceNorm bound of the other half)
    if bad:
        for blk in (2, 9):
            w = sd[BLOCKS[blk][0] + '.weight']
            poison(w, 5 * 27 + 3, w.numel() - 2)
    vox = [shape[0] * shape[1] * shape[2] >> (3 * l) for l in range(3)]
    L.nc_set_unet_wprep(1)
    saved = {}
    for on in (0, 1):
        L.nc_set_stream_passes(on)
        net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0])
        net.load_state_dict(sd)
        y = net(x.clone().requires_grad_(True))
        assert int(y.grad_fn.kept) & WPREP_BIT
        torch.cuda.synchronize()
        saved[on] = y.grad_fn.saved_tensors[2].view(torch.uint8).clone()
        del y, net

    def word(buf, off):
        return int(buf[off:off + 4].view(torch.int32).item()) & 0xffffffff

    def dev_word(bits):
        return torch.tensor([bits if bits < 2 ** 31 else bits - 2 ** 32], dtype=torch.int32, device=DEV)
    zs = ctypes.c_size_t
    for blk in (2, 9):
        key, C, K, lvl = BLOCKS[blk]
        w = sd[key + '.weight'].contiguous()
        a_bits = int(np.sqrt(np.float32(vox[lvl])).view(np.uint32))
        for form in (0, 1):
            po, pb, co, bo = zs(0), zs(0), zs(0), zs(0)
            assert L.nc_unet_wprep_layout(1, *shape, blk, form, ctypes.byref(po), ctypes.byref(pb), ctypes.byref(co), ctypes.byref(bo)) == 0
            b_bits = word(saved[0], bo.value) if blk == 9 else a_bits
            if blk == 9:
                assert b_bits >> 23 != a_bits >> 23 and word(saved[1], bo.value) == b_bits
            wp = torch.full((pb.value,), 0xa5, dtype=torch.uint8, device=DEV)
            wc = torch.full((1,), -1, dtype=torch.int32, device=DEV)
            ca, cb = dev_word(a_bits), dev_word(b_bits)
            assert L.nc_s3x_pack_h2_debug(P(w), C, K, form, P(ca), P(cb), P(wp), P(wc), None) == 0
            torch.cuda.synchronize()
            cell = int(wc.item()) & 0xffffffff
            print('block %d form %d: cell %#x, %d bytes' % (blk, form, cell, pb.value))
            assert 0 < cell < 0x7f800000
            for on in (0, 1):
                assert word(saved[on], co.value) == cell, (blk, form, on)
                assert torch.equal(saved[on][po.value:po.value + pb.value], wp), (blk, form, on)
