"""The folded InstanceNorm backward of the two-term Unet_deconv training step (nc_set_in_bwd_fold; csrc/norm_act.hip, csrc/gen_nets.hip):

  * the sums pass keeps the loads of four iterations in flight -- the same element sequence and order of additions per thread;
  * the apply pass takes the tensor's bound itself, the guard's words are zeroed with the cells, and the bias sums and the guard's decision are
    one launch: four launches per two-term block instead of six;
  * blocks 1 and 3, whose output feeds a max-pool and a skip connection, form `skip + pool gradient` per element from the winner bytes the
    forward's pool kernel left in `saved`: nc_maxpool2_bwd_add and its tensor are gone.

No stored value and no order of summation changes, so every comparison here is bitwise; the POOL form is also held to the fp64 bounds of
tests/test_gpu_h2_writers.py, through that file's own check.

Two figures of the issue do not fit the code it changes and are asked for at the nearest shapes that do (the reasoning, not a measurement):
the two-term norm backward exists only for instances of more than 2048 voxels (shorter ones take the one-kernel row form, which has none of
these launches), so `16 instances of 8 x 12 x 20` (1920 voxels) is refused by the entry point -- asserted -- and 8 x 14 x 20 (2240 voxels: 8.75
x 256, a chunk that is no multiple of 256 x the unroll and not even of 256) stands in; and at 24^3 only the two full-resolution blocks (13824
voxels; 12^3 = 1728, 6^3 = 216) run it, so a backward call there saves 2 x 2 launches and one pool, and the 18 + 2 of all nine blocks are asserted
at 56^3 (14^3 = 2744 voxels at the lowest level)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_h2_writers as hw  # noqa: E402
from neuroclear_amd import ops  # noqa: E402
from neuroclear_amd._lib import lib  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402
from test_gpu_h2_writers import FL, LG, I, P, Z, cells_of, ck, h2_alloc, stats, stream  # noqa: E402
from test_gpu_unet_lean import _Poison  # noqa: E402

DEV = 'cuda'
POOL_BIT = 1 << 26
ROWS_MAX = 2048  # norm_act.hip kRowsMaxS: instances up to this length take the row kernels
NC_ERR_SHAPE = -1  # include/nc_hip.h


@pytest.fixture
def switches():
    L = lib()
    prev = (L.nc_get_split_terms(), L.nc_get_unet_lean(), L.nc_get_h2_guard(), ops.set_conv_split(True), L.nc_get_unet_wprep(),
            L.nc_get_in_bwd_fold())
    L.nc_set_split_terms(2)
    yield L
    L.nc_set_split_terms(prev[0])
    L.nc_set_unet_lean(prev[1])
    L.nc_set_h2_guard(prev[2])
    ops.set_conv_split(prev[3])
    L.nc_set_unet_wprep(prev[4])
    L.nc_set_in_bwd_fold(prev[5])


def test_switch_round_trip(switches):
    before = switches.nc_get_in_bwd_fold()
    assert switches.nc_set_in_bwd_fold(0) == before and switches.nc_get_in_bwd_fold() == 0
    assert switches.nc_set_in_bwd_fold(1) == 0 and switches.nc_get_in_bwd_fold() == 1


# ---------------------------------------------------------------------------------------------------------------------------------------------
# whole network
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _run(sd, x, r, L, fold_fwd, fold_bwd):
    """One whole-network training forward + backward -> ((y, dx, gradients by name), kept, (norm backward launches, pool backward launches))."""
    net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0])
    net.load_state_dict(sd)
    xi = x.clone().requires_grad_(True)
    L.nc_set_in_bwd_fold(fold_fwd)
    y = net(xi)
    kept = int(y.grad_fn.kept)
    L.nc_set_in_bwd_fold(fold_bwd)
    L.nc_in_bwd_launches(0, 1)
    L.nc_in_bwd_launches(1, 1)
    (y * r).mean().backward()
    torch.cuda.synchronize()
    counts = (L.nc_in_bwd_launches(0, 1), L.nc_in_bwd_launches(1, 1))
    return (y.detach().clone(), xi.grad.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}), kept, counts


def _same(a, b):
    (y0, dx0, g0), (y1, dx1, g1) = a, b
    assert torch.isfinite(y1).all() and torch.isfinite(dx1).all()
    assert torch.equal(y0, y1)
    assert torch.equal(dx0, dx1)
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        assert torch.equal(g0[k], g1[k]), k


def _data(shape, n, seed=5):
    sd = S.state_dict_from_seed(S.unet_deconv_spec(), seed, DEV)
    x = torch.from_numpy(np.random.default_rng(31).random((n, 1) + shape, dtype=np.float32)).to(DEV)
    r = torch.from_numpy(np.random.default_rng(32).standard_normal((n, 1) + shape).astype(np.float32)).to(DEV)
    return sd, x, r


def _expected(shape, n):
    """(two-term norm backwards of blocks 1 .. 9, pools folded) from the shape alone: a level runs the two-term norm backward when its instances
    are longer than the row kernels' limit; block 1's pool sits on level 0, block 3's on level 1."""
    vox = [shape[0] * shape[1] * shape[2] >> (3 * l) for l in range(3)]
    per_level = (2, 4, 3)  # blocks 1, 9 | 2, 3, 7, 8 | 4, 5, 6
    blocks = sum(c for c, v in zip(per_level, vox) if v > ROWS_MAX)
    pools = [l for l in (0, 1) if vox[l] > ROWS_MAX]
    return blocks, len(pools) * n


@pytest.mark.parametrize('wprep', [1, 0])
@pytest.mark.parametrize('lean', [1, 0])
@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('shape', [(24, 24, 24), (40, 24, 32)])
def test_fold_changes_no_bit(shape, n, lean, wprep, switches, monkeypatch):
    """Switch on against off, each on a NaN-filled `saved`: y, dx and every parameter gradient torch.equal; the forward reports the winner bytes
    (kept bit 26) with the switch on only; the backward launched two kernels fewer per two-term norm backward and no nc_maxpool2_bwd_add where
    the pool was folded.  (24^3: a thread of the sums pass has 27 iterations per chunk -- six rounds of four and a tail of three.)"""
    assert networks._FUSED_GEN
    sd, x, r = _data(shape, n)
    _Poison(monkeypatch, shape, n)
    switches.nc_set_unet_lean(lean)
    switches.nc_set_unet_wprep(wprep)
    off, kept_off, c_off = _run(sd, x, r, switches, 0, 0)
    on, kept_on, c_on = _run(sd, x, r, switches, 1, 1)
    blocks, pools = _expected(shape, n)
    print(shape, n, lean, wprep, 'kept: off %#x on %#x; launches (norm bwd, pool bwd): off %s on %s; expected blocks %d pools %d'
          % (kept_off, kept_on, c_off, c_on, blocks, pools))
    assert kept_on & POOL_BIT and not kept_off & POOL_BIT
    assert kept_on & ~POOL_BIT == kept_off
    _same(off, on)
    assert c_off == (6 * blocks, 2 * n) and c_on == (4 * blocks, 2 * n - pools)


@pytest.mark.parametrize('shape,blocks,pools', [((24, 24, 24), 2, 1), ((56, 56, 56), 9, 2)])
def test_launch_count(shape, blocks, pools, switches):
    """Per backward call, counted by the library (nc_in_bwd_launches: no profiler): two launches fewer for the bookkeeping of every two-term norm
    backward and one nc_maxpool2_bwd_add fewer per folded pool -- 18 + 2 when all nine blocks run it (56^3), 4 + 1 at 24^3 (module docstring)."""
    assert (blocks, pools) == _expected(shape, 1)
    sd, x, r = _data(shape, 1)
    off, _, c_off = _run(sd, x, r, switches, 0, 0)
    on, _, c_on = _run(sd, x, r, switches, 1, 1)
    print(shape, 'launches (norm bwd, pool bwd): off %s on %s' % (c_off, c_on))
    assert c_off[0] - c_on[0] == 2 * blocks
    assert c_off[1] - c_on[1] == pools
    if blocks == 9:
        assert c_off[0] - c_on[0] == 18 and c_off[1] - c_on[1] == 2
    _same(off, on)


@pytest.mark.parametrize('n', [1, 2])
def test_guard_that_may_switch_launches_the_parents_path(n, switches, monkeypatch):
    """nc_set_h2_guard(2): the range guard may switch kernels inside the call, so every launch is the parent's -- same counts with the switch on
    and off -- although the forward left the winner bytes; results equal."""
    shape = (40, 24, 32)
    sd, x, r = _data(shape, n)
    _Poison(monkeypatch, shape, n)
    switches.nc_set_h2_guard(2)
    off, kept_off, c_off = _run(sd, x, r, switches, 0, 0)
    on, kept_on, c_on = _run(sd, x, r, switches, 1, 1)
    print('guard 2: launches off %s on %s' % (c_off, c_on))
    assert kept_on & POOL_BIT and not kept_off & POOL_BIT
    assert c_on == c_off and c_off[1] == 2 * n
    _same(off, on)


@pytest.mark.parametrize('fwd,bwd', [(0, 1), (1, 0)])
def test_switch_flips_between_forward_and_backward(fwd, bwd, switches, monkeypatch):
    """`saved` starts as NaN: a backward under the switch after a forward without it must not read winner bytes that were never written (it
    launches the parent's path: the kept bit is clear), and a backward without the switch ignores the bytes."""
    shape = (40, 24, 32)
    sd, x, r = _data(shape, 1)
    poison = _Poison(monkeypatch, shape)
    ref, _, c_ref = _run(sd, x, r, switches, 0, 0)
    got, kept, c = _run(sd, x, r, switches, fwd, bwd)
    tail = poison.saved[-(64 * 20 * 12 * 16 // 4 + 128 * 10 * 6 * 8 // 4):]  # the two regions of winner bytes end `saved` (both multiples of 64 floats)
    assert bool(torch.isnan(tail).all()) == (fwd == 0)
    assert bool(kept & POOL_BIT) == (fwd == 1)
    print('forward %d backward %d: launches %s, parent %s' % (fwd, bwd, c, c_ref))
    # (a backward under the switch still folds its bookkeeping launches, four instead of six; the pool's backward is the parent's in both)
    assert c[1] == c_ref[1] == 2 and c[0] * 6 == c_ref[0] * (4 if bwd else 6)
    _same(ref, got)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------------------------------
def winner_cpu(act):
    """[NC][D][H][W] -> the winner's index per window, the rule of pool_winner in torch on the CPU: the first element in (a, b, c) order that is
    greater than every one before it, a NaN taking over from anything."""
    a = act.cpu()
    NC, D, H, W = a.shape
    w = a.view(NC, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4, 6).reshape(NC, D // 2, H // 2, W // 2, 8)
    best = torch.full(w.shape[:-1], float('-inf'))
    arg = torch.zeros(w.shape[:-1], dtype=torch.uint8)
    for k in range(8):
        v = w[..., k]
        take = (v > best) | torch.isnan(v)
        best = torch.where(take, v, best)
        arg = torch.where(take, torch.full_like(arg, k), arg)
    return arg


def pool_case(N, C, D, H, W, seed, dark=False):
    """Inputs of one block's norm backward behind a pool: raw convolution output x, the activation `act` the pool saw (three pinned windows), the
    concat gradient (2 C channels per sample: the skip half is [:, :C]) and the dense pooled gradient.  dark: the gradient of the first 8-channel
    block is 2^-22 of the rest, so the range guard counts its chunks as low ('dark_channels' of tests/test_gpu_h2.py)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    Sv = D * H * W
    x = torch.randn(N, C, Sv, device=DEV, generator=g) * 2 + 0.5
    act = torch.relu(torch.randn(N * C, D, H, W, device=DEV, generator=g))
    act[0, 0:2, 0:2, 0:2] = 0.75                               # all equal: the first wins
    act[1, 2:4, 2:4, 2:4] = torch.tensor([0.5, 2.0, 0.25, 1.0, 3.0, float('nan'), 9.0, 0.125], device=DEV).view(2, 2, 2)  # a NaN: it wins
    act[2, 0:2, 2:4, 4:6] = torch.tensor([-0.0, 0.0, -0.0, 0.0, 0.0, -0.0, 0.0, -0.0], device=DEV).view(2, 2, 2)          # +-0: the first wins
    dcat = torch.randn(N, 2 * C, Sv, device=DEV, generator=g)
    dcat[:, C:] = 1.0e30                                        # (the other half of the concat gradient: never read)
    gp = torch.randn(N, C, Sv // 8, device=DEV, generator=g)
    if dark:
        dcat[:, :8] *= 2.0 ** -22
        gp[:, :8] *= 2.0 ** -22
    return x, act, dcat, gp


def pool_fwd(act):
    NC, D, H, W = act.shape
    y = torch.full((NC, D // 2, H // 2, W // 2), float('nan'), device=DEV)
    arg = torch.full((NC, D // 2, H // 2, W // 2), 0xA5, dtype=torch.uint8, device=DEV)
    ck(lib().nc_maxpool2_fwd_arg_debug(P(act), P(y), P(arg), I(NC), I(D), I(H), I(W), stream()), 'nc_maxpool2_fwd_arg_debug')
    torch.cuda.synchronize()
    return y, arg


def in_bwd(x, dy, dy_stride, gp, arg, mean, rstd, slope, dims, guard=True, expect=0):
    """nc_instnorm_act_bwd_dbias_h2_pool_debug -> the raw dxs buffer, its cells' byte offset, dbias, the guard words."""
    N, C, Sv = x.shape
    L = lib()
    buf, off = h2_alloc(N, C, Sv, capacity=int(L.nc_s3_bytes(I(N), I(C), LG(Sv))))
    nb = int(L.nc_instnorm_bwd_dbias_ws_bytes(I(N * C), LG(Sv)))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    db = torch.full((C,), float('nan'), device=DEV)
    gw = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) if guard else None
    code = L.nc_instnorm_act_bwd_dbias_h2_pool_debug(P(dy), LG(dy_stride), P(gp), P(arg), P(x), P(mean), P(rstd), FL(slope), P(buf), P(db), I(N),
                                                     I(C), I(dims[0]), I(dims[1]), I(dims[2]), P(ws), Z(nb), P(gw), stream())
    if expect:
        assert code == expect
        return None
    ck(code, 'nc_instnorm_act_bwd_dbias_h2_pool_debug')
    torch.cuda.synchronize()
    return buf, off, db, (gw.clone() if guard else None)


def pool_bwd_add(gp, act, dcat, N, C, dims):
    """nc_maxpool2_bwd_add per sample, as nc_unet_deconv_bwd launches it -> the dense [N][C][S] gradient at the block's output."""
    D, H, W = dims
    Sv = D * H * W
    out = torch.full((N, C, Sv), float('nan'), device=DEV)
    for n in range(N):
        ck(lib().nc_maxpool2_bwd_add(P(gp, n * C * (Sv // 8) * 4), P(act, n * C * Sv * 4), P(dcat, n * 2 * C * Sv * 4), P(out, n * C * Sv * 4), I(C),
                                     I(D), I(H), I(W), stream()), 'nc_maxpool2_bwd_add')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('N,C,dims,slope', [(1, 16, (8, 14, 20), 0.0), (2, 16, (8, 14, 20), 0.2), (1, 8, (18, 12, 28), 0.0)])
def test_pool_form_matches_pool_backward_then_plain_form(N, C, dims, slope, switches):
    """The winner bytes equal the index computed on the CPU; the POOL form then writes the H2 units, cells, bias gradient and guard words that
    nc_maxpool2_bwd_add followed by the plain form writes -- the plain form with the switch off (the parent's six launches) and on."""
    D, H, W = dims
    Sv = D * H * W
    x, act, dcat, gp = pool_case(N, C, D, H, W, 11 + N, dark=N == 2)
    y, arg = pool_fwd(act)
    want = winner_cpu(act)
    assert torch.equal(arg.cpu(), want)
    assert int(want[0, 0, 0, 0]) == 0 and int(want[1, 1, 1, 1]) == 5 and int(want[2, 0, 1, 2]) == 0  # the pinned windows
    ymax = torch.nn.functional.max_pool3d(act.view(N * C, 1, D, H, W), 2).view_as(y)
    assert torch.equal(torch.isnan(y), torch.isnan(ymax)) and torch.equal(torch.nan_to_num(y, 7.0), torch.nan_to_num(ymax, 7.0))
    mean, rstd = stats(x, N * C, Sv)
    dense = pool_bwd_add(gp, act, dcat, N, C, dims)
    assert bool(torch.isfinite(dense).all())
    switches.nc_set_in_bwd_fold(0)
    ref = in_bwd(x, dense, C * Sv, None, None, mean, rstd, slope, dims)
    in_bwd(x, dcat, 2 * C * Sv, gp, arg, mean, rstd, slope, dims, expect=NC_ERR_SHAPE)  # (switch off: the POOL form is refused, nothing runs)
    switches.nc_set_in_bwd_fold(1)
    plain = in_bwd(x, dense, C * Sv, None, None, mean, rstd, slope, dims)
    pool = in_bwd(x, dcat, 2 * C * Sv, gp, arg, mean, rstd, slope, dims)
    cells = cells_of(ref[0], ref[1])
    total = N * C // 8 * ((Sv + 63) // 64)
    print('cells %#x %#x, guard words %s of %d chunks, dbias[0] %.6g' % (cells[0], cells[1], ref[3][:3].tolist(), total, float(ref[2][0])))
    assert cells[0] == cells[1] and 0 < cells[0] < 0x7F800000 and all(c == 0 for c in cells[2:])
    assert int(ref[3][2]) == 0 and all(int(v) == 0 for v in ref[3][3:])  # (inside a whole-network scope mode 1 counts and flags nothing)
    assert (int(ref[3][0]) > 0) == (N == 2)                               # the dark block's chunks were counted as low
    for name, got in (('plain form, switch on', plain), ('POOL form', pool)):
        assert torch.equal(got[0][:ref[1] + 256], ref[0][:ref[1] + 256]), name   # H2 units and the 64 cell words
        assert torch.equal(got[2], ref[2]) and bool(torch.isfinite(got[2]).all()), name
        assert torch.equal(got[3], ref[3]), name


def test_rows_sized_instances_are_refused(switches):
    """8 x 12 x 20 = 1920 voxels: such instances take the row kernels; the two-term norm backward (either form) refuses the shape."""
    N, C, dims = 1, 16, (8, 12, 20)
    Sv = 1920
    assert Sv <= ROWS_MAX
    x, act, dcat, gp = pool_case(N, C, *dims, 3)
    _, arg = pool_fwd(act)
    mean, rstd = stats(x, N * C, Sv)
    in_bwd(x, dcat, 2 * C * Sv, gp, arg, mean, rstd, 0.0, dims, expect=NC_ERR_SHAPE)
    in_bwd(x, dcat, C * Sv, None, None, mean, rstd, 0.0, dims, expect=NC_ERR_SHAPE)


def test_rank_one_form_on_against_off(switches):
    """k_in_bwd_*_h2<true> at 64 x 24^3 (27 iterations per thread and chunk): the same buffer, bias gradient with the switch on and off."""
    C, Sv = 64, 24 ** 3
    g = torch.Generator(device=DEV).manual_seed(77)
    x = torch.randn(1, C, Sv, device=DEV, generator=g) * 2 + 0.5
    dy1 = torch.randn(1, 1, Sv, device=DEV, generator=g)
    w1 = torch.randn(C, device=DEV, generator=g)
    mean, rstd = stats(x, C, Sv)
    res = {}
    for on in (0, 1):
        switches.nc_set_in_bwd_fold(on)
        lib().nc_in_bwd_launches(0, 1)
        res[on] = hw.in_bwd_h2(x, dy1, w1, mean, rstd, 0.0)
        res[on] += (lib().nc_in_bwd_launches(0, 1),)
    off = res[0][1]
    print('rank one: launches off %d on %d' % (res[0][4], res[1][4]))
    assert res[0][4] == 5 and res[1][4] == 4  # (no guard words: no decision to launch)
    assert torch.equal(res[0][0][:off + 256], res[1][0][:off + 256])
    assert torch.equal(res[0][2], res[1][2]) and bool(torch.isfinite(res[1][2]).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# against fp64: tests/test_gpu_h2_writers.py check_in_bwd (its reference, its fp32 kernel, its bounds) with the POOL form as the entry under test
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,C,dims,slope', [(1, 16, (8, 14, 20), 0.0), (2, 16, (8, 14, 20), 0.2), (1, 64, (16, 16, 16), 0.0)])
def test_pool_form_against_fp64(N, C, dims, slope, switches, monkeypatch):
    D, H, W = dims
    Sv = D * H * W
    x, act, dcat, gp = pool_case(N, C, D, H, W, 21 + C)
    _, arg = pool_fwd(act)
    dense = pool_bwd_add(gp, act, dcat, N, C, dims)  # the gradient the reference and the fp32 kernel see

    def entry(x_, dy_arg, w1, mean, rstd, slope_, guard=False):
        assert w1 is None and dy_arg is dcat
        buf, off, db, gw = in_bwd(x_, dcat, 2 * C * Sv, gp, arg, mean, rstd, slope_, dims, guard=guard)
        return buf, off, db, ([int(v) & 0xFFFFFFFF for v in gw.tolist()] if guard else None)
    monkeypatch.setattr(hw, 'in_bwd_h2', entry)
    switches.nc_set_in_bwd_fold(1)
    hw.check_in_bwd(x, dense, dcat, None, slope, 'in_bwd_h2 POOL %s' % ((N, C, dims, slope),))
