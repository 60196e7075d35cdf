"""Three more lean forms of the two-term Unet_deconv training step (nc_set_unet_lean, csrc/gen_nets.hip; `kept` bits 27 .. 31): the forward leaves out
  e1                        one_by_one's flat 1 x 1 kernels normalise raw[9] as they read it (csrc/conv_1x1.hip, the NORM forms),
  the upper halves of cat1 / cat2   the transposed convolutions write the H2 half of block 9 / 7's operand alone,
  the lower halves of cat1 / cat2   blocks 1 / 3 write the H2 half, the fp32 pooled tensor and the winner bytes in one pass (csrc/h2.hip).
No operand and no summation changes, so with the switch on and off y, dx and EVERY parameter gradient are torch.equal -- also where the backward
needs a left-out tensor after all and writes it again (the fallbacks).  `saved` starts as NaN in every run (test_gpu_unet_lean._Poison): a
tensor the forward did not write stays NaN, and a backward that read it could not pass.  The new kernels are also held byte for byte to the
kernels they stand in for, through debug entry points."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_h2_writers as hw  # noqa: E402
import test_gpu_unet_lean as tl  # noqa: E402
from test_gpu_h2_writers import FL, I, LG, P, Z, ck, stream  # noqa: E402
from test_gpu_unet_lean import switches  # noqa: E402,F401  (the fixture: two terms, split kernels on, everything restored)
from neuroclear_amd import ops  # noqa: E402
from neuroclear_amd._lib import lib  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

DEV = 'cuda'
FLAT_MIN = 16384  # csrc/conv_1x1.hip flat_1x1_supported / wgrad_1x1_supported: the flat 1 x 1 kernels take planes of at least this many voxels


def up64(k):
    return (k + 63) // 64 * 64


def slots(n, shape):
    """Element ranges in `saved` of e1 and of the four concat halves, per sample, from u_plan's order (csrc/gen_nets.hip): a1, cat1, p1, a2, cat2,
    p2, b1, b2, b3, e2a, e2b, e1, each rounded up to 64 floats."""
    s0 = shape[0] * shape[1] * shape[2]
    sh, sq = s0 // 8, s0 // 64
    sizes = [('a1', 64 * s0), ('cat1', 128 * s0), ('p1', 64 * sh), ('a2', 128 * sh), ('cat2', 256 * sh), ('p2', 128 * sq), ('b1', 256 * sq),
             ('b2', 256 * sq), ('b3', 256 * sq), ('e2a', 128 * sh), ('e2b', 128 * sh), ('e1', 64 * s0)]
    off, at = 0, {}
    for name, k in sizes:
        at[name] = off
        off += up64(n * k)
    out = {'e1': [(at['e1'], at['e1'] + n * 64 * s0)]}
    for cat, c, sl in (('cat1', 64, s0), ('cat2', 128, sh)):
        out[cat + '_lo'] = [(at[cat] + i * 2 * c * sl, at[cat] + i * 2 * c * sl + c * sl) for i in range(n)]
        out[cat + '_up'] = [(at[cat] + i * 2 * c * sl + c * sl, at[cat] + (i + 1) * 2 * c * sl) for i in range(n)]
    return out


def written(saved, ranges):
    """True / False: all / none of the ranges are written (anything else fails)."""
    nan = torch.cat([torch.isnan(saved[a:b]) for a, b in ranges])
    assert bool(nan.all()) or not bool(nan.any())
    return not bool(nan.any())


def run(sd, x, r, before_bwd=None, poison=None):
    """tl._run with a hook between the two calls; -> (y, dx, gradients by name) and, with poison, which tensors the FORWARD wrote."""
    net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0])
    net.load_state_dict(sd)
    xi = x.clone().requires_grad_(True)
    y = net(xi)
    state = None
    if poison is not None:
        torch.cuda.synchronize()
        sl = slots(x.shape[0], tuple(x.shape[2:]))
        state = {k: written(poison.saved, v) for k, v in sl.items()}
    if before_bwd:
        before_bwd()
    (y * r).mean().backward()
    return (y.detach().clone(), xi.grad.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}), state


def data(n, shape, seed):
    x = torch.from_numpy(np.random.default_rng(seed).random((n, 1) + shape, dtype=np.float32)).to(DEV)
    r = torch.from_numpy(np.random.default_rng(seed + 1).standard_normal((n, 1) + shape).astype(np.float32)).to(DEV)
    return x, r


def assert_same(a, b):
    (y0, dx0, g0), (y1, dx1, g1) = a, b
    assert torch.equal(y0, y1)
    assert torch.equal(dx0, dx1)
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        assert torch.equal(g0[k], g1[k]), k


# 24^3: the 1 x 1 layers stay off the flat kernels (e1 must be written); 40 x 24 x 32: 30720 voxels, a multiple of the 128-voxel chunk;
# 28^3 = 21952 is not: the flat kernels' zero-page columns are normalised too
@pytest.mark.parametrize('n,shape', [(1, (24, 24, 24)), (1, (40, 24, 32)), (1, (28, 28, 28)), (2, (24, 24, 24))])
def test_lean_on_against_off(n, shape, switches, monkeypatch):
    sd = S.state_dict_from_seed(S.unet_deconv_spec(), 5, DEV)
    x, r = data(n, shape, 31)
    poison = tl._Poison(monkeypatch, shape, n)
    res, state = {}, {}
    for lean in (0, 1):
        switches.nc_set_unet_lean(lean)
        res[lean], state[lean] = run(sd, x, r, poison=poison)
    print(n, shape, 'written by the forward: full', state[0], 'lean', state[1])
    assert all(state[0].values())                                   # the full forward writes all five
    flat = shape[0] * shape[1] * shape[2] >= FLAT_MIN
    assert state[1] == {'e1': not flat, 'cat1_lo': False, 'cat1_up': False, 'cat2_lo': False, 'cat2_up': False}
    assert_same(res[0], res[1])


def dark(sd, key):
    w = sd[key].clone()
    w[:, :16] *= 2.0 ** -24
    sd[key] = w


@pytest.mark.parametrize('case', ['fold_off_at_backward', 'guard_block9', 'guard_block7'])
def test_fallbacks_rebuild_the_same_bits(case, switches, monkeypatch):
    """A backward that reads a left-out tensor after all writes it again first; lean against full under the same settings, torch.equal.
    fold_off_at_backward: nc_set_in_bwd_fold(0) between the calls -- the pools' backward runs as a pass of its own and reads its source, the
      lower halves.
    guard_block9 / guard_block7: nc_set_h2_guard(2) and a dY of block 9 / 7 with 16 channels 2^-24 below the rest (the layer behind all but
      ignores them), which the range guard flags: the weight gradient builds its three-term x operand from the fp32 cat1 / cat2."""
    L = switches
    shape = (32, 32, 32)
    sd = S.state_dict_from_seed(S.unet_deconv_spec(), 4, DEV)
    x, r = data(1, shape, 7)
    poison = tl._Poison(monkeypatch, shape)
    fold = L.nc_get_in_bwd_fold()
    out4 = (ctypes.c_ulonglong * 4)()

    def fell():
        torch.cuda.synchronize()
        assert L.nc_h2_guard_stats(out4, 0) == 0
        return int(out4[1])
    try:
        hook = None
        if case == 'fold_off_at_backward':
            hook = lambda: L.nc_set_in_bwd_fold(0)  # noqa: E731
        else:
            dark(sd, 'one_by_one.weight' if case == 'guard_block9' else 'ex_double_conv2.convolution.3.weight')
            L.nc_set_h2_guard(2)
        res, state, nfell = {}, {}, {}
        for lean in (0, 1):
            L.nc_set_unet_lean(lean)
            L.nc_set_in_bwd_fold(1)
            before = fell()
            res[lean], state[lean] = run(sd, x, r, before_bwd=hook, poison=poison)
            nfell[lean] = fell() - before
        print(case, 'calls that fell back to the three-term kernels:', nfell)
        assert all(state[0].values()) and not any(state[1].values())          # (32^3: every form applies)
        if case != 'fold_off_at_backward':
            assert nfell[0] == nfell[1] >= 1
        assert_same(res[0], res[1])
    finally:
        L.nc_set_in_bwd_fold(fold)


def test_switches_moved_between_forward_and_backward(switches, monkeypatch):
    """The split kernels on in the forward and off in the backward, the reverse, and the number of terms 2 -> 3 and 3 -> 2 between the calls: the
    kept H2 copies are of no use to such a backward, which writes the concat halves again (24^3: e1 is written anyway).  Lean against full under
    the same moves: torch.equal; and finite and within 5e-3 (relative L2 of the weight gradients) of the all-fp32 run, on the network and data
    of tests/test_gpu_unet_lean.py::test_lean_forward_then_another_backward, which asks the same of the earlier lean forms."""
    L = switches
    shape = (24, 24, 24)
    torch.manual_seed(21)
    sd = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'normal', 0.02, [0]).state_dict()
    x = torch.rand((1, 1) + shape, device=DEV)
    r = torch.randn((1, 1) + shape, device=DEV)
    tl._Poison(monkeypatch, shape)
    cat = lambda g_: torch.cat([v.reshape(-1) for v in g_.values() if v.dim() > 1]).double()  # noqa: E731
    moves = [('split', a, b, lambda a=a: ops.set_conv_split(a), lambda b=b: ops.set_conv_split(b)) for a, b in ((False, False), (True, False), (False, True))]
    moves += [('terms', a, b, lambda a=a: L.nc_set_split_terms(a), lambda b=b: L.nc_set_split_terms(b)) for a, b in ((2, 3), (3, 2))]
    grads = {}
    for what, a, b, before_fwd, before_bwd in moves:
        res = {}
        for lean in (0, 1):
            L.nc_set_unet_lean(lean)
            before_fwd()
            res[lean], _ = run(sd, x, r, before_bwd=before_bwd)
        ops.set_conv_split(True)
        L.nc_set_split_terms(2)
        assert_same(res[0], res[1])
        grads[(what, a, b)] = cat(res[1][2])
    ref = grads[('split', False, False)]
    for k, v in grads.items():
        assert torch.isfinite(v).all(), k
        d = float((v - ref).norm() / ref.norm())
        print(k, 'relative L2 difference of the weight gradients to the all-fp32 run: %.2e' % d)
        assert d < 5e-3, (k, d)


# ---- kernel level -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['ties', 'every_position'])
@pytest.mark.parametrize('C', [8, 16])
@pytest.mark.parametrize('D,H,W', [(4, 4, 8), (6, 4, 8)])
def test_pool_form_against_act_split2h_and_maxpool(D, H, W, C, kind):
    """k_act_split2h_pool<true> against k_act_split2h (fp32 + H2) followed by the max-pool with winner bytes on that fp32 tensor: the pooled
    values, the winner bytes and the H2 bytes (channels [0, C) of a 2C-channel tensor, as in cat1 / cat2), byte for byte.
    ties: most voxels are zeros behind the ReLU, so most windows hold several equal maxima (+0 and -0 among them) and the first must win;
    every_position: the maximum of window i of channel c sits at position (i + c) % 8."""
    N, Sv = 2, D * H * W
    So = Sv // 8
    g = torch.Generator(device=DEV).manual_seed(D * 100 + C)
    if kind == 'ties':
        x = torch.randn(N, C, D, H, W, device=DEV, generator=g) - 2.0
        x[:, :, 0, 0, 1] = 0.0                                      # +0 behind -0 in one window, in front of it in another
        x[:, :, 1, 1, 2] = 0.0
        mean, rstd = torch.zeros(N * C, device=DEV), torch.full((N * C,), 1.5, device=DEV)
    else:
        x = torch.rand(N, C, D, H, W, device=DEV, generator=g) * 0.5 + 0.1
        win = torch.arange(So, device=DEV).view(1, 1, D // 2, H // 2, W // 2) + torch.arange(C, device=DEV).view(1, C, 1, 1, 1)
        pos = (win % 8).expand(N, C, -1, -1, -1)
        xv = x.view(N, C, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(N, C, D // 2, H // 2, W // 2, 8)
        xv = xv.scatter_add(-1, pos.unsqueeze(-1), torch.ones_like(xv[..., :1]))
        x = xv.view(N, C, D // 2, H // 2, W // 2, 2, 2, 2).permute(0, 1, 2, 5, 3, 6, 4, 7).reshape(N, C, D, H, W)
        mean, rstd = torch.full((N * C,), 0.05, device=DEV), torch.full((N * C,), 0.9, device=DEV)
    x = x.reshape(N, C, Sv).contiguous()
    ctot = 2 * C
    full, off, yflat, ystride = hw.act_split2h(x, mean, rstd, 0.0, N, C, Sv, ctot, 0)
    p_ref = torch.full((N * C * So,), float('nan'), device=DEV)
    a_ref = torch.full((N * C * So,), hw.SENT, dtype=torch.uint8, device=DEV)
    for n in range(N):   # (the fp32 tensor has a gap between its samples: one pool call per sample)
        ck(lib().nc_maxpool2_fwd_arg_debug(P(yflat, n * ystride * 4), P(p_ref, n * C * So * 4), P(a_ref, n * C * So), I(C), I(D), I(H), I(W), stream()),
           'nc_maxpool2_fwd_arg_debug')
    buf, off2 = hw.h2_alloc(N, ctot, Sv)
    p_new = torch.full((N * C * So,), float('nan'), device=DEV)
    a_new = torch.full((N * C * So,), hw.SENT, dtype=torch.uint8, device=DEV)
    ck(lib().nc_act_split2h_pool_arg_debug(P(x), P(mean), P(rstd), FL(0.0), P(buf), P(p_new), P(a_new), I(N), I(C), I(D), I(H), I(W), I(ctot), I(0),
                                           FL(math.sqrt(Sv)), P(buf, off2), stream()), 'nc_act_split2h_pool_arg_debug')
    torch.cuda.synchronize()
    # the inputs are what the docstring says
    y = torch.stack([yflat[n * ystride:n * ystride + C * Sv].view(C, D // 2, 2, H // 2, 2, W // 2, 2) for n in range(N)])
    wins = y.permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(N, C, So, 8)
    if kind == 'ties':
        tied = ((wins == wins.amax(-1, keepdim=True)).sum(-1) > 1).float().mean()
        assert float(tied) > 0.5 and bool(((y == 0) & (y.view(torch.int32) < 0)).any()), float(tied)
    else:
        assert sorted(set(a_ref.tolist())) == list(range(8))
    assert torch.equal(p_new.view(torch.int32), p_ref.view(torch.int32))
    assert torch.equal(a_new, a_ref)
    assert hw.cells_of(buf, off2)[0] == hw.f32_bits(math.sqrt(Sv))
    # (act_split2h was given both cells, the pool form the first one only: the unit bytes are compared, the cells above)
    assert torch.equal(buf[:off2], full[:off])
    assert bool((hw.block_bytes(buf, N, ctot, Sv, C, ctot) == hw.SENT).all())


@pytest.mark.parametrize('slope', [0.0, 0.2])
@pytest.mark.parametrize('dims', [(1, 1, FLAT_MIN + 4), (28, 28, 28)])
def test_normalising_1x1_kernels_against_the_plain_ones(dims, slope):
    """k_flat_1x1<true> / k_wgrad_1x1<true> on raw, mean, rstd against k_in_act_fwd followed by the plain kernels, 64 -> 1: y, dW and db are
    torch.equal.  16388 voxels leave 4 of the last 128-voxel chunk, 21952 leave 64: the other columns come from the zero page and are normalised
    too.  Channel 0 is negative throughout (at slope 0 the operand is -0 everywhere), channel 1 positive throughout."""
    L = lib()
    C, K = 64, 1
    Sv = dims[0] * dims[1] * dims[2]
    g = torch.Generator(device=DEV).manual_seed(Sv)
    mean = torch.randn(C, device=DEV, generator=g) * 0.3
    rstd = torch.rand(C, device=DEV, generator=g) + 0.5
    raw = torch.randn(C, Sv, device=DEV, generator=g) * 1.5 + mean.view(C, 1)
    raw[0] = mean[0] - raw[0].abs() - 0.1
    raw[1] = mean[1] + raw[1].abs() + 0.1
    w = torch.randn(K, C, device=DEV, generator=g) * 0.2
    b = torch.randn(K, device=DEV, generator=g)
    dy = torch.randn(K, Sv, device=DEV, generator=g)
    nb = int(L.nc_conv_ws_bytes(I(1), I(C), I(dims[0]), I(dims[1]), I(dims[2]), I(K), I(1), I(1), I(1), I(1), I(0)))
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=DEV)
    shp = (I(1), I(C), I(dims[0]), I(dims[1]), I(dims[2]), I(K))
    k1 = (I(1), I(1), I(1), I(1), I(0))
    act = torch.empty_like(raw)
    ck(L.nc_instnorm_act_fwd(P(raw), P(mean), P(rstd), FL(slope), P(act), I(C), LG(Sv), stream()), 'nc_instnorm_act_fwd')
    if slope == 0.0:
        assert bool((act[0].view(torch.int32) == -2 ** 31).all()) and bool((act[1] > 0).all())       # -0 throughout / positive throughout
    y0, y1 = torch.full((K, Sv), float('nan'), device=DEV), torch.full((K, Sv), float('nan'), device=DEV)
    ck(L.nc_conv_fwd(P(act), P(w), P(b), P(y0), *shp, *k1, P(ws), Z(ws.numel()), stream()), 'nc_conv_fwd')
    ck(L.nc_conv_fwd_norm_1x1_debug(P(raw), P(mean), P(rstd), FL(slope), P(w), P(b), P(y1), *shp, P(ws), Z(ws.numel()), stream()),
       'nc_conv_fwd_norm_1x1_debug')
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))
    dw0, db0, dw1, db1 = (torch.full(s_, float('nan'), device=DEV) for s_ in ((K, C), (K,), (K, C), (K,)))
    ck(L.nc_conv_wgrad(P(act), P(dy), P(dw0), P(db0), *shp, *k1, P(ws), Z(ws.numel()), stream()), 'nc_conv_wgrad')
    ck(L.nc_conv_wgrad_norm_1x1_debug(P(raw), P(mean), P(rstd), FL(slope), P(dy), P(dw1), P(db1), *shp, P(ws), Z(ws.numel()), stream()),
       'nc_conv_wgrad_norm_1x1_debug')
    assert torch.isfinite(dw1).all()
    assert torch.equal(dw0.view(torch.int32), dw1.view(torch.int32))
    assert torch.equal(db0.view(torch.int32), db1.view(torch.int32))
    # the plain calls really ran on the flat kernels (else the comparison is not the one the training step relies on)
    k7 = (I(C), I(K), I(1), I(1), I(1), I(1), I(0))
    assert L.nc_conv_fwd_path(*k7) == 3 and L.nc_conv_wgrad_path(*k7) == 3
