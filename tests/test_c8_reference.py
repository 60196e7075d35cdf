"""CPU: tests/c8_reference.py (layout, float64 references, the 16-bit criterion, cases, refusals of tests/test_gpu_c8_ops.py) is itself held to
torch's float64 operators; the criterion accepts an fp32 evaluation rounded once to nearest even at every case and rejects a truncating
conversion, one element moved by one ulp, two exchanged 8-channel units, the pool gradient at the last maximum and permuted taps; the case
tables reach what their comments say."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c8_reference as R  # noqa: E402

BIG = 1 << 23   # cases with more elements than this are evaluated on the GPU only (tests/test_gpu_c8_ops.py); here their reach is asserted


def close(a, r, tol=1e-12):
    assert a.shape == r.shape and a.dtype == torch.float64, (a.shape, r.shape, a.dtype)
    assert float((a - r).abs().max()) <= tol * max(float(r.abs().max()), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_layout_round_trips_and_addresses_channel_ranges():
    x = torch.arange(2 * 24 * 3 * 5, dtype=torch.float32).reshape(2, 24, 3, 5)
    h = R.pack(x)
    assert h.shape == (2, 3, 15, 8)
    assert h[1, 2, 7, 5] == x[1, 2 * 8 + 5].reshape(-1)[7]
    assert torch.equal(R.unpack(h, x.shape), x)
    buf = torch.full((2, 5, 15, 8), -1.0)
    R.pack_into(buf, x, 8)
    assert torch.equal(R.unpack(R.view(buf, 8, 24), x.shape), x)
    assert bool((buf[:, 0] == -1).all()) and bool((buf[:, 4] == -1).all())
    v = torch.arange(2 * 8 * 4 * 2 * 6, dtype=torch.float32).reshape(2, 8, 4, 2, 6)
    w = R.windows(v)
    assert w.shape == (2, 8, 2, 1, 3, 8) and w[1, 3, 1, 0, 2].tolist() == [float(v[1, 3, 2 + a, b, 4 + c]) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    assert torch.equal(R.unwindows(w), v)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the references against torch's float64 operators
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slope', [0.0, 0.2])
def test_norm_references_are_the_float64_operators(slope):
    g = torch.Generator().manual_seed(5)
    x = (1.7 * torch.randn(2, 8, 301, generator=g) + 0.6).to(torch.bfloat16)
    gy = torch.randn(2, 8, 301, generator=g).to(torch.bfloat16)
    mean, var, rstd = R.ref_stats(x)
    xa = x.double().requires_grad_(True)
    ya = F.leaky_relu(F.instance_norm(xa, eps=R.EPS), R.f32(slope))
    close(mean, x.double().mean(-1))
    close(var, x.double().var(-1, unbiased=False))
    y, e = R.ref_norm_act(x, mean, rstd, slope)      # float64 statistics: the operator itself
    close(y, ya.detach(), 1e-11)
    assert float(e.min()) > 0
    dx, e = R.ref_norm_bwd(gy, x, mean, rstd, slope)
    (dxa,) = torch.autograd.grad(ya, xa, gy.double())
    close(dx, dxa, 1e-10)
    assert float(e.min()) > 0
    assert float(dx.sum(-1).abs().max()) <= 1e-10     # an instance's dx sums to zero


@pytest.mark.parametrize('kind', ['ties', 'planted', None])
def test_pool_references_are_the_float64_operators(kind):
    name, N, C, dims, _, _, _ = [c for c in R.POOL_CASES if c[6] == kind][0]
    x, dp, skip = R.pool_inputs(N, C, dims, kind, R.BF)
    y, arg = R.ref_pool(x)
    ty, tidx = F.max_pool3d(x.double(), 2, return_indices=True)
    assert torch.equal(torch.nan_to_num(y.double(), nan=7.0), torch.nan_to_num(ty, nan=7.0))
    D, H, W = dims
    od, oh, ow = torch.meshgrid(torch.arange(D // 2), torch.arange(H // 2), torch.arange(W // 2), indexing='ij')
    flat = ((2 * od + (arg >> 2)) * H + 2 * oh + ((arg >> 1) & 1)) * W + 2 * ow + (arg & 1)
    assert torch.equal(flat, tidx)
    if kind == 'planted':
        for (a, b, c), t in R.PLANTED_ARGS.items():
            assert bool((arg[0, :, a, b, c] == t).all()), (a, b, c)
        assert bool(torch.isneginf(y[0, :, 0, 1, 1].float()).all())                                  # eight -inf: -inf
        assert bool((y[0, :, 1, 0, 0].view(torch.int16) == 0).all())                                 # +0.0 first
        assert bool((y[0, :, 1, 0, 1].view(torch.int16) == -32768).all())                            # -0.0 first: its bits
        return
    xa = x.double().requires_grad_(True)
    (ga,) = torch.autograd.grad(F.max_pool3d(xa, 2), xa, dp.double())
    dx, e = R.ref_pool_bwd_add(dp, arg, skip)
    close(dx, ga + skip.double())
    assert float(e.min()) >= 0


def test_head_and_convt_references_are_the_float64_operators():
    x, w, b, g = R.head_inputs(2, 255, R.BF)
    xa, wa, ba = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    out = F.conv1d(xa, wa.view(1, 64, 1), ba).squeeze(1)
    ref, e = R.ref_dot64(x, w, b)
    close(ref, out.detach())
    close(R.ref_dot64(x, w, None)[0], out.detach() - b.double())
    dxa, dwa, dba = torch.autograd.grad(out, (xa, wa, ba), g.double())
    dx, e, dw, db = R.ref_outer64(g, x, w)
    close(dx, dxa), close(dw, dwa), close(db, dba)
    xc, wc, bc, dyc = R.convt_inputs(1, 32, 32, (2, 3, 2))
    xa, wa, ba = xc.double().requires_grad_(True), wc.double().requires_grad_(True), bc.double().requires_grad_(True)
    ya = F.conv_transpose3d(xa, wa, ba, stride=2)
    close(R.ref_convt_fwd(xc, wc, bc)[0], ya.detach())
    (dxa,) = torch.autograd.grad(ya, xa, dyc.double())
    close(R.ref_convt_dgrad(dyc, wc)[0], dxa)
    assert torch.equal(R.taps_permuted(R.taps_permuted(R.taps_permuted(ya.detach()))), ya.detach())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the criterion
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_ulp_and_classes():
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, 0.0, 2.0 ** -14, 2.0 ** -20, 65504.0, 2.0 ** -126, 2.0 ** -130], dtype=torch.float64)
    assert R.ulp16(v, R.FP).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 32.0, 2.0 ** -24,
                                         2.0 ** -24]
    assert R.ulp16(v, R.BF).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133, 2.0 ** -21, 2.0 ** -27, 2.0 ** 8, 2.0 ** -133,
                                         2.0 ** -133]
    for dt in R.DTS:  # the spacing is the distance to the next representable value
        h = torch.tensor([1.0, 3.0, 0.01, 100.0]).to(R.tdt(dt))
        nxt = R.one_ulp_moved(R.one_ulp_moved(R.one_ulp_moved(R.one_ulp_moved(h, 0), 1), 2), 3)
        assert torch.equal(nxt.double() - h.double(), R.ulp16(h.double(), dt))
    inf, nan = math.inf, math.nan
    ref = torch.tensor([inf, -inf, nan, 1.0, inf, nan, 1.0], dtype=torch.float64)
    got = torch.tensor([inf, -inf, nan, 1.0, -inf, 1.0, nan]).to(torch.bfloat16)
    assert R.half_ulp_excess(got, ref, 0.0, R.BF).tolist() == [0.0, 0.0, 0.0, 0.0, inf, inf, inf]
    # half an ulp exactly is inside, anything more needs e
    ref = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=torch.float64)
    got = torch.tensor([1.0, 1.0]).to(torch.bfloat16)
    assert R.half_ulp_excess(got, ref, 2.0 ** -19, R.BF).tolist() == [0.0, 0.5]
    assert R.within_half_ulp(got, ref, 2.0 ** -21, R.BF) == (False, 2.0)


def _mutants(h, dt, v32, swap=True):
    """(name, tensor): what the criterion must reject, from the accepted 16-bit tensor h [N, C, S] and the fp32 values it was rounded from"""
    out = [('truncated', R.truncated(v32, dt))]
    k = int(h.float().abs().reshape(-1).argmax())
    out.append(('one ulp', R.one_ulp_moved(h, k)))
    if swap and h.shape[-1] >= 2:
        out.append(('units swapped', R.unpack(R.units_swapped(R.pack(h), 0, 0, 0), h.shape)))
    return out


def _judge(what, dt, v32, ref, e, reject=True, tight=False):
    """accept the fp32 result rounded to nearest even with excess <= 0.5; reject its mutants.  tight: e is the bound of ONE fp32 rounding (the
    outer product, the pool's add), which is attained: over many elements the largest excess approaches 1, and 1 is what is asked."""
    h = v32.to(R.tdt(dt))
    ok, ex = R.within_half_ulp(h, ref, e, dt)
    print('%-44s %s accepted, excess %.3f' % (what, R.dt_name(dt), ex))
    assert ok and ex <= (1.0 if tight else 0.5), (what, ex)
    if not reject:
        return
    for name, m in _mutants(h, dt, v32):
        if name == 'truncated' and int((h.float() != v32).sum()) <= 64:
            continue   # (a handful of sums of two bf16 values: all exact, or ties, where both roundings sit at half an ulp)
        ok, ex = R.within_half_ulp(m, ref, e, dt)
        beyond = float((R.half_ulp_excess(m, ref, 0.0, dt) > 0).double().mean())
        print('%-44s %s %-14s excess %.3g, %.1f %% of the elements beyond half an ulp' % (what, R.dt_name(dt), name, ex, 100 * beyond))
        assert not ok, (what, name)


SMALL_NORM = [c for c in R.NORM_CASES if c[1] * c[2] * c[3] <= BIG]
SMALL_CONVT = [c for c in R.CONVT_CASES if c[0] * c[2] * 8 * math.prod(c[3]) <= BIG]


def test_only_the_two_largest_cases_are_left_to_the_gpu():
    assert [c[0] for c in R.NORM_CASES if c not in SMALL_NORM] == ['clamp'] and [c[:4] for c in R.CONVT_CASES if c not in SMALL_CONVT] == [(1, 32, 256, (17, 40, 50))]


@pytest.mark.parametrize('case', SMALL_NORM, ids=[c[0] for c in SMALL_NORM])
def test_criterion_on_the_norm_cases(case):
    name, N, C, S, ctot, c0, slope, dts, kind = case
    for dt in dts:
        x, g = R.norm_inputs(N, C, S, kind, dt)
        mean, rstd = R.stats32(x)
        om, orr = R.oracle_stats(x)
        m64, _, r64 = R.ref_stats(x)
        assert R.CR.within(R.CR.err(om, m64), R.CR.err(om, m64)) and math.isfinite(R.CR.err(orr, r64)[0])
        degenerate = S == 1                                   # y = 0 and dx = 0 everywhere: nothing to truncate or to move
        y, e = R.ref_norm_act(x, mean, rstd, slope)
        _judge('%s normalise' % name, dt, R.emu_norm_act(x, mean, rstd, slope), y, e, reject=not degenerate)
        dx, e = R.ref_norm_bwd(g, x, mean, rstd, slope)
        _judge('%s backward' % name, R.BF, R.emu_norm_bwd(g, x, mean, rstd, slope), dx, e, reject=not degenerate)
        lim = R.dbias_limit(dx)
        db = R.emu_norm_bwd(g, x, mean, rstd, slope).sum((0, 2)).double()
        assert bool((db.abs() <= lim).all()) or degenerate


@pytest.mark.parametrize('case', R.POOL_CASES, ids=[c[0] for c in R.POOL_CASES])
def test_criterion_on_the_pool_backward(case):
    name, N, C, dims, ctot, c0, kind = case
    x, dp, skip = R.pool_inputs(N, C, dims, kind, R.BF)
    _, arg = R.ref_pool(x)
    dx, e = R.ref_pool_bwd_add(dp, arg, skip)
    flat = lambda t: t.reshape(N, C, -1)  # noqa: E731
    gw = torch.zeros(arg.shape + (8,)).scatter_(-1, arg.unsqueeze(-1), dp.float().unsqueeze(-1))
    _judge('%s pool backward' % name, R.BF, flat(skip.float() + R.unwindows(gw)), flat(dx), flat(e), tight=True)
    if kind == 'ties':  # the gradient at the LAST maximum is another tensor, and the criterion says so
        _, last = R.ref_pool(x, last=True)
        assert bool((last != arg).any())
        gl = torch.zeros(arg.shape + (8,)).scatter_(-1, last.unsqueeze(-1), dp.float().unsqueeze(-1))
        assert not R.within_half_ulp((skip.float() + R.unwindows(gl)).to(torch.bfloat16), dx, e, R.BF)[0]


@pytest.mark.parametrize('case', R.HEAD_CASES, ids=[R.case_id(c) for c in R.HEAD_CASES])
def test_criterion_on_the_head(case):
    N, S, _ = case
    for dt in R.DTS:
        x, w, b, g = R.head_inputs(N, S, dt)
        for bias in (b, None):
            ref, e = R.ref_dot64(x, w, bias)
            ok, ex = R.bound_excess(R.oracle_dot64(x, w, bias), ref, e)
            assert ok and ex <= 0.5, ex
        dx, e, dw, db = R.ref_outer64(g, x, w)
        _judge('head S = %d dx' % S, R.BF, w.view(1, 64, 1) * g.unsqueeze(1), dx, e, tight=True)
        odw, odb = R.oracle_outer64(g, x)
        assert R.CR.err(odw, dw)[0] < 1e-5 and R.CR.err(odb, db)[0] < 1e-5


@pytest.mark.parametrize('case', SMALL_CONVT, ids=[R.case_id(c[:4]) for c in SMALL_CONVT])
def test_criterion_on_the_transposed_convolution(case):
    N, C, K, n, _ = case
    x, w, b, dy = R.convt_inputs(N, C, K, n)
    for dt in R.DTS:
        xr, wr = x.to(R.tdt(dt)), w.to(R.tdt(dt))
        for bias in (b, None):
            ref, e = R.ref_convt_fwd(xr, wr, bias)
            v32 = F.conv_transpose3d(xr.float(), wr.float(), bias, stride=2)
            flat = lambda t: t.reshape(N, K, -1)  # noqa: E731
            _judge('convT %s fwd bias %d' % (R.case_id(case[:4]), bias is not None), dt, flat(v32), flat(ref), flat(e))
            ok, _ = R.within_half_ulp(R.taps_permuted(v32).to(R.tdt(dt)), ref, e, dt)
            assert not ok
    dyr, wr = dy.to(torch.bfloat16), w.to(torch.bfloat16)
    ref, e = R.ref_convt_dgrad(dyr, wr)
    v32 = F.conv3d(dyr.float(), wr.float(), None, stride=2)
    flat = lambda t: t.reshape(N, C, -1)  # noqa: E731
    _judge('convT %s dgrad' % R.case_id(case[:4]), R.BF, flat(v32), flat(ref), flat(e))
    odw, odb = R.oracle_convt_wgrad(x.to(torch.bfloat16), wr, dyr)
    o = R.CR.err(odw, R.CR.ref_wgrad(x.to(torch.bfloat16), dyr))
    assert math.isfinite(o[0]) and o[0] < 1e-5 and R.CR.err(odb, R.CR.ref_dbias(dyr))[0] < 1e-5


def test_truncation_is_far_outside():
    """the share of the limit a truncating conversion uses (the module text of c8_reference.py quotes it)"""
    x, w, b, _ = R.convt_inputs(1, 96, 64, (3, 4, 5))
    xr, wr = x.to(torch.bfloat16), w.to(torch.bfloat16)
    ref, e = R.ref_convt_fwd(xr, wr, b)
    v32 = F.conv_transpose3d(xr.float(), wr.float(), b, stride=2)
    t = R.truncated(v32, R.BF)
    half = 0.5 * R.ulp16(torch.maximum(t.double().abs(), ref.abs()), R.BF)
    use = ((t.double() - ref).abs() / (half + e)).max().item()
    beyond = float(((t.double() - ref).abs() > half).double().mean())
    print('truncated: %.2f of the limit, %.0f %% beyond half an ulp' % (use, 100 * beyond))
    assert 1.5 < use <= 2.0 and 0.4 < beyond < 0.6


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the cases reach what they say
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_cases_reach_what_they_say():
    by = {c[0]: c for c in R.NORM_CASES}
    S = lambda n: by[n][3]  # noqa: E731
    assert S('S1') == 1
    assert [R.cdiv(S(n), 256) for n in ('S255', 'S256', 'S257')] == [1, 1, 2] and S('S257') % 256 == 1
    assert [R.nbx(S(n)) for n in ('S2047', 'S2048', 'S2049')] == [1, 1, 2] and S('S2049') % 2048 == 1
    assert [R.splits_for(S(n)) for n in ('S16384', 'S16385')] == [1, 2] and R.chain_len(S('S16384')) == 64
    assert R.cdiv(S('clamp'), 256 * 64) == 257 and R.splits_for(S('clamp')) == 256
    assert by['view'][1:3] == (3, 24) and by['view'][4:6] == (40, 8)
    assert {c[6] for c in R.NORM_CASES} == {0.0, 0.2}
    assert by['offset'][7] == (R.FP,) and R.chain_len(S('offset')) == 64
    assert all(N * (C // 8) <= R.GRID_Y_MAX for _, N, C, *_ in R.NORM_CASES)
    f = {c[0]: c[3] for c in R.FUSED_CASES}
    assert f['S300'] <= 2048 and R.cdiv(f['fwd-stride'], 256) > 2048 and R.cdiv(f['bwd-stride'], 1024) > 1024
    assert R.cdiv(f['fwd-stride'] - 300, 256) == 2048 and R.cdiv(f['bwd-stride'] - 300, 1024) == 1024
    p = {c[0]: c for c in R.POOL_CASES}
    so = lambda n: math.prod(d // 2 for d in p[n][3])  # noqa: E731
    assert so('one-window') == 1 and so('view-514') == 514 and R.cdiv(514, 256) == 3 and p['view-514'][4:6] == (40, 16)
    x, _, _ = R.pool_inputs(*p['ties'][1:4], 'ties', R.BF)
    w = R.windows(x).float()
    assert bool(((w == w.max(-1, keepdim=True).values).sum(-1) > 1).any())                       # ties do occur
    c = {k[:4]: k for k in R.CONVT_CASES}
    assert R.convt_fwd_grid(1, 32, 32, (1, 1, 1))[:3] == (1, 1, 1)
    for shape in ((1, 96, 64, (3, 4, 5)), (1, 160, 32, (2, 3, 5)), (1, 320, 32, (2, 2, 9))):
        assert shape in c and R.convt_wgrad_kernel(shape[1]) == 'wgrad_h' and R.convt_dgrad_kernel(shape[1]) == 'dgrad<1>'
    assert sorted(k[1] // 32 for k in R.CONVT_CASES if R.convt_wgrad_kernel(k[1]) == 'wgrad_h') == [3, 5, 10]
    assert R.convt_fwd_lds(320) == 160 * 1024 and R.convt_fwd_lds(352) > 160 * 1024
    assert {R.convt_wgrad_kernel(k[1]) for k in R.CONVT_CASES} == {'wgrad_h', 'wgrad_h2'}
    assert {R.convt_dgrad_kernel(k[1]) for k in R.CONVT_CASES} == {'dgrad<1>', 'dgrad<4>'}
    gx, tiles, walk, partial = R.convt_fwd_grid(1, 32, 256, (17, 40, 50))
    assert (gx, tiles, walk, partial) == (256, 1063, 2, True) and R.cdiv(tiles, 4) > gx
    assert all(R.convt_fwd_grid(*k[:4])[2] == 1 for k in R.CONVT_CASES[:-1])
    assert 2 * 1 * 256 * 8 * 17 * 40 * 50 == 139264000                                              # the largest tensor, bytes
    h = [s for _, s, _ in R.HEAD_CASES]
    assert h == [1, 255, 4096, 4097] and [R.cdiv(s, 256 * 16) for s in h] == [1, 1, 1, 2] and {n for n, _, _ in R.HEAD_CASES} == {1, 2}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_every_base_call_is_valid():
    for op, a in R.BASE.items():
        assert R.EXPECT[op](a) == R.NC_OK, op


@pytest.mark.parametrize('row', R.REFUSALS, ids=[R.refusal_id(r) for r in R.REFUSALS])
def test_refusal_table_agrees_with_the_predicates(row):
    op, what, changed, code = row
    assert code != R.NC_OK and R.EXPECT[op](R.refusal_args(op, changed)) == code


def test_refusal_table_covers_what_it_must():
    what = {(op, w) for op, w, _, _ in R.REFUSALS}
    for op in ('stats', 'apply', 'bwd', 'pool', 'pool_bwd', 'from_c8', 'fused_fwd'):
        assert (op, 'N * C / 8 = 65536') in what
    assert {('dot64', 'N = 65536'), ('outer64', 'N = 65536'), ('convt_fwd', 'C = 352 > 320'), ('convt_fwd', 'out_c0 % 32'),
            ('pool', 'N = 0'), ('pool_bwd', 'N = 0')} <= what
    assert len({R.refusal_id(r) for r in R.REFUSALS}) == len(R.REFUSALS)
