"""InstanceNorm (long path), BatchNorm, the one-pass inference tail, MaxPool(2) and slice / MIP, op level: every dispatch branch of csrc/norm_act.hip
that tests/test_gpu_ops.py does not reach -- more than one split (chunk_range's round-up to 4, the clamp to 64 splits, want < cap, the combination
of the partial sums), the 16-byte and the scalar loads, the unaligned fallback, grid-stride loops that wrap, the NC > 65535 recursion -- against
float64, and the max kernels on inputs WITH ties and NaN against a first-maximum scan.

The entry points are called through the C ABI directly.  References, limits, cases and the reasoning behind them: tests/norm_reference.py (checked
on the CPU by tests/test_norm_reference.py).  The limits are derived from the kernels' fp32 rounding points, not measured; the module prints the
share of its limit every result uses and, at its end, the worst share per kernel.  Outputs are pre-filled with NaN between NaN guard words: an
element that is not written, or one written outside the tensor, fails.

Worst share of the limit per kernel on an MI355X (max, rms; 1.0 = at the limit): WORST_MEASURED below; the module takes 2 s of GPU-side wall time."""
import ctypes
import math
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_reference as R  # noqa: E402

DEV = 'cuda'
NC_ERR_SHAPE, NC_ERR_WS, NC_ERR_ARG = -1, -2, -4
GUARD = 4            # floats of NaN in front of and behind every output (16 bytes: the tensor keeps its alignment)
WORST = {}
T0 = [None]

# measured on an MI355X (the table this module prints): kernel, quantity, max, rms
WORST_MEASURED = """
  k_bn_act_fwd                       max 0.336  rms 0.064
  k_bn_bwd_apply evaluation          max 0.623  rms 0.163
  k_bn_bwd_apply training            max 0.899  rms 0.205
  k_bn_bwd_sums + k_bn_bwd_finalize  max 0.453  rms 0.348
  k_bn_running                       max 0.394  rms 0.242
  k_in_act_fwd float4                max 0.444  rms 0.082
  k_in_act_fwd float4, NC > 65535    max 0.459  rms 0.086
  k_in_act_fwd scalar                max 0.399  rms 0.083
  k_in_act_tail                      max 0.401  rms 0.085
  k_in_bwd_apply, NC > 65535         max 0.902  rms 0.165
  k_in_bwd_sums + k_in_bwd_apply     max 0.926  rms 0.204
  k_in_dbias_final                   max 0.355  rms 0.355
  k_in_dbias_final (its own dx)      max 0.956  rms 0.703
  k_in_stats + k_bn_finalize         max 0.416  rms 0.305
  k_in_stats float4                  max 0.499  rms 0.449
  k_in_stats float4, NC > 65535      max 0.500  rms 0.223
  k_in_stats scalar                  max 0.377  rms 0.377
"""


def L():
    from neuroclear_amd._lib import lib
    return lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(code, what):
    assert code == 0, (what, code, L().nc_last_error())


@pytest.fixture(scope='module', autouse=True)
def _worst_table():
    T0[0] = time.time()
    yield
    torch.cuda.synchronize()
    print('\nworst share of the limit per kernel (max, rms; 1.0 = at the limit)')
    for k in sorted(WORST):
        print('  %-34s max %.3f  rms %.3f' % (k, WORST[k][0], WORST[k][1]))
    print('module wall time %.1f s' % (time.time() - T0[0]))


def judge(kernel, what, sh):
    """sh: (max, rms) share of the limit (norm_reference.share)"""
    print('%-34s %-58s of the limit: max %.3f rms %.3f' % (kernel, what, sh[0], sh[1]))
    w = WORST.get(kernel, (0.0, 0.0))
    WORST[kernel] = (max(w[0], sh[0]), max(w[1], sh[1]))
    assert sh[0] <= 1.0, (kernel, what, sh)


class Out:
    """a NaN-filled fp32 output of n elements between NaN guards; off = 1: one float off a 16-byte boundary"""

    def __init__(self, n, off=0):
        self.whole = torch.full((n + 2 * GUARD + off,), math.nan, device=DEV)
        self.t = self.whole[GUARD + off:GUARD + off + n]
        self.lo, self.hi = self.whole[:GUARD + off], self.whole[GUARD + off + n:]
        assert self.t.data_ptr() % 16 == 4 * off

    def intact(self):
        return bool(torch.isnan(self.lo).all()) and bool(torch.isnan(self.hi).all())

    def untouched(self):
        return bool(torch.isnan(self.whole).all())


def place(t, off=0):
    """t on the device, contiguous, at an address off floats from a 16-byte boundary"""
    whole = torch.empty(t.numel() + 4, device=DEV)
    v = whole[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def workspace(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=DEV)


def test_the_reference_on_the_gpu_is_the_reference_on_the_cpu():
    """the float64 references below run on the device (torch's own fp64 kernels): the same numbers as on the CPU, where tests/test_norm_reference.py
    holds them to autograd"""
    N, C, S, kind, _ = R.IN_CASES[2]
    x, dy, _ = R.in_inputs(N, C, S, kind)
    st = R.stats64(x)
    m, r = st[0].float(), st[2].float()
    on = lambda f, *a: f(*(t.to(DEV) if torch.is_tensor(t) else t for t in a))  # noqa: E731
    for a, b in zip(on(R.stats64, x), st):
        assert float((a.cpu() - b).abs().max()) <= 1e-12 * float(b.abs().max())
    for a, b in zip(on(R.in_bwd, dy, x, m, r, 0.2)[:2] + on(R.in_fwd, x, m, r, 0.2), R.in_bwd(dy, x, m, r, 0.2)[:2] + R.in_fwd(x, m, r, 0.2)):
        assert float((a.cpu() - b).abs().max()) <= 1e-12 * float(b.abs().max())
    x, dy, gamma, beta, rm, rv = R.bn_inputs(*R.BN_CASES[0])
    st = R.stats64(x, (0, 2))
    a = on(R.bn_bwd, dy, x, st[0].float(), st[2].float(), gamma, beta, 0.2, True)
    b = R.bn_bwd(dy, x, st[0].float(), st[2].float(), gamma, beta, 0.2, True)
    for p, q in ((a[0], b[0]), (a[1], b[1]), (a[3][0], b[3][0]), (a[4][0], b[4][0])):
        assert float((p.cpu() - q).abs().max()) <= 1e-12 * float(q.abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# InstanceNorm, long path
# ---------------------------------------------------------------------------------------------------------------------------------------------
def in_ws(NC, S):
    nb = int(L().nc_instnorm_bwd_dbias_ws_bytes(NC, S))
    base = int(L().nc_instnorm_ws_bytes(NC, S))
    assert base == NC * 64 * 2 * 8 and nb == base + NC * min(-(-S // 1024), 1024) * 8     # the long path's sizes: 64 splits, one partial per block
    return workspace(nb), nb


def in_stats(x, NC, S, ws, nb, off=0):
    m, r = Out(NC, off), Out(NC, off)
    ok(L().nc_instnorm_stats(P(x), NC, S, R.EPS, P(m.t), P(r.t), P(ws), nb, stream()), 'nc_instnorm_stats')
    assert m.intact() and r.intact()
    return m.t, r.t


def in_fwd_both(x, m0, r0, slope, NC, S, ws, nb, off=0):
    """nc_instnorm_fwd (statistics and output) and nc_instnorm_act_fwd (statistics given): bit-equal statistics and outputs"""
    m1, r1, y1, y2 = Out(NC, off), Out(NC, off), Out(NC * S, off), Out(NC * S, off)
    ok(L().nc_instnorm_fwd(P(x), R.EPS, slope, P(m1.t), P(r1.t), P(y1.t), NC, S, P(ws), nb, stream()), 'nc_instnorm_fwd')
    ok(L().nc_instnorm_act_fwd(P(x), P(m0), P(r0), slope, P(y2.t), NC, S, stream()), 'nc_instnorm_act_fwd')
    assert all(o.intact() for o in (m1, r1, y1, y2))
    assert torch.equal(m0, m1.t) and torch.equal(r0, r1.t) and torch.equal(y1.t, y2.t)
    assert not bool(torch.isnan(y1.t).any())
    return y1.t.view(NC, S)


def act_fwd(x, m, r, slope, NC, S, yoff):
    y = Out(NC * S, yoff)
    ok(L().nc_instnorm_act_fwd(P(x), P(m), P(r), slope, P(y.t), NC, S, stream()), 'nc_instnorm_act_fwd')
    assert y.intact()
    return y.t.view(NC, S)


def in_bwd_both(dy, x, m, r, slope, N, C, S, ws, nb, off=0):
    """nc_instnorm_act_bwd and nc_instnorm_act_bwd_dbias: bit-equal dx; returns dx, dbias"""
    NC = N * C
    dx1, dx2, db = Out(NC * S, off), Out(NC * S, off), Out(C, off)
    ok(L().nc_instnorm_act_bwd(P(dy), P(x), P(m), P(r), slope, P(dx1.t), NC, S, P(ws), nb, stream()), 'nc_instnorm_act_bwd')
    ok(L().nc_instnorm_act_bwd_dbias(P(dy), P(x), P(m), P(r), slope, P(dx2.t), P(db.t), N, C, S, P(ws), nb, stream()), 'nc_instnorm_act_bwd_dbias')
    assert dx1.intact() and dx2.intact() and db.intact()
    assert torch.equal(dx1.t, dx2.t) and not bool(torch.isnan(dx1.t).any()) and not bool(torch.isnan(db.t).any())
    return dx1.t.view(NC, S), db.t


@pytest.mark.parametrize('case', R.IN_CASES, ids=[R.case_id(c) for c in R.IN_CASES])
def test_instance_norm_long_path_against_fp64(case):
    N, C, S, kind, branch = case
    NC = N * C
    off = 1 if kind == 'unaligned' else 0
    path = 'float4' if S % 4 == 0 and not off else 'scalar'
    assert S > 2048 and NC <= 65535
    splits = R.pick_splits(NC, S)
    cid = '%s (%d splits of %d)' % (R.case_id(case), splits, R.chunk_len(S, splits))
    xc, dyc, noise = R.in_inputs(N, C, S, kind)
    x, dy = place(xc, off), place(dyc, off)
    ws, nb = in_ws(NC, S)
    cap = R.EXCL_CAP_OFFSET if kind == 'offset' else R.EXCL_CAP

    m0, r0 = in_stats(x, NC, S, ws, nb, off)
    st = R.stats64(x)
    judge('k_in_stats ' + path, cid + ' mean', R.mean_share(m0, st))
    judge('k_in_stats ' + path, cid + ' rstd', R.rstd_share(r0, st))
    if kind == 'constant':
        assert float(m0[0]) == float(torch.tensor(1.7)) and abs(float(r0[0]) * math.sqrt(R.EPS) - 1.0) <= 4 * R.U
    mw, rw = R.wrong_stats(m0, r0, noise)
    mw, rw = place(mw, off), place(rw, off)

    for slope in R.SLOPES:
        y = in_fwd_both(x, m0, r0, slope, NC, S, ws, nb, off)
        yr, ylim = R.in_fwd(x, m0, r0, slope)
        judge('k_in_act_fwd ' + path, '%s slope %.1f' % (cid, slope), R.share((y.double() - yr).abs(), ylim))
        if off:
            # only y off its boundary (x, mean, rstd aligned: still the scalar loop), and everything aligned (the 16-byte loop): the same
            # elementwise arithmetic on the same statistics, bit for bit
            xa, ma, ra = place(xc), place(m0), place(r0)
            assert torch.equal(act_fwd(xa, ma, ra, slope, NC, S, 1), y)
            assert torch.equal(act_fwd(xa, ma, ra, slope, NC, S, 0), y)
        del yr, ylim, y
        for which, (m, r) in (('true', (m0, r0)), ('wrong', (mw, rw))):
            dx, db = in_bwd_both(dy, x, m, r, slope, N, C, S, ws, nb, off)
            dxr, lim, excl, corr = R.in_bwd(dy, x, m, r, slope)
            frac = float(excl.double().mean())
            what = '%s slope %.1f %s statistics' % (cid, slope, which)
            print('%-34s %-58s left out: %.2e (cap %.0e)' % ('', what, frac, cap))
            assert frac <= cap
            judge('k_in_bwd_sums + k_in_bwd_apply', what, R.share((dx.double() - dxr).abs(), lim, ~excl))
            dbr, dblim, first = R.dbias_ref(dxr, lim, corr, N, C)
            print('%-34s %-58s dbias, of the first form of its limit: %.3f' % ('', what, R.share((db.double() - dbr).abs(), first)[0]))
            judge('k_in_dbias_final', what, R.share((db.double() - dbr).abs(), dblim))
            own, ownlim = R.dbias_plumbing_limit(dx, N, C)
            judge('k_in_dbias_final (its own dx)', what, R.share((db.double() - own).abs(), ownlim))
            if which == 'wrong':   # the sums are not rounding noise in this set-up (that would be ~ u / sqrt(N S) of the sum of magnitudes)
                assert float((dbr.abs() / dxr.reshape(N, C, S).abs().sum((0, 2))).max()) > 1e-6
            del dx, dxr, lim, excl


def test_instance_norm_more_than_65535_long_instances():
    """NC = 65537 at S = 2052 (538 MB per tensor): nc_instnorm_stats, nc_instnorm_act_fwd and nc_instnorm_act_bwd take the instances in chunks of
    65535; every instance's statistics, y and dx are held to float64 in slices (the first, 65535th, 65536th and last instance are named in the
    output); nc_instnorm_act_bwd_dbias refuses the shape and launches nothing."""
    N, C, S = R.HUGE_CASE[:3]
    NC = N * C
    g = torch.Generator(device=DEV).manual_seed(65537)
    x = torch.randn(NC, S, device=DEV, generator=g).mul_(2.0).add_(0.5)
    dy = torch.randn(NC, S, device=DEV, generator=g)
    nb = int(L().nc_instnorm_ws_bytes(NC, S))
    ws = workspace(nb)
    m0, r0 = in_stats(x, NC, S, ws, nb)
    named = [0, 65534, 65535, NC - 1]
    step = 4096
    for slope in R.SLOPES:
        y = in_fwd_both(x, m0, r0, slope, NC, S, ws, nb)
        dxo = Out(NC * S)
        ok(L().nc_instnorm_act_bwd(P(dy), P(x), P(m0), P(r0), slope, P(dxo.t), NC, S, P(ws), nb, stream()), 'nc_instnorm_act_bwd')
        dx = dxo.t.view(NC, S)
        assert dxo.intact() and not bool(torch.isnan(dx).any())
        left = 0
        for a, b in [(a, min(a + step, NC)) for a in range(0, NC, step)] + [(i, i + 1) for i in named]:
            tag = 'instances [%d, %d) slope %.1f' % (a, b, slope)
            xs, ms, rs = x[a:b], m0[a:b], r0[a:b]
            if slope == R.SLOPES[0]:
                st = R.stats64(xs)
                judge('k_in_stats float4, NC > 65535', tag + ' mean', R.mean_share(ms, st))
                judge('k_in_stats float4, NC > 65535', tag + ' rstd', R.rstd_share(rs, st))
            yr, ylim = R.in_fwd(xs, ms, rs, slope)
            judge('k_in_act_fwd float4, NC > 65535', tag, R.share((y[a:b].double() - yr).abs(), ylim))
            dxr, lim, excl, _ = R.in_bwd(dy[a:b], xs, ms, rs, slope)
            judge('k_in_bwd_apply, NC > 65535', tag, R.share((dx[a:b].double() - dxr).abs(), lim, ~excl))
            if a % step == 0 and (b - a == step or b == NC):   # (the slices, not the named instances again)
                left += int(excl.sum())
        print('left out: %.2e (cap %.0e)' % (left / (NC * S), R.EXCL_CAP))
        assert left / (NC * S) <= R.EXCL_CAP
        del y
    # the bias-gradient form has no chunked path: refused, nothing launched
    dxo.whole.fill_(math.nan)
    db = Out(C)
    nb2 = int(L().nc_instnorm_bwd_dbias_ws_bytes(65535, S))
    ws2 = workspace(nb2)
    code = L().nc_instnorm_act_bwd_dbias(P(dy), P(x), P(m0), P(r0), 0.2, P(dxo.t), P(db.t), N, C, S, P(ws2), nb2, stream())
    torch.cuda.synchronize()
    assert code == NC_ERR_SHAPE and b'more than 65535 long instances' in L().nc_last_error()
    assert dxo.untouched() and db.untouched()


def test_instance_norm_long_path_refuses_bad_arguments():
    """a workspace that is missing or one byte short: NC_ERR_WS; a null pointer: NC_ERR_ARG; nothing is written"""
    NC, S = 2, 2049
    x, dy = torch.randn(NC, S, device=DEV), torch.randn(NC, S, device=DEV)
    ws, nb = in_ws(NC, S)
    base = int(L().nc_instnorm_ws_bytes(NC, S))
    m, r, y, dx, db = Out(NC), Out(NC), Out(NC * S), Out(NC * S), Out(1)
    one = torch.ones(NC, device=DEV)
    st = stream()
    for w, n in ((ws, base - 1), (None, base)):
        assert L().nc_instnorm_stats(P(x), NC, S, R.EPS, P(m.t), P(r.t), P(w), n, st) == NC_ERR_WS
        assert L().nc_instnorm_fwd(P(x), R.EPS, 0.2, P(m.t), P(r.t), P(y.t), NC, S, P(w), n, st) == NC_ERR_WS
        assert L().nc_instnorm_act_bwd(P(dy), P(x), P(one), P(one), 0.2, P(dx.t), NC, S, P(w), n, st) == NC_ERR_WS
    for w, n in ((ws, nb - 1), (None, nb)):
        assert L().nc_instnorm_act_bwd_dbias(P(dy), P(x), P(one), P(one), 0.2, P(dx.t), P(db.t), 1, NC, S, P(w), n, st) == NC_ERR_WS
    assert L().nc_instnorm_stats(P(None), NC, S, R.EPS, P(m.t), P(r.t), P(ws), nb, st) == NC_ERR_ARG
    assert L().nc_instnorm_stats(P(x), NC, S, R.EPS, P(None), P(r.t), P(ws), nb, st) == NC_ERR_ARG
    assert L().nc_instnorm_fwd(P(x), R.EPS, 0.2, P(m.t), P(r.t), P(None), NC, S, P(ws), nb, st) == NC_ERR_ARG
    assert L().nc_instnorm_act_fwd(P(x), P(None), P(one), 0.2, P(y.t), NC, S, st) == NC_ERR_ARG
    assert L().nc_instnorm_act_fwd(P(x), P(one), P(one), 0.2, P(None), NC, S, st) == NC_ERR_ARG
    assert L().nc_instnorm_act_bwd(P(None), P(x), P(one), P(one), 0.2, P(dx.t), NC, S, P(ws), nb, st) == NC_ERR_ARG
    assert L().nc_instnorm_act_bwd(P(dy), P(x), P(one), P(one), 0.2, P(None), NC, S, P(ws), nb, st) == NC_ERR_ARG
    assert L().nc_instnorm_act_bwd_dbias(P(dy), P(x), P(one), P(one), 0.2, P(dx.t), P(None), 1, NC, S, P(ws), nb, st) == NC_ERR_ARG
    assert L().nc_instnorm_stats(P(x), 0, S, R.EPS, P(m.t), P(r.t), P(ws), nb, st) == NC_ERR_SHAPE
    assert L().nc_instnorm_act_bwd(P(dy), P(x), P(one), P(one), 0.2, P(dx.t), NC, 0, P(ws), nb, st) == NC_ERR_SHAPE
    torch.cuda.synchronize()
    assert all(o.untouched() for o in (m, r, y, dx, db))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------------------------------------------------------
def bn_stats(x, N, C, S, training, rm, rv, ws, nb):
    mean, rstd = Out(C), Out(C)
    ok(L().nc_batchnorm_stats(P(x), N, C, S, R.EPS, R.MOMENTUM, training, P(mean.t), P(rstd.t), P(rm), P(rv), P(ws), nb, stream()), 'nc_batchnorm_stats')
    assert mean.intact() and rstd.intact()
    return mean.t, rstd.t


@pytest.mark.parametrize('case', R.BN_CASES, ids=[R.case_id(c) for c in R.BN_CASES])
def test_batch_norm_against_fp64(case):
    N, C, S, kind = case
    M = N * S
    x, dy, gamma, beta, rm0, rv0 = (t.to(DEV) for t in R.bn_inputs(N, C, S, kind))
    nb = int(L().nc_instnorm_ws_bytes(N * C, S))
    ws = workspace(nb)
    cid = '%s (%d splits)' % (R.case_id(case), R.pick_splits(N * C, S))
    st = R.stats64(x, (0, 2))

    # training: statistics of the batch, running statistics updated in place (nullable)
    rm, rv = rm0.clone(), rv0.clone()
    mean, rstd = bn_stats(x, N, C, S, 1, rm, rv, ws, nb)
    judge('k_in_stats + k_bn_finalize', cid + ' mean', R.mean_share(mean, st))
    judge('k_in_stats + k_bn_finalize', cid + ' rstd', R.rstd_share(rstd, st))
    (nm, nmlim), (nv, nvlim) = R.bn_running(rm0, rv0, st, M)
    judge('k_in_stats + k_bn_finalize', cid + ' running_mean', R.share((rm.double() - nm).abs(), nmlim))
    judge('k_in_stats + k_bn_finalize', cid + ' running_var', R.share((rv.double() - nv).abs(), nvlim))
    if M == 1:
        assert float(st[1]) == 0.0 and float(rv) == pytest.approx(0.9 * float(rv0), rel=1e-6)
    m2, r2 = bn_stats(x, N, C, S, 1, None, None, ws, nb)
    assert torch.equal(m2, mean) and torch.equal(r2, rstd)
    # evaluation: the running statistics, read only
    rm, rv = rm0.clone(), rv0.clone()
    emean, erstd = bn_stats(x, N, C, S, 0, rm, rv, ws, nb)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and torch.equal(emean, rm0)
    judge('k_bn_running', cid + ' rstd', R.share((erstd.double() * (rv0.double() + R.EPS).sqrt() - 1.0).abs(), torch.full((C,), 2 * R.U, dtype=torch.float64, device=DEV)))
    o1, o2 = Out(C), Out(C)
    for a, b in ((None, rv), (rm, None)):
        assert L().nc_batchnorm_stats(P(x), N, C, S, R.EPS, R.MOMENTUM, 0, P(o1.t), P(o2.t), P(a), P(b), P(ws), nb, stream()) == NC_ERR_ARG
    torch.cuda.synchronize()
    assert o1.untouched() and o2.untouched()

    for training, (m, r) in ((1, (mean, rstd)), (0, (emean, erstd))):
        for slope in R.SLOPES:
            what = '%s %s slope %.1f' % (cid, 'training' if training else 'evaluation', slope)
            y = Out(N * C * S)
            ok(L().nc_batchnorm_act_fwd(P(x), P(m), P(r), P(gamma), P(beta), slope, P(y.t), N, C, S, stream()), 'nc_batchnorm_act_fwd')
            yr, ylim = R.bn_fwd(x, m, r, gamma, beta, slope)
            assert y.intact()
            judge('k_bn_act_fwd', what, R.share((y.t.view(N, C, S).double() - yr).abs(), ylim))
            dx, dga, dbe, coef = Out(N * C * S), Out(C), Out(C), Out(2 * C)
            ok(L().nc_batchnorm_act_bwd(P(dy), P(x), P(m), P(r), P(gamma), P(beta), slope, training, P(dx.t), P(dga.t), P(dbe.t), P(coef.t), N, C, S,
                                        P(ws), nb, stream()), 'nc_batchnorm_act_bwd')
            assert all(o.intact() for o in (dx, dga, dbe, coef))
            dxr, lim, excl, (dgr, dglim, dgfirst), (dbr, dblim, dbfirst) = R.bn_bwd(dy, x, m, r, gamma, beta, slope, bool(training))
            print('%-34s %-58s of the first form of the limit of the sums: dgamma %.3f dbeta %.3f'
                  % ('', what, R.share((dga.t.double() - dgr).abs(), dgfirst)[0], R.share((dbe.t.double() - dbr).abs(), dbfirst)[0]))
            assert float(excl.double().mean()) <= R.EXCL_CAP
            judge('k_bn_bwd_apply ' + ('training' if training else 'evaluation'), what, R.share((dx.t.view(N, C, S).double() - dxr).abs(), lim, ~excl))
            judge('k_bn_bwd_sums + k_bn_bwd_finalize', what + ' dgamma', R.share((dga.t.double() - dgr).abs(), dglim))
            judge('k_bn_bwd_sums + k_bn_bwd_finalize', what + ' dbeta', R.share((dbe.t.double() - dbr).abs(), dblim))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the inference tail (k_in_act_tail through nc_instnorm_relu_tail_sigmoid_debug)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', R.TAIL_S)
@pytest.mark.parametrize('C', R.TAIL_C)
def test_inference_tail_against_fp64(C, S):
    x, w1, b1, w2, b2 = (t.to(DEV) for t in R.tail_inputs(C, S))
    st = R.stats64(x)
    mean, rstd = st[0].float(), st[2].float()
    y = Out(S)
    ok(L().nc_instnorm_relu_tail_sigmoid_debug(P(x), P(mean), P(rstd), P(w1), P(b1), P(w2), P(b2), P(y.t), C, S, stream()), 'tail')
    yr, lim = R.tail(x, mean, rstd, w1, b1, w2, b2)
    assert y.intact() and not bool(torch.isnan(y.t).any())
    judge('k_in_act_tail', 'C %d S %d' % (C, S), R.share((y.t.double() - yr).abs(), lim))
    if S > 1:
        assert float(yr.max() - yr.min()) > 1e-3     # the output is not a constant


def test_inference_tail_refuses_more_than_256_channels():
    C, S = 257, 16
    x = torch.randn(C, S, device=DEV)
    v = torch.ones(C, device=DEV)
    y = Out(S)
    code = L().nc_instnorm_relu_tail_sigmoid_debug(P(x), P(v), P(v), P(v), P(v), P(v), P(v), P(y.t), C, S, stream())
    assert code == NC_ERR_SHAPE and b'at most 256 channels' in L().nc_last_error()
    assert L().nc_instnorm_relu_tail_sigmoid_debug(P(x), P(v), P(v), P(None), P(v), P(v), P(v), P(y.t), 8, S, stream()) == NC_ERR_ARG
    assert L().nc_instnorm_relu_tail_sigmoid_debug(P(x), P(v), P(v), P(v), P(v), P(v), P(v), P(y.t), 8, 0, stream()) == NC_ERR_SHAPE
    torch.cuda.synchronize()
    assert y.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# MaxPool(2) and slice / MIP: ties and NaN.  The references run on the CPU (tests/norm_reference.py); everything is bit-equal.
# ---------------------------------------------------------------------------------------------------------------------------------------------
def pool_nans(shape):
    """a NaN at each position of the window, in windows of their own, and a window with two (positions 2 and 5 of 8; 1 and 2 of 4)"""
    NC, D, H, W = shape
    wd = 2 if D > 1 else 1
    Ho = H // 2
    pos = []
    for k in range(4 * wd):
        a, b, c = (k >> 2) & 1, (k >> 1) & 1, k & 1
        pos.append((0, a, (k % Ho) * 2 + b, (k // Ho) * 2 + c))
    pos += [(1, 0, 1, 0), (1, 1, 0, 1)] if wd == 2 else [(1, 0, 0, 1), (1, 0, 1, 0)]
    return pos


def run_pool(x, dy, skip):
    NC, D, H, W = x.shape
    wd = 2 if D > 1 else 1
    xg, dyg = x.to(DEV), dy.to(DEV)
    y = Out(dy.numel())
    ok(L().nc_maxpool2_fwd(P(xg), P(y.t), NC, D, H, W, stream()), 'nc_maxpool2_fwd')
    dx = Out(x.numel())
    ok(L().nc_maxpool2_bwd(P(dyg), P(xg), P(dx.t), NC, D, H, W, stream()), 'nc_maxpool2_bwd')
    dxa = Out(x.numel())
    code = L().nc_maxpool2_bwd_add(P(dyg), P(xg), P(skip.to(DEV)), P(dxa.t), NC, D, H, W, stream())
    torch.cuda.synchronize()
    assert y.intact() and dx.intact() and dxa.intact()
    assert torch.equal(R.bits(y.t.cpu().view(dy.shape)), R.bits(R.pool_fwd(x)))
    want = R.pool_bwd(dy, x)
    assert torch.equal(dx.t.cpu().view(x.shape), want)
    if (D % wd) or (H & 1) or (W & 1):   # the border no window covers is zero (the memset path); the skip form refuses odd sizes
        assert float(want[:, (D // wd) * wd:].abs().sum() + want[:, :, (H // 2) * 2:].abs().sum() + want[..., (W // 2) * 2:].abs().sum()) == 0.0
        assert code == NC_ERR_SHAPE and dxa.untouched()
    else:
        assert code == 0 and torch.equal(dxa.t.cpu().view(x.shape), R.pool_bwd(dy, x, skip))
    return want


@pytest.mark.parametrize('shape', R.POOL_CASES, ids=['x'.join(map(str, s)) for s in R.POOL_CASES])
def test_max_pool_ties_and_nan(shape):
    NC, D, H, W = shape
    wd = 2 if D > 1 else 1
    x = R.tied(shape, 21)
    g = torch.Generator().manual_seed(22)
    dy = torch.randn(NC, D // wd, H // 2, W // 2, generator=g)
    skip = torch.randn(*shape, generator=g)
    cols, _ = R._windows(x)
    assert int((cols == 0).all(-1).sum()) >= 1 and int(((cols == cols.max(-1, keepdim=True)[0]).sum(-1) > 1).sum()) >= 2   # whole windows tie
    want = run_pool(x, dy, skip)
    # a tied window sends its gradient to its FIRST element
    zero = (cols == 0).all(-1).nonzero()[0]
    n, od, oh, ow = (int(v) for v in zero)
    assert float(want[n, od * wd, oh * 2, ow * 2]) == float(dy[n, od, oh, ow])
    run_pool(R.plant_nans(x, pool_nans(shape)), dy, skip)


def test_c8_max_pool_routes_ties_like_the_fp32_kernel():
    """nc_c8_maxpool2_fwd / _bwd_add on a tied input: the 16-bit form of what nc_maxpool2_fwd / _bwd_add give on the same (16-bit exact) values"""
    from test_gpu_c8 import BF, FP, tdt, to_c8
    N, C, D, H, W = 2, 16, 6, 8, 10
    S = D * H * W
    g = torch.Generator().manual_seed(23)
    for dt in (BF, FP):
        x = R.tied((N, C, D, H, W), 24).to(tdt(dt)).float().to(DEV)
        dp = torch.randn(N, C, D // 2, H // 2, W // 2, generator=g).to(torch.bfloat16).float().to(DEV)
        skip = torch.randn(N, C, D, H, W, generator=g).to(torch.bfloat16).float().to(DEV)
        y32, dx32 = Out(N * C * S // 8), Out(N * C * S)
        ok(L().nc_maxpool2_fwd(P(x), P(y32.t), N * C, D, H, W, stream()), 'nc_maxpool2_fwd')
        ok(L().nc_maxpool2_bwd_add(P(dp), P(x), P(skip), P(dx32.t), N * C, D, H, W, stream()), 'nc_maxpool2_bwd_add')
        xh, sh, dph = to_c8(x, dt), to_c8(skip, BF), to_c8(dp, BF)
        yh = torch.empty(N * C * S // 8 * 2, dtype=torch.uint8, device=DEV)
        dxh = torch.empty(N * C * S * 2, dtype=torch.uint8, device=DEV)
        ok(L().nc_c8_maxpool2_fwd(P(xh), C, 0, P(yh), N, C, D, H, W, dt, stream()), 'nc_c8_maxpool2_fwd')
        ok(L().nc_c8_maxpool2_bwd_add(P(dph), P(xh), C, 0, P(sh), C, 0, P(dxh), N, C, D, H, W, dt, stream()), 'nc_c8_maxpool2_bwd_add')
        assert torch.equal(yh.view(tdt(dt)).reshape(N, C // 8, S // 8, 8), to_c8(y32.t.view(N, C, D // 2, H // 2, W // 2), dt))
        assert torch.equal(dxh.view(torch.bfloat16).reshape(N, C // 8, S, 8), to_c8(dx32.t.view(N, C, D, H, W), BF))


MIP_NANS = [(0, s, s, s) for s in range(5)] + [(0, 0, 5, 5), (1, 2, 3, 1), (1, 2, 3, 4), (1, 1, 0, 0), (1, 3, 0, 0), (1, 4, 2, 6), (1, 4, 5, 6)]


@pytest.mark.parametrize('with_nan', [False, True], ids=['ties', 'ties+nan'])
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_slice_and_mip_ties_and_nan(axis, with_nan):
    shape = R.MIP_SHAPE
    NC, D, H, W = shape
    vol = R.tied(shape, 31)
    if with_nan:
        vol = R.plant_nans(vol, MIP_NANS)
    vg = vol.to(DEV)
    Ln = shape[axis + 1]
    plane = tuple(v for i, v in enumerate(shape) if i != axis + 1)
    g = torch.Generator().manual_seed(32)
    dout = torch.randn(*plane, generator=g)
    for start, depth in ((0, Ln), (0, 2), (Ln - 2, 2), (1, 3), (0, 1), (Ln - 1, 1)):
        out, arg = Out(dout.numel()), torch.full(plane, -7, dtype=torch.int32, device=DEV)
        ok(L().nc_mip_fwd(P(vg), P(out.t), P(arg), NC, D, H, W, axis, start, depth, stream()), 'nc_mip_fwd')
        ro, ra = R.mip_fwd(vol, axis, start, depth)
        assert out.intact() and torch.equal(R.bits(out.t.cpu().view(plane)), R.bits(ro)), (axis, start, depth)
        assert torch.equal(arg.cpu(), ra), (axis, start, depth)
        dvol = Out(vol.numel())
        ok(L().nc_mip_bwd(P(dout.to(DEV)), P(arg), P(dvol.t), NC, D, H, W, axis, stream()), 'nc_mip_bwd')
        assert dvol.intact() and torch.equal(dvol.t.cpu().view(shape), R.mip_bwd(dout, ra, shape, axis))
    if not with_nan:   # ties exist along this axis, and the first one is taken
        cols = vol.movedim(axis + 1, -1)
        assert int(((cols == cols.max(-1, keepdim=True)[0]).sum(-1) > 1).sum()) >= 1
    for index in (0, Ln // 2, Ln - 1):
        out, dvol = Out(dout.numel()), Out(vol.numel())
        ok(L().nc_slice_fwd(P(vg), P(out.t), NC, D, H, W, axis, index, stream()), 'nc_slice_fwd')
        ok(L().nc_slice_bwd(P(dout.to(DEV)), P(dvol.t), NC, D, H, W, axis, index, stream()), 'nc_slice_bwd')
        assert out.intact() and dvol.intact()
        assert torch.equal(R.bits(out.t.cpu().view(plane)), R.bits(vol.select(axis + 1, index)))
        want = torch.zeros(shape)
        want.select(axis + 1, index).copy_(dout)
        assert torch.equal(dvol.t.cpu().view(shape), want)
    o = Out(dout.numel())
    assert L().nc_slice_fwd(P(vg), P(o.t), NC, D, H, W, axis, Ln, stream()) == NC_ERR_SHAPE
    assert L().nc_mip_fwd(P(vg), P(o.t), P(arg), NC, D, H, W, axis, Ln - 1, 2, stream()) == NC_ERR_SHAPE
    torch.cuda.synchronize()
    assert o.untouched()
