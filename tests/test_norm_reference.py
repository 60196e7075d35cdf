"""CPU: the references and limits of the op-level norm / pool tests (tests/norm_reference.py) are themselves checked -- the closed-form backward
against float64 autograd, the first-maximum scans against torch's CPU operators on tie-free inputs, every case against its exclusion cap, and the
derived limits against an fp32 emulation of the kernels' arithmetic (met) and two deliberately wrong variants of it (missed)."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_reference as R  # noqa: E402

# the emulation (several fp32 and fp64 passes on the CPU) runs on the cases up to this many elements; the larger ones have the same Gaussian inputs
EMU_MAX = 1 << 21


def _close(a, r, tol=1e-11):
    assert a.shape == r.shape and a.dtype == torch.float64
    assert float((a - r).abs().max()) <= tol * max(float(r.abs().max()), 1e-300)


@pytest.mark.parametrize('slope', R.SLOPES)
def test_instance_norm_closed_form_is_float64_autograd(slope):
    """with the TRUE float64 statistics passed as mean / rstd"""
    g = torch.Generator().manual_seed(5)
    N, C, S = 2, 3, 37
    x = (torch.randn(N, C, S, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    dy = torch.randn(N, C, S, generator=g, dtype=torch.float64)
    y = F.leaky_relu(F.instance_norm(x, eps=R.EPS), R.f32(slope))   # (the slope the op receives: a float)
    (dx,) = torch.autograd.grad(y, x, dy)
    x2 = x.detach().reshape(N * C, S)
    mean, var, rstd, _, _ = R.stats64(x2)
    _close(mean, x2.mean(1))
    _close(var, x2.var(1, unbiased=False))
    yr, _ = R.in_fwd(x2, mean, rstd, slope)
    dxr, lim, excl, corr = R.in_bwd(dy.reshape(N * C, S), x2, mean, rstd, slope)
    _close(yr, y.detach().reshape(N * C, S))
    _close(dxr, dx.reshape(N * C, S))
    assert bool((lim > 0).all()) and not bool(excl.any())
    db, dlim, _ = R.dbias_ref(dxr, lim, corr, N, C)
    # (with the true statistics the sum is zero up to rounding: judged against the sum of magnitudes)
    assert db.shape == (C,) and float((db - dx.sum((0, 2))).abs().max()) <= 1e-13 * float(dx.abs().sum((0, 2)).max())
    assert bool((dlim > 0).all())


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('slope', R.SLOPES)
def test_batch_norm_closed_form_is_float64_autograd(slope, training):
    g = torch.Generator().manual_seed(6)
    N, C, S = 3, 4, 29
    x = (torch.randn(N, C, S, generator=g, dtype=torch.float64) * 1.5 + 0.3).requires_grad_(True)
    dy = torch.randn(N, C, S, generator=g, dtype=torch.float64)
    gamma = torch.tensor([0.7, -1.3, 1.1, -0.4], dtype=torch.float64, requires_grad=True)
    beta = torch.tensor([0.5, 0.6, -0.4, -0.3], dtype=torch.float64, requires_grad=True)
    rm0 = torch.randn(C, generator=g, dtype=torch.float64) * 0.2
    rv0 = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    y = F.leaky_relu(F.batch_norm(x, rm, rv, gamma, beta, training, R.MOMENTUM, R.EPS), R.f32(slope))
    dx, dga, dbe = torch.autograd.grad(y, (x, gamma, beta), dy)
    st = R.stats64(x.detach(), (0, 2))
    mean, rstd = (st[0], st[2]) if training else (rm0, 1.0 / (rv0 + R.EPS).sqrt())
    yr, _ = R.bn_fwd(x.detach(), mean, rstd, gamma.detach(), beta.detach(), slope)
    dxr, lim, excl, (dg, _, _), (db, _, _) = R.bn_bwd(dy, x.detach(), mean, rstd, gamma.detach(), beta.detach(), slope, training)
    _close(yr, y.detach())
    _close(dxr, dx)
    _close(dg, dga)
    _close(db, dbe)
    assert not bool(excl.any())
    if training:   # torch updated rm, rv in place
        (nm, _), (nv, _) = R.bn_running(rm0, rv0, st, N * S)
        _close(nm, rm)
        _close(nv, rv)


def test_running_variance_of_one_element_is_the_biased_one():
    x = torch.tensor([[[2.5]]])
    st = R.stats64(x, (0, 2))
    (nm, _), (nv, _) = R.bn_running(torch.tensor([1.0]), torch.tensor([2.0]), st, 1)
    assert nm.item() == pytest.approx(0.9 + 0.25) and nv.item() == pytest.approx(1.8)


def test_tail_reference_is_the_composition_of_its_layers():
    C, S = 5, 17
    x, w1, b1, w2, b2 = (t.double() for t in R.tail_inputs(C, S))
    mean, _, rstd, _, _ = R.stats64(x)
    t = F.relu(F.instance_norm(x.unsqueeze(0), eps=R.EPS))[0]
    want = torch.sigmoid(F.conv1d(F.conv1d(t.unsqueeze(0), w1.view(1, C, 1), b1), w2.view(1, 1, 1), b2))[0, 0]
    y, lim = R.tail(x, mean, rstd, w1, b1, w2, b2)
    _close(y, want)
    assert bool((lim >= 4 * R.U).all())


@pytest.mark.parametrize('shape', R.POOL_CASES + [(2, 6, 6, 6)])
def test_pool_reference_is_torch_on_tie_free_inputs(shape):
    g = torch.Generator().manual_seed(8)
    x = torch.randn(*shape, generator=g).requires_grad_(True)
    y = F.max_pool3d(x, 2) if shape[1] > 1 else F.max_pool2d(x[:, 0], 2).unsqueeze(1)
    dy = torch.randn(*y.shape, generator=g)
    (dx,) = torch.autograd.grad(y, x, dy)
    assert torch.equal(R.pool_fwd(x.detach()), y.detach())
    assert torch.equal(R.pool_bwd(dy, x.detach()), dx)
    skip = torch.randn(*shape, generator=g)
    assert torch.equal(R.pool_bwd(dy, x.detach(), skip), skip + dx)


def test_pool_reference_takes_the_first_maximum_and_the_last_nan():
    x = torch.zeros(1, 2, 2, 2)
    assert R.pool_bwd(torch.ones(1, 1, 1, 1), x).flatten().tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    x = R.plant_nans(torch.arange(8.0).reshape(1, 2, 2, 2), [(0, 0, 1, 0), (0, 1, 0, 1)])
    assert math.isnan(R.pool_fwd(x).item())
    assert R.pool_bwd(torch.ones(1, 1, 1, 1), x).flatten().tolist() == [0, 0, 0, 0, 0, 1, 0, 0]


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_mip_reference_is_torch_on_tie_free_inputs(axis):
    g = torch.Generator().manual_seed(9)
    vol = torch.randn(*R.MIP_SHAPE, generator=g).requires_grad_(True)
    L = R.MIP_SHAPE[axis + 1]
    for start, depth in ((0, L), (0, 2), (L - 2, 2), (1, 1), (L - 1, 1)):
        ref = vol.narrow(axis + 1, start, depth).max(axis + 1)[0]
        r = torch.randn(*ref.shape, generator=g)
        (gv,) = torch.autograd.grad(ref, vol, r)
        out, arg = R.mip_fwd(vol.detach(), axis, start, depth)
        assert torch.equal(out, ref.detach()) and arg.dtype == torch.int32
        assert int(arg.min()) >= start and int(arg.max()) < start + depth
        assert torch.equal(R.mip_bwd(r, arg, vol.shape, axis), gv)


def test_mip_reference_takes_the_first_maximum_and_the_first_nan():
    vol = torch.zeros(1, 4, 1, 1)
    assert R.mip_fwd(vol, 0, 1, 3)[1].item() == 1
    vol = R.plant_nans(torch.arange(4.0).reshape(1, 4, 1, 1), [(0, 1, 0, 0), (0, 2, 0, 0)])
    out, arg = R.mip_fwd(vol, 0, 0, 4)
    assert math.isnan(out.item()) and arg.item() == 1


def test_dispatch_arithmetic_of_the_case_table():
    """the branch each long-path case names, restated from pick_splits / chunk_range"""
    want = {(2, 2049): (1, 2052), (3, 2052): (1, 2052), (2, 8193): (2, 4100), (2, 8196): (2, 4100), (5, 13824): (2, 6912), (1, 531441): (64, 8304),
            (1, 524292): (64, 8196), (1100, 24580): (2, 12292), (2100, 8196): (1, 8196), (1, 1048580): (64, 16388), (1, 4194308): (64, 65540),
            (3, 8196): (2, 4100), (2, 16384): (2, 8192)}
    for N, C, S, kind, _ in R.IN_CASES:
        assert S > 2048
        assert (R.pick_splits(N * C, S), R.chunk_len(S, R.pick_splits(N * C, S))) == want[(N * C, S)], (N * C, S)
    assert -(-531441 // 8192) == 65 and -(-524292 // 64) == 8193 and -(-24580 // 8192) == 4 and -(-2048 // 1100) == 2
    assert -(-1048580 // 1024) > 1024 and -(-4194308 // 4096) > 1024 and -(-1048580 // 4096) <= 1024
    N, C, S = R.HUGE_CASE[:3]
    assert N * C > 65535 and S > 2048 and S % 4 == 0 and R.pick_splits(65535, S) == 1


@pytest.mark.parametrize('case', R.IN_CASES, ids=[R.case_id(c) for c in R.IN_CASES])
def test_instance_norm_cases_stay_inside_their_exclusion_cap(case):
    """from the inputs alone: float64 statistics rounded to fp32, as the op is given them.  (The one large case makes its inputs on the device
    and asserts its cap there.)"""
    N, C, S, kind, _ = case
    x, dy, noise = R.in_inputs(N, C, S, kind)
    st = R.stats64(x)
    cap = R.EXCL_CAP_OFFSET if kind == 'offset' else R.EXCL_CAP
    mean, rstd = st[0].float(), st[2].float()
    for m, r in ((mean, rstd), R.wrong_stats(mean, rstd, noise)):
        xhat, _, d = R._xhat(x, m, r)
        frac = float(((xhat != 0) & (xhat.abs() <= d)).double().mean())
        print('%s: share left out %.2e (cap %.0e)' % (R.case_id(case), frac, cap))
        assert frac <= cap
    if kind == 'constant':
        assert float(st[1][0]) == 0.0 and float(st[0][0]) == float(torch.tensor(1.7))
    if kind == 'offset':
        assert 3e3 < float((st[2] * st[0].abs()).max()) < 4e3


@pytest.mark.parametrize('case', R.BN_CASES, ids=[R.case_id(c) for c in R.BN_CASES])
def test_batch_norm_cases_stay_inside_their_exclusion_cap(case):
    N, C, S, kind = case
    x, dy, gamma, beta, rm, rv = R.bn_inputs(N, C, S, kind)
    st = R.stats64(x, (0, 2))
    for mean, rstd in ((st[0].float(), st[2].float()), (rm, (1.0 / (rv.double() + R.EPS).sqrt()).float())):
        excl = R.bn_bwd(dy, x, mean, rstd, gamma, beta, 0.2, True)[2]
        print('%s: %d of %d left out' % (R.case_id(case), int(excl.sum()), excl.numel()))
        assert float(excl.double().mean()) <= R.EXCL_CAP
    if kind == 'signs':   # the offset moves the mask: neither half of a channel is empty, and it is not the mask of xhat
        assert bool((gamma < 0).any()) and bool((gamma > 0).any())
        xhat, z = R._bn_z(x, st[0].float(), st[2].float(), gamma, beta)[:2]
        pos = (z > 0).double().mean((0, 2))
        assert bool((pos > 0.1).all()) and bool((pos < 0.9).all())
        assert float(((z > 0) != (xhat > 0)).double().mean()) > 0.2


EMU_CASES = [c for c in R.IN_CASES if c[0] * c[1] * c[2] <= EMU_MAX]


@pytest.mark.parametrize('case', EMU_CASES, ids=[R.case_id(c) for c in EMU_CASES])
def test_fp32_emulation_meets_the_limits_and_wrong_variants_do_not(case):
    N, C, S, kind, _ = case
    x, dy, noise = R.in_inputs(N, C, S, kind)
    st = R.stats64(x)
    mean, rstd = st[0].float(), st[2].float()
    assert R.mean_share(mean, st)[0] <= 1 and R.rstd_share(rstd, st)[0] <= 1          # a correctly rounded fp32 store meets the statistics limits
    splits = R.pick_splits(N * C, S)
    for slope in R.SLOPES:
        yr, ylim = R.in_fwd(x, mean, rstd, slope)
        sy = R.share((R.emu_in_fwd(x, mean, rstd, slope).double() - yr).abs(), ylim)
        for m, r in ((mean, rstd), R.wrong_stats(mean, rstd, noise)):
            dxr, lim, excl, corr = R.in_bwd(dy, x, m, r, slope)
            emu = R.emu_in_bwd(dy, x, m, r, slope, splits).double()
            sd = R.share((emu - dxr).abs(), lim, ~excl)
            dbr, dblim, quad = R.dbias_ref(dxr, lim, corr, N, C)
            sb = R.share((emu.reshape(N, C, S).sum((0, 2)) - dbr).abs(), dblim)
            sq = R.share((emu.reshape(N, C, S).sum((0, 2)) - dbr).abs(), quad)
            print('%s slope %.1f: y %.3f %.3f  dx %.3f %.3f  dbias %.3f (of the first form: %.3f)' % (R.case_id(case), slope, *sy, *sd, sb[0], sq[0]))
            assert sy[0] <= 1 and sd[0] <= 1 and sb[0] <= 1
        if kind == 'constant':
            continue   # (1.7 and a mean of 0.5 +- 0.02 happen to survive bf16 poorly or well by luck: the wrong variants are judged on the other cases)
        # wrong variant 1: the mean rounded to bf16 (2^-9 relative: far outside 4u)
        assert R.share((R.emu_in_fwd(x, mean, rstd, slope, bf16_mean=True).double() - yr).abs(), ylim)[0] > 1
        dxr, lim, excl, _ = R.in_bwd(dy, x, mean, rstd, slope)
        assert R.share((R.emu_in_bwd(dy, x, mean, rstd, slope, splits, bf16_mean=True).double() - dxr).abs(), lim, ~excl)[0] > 1
        # wrong variant 2: the last split missing from m2
        if splits > 1:
            assert R.share((R.emu_in_bwd(dy, x, mean, rstd, slope, splits, drop_last_split=True).double() - dxr).abs(), lim, ~excl)[0] > 1
