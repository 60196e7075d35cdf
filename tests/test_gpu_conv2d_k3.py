"""Conv2d(kernel 3, stride 1, padding 1) of the 2-D generators, op level: the image-tiled fp32 matrix-core kernel of csrc/conv2d_k3.hip (forward and
data gradient, through nc_conv_fwd / nc_conv_dgrad) and the gather GEMM the same calls take with nc_set_conv2d_k3(0), each against a float64
reference.

References, yardstick (the one-accumulator fp32 chain in (channel, ty, tx) order -- the kernel's own order -- against the same float64 reference,
evaluated with torch on the GPU), error measure, limit and the case lists: tests/conv2d_reference.py.  Which path a call takes is asked of the
library (nc_conv2d_k3_active) and held to the coverage rule restated in conv2d_reference.k3_covered.  Outputs are NaN-filled with guard elements
behind them."""
import contextlib
import functools
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv2d_reference as R  # noqa: E402

DEV = 'cuda'
GUARD = 64
WORST = {}
IDS = [R.case_id(c[:5]) for c in R.K3_CASES]


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


@contextlib.contextmanager
def k3(on=1, cfg=-1, direct=0):
    prev = L().nc_get_conv2d_k3()
    L().nc_set_conv2d_k3(on)
    L().nc_conv2d_k3_set_cfg(cfg)
    L().nc_set_force_direct(direct)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        L().nc_set_conv2d_k3(prev)
        L().nc_conv2d_k3_set_cfg(-1)
        L().nc_set_force_direct(0)


@pytest.fixture(scope='module', autouse=True)
def _worst_table():
    yield
    print('\nworst use of the limit per path (max, rms; 1.0 = at the limit)')
    for k in sorted(WORST):
        print('  %-28s max %.3f  rms %.3f' % (k, WORST[k][0], WORST[k][1]))


@functools.lru_cache(maxsize=None)
def gpu_inputs(N, C, K, H, W):
    return tuple(t.to(DEV) for t in R.inputs3(N, C, K, H, W))


@functools.lru_cache(maxsize=None)
def reference(what, N, C, K, H, W):
    """(float64 reference, (max, rms) of the fp32 chain against it), on the GPU, once per shape; the forward reference carries the bias."""
    x, w, b, dy = gpu_inputs(N, C, K, H, W)
    if what == 0:
        ref = R.ref3_fwd(x, w, b)
        return ref, R.err(R.chain3_fwd(x, w, b), ref)
    ref = R.ref3_dgrad(dy, w)
    return ref, R.err(R.chain3_dgrad(dy, w), ref)


def judge(path, what, got, orc):
    r = R.ratios(got, orc)
    print('%-14s %-34s product max %.2e rms %.2e | chain max %.2e rms %.2e | of the limit %.3f %.3f' % (path, what, got[0], got[1], orc[0], orc[1], r[0], r[1]))
    if math.isfinite(r[0]) and math.isfinite(r[1]):
        w = WORST.get(path, (0.0, 0.0))
        WORST[path] = (max(w[0], r[0]), max(w[1], r[1]))
    assert R.within(got, orc), (path, what, got, orc)


def run(what, N, C, K, H, W):
    """nc_conv_fwd (what 0, with bias) or nc_conv_dgrad (what 1) under the current switches -> the output, checked for unwritten elements and
    writes past its end."""
    x, w, b, dy = gpu_inputs(N, C, K, H, W)
    nb = int(L().nc_conv_ws_bytes(N, C, 1, H, W, K, 1, 3, 3, 1, 1))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    n = N * (K if what == 0 else C) * H * W
    buf = torch.full((n + GUARD,), float('nan'), device=DEV)
    out = buf[:n].view(N, K if what == 0 else C, H, W)
    if what == 0:
        ck(L().nc_conv_fwd(P(x), P(w), P(b), P(out), N, C, 1, H, W, K, 1, 3, 3, 1, 1, P(ws), nb, stream()), 'nc_conv_fwd')
    else:
        ck(L().nc_conv_dgrad(P(dy), P(w), P(out), N, C, 1, H, W, K, 1, 3, 3, 1, 1, P(ws), nb, stream()), 'nc_conv_dgrad')
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()), 'an output element was not written'
    assert bool(torch.isnan(buf[n:]).all()), 'a write past the end of the output'
    return out


def test_the_switch_and_the_query():
    assert L().nc_get_conv2d_k3() == 1 and L().nc_conv2d_k3_num_cfgs() == 2
    N, C, K, H, W = R.K3_CASES[0][:5]
    assert L().nc_conv2d_k3_active(0, N, C, H, W, K) == 1 and L().nc_conv2d_k3_active(1, N, C, H, W, K) == 1
    assert L().nc_conv2d_k3_active(2, N, C, H, W, K) == 0          # the weight gradient stays on the gather GEMM
    with k3(on=0):
        assert L().nc_get_conv2d_k3() == 0
        assert L().nc_conv2d_k3_active(0, N, C, H, W, K) == 0 and L().nc_conv2d_k3_active(1, N, C, H, W, K) == 0
    with k3(direct=1):
        assert L().nc_conv2d_k3_active(0, N, C, H, W, K) == 0
    assert L().nc_get_conv2d_k3() == 1 and L().nc_conv2d_k3_active(0, N, C, H, W, K) == 1


@pytest.mark.parametrize('what', [0, 1], ids=['fwd', 'dgrad'])
@pytest.mark.parametrize('case', R.K3_CASES, ids=IDS)
def test_against_fp64_switch_on_and_off(case, what):
    """The kernel where it covers the call (asserted), the gather GEMM with the switch off: both under the yardstick; two runs are bit-equal; both
    tile configurations give the same bits."""
    N, C, K, H, W = case[:5]
    covered = R.k3_covered(what, N, C, K, H, W)
    assert L().nc_conv2d_k3_active(what, N, C, H, W, K) == (1 if covered else 0)
    ref, orc = reference(what, N, C, K, H, W)
    name = '%s %s' % (R.case_id(case[:5]), 'fwd' if what == 0 else 'dgrad')
    with k3(on=1):
        y = run(what, N, C, K, H, W)
        judge('k_conv2d_k3' if covered else 'gather GEMM', name, R.err(y, ref), orc)
        assert torch.equal(y, run(what, N, C, K, H, W))
    with k3(on=0):
        assert L().nc_conv2d_k3_active(what, N, C, H, W, K) == 0
        y_off = run(what, N, C, K, H, W)
        judge('gather GEMM', name + ' (switch off)', R.err(y_off, ref), orc)
    if covered:
        out_side = K if what == 0 else C
        for cfg in range(L().nc_conv2d_k3_num_cfgs()):
            with k3(on=1, cfg=cfg):
                assert torch.equal(run(what, N, C, K, H, W), y), 'tile configuration %d' % cfg
        assert out_side % 64 == 0


def test_the_launcher_picks_both_tiles():
    """conv2d_reference.k3_auto_cfg restates the launcher's rule; the cases reach both of its outcomes (and the test above ran each case on both)."""
    picks = {R.k3_auto_cfg(what, *c[:5]) for c in R.K3_CASES for what in (0, 1) if R.k3_covered(what, *c[:5])}
    assert picks == {0, 1}


@pytest.mark.parametrize('case', R.K3_OUTSIDE, ids=[R.case_id(c[:5]) for c in R.K3_OUTSIDE])
def test_shapes_outside_the_coverage_report_zero_and_still_compute(case):
    N, C, K, H, W = case[:5]
    for what in (0, 1):
        covered = R.k3_covered(what, N, C, K, H, W)
        assert L().nc_conv2d_k3_active(what, N, C, H, W, K) == (1 if covered else 0)
        ref, orc = reference(what, N, C, K, H, W)
        y = run(what, N, C, K, H, W)
        judge('k_conv2d_k3' if covered else 'gather GEMM', '%s %s' % (R.case_id(case[:5]), 'fwd' if what == 0 else 'dgrad'), R.err(y, ref), orc)
    assert not R.k3_covered(0, N, C, K, H, W)


def test_a_pinned_configuration_that_does_not_exist_is_the_launchers_choice():
    N, C, K, H, W = R.K3_CASES[0][:5]
    with k3(on=1):
        y = run(0, N, C, K, H, W)
    with k3(on=1, cfg=7):
        assert torch.equal(run(0, N, C, K, H, W), y)


def test_the_profiler_reports_the_kernel_under_its_own_path():
    """Path 13 / 'k3img' (12 is the learned-PSF kernels' number, 'lk'): cls of one forward and one data-gradient call at the smallest layer of
    K3_CASES both cover, and the tag ops.prof_stop() makes of it."""
    import ctypes
    from neuroclear_amd import ops
    N, C, K, H, W = min((c[:5] for c in R.K3_CASES if R.k3_covered(0, *c[:5]) and R.k3_covered(1, *c[:5])), key=lambda c: c[0] * c[1] * c[3] * c[4])
    cls, flop, ms = (ctypes.c_int * 4)(), (ctypes.c_double * 4)(), (ctypes.c_float * 4)()
    with k3(on=1):
        L().nc_prof_begin(0.0)
        run(0, N, C, K, H, W)
        run(1, N, C, K, H, W)
        assert L().nc_prof_end(4, cls, flop, ms) == 2
        assert [cls[0], cls[1]] == [0 | 13 << 4 | 3 << 8, 1 | 13 << 4 | 3 << 8]
        assert L().nc_conv_route(0, N, C, 1, H, W, K, 1, 3, 3, 1, 1, 0) & 255 == 13
        ops.prof_start()
        run(0, N, C, K, H, W)
        run(1, N, C, K, H, W)
        stats, _ = ops.prof_stop()
    assert sorted(stats) == ['dgrad_k3img_k3', 'fwd_k3img_k3'] and all(v[0] == 1 for v in stats.values())
