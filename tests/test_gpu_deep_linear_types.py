"""deep_linear_gen's position-typed evaluation (nc_set_dl_collapse(2), csrc/dl_typed.hip) against the float64 oracle, TYPE BY TYPE: the forward's
error per position type (27: low face / inside / high face per axis), the backward with dy on the whole volume, on one type at a time and on
one kernel family at a time -- at the extents where the boundary kernels' indexing changes (tests/deep_linear_reference.py: cases, reference,
yardstick and limits; tests/test_deep_linear_reference.py checks on the CPU that those limits tell an evaluation with uncorrected faces from the
right one by 100 x and more in every boundary type).

Which form ran is asserted from the forward's own word: bit 29 of `kept` (include/nc_hip.h, nc_deep_linear_fwd) is set in the typed arm and clear
in the fallback arm, so a planner change that sends the typed shapes back to nc_set_dl_collapse(1) fails here instead of passing unseen.

LIMITS.  Forward: every type's error (maximum over its voxels, over the largest |y|) <= min(3 Y + F_FLOOR, 1e-5), Y = the fp32 oracle's WORST
type on the same case.  Backward: relative L2 against float64 <= 3 x the fp32 oracle's own + 2e-5 for dx and each of the six weight gradients
(tests/test_gpu_grad_fp64.py's rule)."""
import contextlib
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deep_linear_reference as R  # noqa: E402
from neuroclear_amd import ops  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

DEV = 'cuda'
KEPT_TYPED = 1 << 29   # kKeptTyped, csrc/gen_nets.hip:686
F_FLOOR = 6e-7          # see test_forward_per_type


def _lib():
    from neuroclear_amd._lib import lib
    return lib()


@contextlib.contextmanager
def _switches(terms, collapse=2):
    L = _lib()
    prev = L.nc_get_split_terms(), L.nc_get_dl_collapse()
    try:
        L.nc_set_split_terms(terms)
        L.nc_set_dl_collapse(collapse)
        assert (L.nc_get_split_terms(), L.nc_get_dl_collapse()) == (terms, collapse)
        yield
    finally:
        L.nc_set_split_terms(prev[0])
        L.nc_set_dl_collapse(prev[1])


_NET = []


def _net():
    if not _NET:
        net = networks.define_G(1, 1, 64, 'deep_linear_gen', 'instance', False, 'kaiming', 0.02, [0])
        net.load_state_dict(S.state_dict_from_seed(S.deep_linear_spec(), R.W_SEED, DEV))
        _NET.append(net)
    return _NET[0]


@pytest.fixture(scope='module', autouse=True)
def _leave_nothing_behind():
    """the network and the oracle's cached runs live for this module only"""
    yield
    _NET.clear()
    R.clear()


def _inference(net, x):
    """The inference form, nc_deep_linear_fwd with saved == NULL, through the C ABI itself: under torch.no_grad() a Function's forward still sees
    needs_input_grad of its parameters, so ops._DeepLinear allocates `saved` and runs the training form there unless the parameters are frozen.
    -> y, kept"""
    L = _lib()
    packed = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).contiguous()
    assert packed.numel() == L.nc_deep_linear_param_floats()
    N, _, D, H, W = x.shape
    ws = torch.empty(L.nc_deep_linear_ws_bytes(N, D, H, W), dtype=torch.uint8, device=DEV)
    y = torch.full_like(x, float('nan'))
    kept = ctypes.c_uint(0)
    rc = L.nc_deep_linear_fwd(ops._ptr(packed), ops._ptr(x), ops._ptr(y), ops._ptr(None), N, D, H, W, ops._ptr(ws), ws.numel(), ops._stream(),
                              ctypes.byref(kept))
    assert rc == 0, (rc, L.nc_last_error())
    return y, kept.value


def _product(case, mask=None, want_dx=True, inference=False):
    """one forward + backward of the product under the case's switches: y, the forward's `kept`, dx (or None), {key: weight gradient} and, asked
    for, the inference form's (y, kept)"""
    shape, terms, _ = R.ALL_CASES[case]
    net = _net()
    x_np, r_np = R.inputs(shape, mask)
    with _switches(terms):
        for p in net.parameters():
            p.grad = None
        x = torch.from_numpy(x_np).to(DEV).requires_grad_(want_dx)
        y = net(x)
        kept = int(y.grad_fn.kept)
        (y * torch.from_numpy(r_np).to(DEV)).sum().backward()
        yi = None
        if inference:
            yi = _inference(net, x.detach().contiguous())
        torch.cuda.synchronize()
    return y.detach(), kept, (x.grad if want_dx else None), {k: p.grad.clone() for k, p in net.named_parameters()}, yi


def _form(case, kept):
    if case in R.TYPED_CASES:
        assert kept & KEPT_TYPED, '%s %s: the forward did not take the position-typed form (kept = %#x)' % (case, R.ALL_CASES[case][0], kept)
    else:
        assert not kept & KEPT_TYPED, '%s %s: the forward took the position-typed form (kept = %#x)' % (case, R.ALL_CASES[case][0], kept)


def _check_grads(case, mask, dx, g):
    (_, dx64, g64), (_, dx32, g32) = R.oracle(R.ALL_CASES[case][0], mask)
    rows = [('dx', dx, dx32, dx64)] + [(k, g[k], g32[k], g64[k]) for k in g64]
    out = [(k, R.rel(a, ref), R.rel(o, ref)) for k, a, o, ref in rows]
    for k, ep, eo in out:
        print('  %s mask %-8s %-24s fp32 oracle %.2e  product %.2e' % (case, mask, k, eo, ep))
    print('  %s mask %s worst ratio product / fp32 oracle: %.2f' % (case, mask, max(ep / max(eo, 1e-7) for _, ep, eo in out)))
    for k, ep, eo in out:
        assert ep <= R.FACTOR * eo + R.GRAD_FLOOR, (case, mask, k, ep, eo)


@pytest.mark.parametrize('case', list(R.ALL_CASES))
def test_forward_per_type(case):
    """Every position type of y within min(3 Y + F_FLOOR, 1e-5) of the float64 oracle, for the training forward and for the inference form.

    MEASURED on the MI355X (errors in units of 1e-7 of max |y|; Y = the fp32 oracle's worst type; inf. = the inference form's worst type).
    The training forward of the typed arm, per type (tz ty tx):
        type     A     B     C     D     E     F     G     H     I
         0 000 0.1   0.3   0.1   0.0   0.0   0.0   0.0   0.0   0.0
         1 001 1.3   1.4   1.3   1.8   1.4   1.4   1.1   0.8   2.3
         2 002 0.0   0.2   0.2   0.1   0.2   0.1   0.0   0.1   0.3
         3 010 1.2   1.3   0.9   2.4   1.4   1.7   1.7   1.6   1.5
         4 011 4.2   5.2   4.9   5.3   4.4   4.4   4.1   4.6   4.3
         5 012 1.3   1.8   1.6   1.4   1.6   1.0   1.7   1.6   1.1
         6 020 0.0   0.1   0.0   0.1   0.1   0.0   0.0   0.2   0.1
         7 021 0.7   1.8   1.1   1.7   1.2   1.6   1.8   1.1   1.7
         8 022 0.0   0.1   0.1   0.0   0.1   0.0   0.0   0.1   0.0
         9 100 0.5   0.2   0.3   0.1   0.2   0.2   0.2   0.2   0.3
        10 101 3.4   2.7   2.4   2.9   3.0   3.0   2.6   2.4   3.8
        11 102 0.2   0.3   0.3   0.3   0.3   0.4   0.1   0.2   0.3
        12 110 3.5   2.6   2.1   2.5   2.2   3.0   2.4   2.8   1.8
        13 111 2.2   2.8   2.4   2.7   3.2   2.9   2.4   2.8   2.8
        14 112 2.5   2.8   2.0   2.6   2.3   3.2   2.5   3.3   1.4
        15 120 0.2   0.4   0.4   0.2   0.2   0.3   0.2   0.2   0.2
        16 121 3.2   3.2   3.0   2.3   3.4   2.9   2.2   3.1   3.2
        17 122 0.5   0.4   0.7   0.3   0.4   0.1   0.2   0.3   0.3
        18 200 0.1   0.1   0.1   0.1   0.1   0.1   0.1   0.1   0.2
        19 201 1.9   1.6   2.0   1.4   1.7   1.6   0.7   1.6   3.0
        20 202 0.0   0.1   0.2   0.1   0.1   0.0   0.1   0.1   0.1
        21 210 1.7   1.0   1.6   1.2   1.1   1.1   1.7   1.7   1.1
        22 211 4.2   7.5   3.8   5.0   5.0   5.4   4.0   5.9   4.6
        23 212 1.1   1.7   1.1   1.6   1.0   1.4   1.6   1.8   0.7
        24 220 0.5   0.2   0.3   0.0   0.0   0.1   0.1   0.0   0.1
        25 221 1.8   1.7   1.4   1.6   1.2   1.2   1.1   1.1   2.0
        26 222 0.1   0.1   0.2   0.2   0.0   0.0   0.0   0.0   0.0
        Y      8.4  12.7   8.9  12.0   9.3   9.2   9.0   8.8   9.7
        inf.   6.1   7.4   5.4   5.5   6.6   6.1   4.8   5.5   6.6
    (the two z faces without their edges, types 4 and 22, are the product's worst in every case, at 0.44 .. 0.67 of the fp32 oracle's worst.)
    The fallback arm, worst type (always 13):
        below8    Y  9.6  product  2.8  inference  6.0
        w_mod4    Y  8.2  product  2.9  inference 15.1
        w196      Y  9.9  product  3.7  inference  9.4
        B_terms3  Y 12.7  product  6.6  inference  6.6
        w8        Y  6.9  product  3.1  inference  3.4
        w12       Y  9.9  product  3.4  inference  5.3
        w192      Y  8.8  product  3.8  inference  6.7
    F_FLOOR: 3 Y alone leaves every training forward a margin of 4.5 x and more (worst: H, 5.9 against 3 x 8.8) and every inference run 2 x
    and more except w_mod4 (W % 4 != 0: the inference form runs its first two layers on the plain fp32 kernels, 15.1 against 3 x 8.2 = 24.7).
    2 x 15.1 - 24.7 = 5.5, rounded up: F_FLOOR = 6e-7.  The limits are then 3.1e-6 .. 4.4e-6, below the cap of 1e-5."""
    shape = R.ALL_CASES[case][0]
    types = R.position_types(*shape[2:])
    (y64, _, _), (y32, _, _) = R.oracle(shape)
    y, kept, _, _, (yi, kept_i) = _product(case, inference=True)
    Y, P, I = (R.per_type_error(a, y64, types) for a in (y32, y, yi))
    lim = min(R.FACTOR * Y.max() + F_FLOOR, R.FWD_CAP)
    print('\n%s %s: limit %.2e (fp32 oracle worst type %.2e)' % (case, shape, lim, Y.max()))
    for tau in range(27):
        print('  type %2d (%d%d%d) %6d voxels  fp32 oracle %.2e  product %.2e  inference %.2e' %
              (tau, tau // 9, (tau // 3) % 3, tau % 3, R.type_count(tau, *shape[2:]), Y[tau], P[tau], I[tau]))
    print('  %s worst type: product %.2e (type %d), inference %.2e; ratio to the fp32 oracle\'s worst %.2f' %
          (case, P.max(), int(P.argmax()), I.max(), P.max() / Y.max()))
    _form(case, kept)
    assert not kept_i & KEPT_TYPED, hex(kept_i)   # (saved == NULL never takes the typed form: it keeps act0 for nobody)
    for tau in range(27):
        assert P[tau] <= lim, (case, tau, P[tau], lim)
        assert I[tau] <= lim, (case, 'inference', tau, I[tau], lim)


@pytest.mark.parametrize('case', list(R.ALL_CASES))
def test_backward_whole_dy(case):
    y, kept, dx, g, _ = _product(case)
    _form(case, kept)
    _check_grads(case, None, dx, g)


@pytest.mark.parametrize('tau', range(27))
@pytest.mark.parametrize('case', ['A', 'B'])
def test_backward_one_type(case, tau):
    """dy on ONE position type: everything flows through that type's H_tau and dH_tau, and dH_13 is a pure cancellation (the full correlation minus
    the boundary types' sums) -- a wrong progression of row numbers in k_dl_bnd_reduce or a wrong tap_ok in k_dl_p_from_dh shows here"""
    y, kept, dx, g, _ = _product(case, tau)
    _form(case, kept)
    _check_grads(case, tau, dx, g)


@pytest.mark.parametrize('group', R.GROUP_MASKS)
@pytest.mark.parametrize('case', ['E', 'F', 'G', 'H', 'I'])
def test_backward_one_kernel_family(case, group):
    """dy on the boundary rows (R: lanes along x), on the x faces (X: lanes along y through the transposed copies) or inside, at the segmented shapes"""
    y, kept, dx, g, _ = _product(case, group)
    _form(case, kept)
    _check_grads(case, group, dx, g)


@pytest.mark.parametrize('case', ['B', 'F'])
def test_bits_repeat_and_dx_is_optional(case):
    """two forward + backward passes give equal bits; without dx (x.requires_grad_(False): dx == NULL) the six weight gradients keep theirs"""
    y1, k1, dx1, g1, _ = _product(case)
    y2, k2, dx2, g2, _ = _product(case)
    y3, k3, dx3, g3, _ = _product(case, want_dx=False)
    for k in (k1, k2, k3):
        _form(case, k)
    assert k1 == k2 == k3
    assert torch.equal(y1, y2) and torch.equal(y1, y3) and torch.equal(dx1, dx2) and dx3 is None
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
        assert torch.equal(g1[k], g3[k]), k
