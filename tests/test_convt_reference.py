"""CPU: the reference helper of the op-level ConvTranspose3d tests (tests/convt_reference.py) is itself held to torch's float64 operator, and the
fp32 oracle is a usable yardstick (finite, non-degenerate) at every case tests/test_gpu_convt.py lists."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convt_reference as R  # noqa: E402


@pytest.mark.parametrize('N,C,K,n', [(2, 5, 3, (2, 3, 4)), (1, 12, 8, (3, 1, 5))])
def test_einsum_reference_is_the_float64_operator(N, C, K, n):
    """Forward (with and without bias) and the three gradients of the einsum against F.conv_transpose3d + autograd in float64, to 1e-12 of the
    largest magnitude."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, C, *n, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(C, K, 2, 2, 2, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(K, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(N, K, *(2 * v for v in n), generator=g, dtype=torch.float64)
    y = F.conv_transpose3d(x, w, b, stride=2)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), dy)

    def close(a, r):
        assert a.shape == r.shape and a.dtype == torch.float64
        assert float((a - r).abs().max()) <= 1e-12 * float(r.abs().max())
    close(R.ref_fwd(x.detach(), w.detach(), b.detach()), y.detach())
    close(R.ref_fwd(x.detach(), w.detach()), F.conv_transpose3d(x, w, None, stride=2).detach())
    close(R.ref_dgrad(dy, w.detach()), dx)
    close(R.ref_wgrad(x.detach(), dy), dw)
    close(R.ref_dbias(dy), db)


def test_error_measure_and_limit():
    ref = torch.tensor([3.0, -4.0, 0.0, 5.0], dtype=torch.float64)
    s = math.sqrt(50.0 / 4)
    m, r = R.err(torch.tensor([3.0, -4.5, 0.0, 5.0]), ref)
    assert m == pytest.approx(0.5 / s) and r == pytest.approx(0.25 / s)
    assert R.within((3e-7 + 2.0 ** -21, 3e-8 + 2.0 ** -23), (1e-7, 1e-8))
    assert not R.within((3.01e-7 + 2.0 ** -21, 0.0), (1e-7, 1e-8)) and not R.within((0.0, 3.01e-8 + 2.0 ** -23), (1e-7, 1e-8))
    assert R.within((0.0, 0.0), (0.0, 0.0))


def _finite_yardstick(o, what):
    assert math.isfinite(o[0]) and math.isfinite(o[1]) and o[1] <= o[0], (what, o)
    assert o[0] < 1e-5, (what, o)      # an fp32 evaluation: a yardstick this far off would let anything pass
    assert R.within(o, o)


FWD_SHAPES = sorted({c[:4] for c in R.FWD_CASES + R.SPLIT_CASES + R.S3_CASES})
BWD_SHAPES = sorted({c[:4] for c in R.DGRAD_CASES + R.WGRAD_CASES})


@pytest.mark.parametrize('shape', FWD_SHAPES, ids=[R.case_id(s) for s in FWD_SHAPES])
def test_fp32_oracle_forward_is_a_yardstick(shape):
    x, w, b, _ = R.inputs(*shape)
    lin = R.ref_fwd(x, w)
    for with_bias in (True, False):
        ref = lin + b.double().view(1, -1, 1, 1, 1) if with_bias else lin
        o = R.err(F.conv_transpose3d(x, w, b if with_bias else None, stride=2), ref)
        print('%s bias %d: oracle max %.2e rms %.2e' % (shape, with_bias, o[0], o[1]))
        _finite_yardstick(o, (shape, with_bias))


@pytest.mark.parametrize('shape', BWD_SHAPES, ids=[R.case_id(s) for s in BWD_SHAPES])
def test_fp32_oracle_gradients_are_yardsticks(shape):
    x, w, b, dy = R.inputs(*shape)
    dx, dw, db = R.oracle_bwd(*shape)
    for name, got, ref in (('dx', dx, R.ref_dgrad(dy, w)), ('dw', dw, R.ref_wgrad(x, dy)), ('db', db, R.ref_dbias(dy))):
        o = R.err(got, ref)
        print('%s %s: oracle max %.2e rms %.2e' % (shape, name, o[0], o[1]))
        _finite_yardstick(o, (shape, name))
