"""tests/conv2d_reference.py on the CPU: the float64 einsums are torch's float64 operators and autograd to 1e-12; the chain oracle evaluated in
float64 is the reference again (so its indexing and its order are right), and in float32 it is what it claims to be -- a serial fp32 sum whose
error against float64 is of the size of a chain of that length."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv2d_reference as R  # noqa: E402

SHAPES = [(2, 10, 6, (5, 13)), (1, 3, 5, (1, 3)), (2, 32, 16, (4, 6))]


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize('shape', SHAPES, ids=[R.case_id(s) for s in SHAPES])
def test_transposed_references_are_torch_float64(shape):
    x, w, b, dy = (t.double() for t in R.inputs(*shape))
    x, w, b = x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    y = F.conv_transpose2d(x, w, b, stride=2)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), dy)
    assert close(R.ref_fwd(x.detach(), w.detach(), b.detach()), y.detach())
    assert close(R.ref_fwd(x.detach(), w.detach()), F.conv_transpose2d(x, w, None, stride=2).detach())
    assert close(R.ref_dgrad(dy, w.detach()), dx)
    assert close(R.ref_wgrad(x.detach(), dy), dw)
    assert close(R.ref_dbias(dy), db)


@pytest.mark.parametrize('shape', SHAPES, ids=[R.case_id(s) for s in SHAPES])
def test_transposed_chain_in_float64_is_the_reference(shape):
    x, w, b, dy = R.inputs(*shape)
    f64 = torch.float64
    assert close(R.chain_fwd(x, w, b, f64), R.ref_fwd(x, w, b))
    assert close(R.chain_fwd(x, w, None, f64), R.ref_fwd(x, w))
    assert close(R.chain_dgrad(dy, w, f64), R.ref_dgrad(dy, w))
    assert close(R.chain_wgrad(x, dy, f64), R.ref_wgrad(x, dy))
    assert close(R.chain_dbias(dy, f64), R.ref_dbias(dy))


def _inputs3(N, C, K, H, W):
    g = torch.Generator().manual_seed(100 * C + K + H * W)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = 1.0 + 0.25 * torch.randn(K, generator=g)
    dy = torch.randn(N, K, H, W, generator=g)
    return x, w, b, dy


@pytest.mark.parametrize('shape', [(2, 6, 4, 5, 7), (1, 16, 8, 1, 3), (1, 3, 5, 2, 1)], ids=str)
def test_3x3_references_and_chain(shape):
    x, w, b, dy = _inputs3(*shape)
    xd, wd, bd = x.double().requires_grad_(True), w.double(), b.double()
    y = F.conv2d(xd, wd, bd, stride=1, padding=1)
    dx, = torch.autograd.grad(y, xd, dy.double())
    assert close(R.ref3_fwd(x, w, b), y.detach())
    assert close(R.ref3_dgrad(dy, w), dx)
    assert close(R.chain3_fwd(x, w, b, torch.float64), R.ref3_fwd(x, w, b))
    assert close(R.chain3_dgrad(dy, w, torch.float64), R.ref3_dgrad(dy, w))


def test_the_float32_chain_is_a_serial_sum():
    """At C = 256 the transposed forward's chain has 256 terms: its error against float64 is a rounding random walk of that length (rms between
    2^-24 and 256^0.5 * 2^-23 of the output's rms, far from exact and far from wrong).  torch's own fp32 operator is printed beside it."""
    x, w, b, dy = R.inputs(1, 256, 32, (5, 13))
    ref = R.ref_fwd(x, w)
    cmax, crms = R.err(R.chain_fwd(x, w), ref)
    tmax, trms = R.err(F.conv_transpose2d(x, w, None, stride=2), ref)
    print('chain max %.2e rms %.2e | torch fp32 max %.2e rms %.2e' % (cmax, crms, tmax, trms))
    assert 2.0 ** -24 < crms < 16 * 2.0 ** -23 and cmax < 64 * 2.0 ** -23
    # the 3 x 3 chain at C = 64 (576 terms)
    x3, w3, b3, dy3 = _inputs3(1, 64, 8, 6, 7)
    r3 = R.ref3_fwd(x3, w3)
    c3 = R.err(R.chain3_fwd(x3, w3), r3)
    t3 = R.err(F.conv2d(x3, w3, None, padding=1), r3)
    print('3x3 chain max %.2e rms %.2e | torch fp32 max %.2e rms %.2e' % (c3 + t3))
    assert 2.0 ** -24 < c3[1] < 24 * 2.0 ** -23


def test_cases_name_a_branch_of_every_kernel():
    fwd = {c[5] for c in R.FWD_CASES}
    assert fwd == {'mfma', 'fwd<4>', 'fwd<2>', 'fwd<1>'}
    assert {c[5] for c in R.DGRAD_CASES} == {'gemm', 'dgrad<8>', 'dgrad<4>', 'dgrad<1>'}
    assert {c[5].split(',')[0] if c[5].startswith('gemm') else c[5] for c in R.WGRAD_CASES} == {'gemm', 'wgrad<4,4>', 'wgrad<1,1>'}
    for C, K in R.UNET_PAIRS:
        for n in (R.P65, R.P3):
            for N in (1, 2):
                assert (N, C, K, n, None, 'mfma') in R.FWD_CASES
    assert len({R.case_id(c) for c in R.FWD_CASES}) == len(R.FWD_CASES)
