"""GPU parity of the 16-bit END-TO-END ("C8") operators through the C ABI (include/nc_hip.h, BASELINE.json configs[3]).

Every operator is compared with the same operation done by torch in fp32 on the SAME 16-bit values (so only summation
order and the final rounding to 16 bits differ):
  * nc_conv_fwd_c8 / nc_conv_dgrad_c8: bit-identical to nc_to_c8 of the fp32-output kernels' result (same accumulators,
    one rounding), also when written into a channel range of a wider buffer;
  * nc_c8_instnorm_*: statistics vs fp64 (1e-5), normalise + ReLU bit-identical to torch's bf16 rounding of the same
    fp32 expression, backward against float64 by the criterion of tests/c8_reference.py (half a bf16 ulp + the fp32 bound);
  * nc_c8_maxpool2_*: forward bit-identical; backward = skip + gradient routed to the FIRST maximum of each window;
  * nc_convT_k2s2_*_c8 against float64 on the rounded operands: 16-bit outputs by the same criterion, dw / dbias by the factor-3 rule;
  * whole-network nc_unet_deconv_lp_* / nc_deep_linear_lp_* against the layer-by-layer 16-bit path and fp32.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c8_reference as R8  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF, FP = 2, 1


@pytest.fixture(autouse=True)
def _restore_precision():
    from neuroclear_amd import ops
    yield
    ops.set_conv_precision('fp32')


def L():
    from neuroclear_amd import _lib
    return _lib.lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def ok(rc, what=''):
    assert rc == 0, (what, rc, L().nc_last_error())


def tdt(dt):
    return torch.bfloat16 if dt == BF else torch.float16


def to_c8(x, dt):
    """torch restatement of the layout: [N,C,...] fp32 -> [N, C/8, S, 8] 16-bit."""
    N, C = x.shape[:2]
    return x.reshape(N, C // 8, 8, -1).permute(0, 1, 3, 2).contiguous().to(tdt(dt))


def from_c8(xh, shape):
    N, C = shape[:2]
    return xh.float().permute(0, 1, 3, 2).reshape(shape).contiguous()


def ws(nbytes):
    return torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=DEV)


def test_layout_roundtrip_and_from_c8():
    from neuroclear_amd import ops
    x = torch.randn(2, 24, 3, 5, 7, device=DEV)
    for dt in (BF, FP):
        xh = ops.to_c8(x, dt)
        ref = to_c8(x, dt)
        assert torch.equal(xh.view(tdt(dt)).reshape(ref.shape), ref)
        y = torch.empty(2, 16, 3, 5, 7, device=DEV)
        ok(L().nc_from_c8(P(xh), 24, 8, P(y), 2, 16, ctypes.c_long(105), dt, None))
        assert torch.equal(y, ref.float().permute(0, 1, 3, 2).reshape(2, 24, 3, 5, 7)[:, 8:24])


@pytest.mark.parametrize('dt', [BF, FP])
@pytest.mark.parametrize('N,C,K,dims,ks', [(2, 32, 64, (5, 9, 13), 3), (1, 64, 128, (12, 12, 12), 3), (2, 64, 64, (6, 11, 23), 5)])
def test_conv_c8_bit_identical_to_fp32_output_kernels(N, C, K, dims, ks, dt):
    from neuroclear_amd import ops
    D, H, W = dims
    S = D * H * W
    pad = ks // 2
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(N, C, D, H, W, device=DEV, generator=g)
    w = torch.randn(K, C, ks, ks, ks, device=DEV, generator=g) / (C * ks ** 3) ** 0.5
    b = torch.randn(K, device=DEV, generator=g)
    dy = torch.randn(N, K, D, H, W, device=DEV, generator=g)
    ops.set_conv_precision('bf16' if dt == BF else 'fp16')
    xh = ops.to_c8(x, dt)
    y32 = ops.conv_fwd_raw(x, w, b, 1, pad, xh=xh)
    nb = L().nc_conv_lp_ws_bytes(N, C, D, H, W, K, ks, ks, ks, 1, pad)
    wsb = ws(nb)
    # dense output
    yh = torch.empty(N * K * S * 2, dtype=torch.uint8, device=DEV)
    ok(L().nc_conv_fwd_c8(P(xh), P(w), P(b), P(yh), K, 0, N, C, D, H, W, K, ks, ks, ks, 1, pad, dt, P(wsb), ctypes.c_size_t(wsb.numel()), None))
    assert torch.equal(yh, ops.to_c8(y32, dt))
    # into channels [K, 2K) of a 2K + 8 channel buffer; the rest must stay untouched
    ctot = 2 * K + 8
    buf = torch.full((N * ctot * S * 2,), 0x5a, dtype=torch.uint8, device=DEV)
    ok(L().nc_conv_fwd_c8(P(xh), P(w), P(b), P(buf), ctot, K, N, C, D, H, W, K, ks, ks, ks, 1, pad, dt, P(wsb), ctypes.c_size_t(wsb.numel()), None))
    v = buf.view(N, ctot // 8, S * 16)
    assert torch.equal(v[:, K // 8:2 * K // 8].reshape(-1), yh)
    assert bool((v[:, :K // 8] == 0x5a).all()) and bool((v[:, 2 * K // 8:] == 0x5a).all())
    # data gradient (bf16 operands in both modes); needs C % 64 == 0
    if not L().nc_conv_lp_supported(1, N, C, D, H, W, K, ks, ks, ks, 1, pad):
        return
    ops.set_conv_precision('bf16')
    dyh = ops.to_c8(dy, BF)
    dx32 = ops.conv_dgrad_raw(dy, w, x.shape, 1, pad, dyh=dyh)
    dxh = torch.empty(N * C * S * 2, dtype=torch.uint8, device=DEV)
    ok(L().nc_conv_dgrad_c8(P(dyh), P(w), P(dxh), N, C, D, H, W, K, ks, ks, ks, 1, pad, BF, P(wsb), ctypes.c_size_t(wsb.numel()), None))
    assert torch.equal(dxh, ops.to_c8(dx32, BF))


@pytest.mark.parametrize('dt', [BF, FP])
@pytest.mark.parametrize('N,C,dims,slope', [(2, 16, (6, 10, 14), 0.0), (1, 64, (20, 20, 20), 0.0), (3, 8, (1, 33, 17), 0.2)])
def test_c8_instnorm_forward_and_backward(N, C, dims, slope, dt):
    from neuroclear_amd import ops
    D, H, W = dims
    S = D * H * W
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(N, C, D, H, W, device=DEV, generator=g) * 1.7 + 0.6
    xh = ops.to_c8(x, dt)
    xr = x.to(tdt(dt)).float()
    mean = torch.empty(N * C, device=DEV)
    rstd = torch.empty(N * C, device=DEV)
    wsb = ws(L().nc_c8_instnorm_ws_bytes(N, C, ctypes.c_long(S)))
    ok(L().nc_c8_instnorm_stats(P(xh), N, C, ctypes.c_long(S), ctypes.c_float(1e-5), P(mean), P(rstd), dt, P(wsb),
                                ctypes.c_size_t(wsb.numel()), None))
    m64 = xr.double().mean((2, 3, 4)).reshape(-1)
    v64 = xr.double().var((2, 3, 4), unbiased=False).reshape(-1)
    assert float((mean.double() - m64).abs().max()) < 1e-5
    assert float((rstd.double() * torch.sqrt(v64 + 1e-5) - 1).abs().max()) < 1e-5
    # normalise + activation into channels [8, 8 + C) of a wider buffer: bit-identical to torch's rounding of the same fp32 expression
    ctot = C + 16
    buf = torch.zeros(N * ctot * S * 2, dtype=torch.uint8, device=DEV)
    ok(L().nc_c8_instnorm_act_fwd(P(xh), P(mean), P(rstd), ctypes.c_float(slope), P(buf), ctot, 8, N, C, ctypes.c_long(S), dt, None))
    t = (xr - mean.view(N, C, 1, 1, 1)) * rstd.view(N, C, 1, 1, 1)
    yref = torch.where(t > 0, t, t * slope)
    got = buf.view(tdt(dt)).reshape(N, ctot // 8, S, 8)[:, 1:1 + C // 8]
    assert torch.equal(got, to_c8(yref, dt))
    # backward against its float64 restatement on the rounded tensors (gradient operands are bf16)
    gy = torch.randn(N, C, D, H, W, device=DEV, generator=g)
    gbuf = torch.zeros(N * ctot * S * 2, dtype=torch.uint8, device=DEV)
    gbuf.view(torch.bfloat16).reshape(N, ctot // 8, S, 8)[:, 1:1 + C // 8] = to_c8(gy, BF)
    dxh = torch.empty(N * C * S * 2, dtype=torch.uint8, device=DEV)
    db = torch.empty(C, device=DEV)
    ok(L().nc_c8_instnorm_act_bwd(P(gbuf), ctot, 8, P(xh), P(mean), P(rstd), ctypes.c_float(slope), P(dxh), P(db), N, C, ctypes.c_long(S),
                                  dt, P(wsb), ctypes.c_size_t(wsb.numel()), None))
    got = from_c8(dxh.view(torch.bfloat16).reshape(N, C // 8, S, 8), x.shape)
    # the criterion of tests/c8_reference.py: within half a bf16 ulp of the float64 value plus the fp32 evaluation bound, element by element
    ref, e = R8.ref_norm_bwd(gy.to(torch.bfloat16).reshape(N, C, S), x.to(tdt(dt)).reshape(N, C, S), mean.view(N, C), rstd.view(N, C), slope)
    inside, excess = R8.within_half_ulp(got.reshape(N, C, S), ref, e, BF)
    assert inside, excess
    assert bool((db.double().abs() <= R8.dbias_limit(ref)).all())  # sum of dx per channel: zero up to rounding


@pytest.mark.parametrize('dt', [BF, FP])
def test_c8_maxpool_forward_and_backward_add(dt):
    from neuroclear_amd import ops
    N, C, D, H, W = 2, 16, 6, 8, 10
    S, So = D * H * W, D * H * W // 8
    g = torch.Generator(device=DEV).manual_seed(3)
    # coarse values so that ties inside a window DO occur: the first maximum must win
    x = (torch.randint(-3, 4, (N, C, D, H, W), device=DEV, generator=g)).float() * 0.5
    ctot = C + 8
    xb = torch.zeros(N, ctot // 8, S, 8, dtype=tdt(dt), device=DEV)
    xb[:, 1:] = to_c8(x, dt)
    yh = torch.empty(N * C * So * 2, dtype=torch.uint8, device=DEV)
    ok(L().nc_c8_maxpool2_fwd(P(xb), ctot, 8, P(yh), N, C, D, H, W, dt, None))
    ref = F.max_pool3d(x, 2)
    assert torch.equal(yh.view(tdt(dt)).reshape(N, C // 8, So, 8), to_c8(ref, dt))
    dp = torch.randn(N, C, D // 2, H // 2, W // 2, device=DEV, generator=g)
    skip = torch.randn(N, C, D, H, W, device=DEV, generator=g)
    sb = torch.zeros(N, ctot // 8, S, 8, dtype=torch.bfloat16, device=DEV)
    sb[:, :C // 8] = to_c8(skip, BF)
    dxh = torch.empty(N * C * S * 2, dtype=torch.uint8, device=DEV)
    ok(L().nc_c8_maxpool2_bwd_add(P(to_c8(dp, BF)), P(xb), ctot, 8, P(sb), ctot, 0, P(dxh), N, C, D, H, W, dt, None))
    # reference: windows as a trailing axis of 8 in scan order (a, b, c); torch.argmax returns the FIRST maximum
    xw = x.reshape(N, C, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(N, C, D // 2, H // 2, W // 2, 8)
    arg = xw.argmax(-1)
    gw = torch.zeros_like(xw)
    gw.scatter_(-1, arg.unsqueeze(-1), dp.to(torch.bfloat16).float().unsqueeze(-1))
    gfull = gw.reshape(N, C, D // 2, H // 2, W // 2, 2, 2, 2).permute(0, 1, 2, 5, 3, 6, 4, 7).reshape(N, C, D, H, W)
    want = (skip.to(torch.bfloat16).float() + gfull).to(torch.bfloat16)
    got = dxh.view(torch.bfloat16).reshape(N, C // 8, S, 8)
    assert torch.equal(got, to_c8(want.float(), BF))


@pytest.mark.parametrize('N,C,K,dims', [(2, 64, 32, (3, 5, 7)), (1, 256, 128, (6, 6, 6)), (3, 128, 64, (4, 9, 10))])
def test_convT_c8(N, C, K, dims):
    D, H, W = dims
    Sc, Sf = D * H * W, 8 * D * H * W
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(N, C, D, H, W, device=DEV, generator=g)
    w = torch.randn(C, K, 2, 2, 2, device=DEV, generator=g) / C ** 0.5
    b = torch.randn(K, device=DEV, generator=g)
    dy = torch.randn(N, K, 2 * D, 2 * H, 2 * W, device=DEV, generator=g)
    wsb = ws(L().nc_convT_c8_ws_bytes(N, C, D, H, W, K))
    nb = ctypes.c_size_t(wsb.numel())
    ctot = 2 * K
    out = torch.zeros(N, ctot // 8, Sf, 8, dtype=torch.bfloat16, device=DEV)
    ok(L().nc_convT_k2s2_fwd_c8(P(to_c8(x, BF)), P(w), P(b), P(out), ctot, K, N, C, D, H, W, K, BF, P(wsb), nb, None))
    x16, w16, dy16 = x.to(torch.bfloat16), w.to(torch.bfloat16), dy.to(torch.bfloat16)
    ref, e = R8.ref_convt_fwd(x16, w16, b)
    got = from_c8(out[:, K // 8:], ref.shape)
    inside, excess = R8.within_half_ulp(got, ref, e, BF)
    assert inside, excess
    assert float(out[:, :K // 8].float().abs().max()) == 0.0
    # dgrad: dy lives in channels [K, 2K) of the wide buffer
    dyb = torch.zeros(N, ctot // 8, Sf, 8, dtype=torch.bfloat16, device=DEV)
    dyb[:, K // 8:] = to_c8(dy, BF)
    dxh = torch.empty(N, C // 8, Sc, 8, dtype=torch.bfloat16, device=DEV)
    ok(L().nc_convT_k2s2_dgrad_c8(P(dyb), ctot, K, P(w), P(dxh), N, C, D, H, W, K, P(wsb), nb, None))
    ref, e = R8.ref_convt_dgrad(dy16, w16)
    got = from_c8(dxh, ref.shape)
    inside, excess = R8.within_half_ulp(got, ref, e, BF)
    assert inside, excess
    # wgrad + bias gradient (fp32 results)
    dw = torch.empty_like(w)
    db = torch.empty(K, device=DEV)
    ok(L().nc_convT_k2s2_wgrad_c8(P(to_c8(x, BF)), P(dyb), ctot, K, P(dw), P(db), N, C, D, H, W, K, P(wsb), nb, None))
    # fp32 results: the factor-3 rule of tests/convt_reference.py against torch's fp32 operator on the CPU
    odw, odb = R8.oracle_convt_wgrad(x16, w16, dy16)
    rdw, rdb = R8.CR.ref_wgrad(x16, dy16), R8.CR.ref_dbias(dy16)
    assert R8.CR.within(R8.CR.err(dw, rdw), R8.CR.err(odw.to(DEV), rdw))
    assert R8.CR.within(R8.CR.err(db, rdb), R8.CR.err(odb.to(DEV), rdb))


@pytest.mark.parametrize('ks', [3, 7])
@pytest.mark.parametrize('N,dims', [(1, (9, 12, 20)), (2, (8, 17, 33)), (1, (20, 40, 148))])
def test_one_channel_layers_pseudo_channel_form(N, dims, ks):
    """Conv3d(1, 64, ks) forward and its data gradient on the 16-bit cores (taps along x folded into 8 pseudo-channels)
    against torch on the bf16-rounded operands; the result is rounded to bf16 once (forward) / the 8 partial sums per
    voxel are rounded to bf16 before the fold (data gradient): 2^-7 of the largest value."""
    D, H, W = dims
    S = D * H * W
    g = torch.Generator(device=DEV).manual_seed(6)
    x = torch.randn(N, 1, D, H, W, device=DEV, generator=g)
    w = torch.randn(64, 1, ks, ks, ks, device=DEV, generator=g) / ks ** 1.5
    b = torch.randn(64, device=DEV, generator=g)
    dy = torch.randn(N, 64, D, H, W, device=DEV, generator=g)
    xr, wr, dyr = x.to(torch.bfloat16).float(), w.to(torch.bfloat16).float(), dy.to(torch.bfloat16).float()
    nb = L().nc_conv_c1_c8_ws_bytes(N, D, H, W, ks)
    assert nb > 0
    wsb = ws(nb)
    ctot = 64 + 16
    out = torch.zeros(N, ctot // 8, S, 8, dtype=torch.bfloat16, device=DEV)
    ok(L().nc_conv_c1_fwd_c8(P(x), P(w), P(b), P(out), ctot, 8, N, D, H, W, ks, BF, P(wsb), ctypes.c_size_t(wsb.numel()), None))
    ref = F.conv3d(xr, wr, b, padding=ks // 2)
    got = from_c8(out[:, 1:9], ref.shape)
    assert float((got - ref).abs().max()) <= 2 ** -7 * float(ref.abs().max())
    assert float(out[:, 0].float().abs().max()) == 0.0 and float(out[:, 9].float().abs().max()) == 0.0
    dx = torch.empty(N, 1, D, H, W, device=DEV)
    ok(L().nc_conv_c1_dgrad_c8(P(to_c8(dy, BF)), P(w), P(dx), N, D, H, W, ks, P(wsb), ctypes.c_size_t(wsb.numel()), None))
    ref = F.conv_transpose3d(dyr, wr, padding=ks // 2)
    assert float((dx - ref).abs().max()) <= 2 ** -7 * float(ref.abs().max())
    assert float((dx - ref).abs().mean()) <= 2 ** -9 * float(ref.abs().max())
    # weight gradient on the 16-bit cores (c1_wgrad_h.hip): exact products of the bf16-rounded operands, fp32 accumulation
    nbw = L().nc_conv_c1_wgrad_c8_ws_bytes(N, D, H, W, ks)
    assert nbw > 0
    wsw = ws(nbw)
    dw = torch.empty(64, 1, ks, ks, ks, device=DEV)
    ok(L().nc_conv_c1_wgrad_c8(P(x), P(to_c8(dy, BF)), P(dw), N, D, H, W, ks, P(wsw), ctypes.c_size_t(wsw.numel()), None))
    refw = torch.nn.grad.conv3d_weight(xr.double(), w.shape, dyr.double(), padding=ks // 2)
    assert float((dw.double() - refw).abs().max()) <= 1e-4 * float(refw.abs().max()), float((dw.double() - refw).abs().max() / refw.abs().max())
    dw2 = torch.empty_like(dw)
    ok(L().nc_conv_c1_wgrad_c8(P(x), P(to_c8(dy, BF)), P(dw2), N, D, H, W, ks, P(wsw), ctypes.c_size_t(wsw.numel()), None))
    assert torch.equal(dw, dw2)


def _nets():
    from neuroclear_amd.models import networks
    from neuroclear_amd.util import seed as S
    ga = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0])
    ga.load_state_dict(S.state_dict_from_seed(S.unet_deconv_spec(), 11, device=DEV))
    gb = networks.define_G(1, 1, 64, 'deep_linear_gen', 'instance', False, 'kaiming', 0.02, [0])
    gb.load_state_dict(S.state_dict_from_seed(S.deep_linear_spec(), 12, device=DEV))
    return ga, gb


@pytest.mark.parametrize('kind,shape', [('unet', (1, 1, 32, 32, 32)), ('unet', (2, 1, 24, 32, 40)), ('linear', (1, 1, 24, 24, 24)),
                                        ('linear', (2, 1, 16, 20, 28))])
def test_whole_network_16bit_paths(kind, shape, monkeypatch):
    """nc_unet_deconv_lp_* / nc_deep_linear_lp_* (bf16 activations end to end) against (a) the layer-by-layer 16-bit path
    (fp32 tensors between the layers) and (b) fp32: outputs within the 16-bit tolerance of DESIGN.md 2 (after the sigmoid
    |err| <= 1.5e-2, mean <= 3e-3; deep_linear 2e-2 of the largest value), weight gradients of the big layers within
    2.5 x the change a 1e-3 relative input perturbation causes in pure fp32, + 3 % (ReLU / max-pool flips dominate)."""
    from neuroclear_amd import ops
    from neuroclear_amd.models import networks
    ga, gb = _nets()
    net = ga if kind == 'unet' else gb
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.rand(shape, device=DEV, generator=gen)
    r = torch.randn(shape, device=DEV, generator=gen)
    noise = 1 + 1e-3 * torch.randn(shape, device=DEV, generator=gen)

    def run(prec, fused, xi):
        ops.set_conv_precision(prec)
        monkeypatch.setattr(networks, '_FUSED_GEN', fused)
        assert (not fused) or prec == 'fp32' or ops.gen_lp_supported(kind, xi.shape)
        for q in net.parameters():
            q.grad = None
        xi = xi.clone().requires_grad_(True)
        y = net(xi)
        (y * r).mean().backward()
        ops.set_conv_precision('fp32')
        return y.detach().clone(), xi.grad.clone(), {n: q.grad.clone() for n, q in net.named_parameters()}

    y32, dx32, g32 = run('fp32', True, x)
    _, _, gp = run('fp32', True, x * noise)
    yl, dxl, gl = run('bf16', False, x)   # layer by layer
    yw, dxw, gw = run('bf16', True, x)    # whole-network, C8 end to end
    scale = 1.0 if kind == 'unet' else float(y32.abs().max())
    for y16 in (yl, yw):
        assert float((y16 - y32).abs().max()) <= (1.5e-2 if kind == 'unet' else 2e-2) * scale
        assert float((y16 - y32).abs().mean()) <= 3e-3 * scale
    assert float((yw - yl).abs().max()) <= 1.5e-2 * scale
    assert float((dxw - dx32).norm() / dx32.norm()) <= 2.5 * float((run('fp32', True, x * noise)[1] - dx32).norm() / dx32.norm()) + 0.05
    for n, g in g32.items():
        if g.dim() == 5 and g.numel() >= 4096:
            floor = float((gp[n] - g).norm() / g.norm())
            rel = float((gw[n] - g).norm() / g.norm())
            assert rel <= 2.5 * floor + 0.03, (n, rel, floor)
            assert torch.isfinite(gw[n]).all()


@pytest.mark.parametrize('shape', [(1, 1, 24, 24, 24), (2, 1, 16, 20, 28), (1, 1, 40, 40, 40)])
def test_deep_linear_16bit_collapsed_tail(shape):
    """nc_deep_linear_lp_* with layers 2 .. 5 in collapsed form (nc_set_dl_collapse, default on; csrc/gen_nets_lp.hip: the 64 -> 1 convolution is
    the data-gradient form of the one-channel 3^3 kernel with the composed weights, q its weight gradient with dy as the image, df2 its forward)
    against the layered 16-bit evaluation and against fp32: the output within the 16-bit tolerance, EVERY parameter gradient -- the three
    small pointwise tensors too -- as close to fp32 as the layered 16-bit path is, or closer."""
    from neuroclear_amd import ops
    from neuroclear_amd._lib import lib
    _, net = _nets()
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.rand(shape, device=DEV, generator=gen)
    r = torch.randn(shape, device=DEV, generator=gen)
    prev = lib().nc_get_dl_collapse()

    def run(prec, collapse):
        lib().nc_set_dl_collapse(collapse)
        ops.set_conv_precision(prec)
        assert prec == 'fp32' or ops.gen_lp_supported('linear', x.shape)
        for q in net.parameters():
            q.grad = None
        xi = x.clone().requires_grad_(True)
        y = net(xi)
        (y * r).mean().backward()
        ops.set_conv_precision('fp32')
        return y.detach().clone(), xi.grad.clone(), {n: q.grad.clone() for n, q in net.named_parameters()}

    try:
        y32, dx32, g32 = run('fp32', 0)
        yl, dxl, gl = run('bf16', 0)
        yc, dxc, gc = run('bf16', 1)
    finally:
        lib().nc_set_dl_collapse(prev)
        ops.set_conv_precision('fp32')
    scale = float(y32.abs().max())
    assert float((yc - y32).abs().max()) <= 2e-2 * scale and float((yc - y32).abs().mean()) <= 3e-3 * scale
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    print('dx: layered %.2e collapsed %.2e' % (rel(dxl, dx32), rel(dxc, dx32)))
    assert rel(dxc, dx32) <= 1.5 * rel(dxl, dx32) + 5e-3
    for n in g32:
        a, b = rel(gl[n], g32[n]), rel(gc[n], g32[n])
        print('%-24s layered %.2e collapsed %.2e' % (n, a, b))
        assert b <= 1.5 * a + 5e-3, (n, a, b)


@pytest.mark.parametrize('fwd_collapse', [1, 0])
def test_deep_linear_16bit_backward_follows_its_forward_when_the_switch_moves(fwd_collapse):
    """nc_deep_linear_lp_fwd hands the form it took to the caller (`kept`), nc_deep_linear_lp_bwd follows it: with
    nc_set_dl_collapse flipped BETWEEN a forward and its backward, every gradient is bit-identical to the run where the switch stood still
    (before round 6 the backward read buffers its forward had never written).  A `kept` the forward cannot return is refused."""
    from neuroclear_amd import ops
    from neuroclear_amd._lib import lib
    _, net = _nets()
    gen = torch.Generator(device=DEV).manual_seed(11)
    shape = (1, 1, 24, 24, 24)
    x = torch.rand(shape, device=DEV, generator=gen)
    r = torch.randn(shape, device=DEV, generator=gen)
    prev = lib().nc_get_dl_collapse()

    def run(flip):
        lib().nc_set_dl_collapse(fwd_collapse)
        ops.set_conv_precision('bf16')
        assert ops.gen_lp_supported('linear', x.shape)
        for q in net.parameters():
            q.grad = None
        xi = x.clone().requires_grad_(True)
        y = net(xi)
        if flip:
            lib().nc_set_dl_collapse(1 - fwd_collapse)
        (y * r).mean().backward()
        ops.set_conv_precision('fp32')
        return xi.grad.clone(), {n: q.grad.clone() for n, q in net.named_parameters()}

    try:
        dx0, g0 = run(False)
        dx1, g1 = run(True)
    finally:
        lib().nc_set_dl_collapse(prev)
        ops.set_conv_precision('fp32')
    assert torch.equal(dx0, dx1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
        assert float(g0[n].abs().max()) > 0
    # raw C ABI: an impossible `kept`
    L = lib()
    I, Z = ctypes.c_int, ctypes.c_size_t
    dims = (I(1), I(24), I(24), I(24))
    packed = torch.cat([q.detach().reshape(-1) for q in net.parameters()]).contiguous()
    saved = torch.empty(L.nc_deep_linear_lp_saved_bytes(*dims), dtype=torch.uint8, device=DEV)
    ws = torch.empty(L.nc_deep_linear_lp_ws_bytes(*dims), dtype=torch.uint8, device=DEV)
    dpar, dxb = torch.zeros_like(packed), torch.empty_like(x)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.nc_deep_linear_lp_bwd(p(packed), p(x), p(saved), p(r), p(dxb), p(dpar), *dims, I(ops._DT['bf16']), p(ws), Z(ws.numel()),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.c_uint(7))
    assert rc != 0


@pytest.mark.parametrize('seed', [1, 2, 3, 21, 22])
def test_deep_linear_16bit_weights_keep_the_response_to_a_constant(seed):
    """deep_linear_gen has neither biases nor norms, and for the nearly constant `fake` of the first iterations its output is a
    heavily cancelling sum of the layers' responses to a constant -- the tap sums of the (co, ci) pairs.  The 16-bit whole-
    network path therefore rounds this stack's weights tap-diffused (conv_h.hip, wvalue): the running sums of the rounded
    weights follow the exact ones, and the systematic part of the output error disappears in the (zero-mean) rounding noise
    of the activations.  Measured (tools/w_diffuse_check.py): |mean error| / rms error 0.01-0.11 diffused, 0.43-0.81 with
    round-to-nearest weights; the test asks for <= 0.25."""
    from neuroclear_amd import ops
    from neuroclear_amd.models import networks
    torch.manual_seed(seed)
    net = networks.define_G(1, 1, 64, 'deep_linear_gen', 'instance', False, 'kaiming', 0.02, [0])
    x = 0.5 + 0.0116 * torch.randn(2, 1, 40, 40, 40, device=DEV)
    with torch.enable_grad():
        y32 = net(x).detach()
        ops.set_conv_precision('bf16')
        try:
            assert ops.gen_lp_supported('linear', x.shape)
            y16 = net(x).detach()
        finally:
            ops.set_conv_precision('fp32')
    d = (y16 - y32).double()
    bias, rms = abs(float(d.mean())), float(d.pow(2).mean().sqrt())
    assert rms <= 2.5e-2 and bias <= 0.25 * rms, (bias, rms)
