"""CPU checks of tests/kgan_reference.py, the reference side of tests/test_gpu_kernelgan_fp64.py: the stage references composed equal float64
autograd of the layered network; the fp32 emulations of the kernels' orders stay within the limits of their references and deliberately wrong
variants do not; the restated geometry, plan and saved layout equal the library's host-side answers; every label has a case."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kgan_reference as K  # noqa: E402
import norm_reference as N  # noqa: E402


@pytest.mark.parametrize('nd,shape', [(2, (2, 1, 13, 11)), (3, (1, 1, 9, 10, 8))])
def test_stage_references_composed_equal_fp64_autograd_of_the_layered_network(nd, shape):
    """y, dx and all ten parameter gradients (the construction of tests/test_kernelgan.py::test_collapse_algebra_fp64), to 1e-11."""
    conv = F.conv2d if nd == 2 else F.conv3d
    p32 = K.unpack(K.params(nd), nd)
    p = {k: v.double() for k, v in p32.items()}
    k7, k1 = (7,) * nd, (1,) * nd
    prm = [p['W1'].reshape(64, 1, *k7), p['b1'], p['W2'].reshape(64, 64, *k1), p['b2'], p['W3'].reshape(64, 64, *k1), p['b3'],
           p['W4'].reshape(64, 64, *k1), p['b4'], p['W5'].reshape(1, 64, *k1), p['b5']]
    prm = [t.clone().requires_grad_(True) for t in prm]
    w1, b1, w2, b2, w3, b3, w4, b4, w5, b5 = prm
    x = (torch.from_numpy(np.random.default_rng(3).random(shape)) - 0.5).requires_grad_(True)
    h = F.relu(F.instance_norm(conv(conv(x, w1, b1), w2, b2), eps=K.EPS))
    h = F.relu(F.instance_norm(conv(h, w3, b3), eps=K.EPS))
    h = F.relu(F.instance_norm(conv(h, w4, b4), eps=K.EPS))
    y = conv(h, w5, b5)
    dy = torch.from_numpy(np.random.default_rng(4).standard_normal(tuple(y.shape)))
    (y * dy).sum().backward()

    B = shape[0]
    D, H, W = (shape[2:] if nd == 3 else (1,) + tuple(shape[2:]))
    g, code = K.geo(B, D, H, W, nd)
    assert code == K.NC_OK
    xs = x.detach().reshape(B, D, H, W)
    fwd = K.ref_forward(xs, p, g)
    assert float((fwd['y'] - y.detach().reshape(B, g.P)).abs().max()) <= 1e-11 * float(y.detach().abs().max())
    bwd = K.ref_backward(xs, dy.reshape(B, g.P), fwd, p, g)
    assert float((bwd['dx'] - x.grad.reshape(B, D, H, W)).abs().max()) <= 1e-11 * float(x.grad.abs().max())
    wscale = max(float(t.grad.abs().max()) for t in prm if t.dim() > 1)
    for name, got, t in zip(K.GRAD_NAMES, K.pack_grads(bwd), prm):
        # db1 .. db4 are zero up to rounding (the InstanceNorm behind them cancels any bias): judged on the weight gradients' scale
        scale = wscale if name in ('db1', 'db2', 'db3', 'db4') else float(t.grad.abs().max())
        assert float((got.reshape(-1) - t.grad.reshape(-1)).abs().max()) <= 1e-11 * scale, name


def blocked_1x1(a, W, b):
    """k_kg_1x1's own order in fp32: the matrix core adds four products (channels 4 ks .. 4 ks + 3) to the accumulator per step."""
    acc = torch.zeros_like(a)
    for ks in range(16):
        blk = torch.zeros_like(a)
        for k in range(4 * ks, 4 * ks + 4):
            blk = blk + a[:, k:k + 1] * W[:, k].view(1, 64, 1)
        acc = acc + blk
    return acc + b.view(1, 64, 1)


@pytest.fixture(scope='module')
def stage():
    """One small 2-D case in fp32: P = 258 (scalar path, a tail quad of two pixels), the maps of the float64 forward rounded to fp32."""
    case = (2, 1, 12, 49, 2, 0.0)
    g, _ = K.geo(*case[:5])
    p = K.unpack(K.params(2), 2)
    x, dy = K.inputs(case)
    fwd = K.ref_forward(x, p, g)
    saved = {k: fwd[k].float() for k in ('z2', 'z3', 'z4')}
    for k in ('2', '3', '4'):
        saved['st' + k] = K.emu_stats(saved['z' + k])
    return case, g, p, x, dy, saved


def test_chain_and_blocked_order_within_the_limit_and_wrong_variants_not(stage):
    """The 1x1 forward: the chain is its own yardstick (1 / 3 of the limit), the kernel's blocked order is within the limit; one dropped term of
    64 and one dropped pixel of the tail quad are not."""
    case, g, p, x, dy, saved = stage
    ref = K.ref_1x1(saved['z2'], saved['st2'], p['W3'], p['b3'])
    a = K.act32(saved['z2'], saved['st2'])
    orc = K.err(K.chain_1x1(a, p['W3'], p['b3']), ref)
    assert K.within(orc, orc)
    assert K.within(K.err(blocked_1x1(a, p['W3'], p['b3']), ref), orc)
    assert not K.within(K.err(K.chain_1x1(a, p['W3'], p['b3'], drop=37), ref), orc)
    tail = blocked_1x1(a, p['W3'], p['b3'])
    assert g.P % 4 == 2
    tail[1, 5, g.P - 1] = 0.0            # one channel's last pixel of the last plane left unwritten
    assert not K.within(K.err(tail, ref), orc)
    # the chain in float64, on the float64 activations, is the reference
    a64 = torch.relu(K.n64(saved['z2'], saved['st2']))
    assert float((K.chain_1x1(a64, p['W3'], p['b3'], dtype=torch.float64) - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_z2_dx_and_weight_gradient_chains_sum_the_reference_terms(stage):
    """Every chain in float64 equals its reference (the same terms, another order); in fp32 it is within its own limit."""
    case, g, p, x, dy, saved = stage
    z2 = K.ref_z2(x, p, g)
    assert float((K.chain_z2(x, p, g, torch.float64) - z2).abs().max()) <= 1e-12 * float(z2.abs().max())
    assert K.within(K.err(K.chain_z2(x, p, g), z2), K.err(K.chain_z2(x, p, g), z2))
    small = (1, 1, 9, 8, 2, 0.0)
    gs, _ = K.geo(*small[:5])
    gz = torch.from_numpy(np.random.default_rng(1).standard_normal((1, 64, gs.P)).astype(np.float32))
    xs = K.inputs(small)[0]
    wc = p['W2'].double() @ p['W1'].double()
    dx = K.ref_dx(gz, p, gs)
    assert float((K.chain_dx(gz, wc, gs, torch.float64) - dx).abs().max()) <= 1e-12 * float(dx.abs().max())
    G, s, _ = K.ref_G(gz, xs, gs)
    got, = K.chain_outer([(K.rows_bp(gz), K.rows_bp(K.patches(xs, gs)))], torch.float64)
    assert float((got - G).abs().max()) <= 1e-12 * float(G.abs().max())
    dW1, db1, dW2, _ = K.ref_first(G, s, p)
    c1, cb, c2 = K.chain_first(G, s, p, torch.float64)
    for a, b in ((c1, dW1), (cb, db1), (c2, dW2)):
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    y = K.ref_y(saved['z4'], saved['st4'], p['W5'], p['b5'])
    assert K.within(K.err(K.chain_y(saved['z4'], saved['st4'], p['W5'], p['b5']), y), K.err(K.chain_y(saved['z4'], saved['st4'], p['W5'], p['b5']), y))


def test_row_kernel_emulations_within_their_limits_and_wrong_variants_not(stage):
    case, g, p, x, dy, saved = stage
    # statistics of rows with a mean 8e5 times the spread (4096 +- ten ulps, P = 300): the shifted sums hold the limit, unshifted fp64 sums do
    # not.  (At P <= 32 they would: squares of fp32 values and sums of 32 of them are exact in fp64.)
    gen = torch.Generator().manual_seed(9)
    z = 4096.0 + 2.0 ** -11 * torch.randint(-10, 11, (3, 64, 300), generator=gen).float()
    m, r, st64 = K.ref_stats(z)
    for shift, ok in ((True, True), (False, False)):
        st = K.emu_stats(z, shift)
        assert N.mean_share(st[..., 0].reshape(-1), st64)[0] <= 1.0
        worst = float(((st[..., 1].reshape(-1).double() / st64[2] - 1.0).abs() / K.rstd_limit(z, st64)).max())
        assert (worst <= 1.0) == ok, (shift, worst)
    # ... and at the stage's own maps
    m, r, st64 = K.ref_stats(saved['z3'])
    st = saved['st3']
    assert N.mean_share(st[..., 0].reshape(-1), st64)[0] <= 1.0
    assert float(((st[..., 1].reshape(-1).double() / st64[2] - 1.0).abs() / K.rstd_limit(saved['z3'], st64)).max()) <= 1.0
    # norm backward at the top layer; a variant whose second mean misses the row's last element fails
    ref, lim = K.ref_gz4(dy, p['W5'], saved['z4'], saved['st4'])
    gn = K.emu_top_gn(dy, p['W5'], saved['z4'], saved['st4'])
    got = K.emu_norm_bwd(gn, saved['z4'], saved['st4'])
    assert N.share((got.double() - ref).abs(), lim)[0] <= 1.0
    n = K.n32(saved['z4'], saved['st4']).double()
    m1 = gn.double().mean(-1, keepdim=True)
    m2 = (gn.double() * n)[..., :-1].sum(-1, keepdim=True) / g.P
    wrong = (saved['st4'][..., 1:2].double() * (gn.double() - m1 - n * m2)).float()
    assert N.share((wrong.double() - ref).abs(), lim)[0] > 1.0
    # the fp32 sums' limit: a serial fp32 chain over every pixel holds it, a sum that loses one workgroup's slab does not
    gz = got
    ref_s, abs_s = gz.double().sum((0, 2)), gz.double().abs().sum((0, 2))
    acc = torch.zeros(64)
    for row in K.rows_bp(gz):
        acc = acc + row
    assert bool(((acc.double() - ref_s).abs() <= K.fp32_sum_limit(ref_s, abs_s)).all())
    lost = gz[:, :, 64:].double().sum((0, 2))
    assert not bool(((lost - ref_s).abs() <= K.fp32_sum_limit(ref_s, abs_s)).all())


def test_emulated_backward_is_close_to_the_reference_backward(stage):
    """emu_backward (the yardstick of the end-to-end comparisons) computes the same quantities as ref_backward."""
    case, g, p, x, dy, saved = stage
    ref = K.ref_backward(x, dy, saved, p, g)
    emu = K.emu_backward(x, dy, saved, p, g, fed={'gz3': ref['gz3'].float(), 'gz2': ref['gz2'].float()})
    for k in ('gz4', 'gz3', 'gz2', 'dW4', 'dW3', 'G', 'dW1', 'dW2', 'dx'):
        e = K.err(emu[k], ref[k])
        assert e[0] < 1e-4, (k, e)
    assert K.err(emu['fed_dW3'], ref['dW3'])[0] < 1e-4 and K.err(emu['fed_G'], ref['G'])[0] < 1e-4


# ---- geometry, plan, saved layout against the library's host-side answers ---------------------------------------------------------------------
REFUSED = [(65536, 1, 8, 8, 2, 64), (9363, 7, 8, 8, 3, 64), (1, 2, 8, 8, 2, 64), (1, 1, 8, 8, 2, 32), (1, 1, 7, 7, 2, 64), (1, 1, 6, 9, 2, 64),
           (1, 6, 9, 9, 3, 64), (0, 1, 8, 8, 2, 64), (1, 1, 8, 8, 4, 64)]


def test_plan_saved_layout_and_refusals_equal_the_library():
    from neuroclear_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libnc_hip.so is not built')
    L = _lib.lib()
    shapes = [c[:5] for c in K.CASES] + [(108, 1, 108, 108, 2), (300, 1, 12, 49, 2), (1030, 1, 12, 49, 2), (65535, 1, 8, 7, 2), (9362, 7, 8, 8, 3)]
    for B, D, H, W, nd in shapes:
        g, code = K.geo(B, D, H, W, nd)
        assert code == K.NC_OK
        assert L.nc_kgan_ws_bytes(B, D, H, W, 64, nd) == K.plan(g).total * 4, (B, D, H, W, nd)
        assert L.nc_kgan_saved_floats(B, D, H, W, 64, nd) == K.saved_layout(g)['total']
        oD, oH, oW = (_lib.I * 1)(), (_lib.I * 1)(), (_lib.I * 1)()
        assert L.nc_kgan_out_shape(B, D, H, W, 64, nd, oD, oH, oW) == K.NC_OK
        assert (oD[0], oH[0], oW[0]) == (g.Do, g.Ho, g.Wo)
    for B, D, H, W, nd, ndf in REFUSED:
        g, code = K.geo(B, D, H, W, nd, ndf)
        assert g is None and code != K.NC_OK
        assert L.nc_kgan_out_shape(B, D, H, W, ndf, nd, None, None, None) == code, (B, D, H, W, nd, ndf)
        assert L.nc_kgan_ws_bytes(B, D, H, W, ndf, nd) == 0 and L.nc_kgan_saved_floats(B, D, H, W, ndf, nd) == 0
    assert L.nc_kgan_param_floats(64, 2) == K.param_floats(2) and L.nc_kgan_param_floats(64, 3) == K.param_floats(3)


def test_plan_of_the_named_shapes():
    """The figures the case list quotes, from the restated plan."""
    pl = K.plan(K.geo(2049, 1, 11, 19, 2)[0])
    assert (pl.cp, pl.units, pl.per, pl.p1, pl.units - (pl.p1 - 1) * pl.per) == (2, 4098, 5, 820, 3)
    pl = K.plan(K.geo(513, 1, 11, 19, 2)[0])
    assert (pl.units, pl.per, pl.p1, pl.p1 % 16) == (1026, 2, 513, 1)
    pl = K.plan(K.geo(33, 17, 17, 17, 3)[0])
    assert (pl.per, pl.p7, pl.units - (pl.p7 - 1) * pl.per) == (5, 139, 3)
    assert K.plan(K.geo(5, 20, 20, 20, 3)[0]).per == 2
    assert K.plan(K.geo(16, 1, 8, 7, 2)[0]).p1 == 16 and K.plan(K.geo(1, 1, 22, 22, 2)[0]).units == 4
    for o in K.plan(K.geo(2, 1, 7, 263, 2)[0])[5:]:
        assert o % 64 == 0 or o == K.plan(K.geo(2, 1, 7, 263, 2)[0]).total


def test_every_label_has_a_case():
    reached = {}
    for c in K.CASES:
        for label in K.branches(c):
            assert label in K.LABELS, label
            reached.setdefault(label, []).append(K.case_id(c))
    missing = [label for label in K.LABELS if label not in reached]
    assert not missing, missing
    assert len(set(K.case_id(c) for c in K.CASES)) == len(K.CASES)


def test_branches_of_the_cases_chosen_for_them():
    b = {K.case_id(c): K.branches(c) for c in K.CASES}
    assert {'rows/P2', '1x1/scalar', '1x1/ragged-quad', 'conv7/16-off', 'wgrad/cp1', 'grads/B1'} <= b['2d-1-8x7']
    assert {'rows/P>256', '1x1/scalar'} <= b['2d-1-12x49+100000']
    assert 'conv7/Ho1' in b['2d-2-7x9'] and 'conv7/Wo1' in b['2d-3-10x7'] and {'1x1/V', '1x1/quads-out'} <= b['2d-3-10x7']
    assert {'1x1/last-full', '1x1/one-tile', 'conv7/full', 'dx/H%16'} <= b['2d-1-22x22'] and 'wgrad/ragged-unit' not in b['2d-1-22x22']
    assert {'1x1/scalar', '1x1/tiles', 'dx/xtiles>1', 'dx/W%4'} <= b['2d-2-7x263']
    assert {'1x1/V', '1x1/tiles', '1x1/last-partial'} <= b['2d-1-19x26']
    assert {'rows/P>256', 'wgrad/ragged-unit'} <= b['2d-1-33x71']
    assert {'wgrad/per2-3', 'reduce/>16+tail'} <= b['2d-513-11x19'] and {'wgrad/per>=5', 'wgrad/short-last'} <= b['2d-2049-11x19']
    assert 'reduce/16' in b['2d-16-8x7']
    assert 'conv7/Do1' in b['3d-1-7x8x8'] and {'wgrad/tapblocks6', 'dx/depth-low', 'dx/depth-high'} <= b['3d-2-13x13x13']
    assert 'wgrad/per2-3' in b['3d-5-20x20x20'] and {'wgrad/per>=5', 'wgrad/short-last'} <= b['3d-33-17x17x17']
