"""The fused KernelGAN discriminator (csrc/kgan.hip: nc_kgan_fwd / nc_kgan_bwd) stage by stage against float64, through the C ABI directly.

Geometry, plan, references, yardsticks, limits and the cases -- the smallest shape per branch of every kernel, counted by
tests/test_kgan_reference.py -- are tests/kgan_reference.py's; Out, judge and the worst-use table are tests/test_gpu_conv_fp32.py's, imported.
Per case:
  * forward: y and `saved` are written into NaN-filled buffers with 64 guard floats behind each; the workspace is exactly nc_kgan_ws_bytes bytes of
    0xFF (NaN as fp32: nothing may be read before it is written) at the head of a larger 0xFF buffer whose tail stays unchanged.  z2, st2, z3,
    st3, z4, st4 and y are each held to the float64 reference of their stage fed with the device's own previous stage; every value is finite;
  * backward, the same guards: dx and the ten parameter gradients against the float64 backward from the device's `saved`; out of the workspace,
    through the restated offsets, gz2 (region A), gz3 (region B), the reduced slabs r3, r4, r7 and pw5, pb5; dW3, db3, G, s, dx, gz2 and
    k_kg_grads' dW1 / db1 / dW2 once more against references fed with the device's own gz3 / gz2 / G / s, so that a failure names one kernel.
    The ReLU masks of the references are the kernels' own (kgan_reference.n32): no element is left out of any comparison;
  * a second call gives the same bits; dparams = NULL gives the same dx, dx = NULL the same dparams; both NULL returns NC_OK and writes nothing;
  * the refusals come before anything is written.

Worst use of the limit per stage, 1.0 = at the limit, measured on an MI355X -- the table the module prints at its end (GEMM stages: max /
(3 max_chain + 2^-21), rms / (3 rms_chain + 2^-23); row kernels and sums: the largest and the rms share of their limit):
    k_kg_1x1<dgrad, V> + k_kg_norm_bwd: gz2 from gz3           0.351 0.265
    k_kg_1x1<dgrad, scalar> + k_kg_norm_bwd: gz2 from gz3      0.596 0.330
    k_kg_1x1<fwd, V>                                           0.321 0.245
    k_kg_1x1<fwd, scalar>                                      0.411 0.240
    k_kg_conv7                                                 0.435 0.320
    k_kg_dx: dx from gz2                                       0.219 0.258
    k_kg_final_fwd                                             0.338 0.295
    k_kg_grads dW5                                             0.262 0.080
    k_kg_grads db5                                             0.114 0.114
    k_kg_grads: dW1 from G                                     0.368 0.274
    k_kg_grads: dW2 from G, s                                  0.475 0.299
    k_kg_grads: db1 from s                                     0.263 0.291
    k_kg_norm_bwd pb5                                          0.492 0.342
    k_kg_norm_bwd pw5                                          0.494 0.111
    k_kg_stats mean                                            0.500 0.240
    k_kg_stats rstd                                            0.249 0.120
    k_kg_wgrad<1x1> + k_kg_reduce: dW3 from gz3                0.555 0.217
    k_kg_wgrad<1x1> + k_kg_reduce: db3 from gz3                0.383 0.130
    k_kg_wgrad<taps> + k_kg_reduce: G from gz2                 0.306 0.255
    k_kg_wgrad<taps> + k_kg_reduce: s from gz2                 0.404 0.147
    whole bwd: db1 = W2^T s                                    0.012 0.005
    whole bwd: dparams weights                                 0.555 0.551
    whole bwd: gz2 (region A)                                  0.476 0.330
    whole bwd: gz3 (region B)                                  0.386 0.330
    whole bwd: k_kg_dx                                         0.370 0.365
    whole bwd: k_kg_wgrad<1x1> + k_kg_reduce                   0.444 0.330
    whole bwd: k_kg_wgrad<taps> + k_kg_reduce                  0.365 0.331
    whole bwd: sums of gz (db4, db3, s)                        0.141 0.036
No stage uses more than 0.6 of its limit.  k_kg_dx (sums per channel, per depth tap, then over depth taps) and the weight gradients (split-P
partials) sit well under a single chain; the forward GEMMs and k_kg_grads' 64-term chains are the chain itself, a third of the limit.
Scratch mutants of kgan.hip (never committed), failing tests of this file's 36: the store bound of k_kg_1x1 one pixel short 23; `tok` forced true
in k_kg_wgrad<taps> 11; `pz >= g.Do` dropped in k_kg_dx 5 (every 3-D case); k_kg_reduce without its tail loop 16; `ds` over three of the four
lane groups 14; `sh = 0` in k_kg_stats 1 (the offset case).  `full = q0 + 3 < P` -> `q0 + 4 < P` in k_kg_1x1 fails none and cannot: with
16-byte accesses P % 4 == 0 and every quad is whole, and the scalar branch it sends the last quad to is right for any quad -- the same bits.
"""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kgan_reference as K  # noqa: E402
import norm_reference as N  # noqa: E402
import test_gpu_conv_fp32 as T  # noqa: E402  (Out, judge, WORST: shared, not forked)

DEV = T.DEV
WS_TAIL = 4096
MINE = set()
IDS = [K.case_id(c) for c in K.CASES]


@pytest.fixture(scope='module', autouse=True)
def _worst_table():
    yield
    print('\nworst use of the limit per stage (max, rms; 1.0 = at the limit)')
    for k in sorted(MINE):
        if k in T.WORST:
            print('  %-58s %.3f %.3f' % (k, T.WORST[k][0], T.WORST[k][1]))


def judge(kernel, what, got, orc):
    MINE.add(kernel)
    T.judge(kernel, what, got, orc)


def judge_share(kernel, what, err, lim):
    """A row kernel's or a sum's output against its absolute limit: the largest and the rms share of it."""
    s = N.share(err, lim)
    print('%-58s %-44s of the limit %.3f %.3f' % (kernel, what, s[0], s[1]))
    MINE.add(kernel)
    w = T.WORST.get(kernel, (0.0, 0.0))
    T.WORST[kernel] = (max(w[0], s[0]), max(w[1], s[1]))
    assert s[0] <= 1.0, (kernel, what, s)


def finite(t, what):
    assert bool(torch.isfinite(t).all()), '%s: not finite' % what


@functools.lru_cache(maxsize=None)
def gpu_params(nd):
    return K.params(nd).to(DEV)


def ws_buffer(nb):
    return torch.full((nb + WS_TAIL,), 0xFF, dtype=torch.uint8, device=DEV)


def ws_floats(big, nb):
    return big[:nb].view(torch.float32)


class Case:
    """The inputs of a case on the device.  x sits at the head of a zeroed buffer with a few input rows behind it."""

    def __init__(self, case):
        self.case, self.what = case, K.case_id(case)
        self.g, code = K.geo(*case[:5])
        assert code == K.NC_OK
        g = self.g
        x, dy = K.inputs(case)
        self.xbuf = torch.zeros(g.B * g.S + 4 * g.H * g.W + 64, device=DEV)
        self.x = self.xbuf[:g.B * g.S].view(g.B, g.D, g.H, g.W)
        self.x.copy_(x)
        self.dy = dy.to(DEV)
        self.prm = gpu_params(g.nd)
        self.p = K.unpack(self.prm, g.nd)
        self.dims = (g.B, g.D, g.H, g.W, K.C, g.nd)
        self.nb = int(T.L().nc_kgan_ws_bytes(g.B, g.D, g.H, g.W, K.C, g.nd))
        assert self.nb == K.plan(g).total * 4
        assert int(T.L().nc_kgan_saved_floats(g.B, g.D, g.H, g.W, K.C, g.nd)) == K.saved_layout(g)['total']

    def fwd(self, nb=None, null=()):
        g = self.g
        nb = self.nb if nb is None else nb
        y, saved, big = T.Out(g.B, g.P), T.Out(K.saved_layout(g)['total']), ws_buffer(self.nb)
        a = {'params': self.prm, 'x': self.x, 'y': y.t, 'saved': saved.t, 'ws': big}
        a.update({k: None for k in null})
        B, D, H, W, ndf, nd = self.dims
        code = T.L().nc_kgan_fwd(T.P(a['params']), T.P(a['x']), T.P(a['y']), T.P(a['saved']), B, D, H, W, ndf, nd, T.P(a['ws']), nb, T.stream())
        torch.cuda.synchronize()
        assert bool((big[self.nb:] == 0xFF).all()), 'a write behind the workspace'
        return code, y, saved, big

    def bwd(self, saved, nb=None, null=()):
        g = self.g
        nb = self.nb if nb is None else nb
        dx, dprm, big = T.Out(g.B, g.D, g.H, g.W), T.Out(K.param_floats(g.nd)), ws_buffer(self.nb)
        a = {'params': self.prm, 'x': self.x, 'saved': saved, 'dy': self.dy, 'dx': dx.t, 'dparams': dprm.t, 'ws': big}
        a.update({k: None for k in null})
        B, D, H, W, ndf, nd = self.dims
        code = T.L().nc_kgan_bwd(T.P(a['params']), T.P(a['x']), T.P(a['saved']), T.P(a['dy']), T.P(a['dx']), T.P(a['dparams']), B, D, H, W, ndf, nd,
                                 T.P(a['ws']), nb, T.stream())
        torch.cuda.synchronize()
        assert bool((big[self.nb:] == 0xFF).all()), 'a write behind the workspace'
        return code, dx, dprm, big

    def split(self, saved):
        """`saved` as the maps [B, 64, P] and the statistics [B, 64, 2]"""
        g, sl = self.g, K.saved_layout(self.g)
        m, s = g.B * K.C * g.P, 2 * g.B * K.C
        out = {k: saved[sl[k]:sl[k] + m].view(g.B, K.C, g.P) for k in ('z2', 'z3', 'z4')}
        out.update({k: saved[sl[k]:sl[k] + s].view(g.B, K.C, 2) for k in ('st2', 'st3', 'st4')})
        return out


@functools.lru_cache(maxsize=1)
def forward(case):
    """The case and its checked forward call (shared by the forward and the backward test of the case; one case is kept)."""
    c = Case(case)
    code, y, saved, big = c.fwd()
    T.ck(code, 'nc_kgan_fwd')
    y.check(c.what + ' y')
    saved.check(c.what + ' saved')
    finite(y.t, c.what + ' y')
    finite(saved.t, c.what + ' saved')
    return c, y, saved


def test_the_plan_and_the_refusals_are_the_restated_ones():
    """Host side only: nc_kgan_ws_bytes, nc_kgan_saved_floats and nc_kgan_out_shape against kgan_reference's geo(), plan() and saved_layout()."""
    L = T.L()
    for case in K.CASES:
        g, _ = K.geo(*case[:5])
        assert L.nc_kgan_ws_bytes(g.B, g.D, g.H, g.W, K.C, g.nd) == K.plan(g).total * 4
        assert L.nc_kgan_saved_floats(g.B, g.D, g.H, g.W, K.C, g.nd) == K.saved_layout(g)['total']
    for dims in ((65536, 1, 8, 8, 64, 2), (9363, 7, 8, 8, 64, 3), (1, 2, 8, 8, 64, 2), (1, 1, 8, 8, 32, 2), (1, 1, 7, 7, 64, 2), (1, 1, 8, 8, 64, 4)):
        B, D, H, W, ndf, nd = dims
        assert L.nc_kgan_out_shape(B, D, H, W, ndf, nd, None, None, None) == K.geo(B, D, H, W, nd, ndf)[1] != K.NC_OK
        assert L.nc_kgan_ws_bytes(B, D, H, W, ndf, nd) == 0 and L.nc_kgan_saved_floats(B, D, H, W, ndf, nd) == 0


@pytest.mark.parametrize('case', K.CASES, ids=IDS)
def test_forward_stage_by_stage(case):
    c, y, saved = forward(case)
    g, p, what = c.g, c.p, c.what
    s = c.split(saved.t)
    tag = 'V' if g.P % 4 == 0 else 'scalar'
    ref = K.ref_z2(c.x, p, g)
    judge('k_kg_conv7', what + ' z2', K.err(s['z2'], ref), K.err(K.chain_z2(c.x, p, g), ref))
    for k, nxt, W, b in (('2', 'z3', 'W3', 'b3'), ('3', 'z4', 'W4', 'b4'), ('4', 'y', 'W5', 'b5')):
        z, st = s['z' + k], s['st' + k]
        _, _, st64 = K.ref_stats(z)
        judge_share('k_kg_stats mean', what + ' st' + k, (st[..., 0].reshape(-1).double() - st64[0]).abs(), 2 * K.U * st64[0].abs() + 2.0 ** -40 * st64[3])
        judge_share('k_kg_stats rstd', what + ' st' + k, (st[..., 1].reshape(-1).double() / st64[2] - 1.0).abs(), K.rstd_limit(z, st64))
        if nxt == 'y':
            ref = K.ref_y(z, st, p[W], p[b])
            judge('k_kg_final_fwd', what + ' y', K.err(y.t, ref), K.err(K.chain_y(z, st, p[W], p[b]), ref))
        else:
            ref = K.ref_1x1(z, st, p[W], p[b])
            judge('k_kg_1x1<fwd, %s>' % tag, what + ' ' + nxt, K.err(s[nxt], ref), K.err(K.chain_1x1(K.act32(z, st), p[W], p[b]), ref))
    code, y2, saved2, _ = c.fwd()
    T.ck(code, 'nc_kgan_fwd')
    assert torch.equal(y2.t, y.t) and torch.equal(saved2.t, saved.t), '%s: a second call gives other bits' % what


def r7_G(r7, g):
    """[nblk][kWg] -> G [64, T], s [64] (k_kg_grads' own indexing)"""
    blocks = r7.view(g.nblk, K.WG)
    G = blocks[:, :K.C * K.C].view(g.nblk, K.C, K.C).permute(1, 0, 2).reshape(K.C, g.nblk * K.C)[:, :g.T]
    return G, blocks[0, K.C * K.C:]


@pytest.mark.parametrize('case', K.CASES, ids=IDS)
def test_backward_stage_by_stage(case):
    c, y, saved = forward(case)
    g, p, what = c.g, c.p, c.what
    s = c.split(saved.t)
    pl = K.plan(g)
    tag = 'V' if g.P % 4 == 0 else 'scalar'
    code, dx, dprm, big = c.bwd(saved.t)
    T.ck(code, 'nc_kgan_bwd')
    dx.check(what + ' dx')
    dprm.check(what + ' dparams')
    finite(dx.t, what + ' dx')
    finite(dprm.t, what + ' dparams')
    ws = ws_floats(big, c.nb)
    m = g.B * K.C * g.P
    gz2, gz3 = ws[pl.o_a:pl.o_a + m].view(g.B, K.C, g.P), ws[pl.o_b:pl.o_b + m].view(g.B, K.C, g.P)
    r3, r4, r7 = ws[pl.o_r3:pl.o_r3 + K.WG], ws[pl.o_r4:pl.o_r4 + K.WG], ws[pl.o_r7:pl.o_r7 + g.nblk * K.WG]
    pw5, pb5 = ws[pl.o_pw5:pl.o_pw5 + g.B * K.C].view(g.B, K.C), ws[pl.o_pb5:pl.o_pb5 + g.B]
    for t, name in ((gz2, 'gz2'), (gz3, 'gz3'), (r3, 'r3'), (r4, 'r4'), (r7, 'r7'), (pw5, 'pw5'), (pb5, 'pb5')):
        finite(t, what + ' ' + name)
    G, sv = r7_G(r7, g)
    # the columns of the last tap block beyond T (what k_kg_wgrad's `tok` guards) are sums of zeros, and every block carries the same s
    assert bool((r7.view(g.nblk, K.WG)[-1, :K.C * K.C].view(K.C, K.C)[:, g.T - 64 * (g.nblk - 1):] == 0).all()), what + ': taps beyond T'
    assert bool((r7.view(g.nblk, K.WG)[:, K.C * K.C:] == sv).all()), what + ': s differs between tap blocks'
    grads = dict(zip(K.GRAD_NAMES, K.split_grads(dprm.t, g.nd)))

    ref = K.ref_backward(c.x, c.dy, s, p, g)
    emu = K.emu_backward(c.x, c.dy, s, p, g, fed={'gz3': gz3, 'gz2': gz2})

    # ---- against the whole float64 backward from `saved`; the yardstick is the same stages composed in fp32
    def whole(kernel, name, got, key=None, st=None):
        key = key or name
        sc = 1.0 if st is None else K.row_scale(st)
        r = ref[key] / sc
        judge(kernel, '%s %s' % (what, name), K.err(got.double().reshape(r.shape) / sc, r), K.err(emu[key].double() / sc, r))
    for name, got, st in (('gz3', gz3, s['st3']), ('gz2', gz2, s['st2'])):
        r = K.per_row(ref[name], st)
        judge('whole bwd: %s (region %s)' % (name, 'B' if name == 'gz3' else 'A'), '%s %s' % (what, name), K.err(K.per_row(got, st), r),
              K.err(K.per_row(emu[name], st), r))
    whole('whole bwd: k_kg_wgrad<1x1> + k_kg_reduce', 'r4 dW4', r4[:K.C * K.C], 'dW4', s['st4'])
    whole('whole bwd: k_kg_wgrad<1x1> + k_kg_reduce', 'r3 dW3', r3[:K.C * K.C], 'dW3', s['st3'])
    whole('whole bwd: k_kg_wgrad<taps> + k_kg_reduce', 'r7 G', G, 'G', s['st2'])
    whole('whole bwd: k_kg_dx', 'dx', dx.t)
    whole('whole bwd: dparams weights', 'dW1', grads['dW1'])
    for name, st in (('dW2', 'st2'), ('dW3', 'st3'), ('dW4', 'st4')):
        whole('whole bwd: dparams weights', name, grads[name], st=s[st])
    (rw, lw), (rb, lb), (rW5, lW5), (rb5, lb5) = ref['pw5'], ref['pb5'], ref['dW5'], ref['db5']
    judge_share('k_kg_norm_bwd pw5', what, (pw5.double() - rw).abs(), lw)
    judge_share('k_kg_norm_bwd pb5', what, (pb5.double() - rb).abs(), lb)
    judge_share('k_kg_grads dW5', what, (grads['dW5'].double() - rW5).abs(), lW5)
    judge_share('k_kg_grads db5', what, (grads['db5'].double() - rb5).abs(), lb5)
    # the analytically zero bias gradients: the fp32 sums' limit on sum|gz|, and k_kg_norm_bwd's own limit on every term
    lims = {k: K.fp32_sum_limit(ref[r], ref[a]) + ref[lim].sum((0, 2)) for k, r, a, lim in (('db4', 'db4', 'abs4', 'lim4'), ('db3', 'db3', 'abs3', 'lim3'),
                                                                                           ('s', 's', 'abs2', 'lim2'))}
    for name, got in (('db4', r4[K.C * K.C:]), ('db3', r3[K.C * K.C:]), ('s', sv)):
        judge_share('whole bwd: sums of gz (db4, db3, s)', '%s %s' % (what, name), (got.double() - ref['s' if name == 's' else name]).abs(), lims[name])
    judge_share('whole bwd: db1 = W2^T s', what, (grads['db1'].double() - ref['db1']).abs(), K.db1_limit(lims['s'], ref['s'], p))
    # what k_kg_grads only copies
    assert torch.equal(grads['db2'], sv) and torch.equal(grads['dW3'].reshape(-1), r3[:K.C * K.C]) and torch.equal(grads['db3'], r3[K.C * K.C:])
    assert torch.equal(grads['dW4'].reshape(-1), r4[:K.C * K.C]) and torch.equal(grads['db4'], r4[K.C * K.C:])

    # ---- one kernel at a time: references fed with the device's own gz3 / gz2 / G / s
    r = K.ref_norm_bwd(K.ref_dgrad(gz3, p['W3'], s['z2'], s['st2']), s['z2'], s['st2'], False)[0]
    o = K.emu_norm_bwd(K.chain_dgrad(gz3, p['W3'], s['z2'], s['st2']), s['z2'], s['st2'])
    r = K.per_row(r, s['st2'])
    judge('k_kg_1x1<dgrad, %s> + k_kg_norm_bwd: gz2 from gz3' % tag, what, K.err(K.per_row(gz2, s['st2']), r), K.err(K.per_row(o, s['st2']), r))
    rW, rb, ab = K.ref_wgrad(gz3, s['z2'], s['st2'])
    judge('k_kg_wgrad<1x1> + k_kg_reduce: dW3 from gz3', what, K.err(r3[:K.C * K.C], rW), K.err(emu['fed_dW3'], rW))
    judge_share('k_kg_wgrad<1x1> + k_kg_reduce: db3 from gz3', what, (r3[K.C * K.C:].double() - rb).abs(), K.fp32_sum_limit(rb, ab))
    rG, rs, ab = K.ref_G(gz2, c.x, g)
    judge('k_kg_wgrad<taps> + k_kg_reduce: G from gz2', what, K.err(G, rG), K.err(emu['fed_G'], rG))
    judge_share('k_kg_wgrad<taps> + k_kg_reduce: s from gz2', what, (sv.double() - rs).abs(), K.fp32_sum_limit(rs, ab))
    rdx = K.ref_dx(gz2, p, g)
    judge('k_kg_dx: dx from gz2', what, K.err(dx.t, rdx), K.err(emu['fed_dx'], rdx))
    r1, rb1, r2, _ = K.ref_first(G, sv, p)
    c1, cb1, c2 = K.chain_first(G.contiguous(), sv, p)
    judge('k_kg_grads: dW1 from G', what, K.err(grads['dW1'], r1), K.err(c1, r1))
    judge('k_kg_grads: dW2 from G, s', what, K.err(grads['dW2'], r2), K.err(c2, r2))
    judge('k_kg_grads: db1 from s', what, K.err(grads['db1'], rb1), K.err(cb1, rb1))

    # ---- bits
    code, dx2, dprm2, _ = c.bwd(saved.t)
    T.ck(code, 'nc_kgan_bwd')
    assert torch.equal(dx2.t, dx.t) and torch.equal(dprm2.t, dprm.t), '%s: a second call gives other bits' % what
    code, dx3, dprm3, _ = c.bwd(saved.t, null=('dparams',))
    T.ck(code, 'nc_kgan_bwd, dparams = NULL')
    assert torch.equal(dx3.t, dx.t) and dprm3.untouched(), '%s: dparams = NULL' % what
    code, dx4, dprm4, _ = c.bwd(saved.t, null=('dx',))
    T.ck(code, 'nc_kgan_bwd, dx = NULL')
    assert torch.equal(dprm4.t, dprm.t) and dx4.untouched(), '%s: dx = NULL' % what
    code, dx5, dprm5, big5 = c.bwd(saved.t, null=('dx', 'dparams'))
    assert code == K.NC_OK and dx5.untouched() and dprm5.untouched() and bool((big5 == 0xFF).all()), '%s: dx = dparams = NULL' % what


def test_refusals_come_before_anything_is_written():
    c, y, saved = forward(K.CASES[0])
    L = T.L()

    def fwd_refused(want, **kw):
        code, y2, saved2, big = c.fwd(**kw)
        assert code == want, (kw, code, L.nc_last_error())
        assert y2.untouched() and saved2.untouched() and bool((big == 0xFF).all()), kw

    def bwd_refused(want, **kw):
        code, dx, dprm, big = c.bwd(saved.t, **kw)
        assert code == want, (kw, code, L.nc_last_error())
        assert dx.untouched() and dprm.untouched() and bool((big == 0xFF).all()), kw
    fwd_refused(K.NC_ERR_WS, nb=c.nb - 1)
    bwd_refused(K.NC_ERR_WS, nb=c.nb - 1)
    fwd_refused(K.NC_ERR_WS, null=('ws',))
    bwd_refused(K.NC_ERR_WS, null=('ws',))
    for k in ('params', 'x', 'y', 'saved'):
        fwd_refused(K.NC_ERR_ARG, null=(k,))
    for k in ('params', 'x', 'saved', 'dy'):
        bwd_refused(K.NC_ERR_ARG, null=(k,))
    # the launch geometry and the shapes the fused path does not cover: B = 65536; 3-D with B D > 65535; nd = 2 with D != 1; ndf = 32
    for dims in ((65536, 1, 8, 7, 64, 2), (9363, 7, 8, 8, 64, 3), (1, 2, 8, 7, 64, 2), (1, 1, 8, 7, 32, 2)):
        save = c.dims
        c.dims = dims
        try:
            fwd_refused(K.NC_ERR_SHAPE)
            bwd_refused(K.NC_ERR_SHAPE)
        finally:
            c.dims = save
