"""The 16-bit END-TO-END ("C8") operators between the 16-bit convolutions, op level, through the C ABI: every kernel and dispatch branch of
csrc/c8_ops.hip and csrc/convt_h.hip and the fused fp32 -> fp32 + C8 norm passes of csrc/norm_act.hip, each against a float64 restatement on the
exact 16-bit operand values.  References, the criterion (16-bit outputs: within half an ulp of the float64 value plus the rigorous fp32 bound e;
fp32 outputs: the factor-3 rule of tests/convt_reference.py against torch's fp32 operator on the CPU), the cases and the refusal table:
tests/c8_reference.py, held to torch's float64 operators by tests/test_c8_reference.py.

Per case: outputs pre-filled with 0xFF bytes (NaN in every type) with 256 guard bytes in front and behind; the channels outside (c0, C) of a wide
buffer keep their fill (and the inputs' channels outside the range hold NaN: a kernel that reads them shows it); a workspace of exactly
*_ws_bytes between guards; NC_ERR_WS for one byte less with nothing written; a second call identical by bits; every refusal of the table with
outputs and workspace untouched.

MEASURED on an MI355X (the table the module prints at its end): per operator and type the largest `excess` (share of e used beyond half an ulp;
16-bit outputs) and the largest use of the factor-3 limit (max, rms; fp32 outputs).
    operator                   type  largest excess | use of the factor-3 limit (max, rms)
      stats mean                 fp32         | 0.080 0.159          stats rstd                 fp32         | 0.525 0.750  (the 'clamp' case)
      stats mean ('offset')      fp32         | 0.065 0.135          stats rstd ('offset')      fp32         | 0.054 0.105
      normalise + act            bf16   0.013 |                      normalise + act            fp16   0.118 |
      norm backward dx           bf16   0.078 |                      pool backward + skip       bf16   0.000 |
      fused forward twin         fp32         | 0.264 0.162          fused backward twin        fp32         | 0.275 0.178
      dot64                      fp32         | 0.702 0.545          dot64, share of e          bf16 / fp16  0.029 / 0.032
      outer64 dx                 bf16   0.833 |                      outer64 dw / db            fp32         | 0.138 0.177 / 0.227 0.821
      convT forward              bf16   0.015 |                      convT forward              fp16   0.018 |
      convT dgrad<1> / dgrad<4>  bf16   0.000 |                      convT wgrad_h / wgrad_h2   fp32         | 0.201 0.149 / 0.251 0.224
      convT dbias                fp32         | 0.100 0.086
    dbias of the norm backward: at most 1.3e-3 of n u sum|dx| and 0.014 of the chain limit.
One excess is above 0.5: outer64 dx (0.833).  Its e is the bound of a SINGLE fp32 rounding, u |w g|, which is attained: over 64 x 4097 x 2 products
the largest share approaches 1, as it does for torch's own fp32 product (tests/test_c8_reference.py).  Every other operator leaves e nearly unused:
the results are the correctly rounded float64 values almost everywhere.

What this file found.  (1) k_pool_c8 returned +0.0 for a window of eight -inf (the 'planted' case; now -inf).  (2) The launchers of c8_ops.hip
did not refuse N C / 8 > 65535 before their first launch (the refusal rows; now NC_ERR_SHAPE on the host).  (3) k_stats_c8 summed x and x^2
unshifted in fp32 chains: at the 'offset' case (fp16, mean 100, deviation 1) rstd was 7.0e-4 off, 997 x the max limit and 2944 x the rms limit of
the factor-3 rule and more than half an fp16 ulp of every normalised value; it now sums x - pivot (the instance's first voxel).
"""
import ctypes
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c8_reference as R  # noqa: E402

DEV = 'cuda'
FILL, GUARD = 0xFF, 256
WORST = {}


def L():
    from neuroclear_amd._lib import lib
    return lib()


def stream():
    from neuroclear_amd import ops
    return ops._stream()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def err_text():
    return L().nc_last_error().decode()


class Buf:
    """nbytes of 0xFF between two guards of 0xFF"""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.t = torch.full((GUARD + self.n + GUARD,), FILL, dtype=torch.uint8, device=DEV)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + GUARD)

    def body(self):
        return self.t[GUARD:GUARD + self.n]

    def view(self, dtype, *shape):
        return self.body().view(dtype).reshape(shape)

    def guards_ok(self):
        return bool((self.t[:GUARD] == FILL).all()) and bool((self.t[GUARD + self.n:] == FILL).all())

    def untouched(self):
        return bool((self.t == FILL).all())


def ptr_of(b):
    return b.ptr if b is not None else ctypes.c_void_p(0)


def exercise(call, sizes, need):
    """call(outs: {name: Buf or None}, ws pointer, ws bytes) -> code.  (1) NaN-filled outputs between guards and a workspace of exactly `need`
    bytes between guards; (2) the same call again: the same bits; (3) one byte less: NC_ERR_WS, nothing written.  Returns the outputs of (1)."""
    def fresh():
        return {k: (Buf(v) if v is not None else None) for k, v in sizes.items()}

    def run(nbytes):
        outs, ws = fresh(), (Buf(need) if need else None)
        rc = call(outs, ptr_of(ws), nbytes)
        torch.cuda.synchronize()
        return rc, outs, ws

    rc, a, wa = run(need)
    assert rc == R.NC_OK, (rc, err_text())
    assert all(b.guards_ok() for b in a.values() if b is not None), 'an output guard was written'
    assert wa is None or wa.guards_ok(), 'the workspace tail was written'
    rc, b, _ = run(need)
    assert rc == R.NC_OK
    for k in a:
        assert a[k] is None or torch.equal(a[k].t, b[k].t), 'second call differs: %s' % k
    if need:
        rc, c, wc = run(need - 1)
        assert rc == R.NC_ERR_WS, rc
        assert all(v.untouched() for v in c.values() if v is not None) and wc.untouched()
    return a


def note(op, dt, excess=None, ratio=None):
    k = '%-26s %s' % (op, R.dt_name(dt) if dt else 'fp32')
    w = WORST.setdefault(k, [0.0, 0.0, 0.0])
    if excess is not None:
        w[0] = max(w[0], excess)
    if ratio is not None:
        w[1], w[2] = max(w[1], ratio[0]), max(w[2], ratio[1])


@pytest.fixture(scope='module', autouse=True)
def _worst_table():
    yield
    print('\noperator                   type  largest excess | use of the factor-3 limit (max, rms)')
    for k in sorted(WORST):
        print('  %s   %.3f | %.3f %.3f' % (k, *WORST[k]))
    # nothing of this module stays on the device for the modules after it
    _pool.clear()
    for f in (R.norm_inputs, R.fused_inputs, R.convt_inputs):
        f.cache_clear()
    torch.cuda.empty_cache()


def judge16(op, what, dt, got, ref, e):
    ok, ex = R.within_half_ulp(got, ref, e, dt)
    print('%-26s %-40s %s excess %.3f' % (op, what, R.dt_name(dt), ex))
    note(op, dt, excess=ex)
    assert ok, (op, what, ex)


def judge32(op, what, got, ref, oracle):
    g, o = R.CR.err(got, ref), R.CR.err(oracle.to(ref.device), ref)
    r = R.CR.ratios(g, o)
    print('%-26s %-40s product max %.2e rms %.2e | oracle max %.2e rms %.2e | of the limit %.3f %.3f' % (op, what, g[0], g[1], o[0], o[1], r[0], r[1]))
    if math.isfinite(r[0]) and math.isfinite(r[1]):
        note(op, None, ratio=r)
    assert R.CR.within(g, o), (op, what, g, o)


def nan_buffer(N, ctot, S, dt):
    return torch.full((N, ctot // 8, S, 8), float('nan'), dtype=R.tdt(dt), device=DEV)


def outside_keeps_fill(buf, N, ctot, S, c0, C):
    v = buf.view(torch.int16, N, ctot // 8, S, 8)
    return bool((v[:, :c0 // 8] == -1).all()) and bool((v[:, (c0 + C) // 8:] == -1).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# InstanceNorm on C8 tensors
# ---------------------------------------------------------------------------------------------------------------------------------------------
NORM_DT = [(c, dt) for c in R.NORM_CASES for dt in c[7]]
NORM_IDS = ['%s-%s' % (c[0], R.dt_name(dt)) for c, dt in NORM_DT]


@pytest.mark.parametrize('case,dt', NORM_DT, ids=NORM_IDS)
def test_statistics(case, dt):
    """nc_c8_instnorm_stats: fp32 per-thread partials of x - pivot, fp64 reduction, var = q / S - m^2.  The 'offset' case (fp16, mean 100,
    deviation 1) is held to the same rule as every other: unshifted chains of squares of ~1e4 lost what the variance of 1 is made of."""
    name, N, C, S, _, _, _, _, kind = case
    x, _ = R.norm_inputs(N, C, S, kind, dt, DEV)
    xh = R.pack(x)
    need = L().nc_c8_instnorm_ws_bytes(N, C, S)
    assert need > 0

    def call(o, ws, nb):
        return L().nc_c8_instnorm_stats(P(xh), N, C, S, R.EPS, o['mean'].ptr, o['rstd'].ptr, dt, ws, nb, stream())
    o = exercise(call, dict(mean=N * C * 4, rstd=N * C * 4), need)
    m64, _, r64 = R.ref_stats(x)
    om, orr = R.oracle_stats(x)
    judge32('stats mean' + (' (offset)' if kind else ''), name, o['mean'].view(torch.float32, N, C), m64, om)
    judge32('stats rstd' + (' (offset)' if kind else ''), name, o['rstd'].view(torch.float32, N, C), r64, orr)


@pytest.mark.parametrize('case,dt', NORM_DT, ids=NORM_IDS)
def test_normalise_and_activation(case, dt):
    name, N, C, S, ctot, c0, slope, _, kind = case
    x, _ = R.norm_inputs(N, C, S, kind, dt, DEV)
    xh = R.pack(x)
    mean, rstd = R.stats32(x)

    def call(o, ws, nb):
        return L().nc_c8_instnorm_act_fwd(P(xh), P(mean), P(rstd), slope, o['y'].ptr, ctot, c0, N, C, S, dt, stream())
    o = exercise(call, dict(y=N * ctot * S * 2), 0)['y']
    assert outside_keeps_fill(o, N, ctot, S, c0, C)
    got = R.unpack(R.view(o.view(R.tdt(dt), N, ctot // 8, S, 8), c0, C), x.shape)
    ref, e = R.ref_norm_act(x, mean, rstd, slope)
    judge16('normalise + act', name, dt, got, ref, e)
    assert torch.equal(got, R.emu_norm_act(x, mean, rstd, slope).to(R.tdt(dt)))   # the fp32 expression rounded once, bit for bit


@pytest.mark.parametrize('case,dt', NORM_DT, ids=NORM_IDS)
def test_norm_backward(case, dt):
    """nc_c8_instnorm_act_bwd with the gradient in a channel range of a wider buffer; dbias: see c8_reference.py, DBIAS."""
    name, N, C, S, ctot, c0, slope, _, kind = case
    x, g = R.norm_inputs(N, C, S, kind, dt, DEV)
    xh = R.pack(x)
    gb = nan_buffer(N, ctot, S, R.BF)
    R.pack_into(gb, g, c0)
    mean, rstd = R.stats32(x)
    need = L().nc_c8_instnorm_ws_bytes(N, C, S)

    def call(o, ws, nb):
        return L().nc_c8_instnorm_act_bwd(P(gb), ctot, c0, P(xh), P(mean), P(rstd), slope, o['dx'].ptr, ptr_of(o['db']), N, C, S, dt, ws, nb, stream())
    o = exercise(call, dict(dx=N * C * S * 2, db=C * 4), need)
    ref, e = R.ref_norm_bwd(g, x, mean, rstd, slope)
    judge16('norm backward dx', name, R.BF, R.unpack(o['dx'].view(torch.bfloat16, N, C // 8, S, 8), x.shape), ref, e)
    db = o['db'].view(torch.float32, C).double()
    assert bool(torch.isfinite(db).all())
    lim, chain = R.dbias_limit(ref), R.dbias_chain_limit(ref, e)
    use = float(((db - ref.sum((0, 2))).abs() / chain.clamp_min(1e-300)).max()) if S > 1 else 0.0
    print('%-26s %-40s |dbias| / (n u sum|dx|) %.2e, |dbias - sum dx| / chain limit %.3f' % ('norm backward dbias', name, float((db.abs() / lim.clamp_min(1e-300)).max()), use))
    assert bool((db.abs() <= lim).all()) and bool(((db - ref.sum((0, 2))).abs() <= chain).all())
    if S <= 1 << 20:   # dbias = NULL: the same dx
        o2 = exercise(call, dict(dx=N * C * S * 2, db=None), need)
        assert torch.equal(o2['dx'].t, o['dx'].t)


@pytest.mark.parametrize('dt', R.DTS, ids=R.dt_name)
@pytest.mark.parametrize('case', R.FROM_C8_CASES, ids=[R.case_id(c) for c in R.FROM_C8_CASES])
def test_from_c8(case, dt):
    N, C, S, ctot, c0 = case
    x = torch.randn(N, C, S, generator=torch.Generator().manual_seed(S)).to(R.tdt(dt)).to(DEV)
    xb = R.pack_into(nan_buffer(N, ctot, S, dt), x, c0)

    def call(o, ws, nb):
        return L().nc_from_c8(P(xb), ctot, c0, o['y'].ptr, N, C, S, dt, stream())
    o = exercise(call, dict(y=N * C * S * 4), 0)['y']
    assert torch.equal(o.view(torch.float32, N, C, S), x.float())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the fused fp32 -> fp32 + C8 passes of the layer-by-layer 16-bit path
# ---------------------------------------------------------------------------------------------------------------------------------------------
FUSED = [(c, dt, s) for c in R.FUSED_CASES for dt in R.DTS for s in ((0.0, 0.2) if c[0] == 'S300' else (0.2,))]
FUSED_IDS = ['%s-%s-%g' % (c[0], R.dt_name(dt), s) for c, dt, s in FUSED]


@pytest.mark.parametrize('case,dt,slope', FUSED, ids=FUSED_IDS)
def test_fused_forward(case, dt, slope):
    """nc_instnorm_act_fwd_c8: the fp32 twin is nc_instnorm_act_fwd bit for bit, the C8 copy its round-to-nearest-even bit for bit, with and
    without the twin."""
    name, N, C, S = case
    x, _ = R.fused_inputs(N, C, S, DEV)
    mean, rstd = R.stats32(x)
    y0 = torch.full_like(x, float('nan'))
    assert L().nc_instnorm_act_fwd(P(x), P(mean), P(rstd), slope, P(y0), N * C, S, stream()) == 0, err_text()

    def call(o, ws, nb):
        return L().nc_instnorm_act_fwd_c8(P(x), P(mean), P(rstd), slope, ptr_of(o['y']), o['yh'].ptr, N, C, S, dt, stream())
    o = exercise(call, dict(y=N * C * S * 4, yh=N * C * S * 2), 0)
    y = o['y'].view(torch.float32, N, C, S)
    assert torch.equal(y, y0)
    assert torch.equal(o['yh'].view(R.tdt(dt), N, C // 8, S, 8), R.pack(y.to(R.tdt(dt))))
    o2 = exercise(call, dict(y=None, yh=N * C * S * 2), 0)
    assert torch.equal(o2['yh'].t, o['yh'].t)
    ref, _ = R.ref_norm_act(x, mean, rstd, slope)
    judge32('fused forward twin', name, y, ref, R.emu_norm_act(x.cpu(), mean.cpu(), rstd.cpu(), slope))


@pytest.mark.parametrize('case,dt,slope', FUSED, ids=FUSED_IDS)
def test_fused_backward(case, dt, slope):
    """nc_instnorm_act_bwd_c8: dx and dbias are nc_instnorm_act_bwd_dbias bit for bit, the C8 copy the round-to-nearest-even of dx bit for bit,
    with and without dbias."""
    name, N, C, S = case
    x, dy = R.fused_inputs(N, C, S, DEV)
    mean, rstd = R.stats32(x)
    need = L().nc_instnorm_bwd_dbias_ws_bytes(N * C, S)
    dx0, db0, ws0 = torch.full_like(x, float('nan')), torch.full((C,), float('nan'), device=DEV), Buf(need)
    assert L().nc_instnorm_act_bwd_dbias(P(dy), P(x), P(mean), P(rstd), slope, P(dx0), P(db0), N, C, S, ws0.ptr, need, stream()) == 0, err_text()

    def call(o, ws, nb):
        return L().nc_instnorm_act_bwd_c8(P(dy), P(x), P(mean), P(rstd), slope, o['dx'].ptr, o['dxh'].ptr, ptr_of(o['db']), N, C, S, dt, ws, nb, stream())
    o = exercise(call, dict(dx=N * C * S * 4, dxh=N * C * S * 2, db=C * 4), need)
    dx = o['dx'].view(torch.float32, N, C, S)
    assert torch.equal(o['dxh'].view(R.tdt(dt), N, C // 8, S, 8), R.pack(dx.to(R.tdt(dt))))
    o2 = exercise(call, dict(dx=N * C * S * 4, dxh=N * C * S * 2, db=None), need)
    assert torch.equal(o2['dx'].t, o['dx'].t) and torch.equal(o2['dxh'].t, o['dxh'].t)
    ref, _ = R.ref_norm_bwd(dy, x, mean, rstd, slope)
    judge32('fused backward twin', name, dx, ref, R.emu_norm_bwd(dy.cpu(), x.cpu(), mean.cpu(), rstd.cpu(), slope))
    db = o['db'].view(torch.float32, C)
    assert bool((db.double().abs() <= R.dbias_limit(ref)).all())
    same_dx, same_db = torch.equal(dx, dx0), torch.equal(db, db0)
    print('%-26s %-40s dx identical to nc_instnorm_act_bwd_dbias: %s, dbias: %s (max |diff| %.2e / %.2e)'
          % ('fused backward twin', name, same_dx, same_db, float((dx - dx0).abs().max()), float((db - db0).abs().max())))
    assert same_dx and same_db


# ---------------------------------------------------------------------------------------------------------------------------------------------
# MaxPool3d(2)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', R.DTS, ids=R.dt_name)
@pytest.mark.parametrize('case', R.POOL_CASES, ids=[c[0] for c in R.POOL_CASES])
def test_pool_forward_and_backward_add(case, dt):
    """Forward: the bits of the first maximum (a NaN wins; eight -inf give -inf; of +0.0 / -0.0 the first).  Backward: skip + the gradient at the
    first maximum / the last NaN, rounded once."""
    name, N, C, dims, ctot, c0, kind = case
    D, H, W = dims
    S, So = D * H * W, D * H * W // 8
    x, dp, skip = (t.to(DEV) for t in R.pool_inputs(N, C, dims, kind, dt))
    xb = R.pack_into(nan_buffer(N, ctot, S, dt), x, c0)

    def call(o, ws, nb):
        return L().nc_c8_maxpool2_fwd(P(xb), ctot, c0, o['y'].ptr, N, C, D, H, W, dt, stream())
    o = exercise(call, dict(y=N * C * So * 2), 0)['y']
    y, arg = R.ref_pool(x)
    assert torch.equal(o.view(torch.int16, N, C // 8, So, 8), R.pack(y).view(torch.int16))
    sc0 = ctot - C - c0
    sb = R.pack_into(nan_buffer(N, ctot, S, R.BF), skip, sc0)
    dph = R.pack(dp)

    def call(o, ws, nb):
        return L().nc_c8_maxpool2_bwd_add(P(dph), P(xb), ctot, c0, P(sb), ctot, sc0, o['dx'].ptr, N, C, D, H, W, dt, stream())
    o = exercise(call, dict(dx=N * C * S * 2), 0)['dx']
    ref, e = R.ref_pool_bwd_add(dp, arg, skip)
    judge16('pool backward + skip', name, R.BF, R.unpack(o.view(torch.bfloat16, N, C // 8, S, 8), x.shape), ref, e)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the 64 -> 1 head
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', R.DTS, ids=R.dt_name)
@pytest.mark.parametrize('case', R.HEAD_CASES, ids=[R.case_id(c) for c in R.HEAD_CASES])
def test_head_dot(case, dt):
    N, S, _ = case
    x, w, b, _ = (t.to(DEV) for t in R.head_inputs(N, S, dt))
    xh = R.pack(x)
    for bias in (b, None):
        def call(o, ws, nb):
            return L().nc_c8_dot64_debug(P(xh), P(w), P(bias), o['out'].ptr, N, S, dt, stream())
        got = exercise(call, dict(out=N * S * 4), 0)['out'].view(torch.float32, N, S)
        ref, e = R.ref_dot64(x, w, bias)
        ok, ex = R.bound_excess(got, ref, e)
        note('dot64 (share of e)', dt, excess=ex)
        assert ok, ex
        judge32('dot64', 'S = %d bias %d' % (S, bias is not None), got, ref, R.oracle_dot64(x, w, bias))


@pytest.mark.parametrize('dt', R.DTS, ids=R.dt_name)
@pytest.mark.parametrize('case', R.HEAD_CASES, ids=[R.case_id(c) for c in R.HEAD_CASES])
def test_head_outer(case, dt):
    N, S, _ = case
    x, w, _, g = (t.to(DEV) for t in R.head_inputs(N, S, dt))
    xh = R.pack(x)
    need = L().nc_c8_outer64_ws_bytes_debug(N, S)
    assert need > 0

    def call(o, ws, nb):
        return L().nc_c8_outer64_debug(P(g), P(xh), P(w), ptr_of(o['dx']), o['dw'].ptr, ptr_of(o['db']), N, S, dt, ws, nb, stream())
    full = dict(dx=N * 64 * S * 2, dw=64 * 4, db=4)
    o = exercise(call, full, need)
    dx, e, dw, db = R.ref_outer64(g, x, w)
    judge16('outer64 dx', 'S = %d' % S, R.BF, R.unpack(o['dx'].view(torch.bfloat16, N, 8, S, 8), x.shape), dx, e)
    odw, odb = R.oracle_outer64(g, x)
    judge32('outer64 dw', 'S = %d' % S, o['dw'].view(torch.float32, 64), dw, odw)
    judge32('outer64 db', 'S = %d' % S, o['db'].view(torch.float32, 1), db, odb)
    for drop in (('dx',), ('db',), ('dx', 'db')):
        o2 = exercise(call, {k: (None if k in drop else v) for k, v in full.items()}, need)
        for k in full:
            assert o2[k] is None or torch.equal(o2[k].t, o[k].t), (drop, k)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# ConvTranspose3d(2, 2)
# ---------------------------------------------------------------------------------------------------------------------------------------------
CONVT_IDS = [R.case_id(c[:4]) for c in R.CONVT_CASES]


@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('dt', R.DTS, ids=R.dt_name)
@pytest.mark.parametrize('case', R.CONVT_CASES, ids=CONVT_IDS)
def test_convt_forward(case, dt, with_bias):
    """nc_convT_k2s2_fwd_c8 into channels [32, 32 + K) of a K + 64 channel buffer."""
    N, C, K, n, _ = case
    D, H, W = n
    Sf = 8 * D * H * W
    x, w, b, _ = R.convt_inputs(N, C, K, n, DEV)
    xr, wr, bias = x.to(R.tdt(dt)), w.to(R.tdt(dt)), (b if with_bias else None)
    xh = R.pack(xr)
    ctot, c0 = K + 64, 32
    need = L().nc_convT_c8_ws_bytes(N, C, D, H, W, K)
    assert need > 0

    def call(o, ws, nb):
        return L().nc_convT_k2s2_fwd_c8(P(xh), P(w), P(bias), o['y'].ptr, ctot, c0, N, C, D, H, W, K, dt, ws, nb, stream())
    o = exercise(call, dict(y=N * ctot * Sf * 2), need)['y']
    assert outside_keeps_fill(o, N, ctot, Sf, c0, K)
    got = R.unpack(R.view(o.view(R.tdt(dt), N, ctot // 8, Sf, 8), c0, K), (N, K, 2 * D, 2 * H, 2 * W))
    ref, e = R.ref_convt_fwd(xr, wr, bias)
    judge16('convT forward', R.case_id(case[:4]), dt, got, ref, e)


@pytest.mark.parametrize('case', R.CONVT_CASES, ids=CONVT_IDS)
def test_convt_gradients(case):
    """nc_convT_k2s2_dgrad_c8 / _wgrad_c8 (bf16) with dy in channels [8, 8 + K) of a K + 16 channel buffer; dbias NULL and non-NULL."""
    N, C, K, n, _ = case
    D, H, W = n
    Sc, Sf = D * H * W, 8 * D * H * W
    x, w, _, dy = R.convt_inputs(N, C, K, n, DEV)
    xr, wr, dyr = x.to(torch.bfloat16), w.to(torch.bfloat16), dy.to(torch.bfloat16)
    xh = R.pack(xr)
    ctot, c0 = K + 16, 8
    dyb = R.pack_into(nan_buffer(N, ctot, Sf, R.BF), dyr, c0)
    need = L().nc_convT_c8_ws_bytes(N, C, D, H, W, K)

    def call(o, ws, nb):
        return L().nc_convT_k2s2_dgrad_c8(P(dyb), ctot, c0, P(w), o['dx'].ptr, N, C, D, H, W, K, ws, nb, stream())
    o = exercise(call, dict(dx=N * C * Sc * 2), need)['dx']
    ref, e = R.ref_convt_dgrad(dyr, wr)
    judge16('convT %s' % R.convt_dgrad_kernel(C), R.case_id(case[:4]), R.BF, R.unpack(o.view(torch.bfloat16, N, C // 8, Sc, 8), x.shape), ref, e)

    def call(o, ws, nb):
        return L().nc_convT_k2s2_wgrad_c8(P(xh), P(dyb), ctot, c0, o['dw'].ptr, ptr_of(o['db']), N, C, D, H, W, K, ws, nb, stream())
    o = exercise(call, dict(dw=C * K * 8 * 4, db=K * 4), need)
    odw, odb = R.oracle_convt_wgrad(xr, wr, dyr)
    judge32('convT %s' % R.convt_wgrad_kernel(C), R.case_id(case[:4]), o['dw'].view(torch.float32, C, K, 2, 2, 2), R.CR.ref_wgrad(xr, dyr), odw)
    judge32('convT dbias', R.case_id(case[:4]), o['db'].view(torch.float32, K), R.CR.ref_dbias(dyr), odb)
    o2 = exercise(call, dict(dw=C * K * 8 * 4, db=None), need)
    assert torch.equal(o2['dw'].t, o['dw'].t)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# refusals: every row of tests/c8_reference.py REFUSALS returns its code on the host side (NC_ERR_SHAPE / _ARG / _WS, never NC_ERR_HIP: a
# launch the runtime rejected would be one), with outputs and workspace untouched
# ---------------------------------------------------------------------------------------------------------------------------------------------
POOL_BYTES = 32 << 20   # every pointer of a refusal call addresses this much: the largest row (C = 8 * 65536 at 2 x 2 x 2) needs 8 MiB
WS_BYTES = 128 << 20    # ... and the workspace this much: the forward checks it before the C > 320 refusal, and C = 352 asks for 67 MiB
_pool = {}


def pool_buffer(kind, name):
    k = (kind, name)
    if k not in _pool:
        _pool[k] = Buf(WS_BYTES if kind == 'ws' else POOL_BYTES) if kind != 'in' else torch.zeros(POOL_BYTES, dtype=torch.uint8, device=DEV)
    return _pool[k]


def ws_need(op, a):
    D, H, W = a.get('dims', (1, 1, 1))
    if op in ('stats', 'bwd'):
        return L().nc_c8_instnorm_ws_bytes(a['N'], a['C'], a['S'])
    if op.startswith('convt'):
        return L().nc_convT_c8_ws_bytes(a['N'], a['C'], D, H, W, a['K'])
    if op == 'outer64':
        return L().nc_c8_outer64_ws_bytes_debug(a['N'], a['S'])
    if op == 'fused_bwd':
        return L().nc_instnorm_bwd_dbias_ws_bytes(a['N'] * a['C'], a['S'])
    return 0


def refusal_call(op, a):
    """the call of entry `op` with the arguments `a`; pointers from the pool, 'null' = the first required input / output pointer is NULL"""
    seen = set()

    def p(kind, name):
        if kind in ('in', 'out') and a.get('null') == kind and kind not in seen:
            seen.add(kind)
            return ctypes.c_void_p(0)
        b = pool_buffer('out' if kind == 'opt' else kind, name)
        return b.ptr if isinstance(b, Buf) else P(b)
    wsb = ws_need(op, R.BASE[op]) - 1 if a.get('ws', 0) < 0 else WS_BYTES
    ws, st, dt = pool_buffer('ws', 'ws').ptr, stream(), a.get('dt')
    N, C, S, K = a.get('N'), a.get('C'), a.get('S'), a.get('K')
    D, H, W = a.get('dims', (1, 1, 1))
    ctot, c0 = a.get('ctot'), a.get('c0')
    lib = L()
    if op == 'stats':
        return lib.nc_c8_instnorm_stats(p('in', 'x'), N, C, S, R.EPS, p('out', 'mean'), p('out', 'rstd'), dt, ws, wsb, st)
    if op == 'apply':
        return lib.nc_c8_instnorm_act_fwd(p('in', 'x'), p('in', 'mean'), p('in', 'rstd'), 0.2, p('out', 'y'), ctot, c0, N, C, S, dt, st)
    if op == 'bwd':
        return lib.nc_c8_instnorm_act_bwd(p('in', 'g'), ctot, c0, p('in', 'x'), p('in', 'mean'), p('in', 'rstd'), 0.2, p('out', 'dx'), p('opt', 'db'), N, C, S,
                                          dt, ws, wsb, st)
    if op == 'from_c8':
        return lib.nc_from_c8(p('in', 'x'), ctot, c0, p('out', 'y'), N, C, S, dt, st)
    if op == 'pool':
        return lib.nc_c8_maxpool2_fwd(p('in', 'x'), ctot, c0, p('out', 'y'), N, C, D, H, W, dt, st)
    if op == 'pool_bwd':
        return lib.nc_c8_maxpool2_bwd_add(p('in', 'dp'), p('in', 'x'), ctot, c0, p('in', 'skip'), a['sctot'], a['sc0'], p('out', 'dx'), N, C, D, H, W, dt, st)
    if op == 'convt_fwd':
        return lib.nc_convT_k2s2_fwd_c8(p('in', 'x'), p('in', 'w'), p('in', 'b'), p('out', 'y'), ctot, c0, N, C, D, H, W, K, dt, ws, wsb, st)
    if op == 'convt_dgrad':
        return lib.nc_convT_k2s2_dgrad_c8(p('in', 'dy'), ctot, c0, p('in', 'w'), p('out', 'dx'), N, C, D, H, W, K, ws, wsb, st)
    if op == 'convt_wgrad':
        return lib.nc_convT_k2s2_wgrad_c8(p('in', 'x'), p('in', 'dy'), ctot, c0, p('out', 'dw'), p('opt', 'db'), N, C, D, H, W, K, ws, wsb, st)
    if op == 'dot64':
        return lib.nc_c8_dot64_debug(p('in', 'x'), p('in', 'w'), p('in', 'b'), p('out', 'out'), N, S, dt, st)
    if op == 'outer64':
        return lib.nc_c8_outer64_debug(p('in', 'g'), p('in', 'x'), p('in', 'w'), p('opt', 'dx'), p('out', 'dw'), p('opt', 'db'), N, S, dt, ws, wsb, st)
    if op == 'fused_fwd':
        return lib.nc_instnorm_act_fwd_c8(p('in', 'x'), p('in', 'mean'), p('in', 'rstd'), 0.2, p('opt', 'y'), p('out', 'yh'), N, C, S, dt, st)
    if op == 'fused_bwd':
        return lib.nc_instnorm_act_bwd_c8(p('in', 'dy'), p('in', 'x'), p('in', 'mean'), p('in', 'rstd'), 0.2, p('out', 'dx'), p('out', 'dxh'), p('opt', 'db'), N, C, S,
                                          dt, ws, wsb, st)
    raise KeyError(op)


@pytest.mark.parametrize('row', R.REFUSALS, ids=[R.refusal_id(r) for r in R.REFUSALS])
def test_refusals(row):
    op, what, changed, code = row
    a = R.refusal_args(op, changed)
    assert R.EXPECT[op](a) == code
    rc = refusal_call(op, a)
    torch.cuda.synchronize()
    dirty = [k for k, b in _pool.items() if isinstance(b, Buf) and not b.untouched()]
    for k in dirty:
        _pool[k].t.fill_(FILL)
    assert rc == code, (op, what, rc, err_text())
    assert not dirty, (op, what, dirty)


def test_the_library_sizes_the_workspaces_it_is_asked_for():
    """*_ws_bytes of a shape the entry refuses is 0 where the header says so; the sizes of the valid base calls are positive."""
    for op in ('stats', 'convt_fwd', 'outer64', 'fused_bwd'):
        assert ws_need(op, R.BASE[op]) > 0
    assert L().nc_convT_c8_ws_bytes(1, 48, 1, 1, 1, 32) == 0 and L().nc_c8_outer64_ws_bytes_debug(0, 4) == 0 and L().nc_c8_instnorm_ws_bytes(1, 12, 4) == 0
