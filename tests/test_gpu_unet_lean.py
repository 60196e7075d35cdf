"""The lean forms of the two-term Unet_deconv training step (nc_set_unet_lean, csrc/gen_nets.hip): the forward leaves out fp32 activations that
only a two-term convolution with its own H2 copy reads, and the backward never expands the rank-one data gradient behind one_by_one --
block 9's InstanceNorm backward forms w12[c] * s2[v] on the fly.

Neither form changes an operand or a summation: the forward is untouched arithmetic, every block's dY operand must be bit for bit what the full
forms write, and one_by_one's own gradients stay with the matrix kernel.  So with the switch on and off the output, dx and EVERY gradient are
torch.equal; the tail's gradients are also compared with an fp64 evaluation of the network and may be no further from it than the full forms'
are on the same inputs."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neuroclear_amd import ops  # noqa: E402
from neuroclear_amd._lib import lib  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402
from oracle import nets as onets  # noqa: E402

DEV = 'cuda'
TAIL = ('one_by_one.weight', 'one_by_one.bias', 'one_by_one_2.weight', 'one_by_one_2.bias')


@pytest.fixture
def switches():
    L = lib()
    prev = L.nc_get_split_terms(), L.nc_get_unet_lean(), L.nc_get_h2_guard(), ops.set_conv_split(True)
    L.nc_set_split_terms(2)
    yield L
    L.nc_set_split_terms(prev[0])
    L.nc_set_unet_lean(prev[1])
    L.nc_set_h2_guard(prev[2])
    ops.set_conv_split(prev[3])


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _run(sd, x, r):
    """One whole-network training forward + backward; returns y, dx and the parameter gradients by name."""
    net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0])
    net.load_state_dict(sd)
    xi = x.clone().requires_grad_(True)
    y = net(xi)
    (y * r).mean().backward()
    return y.detach().clone(), xi.grad.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}


class _Poison:
    """While active, the `saved` buffer of every whole-network U-Net forward (ops.py allocates it with torch.empty) starts as NaN, and the last
    one is kept: what a forward did not write stays NaN, and a backward that reads it cannot pass for right by finding a previous step's values
    in a recycled allocation."""

    def __init__(self, monkeypatch, shape, n=1):
        self.numel = int(lib().nc_unet_deconv_saved_floats(n, *shape))
        self.a1 = n * 64 * shape[0] * shape[1] * shape[2]  # a1 is the first tensor of `saved` (csrc/gen_nets.hip u_plan)
        self.saved = None
        real = torch.empty

        def empty(*a, **k):
            t = real(*a, **k)
            if t.is_cuda and t.dtype == torch.float32 and t.dim() == 1 and t.numel() == self.numel:
                t.fill_(float('nan'))
                self.saved = t
            return t
        monkeypatch.setattr(torch, 'empty', empty)

    def a1_written(self):
        """True / False: the forward wrote all / none of the fp32 a1."""
        nan = torch.isnan(self.saved[:self.a1])
        assert bool(nan.all()) or not bool(nan.any())
        return not bool(nan.any())


def _pointwise_dgrads(fn):
    """Number of 1 x 1 data-gradient launches (nc_prof: op 1, kernel edge 1) while fn runs."""
    L = lib()
    L.nc_prof_begin(ctypes.c_double(0.0))
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        n = 4096
        cls, flop, ms = (ctypes.c_int * n)(), (ctypes.c_double * n)(), (ctypes.c_float * n)()
        got = L.nc_prof_end(n, cls, flop, ms)
    assert 0 <= got <= n
    return out, sum(1 for i in range(got) if (cls[i] & 15) == 1 and ((cls[i] >> 8) & 255) == 1)


def _fp64(sd_np, x_np, r_np):
    sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd_np.items()}
    x = torch.from_numpy(x_np).double()
    y = onets.unet_deconv(sd, x)
    (y * torch.from_numpy(r_np).double()).mean().backward()
    return {k: v.grad for k, v in sd.items()}


SHAPES = [(24, 24, 24), (40, 24, 32)]  # (the second: >= 16384 voxels at full resolution, where the 1 x 1 layers take the flat matrix kernels as at 108^3)
_RUNS = {}


def _both(shape, L, monkeypatch, tiny=False):
    """The same forward + backward with the lean switch off (0) and on (1), once per shape, each on a NaN-filled `saved`; with what shows that
    the lean forms were TAKEN: whether the forward wrote fp32 a1, and how many 1 x 1 data gradients the backward launched."""
    key = shape + (tiny,)
    if key not in _RUNS:
        spec = S.unet_deconv_spec()
        sd_np = S.weights_from_seed(spec, 5)
        if tiny:  # w12 * s2 in fp32's subnormal range (s2 is ~1e-6 here): the rank-one product against the matrix instruction's, which keeps denormals
            sd_np = dict(sd_np)
            sd_np['one_by_one.weight'] = (sd_np['one_by_one.weight'] * np.float32(2.0 ** -108)).astype(np.float32)
        sd = {k: torch.from_numpy(v).to(DEV) for k, v in sd_np.items()}
        poison = _Poison(monkeypatch, shape)
        x_np = np.random.default_rng(31).random((1, 1) + shape, dtype=np.float32)
        r_np = np.random.default_rng(32).standard_normal((1, 1) + shape).astype(np.float32)
        x, r = torch.from_numpy(x_np).to(DEV), torch.from_numpy(r_np).to(DEV)
        res, taken = [], []
        for lean in (0, 1):
            L.nc_set_unet_lean(lean)
            assert L.nc_get_unet_lean() == lean
            out, ndg = _pointwise_dgrads(lambda: _run(sd, x, r))
            res.append(out)
            taken.append((poison.a1_written(), ndg))
        _RUNS[key] = (sd_np, x_np, r_np, res[0], res[1], taken)
    return _RUNS[key]


@pytest.mark.parametrize('shape,tiny', [(SHAPES[0], False), (SHAPES[1], False), (SHAPES[1], True)])
def test_lean_forms_change_no_operand(shape, tiny, switches, monkeypatch):
    """Switch on against switch off: y, dx and the gradients of blocks 0 .. 9, both transposed convolutions and both 1 x 1 layers are torch.equal --
    the dY operand of every block is the same bits, i.e. the rank-one product w12[c] * s2[v] reproduces the value the fp32 matrix kernel of
    one_by_one's data gradient stores (one fused multiply-add onto a zero accumulator), on the flat-kernel shape and on the small one."""
    assert networks._FUSED_GEN
    _, _, _, (y0, dx0, g0), (y1, dx1, g1), taken = _both(shape, switches, monkeypatch, tiny)
    # the lean forms were taken: fp32 a1 written by the full forward only; one_by_one's data gradient launched by the full backward only
    print(shape, tiny, '(a1 written, 1 x 1 data gradients): full', taken[0], 'lean', taken[1])
    assert taken[0][0] is True and taken[1][0] is False
    assert taken[0][1] == 2 and taken[1][1] == 1
    if tiny:
        big = float(g0['ex_conv1_1.convolution.0.weight'].abs().max())
        assert 0.0 < big < 1e-30, big  # (the gradient behind one_by_one really is down there)
    assert torch.equal(y0, y1)
    assert torch.equal(dx0, dx1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
        assert torch.isfinite(g1[k]).all(), k


@pytest.mark.parametrize('shape', SHAPES)
def test_tail_gradients_against_fp64(shape, switches, monkeypatch):
    """dW12, db12, dW13, db13 against an fp64 evaluation of the network on the same inputs: the lean forms no further from it than the full
    forms (no margin).  They come from the same kernels on the same bits, so the two distances are equal; a sum taken in another order would
    show here (an fp64 sum of the same products inside the norm backward landed 0.4 % further at both shapes, 2.3150e-06 against 2.3068e-06
    at 24^3: both sit at the distance the fp32 network upstream puts them, and that form was dropped)."""
    sd_np, x_np, r_np, (_, _, g0), (_, _, g1), _ = _both(shape, switches, monkeypatch)
    g64 = _fp64(sd_np, x_np, r_np)
    worse = []
    for k in TAIL:
        e0, e1 = rel(g0[k], g64[k]), rel(g1[k], g64[k])
        print('%s %-22s distance to fp64: full forms %.4e, lean %.4e' % (shape, k, e0, e1))
        if not e1 <= e0:
            worse.append((k, e1, e0))
    assert not worse, worse


def test_lean_forms_two_samples(switches):
    """N = 2: the forward's lean form applies per sample, the rank-one backward is routed to the full form -- everything is torch.equal."""
    spec = S.unet_deconv_spec()
    sd = S.state_dict_from_seed(spec, 6, DEV)
    x = torch.from_numpy(np.random.default_rng(41).random((2, 1, 24, 24, 24), dtype=np.float32)).to(DEV)
    r = torch.from_numpy(np.random.default_rng(42).standard_normal((2, 1, 24, 24, 24)).astype(np.float32)).to(DEV)
    switches.nc_set_unet_lean(0)
    y0, dx0, g0 = _run(sd, x, r)
    switches.nc_set_unet_lean(1)
    y1, dx1, g1 = _run(sd, x, r)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def moved_switch_case():
    """The network, input and output gradient of the moved-switch runs below (tests/test_gpu_unet_forms.py repeats one of them)."""
    torch.manual_seed(21)
    net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'normal', 0.02, [0])
    return net, torch.rand(1, 1, 24, 24, 24, device=DEV), torch.randn(1, 1, 24, 24, 24, device=DEV)


def moved_switch_grads(net, x, g, before_fwd, before_bwd):
    """One forward and its backward with before_fwd() / before_bwd() called in front of each; the weight gradients, flattened."""
    for p_ in net.parameters():
        p_.grad = None
    before_fwd()
    y = net(x)
    before_bwd()
    y.backward(g)
    return torch.cat([p_.grad.reshape(-1).clone() for p_ in net.parameters() if p_.dim() > 1])


def test_lean_forward_then_another_backward(switches):
    """A lean forward did not write a1, a2, b1, b2, e2a.  A backward that cannot use the kept H2 copies -- the split kernels were switched off,
    or the number of terms moved, between the two calls -- writes them again; a backward under the lean switch after a full forward needs
    nothing.  All combinations: finite and within 5e-3 (relative L2 of the weight gradients) of the all-fp32 run, as
    tests/test_gpu_split.py::test_switch_toggled_between_forward_and_backward asks of the full forms."""
    net, x, g = moved_switch_case()
    grads = {}

    def one(key, before_fwd, before_bwd):
        grads[key] = moved_switch_grads(net, x, g, before_fwd, before_bwd)
    switches.nc_set_unet_lean(1)
    for fwd_on in (True, False):
        for bwd_on in (True, False):
            one(('split', fwd_on, bwd_on), lambda: ops.set_conv_split(fwd_on), lambda: ops.set_conv_split(bwd_on))
    ops.set_conv_split(True)
    one(('terms', 2, 3), lambda: switches.nc_set_split_terms(2), lambda: switches.nc_set_split_terms(3))
    one(('terms', 3, 2), lambda: switches.nc_set_split_terms(3), lambda: switches.nc_set_split_terms(2))
    switches.nc_set_split_terms(2)
    one(('lean', 1, 0), lambda: switches.nc_set_unet_lean(1), lambda: switches.nc_set_unet_lean(0))
    one(('lean', 0, 1), lambda: switches.nc_set_unet_lean(0), lambda: switches.nc_set_unet_lean(1))
    ref = grads[('split', False, False)].double()
    for k, v in grads.items():
        assert torch.isfinite(v).all(), k
        d = ((v.double() - ref).norm() / ref.norm()).item()
        print(k, 'relative L2 difference of the weight gradients to the all-fp32 run: %.2e' % d)
        assert d < 5e-3, (k, d)


@pytest.mark.parametrize('kind', ['dark_channels', 'dark_half'])
def test_lean_forward_under_a_guard_that_switches(kind, switches, monkeypatch):
    """nc_set_h2_guard(2): a dY tensor the range guard flags sends that block's gradients to the three-term kernels INSIDE the call, and the
    weight gradient then builds its three-term x operand from the block's fp32 input -- which for blocks 1, 3, 5, 6, 8 the lean forward did not
    write.  The backward writes it again first.  `saved` starts as NaN in every run, so a read of an unwritten tensor shows.
    'dark_channels' (tests/test_gpu_h2.py::test_h2_guard_covers_the_norm_backward_output): the layers behind double_conv1 all but ignore 16 of its
    64 channels, so block 1's dY -- the block whose input is the dropped a1 -- has a block of channels 2^-24 below the rest and is flagged: its
    weight gradient differs from the guard-off run's.  'dark_half': the input volume's planes z < D / 2 are 2^-21 of the rest (test_gpu_h2.py
    data('dark_half')) -- measured: no dY of this network is flagged by it (the first InstanceNorm sees one volume), so this case only shows that
    the rematerialising backward of mode 2 is the full form's.  Lean against full: every gradient finite and torch.equal; against the all-fp32 run within 5e-3."""
    size = 32
    spec = S.unet_deconv_spec()
    sd = S.state_dict_from_seed(spec, 4, DEV)
    x = torch.from_numpy(np.random.default_rng(7).random((1, 1, size, size, size), dtype=np.float32)).to(DEV)
    r = torch.from_numpy(np.random.default_rng(8).random((1, 1, size, size, size), dtype=np.float32)).to(DEV)
    if kind == 'dark_channels':
        for k in ('double_conv2.convolution.0.weight', 'ex_conv1_1.convolution.0.weight'):
            w = sd[k].clone()
            w[:, :16] *= 2.0 ** -24
            sd[k] = w
    else:
        x[:, :, :size // 2] *= 2.0 ** -21
    poison = _Poison(monkeypatch, (size, size, size))
    out4 = (ctypes.c_ulonglong * 4)()

    def fell():
        torch.cuda.synchronize()
        assert switches.nc_h2_guard_stats(out4, 0) == 0
        return int(out4[1])
    res, nfell = {}, {}
    for guard, lean in ((0, 0), (2, 0), (2, 1)):
        switches.nc_set_h2_guard(guard)
        switches.nc_set_unet_lean(lean)
        before = fell()
        res[(guard, lean)] = _run(sd, x, r)
        nfell[(guard, lean)] = fell() - before
        assert poison.a1_written() == (lean == 0)
    switches.nc_set_h2_guard(1)
    ops.set_conv_split(False)
    _, _, gref = _run(sd, x, r)
    ops.set_conv_split(True)
    print(kind, 'calls that fell back to the three-term kernels:', nfell)
    assert nfell[(2, 0)] == nfell[(2, 1)] and nfell[(0, 0)] == 0
    (y0, dx0, g0), (y1, dx1, g1) = res[(2, 0)], res[(2, 1)]
    if kind == 'dark_channels':
        assert nfell[(2, 1)] >= 1
        k1 = 'double_conv1.convolution.3.weight'  # block 1: flagged = its gradient ran on other kernels than with the guard off
        assert not torch.equal(res[(0, 0)][2][k1], g0[k1])
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        assert torch.equal(g0[k], g1[k]), k
    cat = lambda g_: torch.cat([v.reshape(-1) for k, v in g_.items() if v.dim() > 1]).double()  # noqa: E731
    d = float((cat(g1) - cat(gref)).norm() / cat(gref).norm())
    print(kind, 'relative L2 difference of the weight gradients to the all-fp32 run: %.2e' % d)
    assert d < 5e-3


def test_lean_rank_one_under_the_range_guard(switches):
    """one_by_one all but ignores 16 of its 64 input channels (weights 2^-24 of the others), so a block of channels of block 9's dY sits 2^-24
    below the rest: the range guard flags the tensor and, in mode 2, the norm backward rewrites it in three-term form.  The rewrite takes the
    gradient from the same source as the pass it repeats: with the lean switch on and off every gradient is torch.equal,
    the call fell back in both, and the gradients are finite and within 5e-3 of the all-fp32 run."""
    size = 32
    spec = S.unet_deconv_spec()
    sd = S.state_dict_from_seed(spec, 4, DEV)
    w = sd['one_by_one.weight'].clone()
    w[:, :16] *= 2.0 ** -24
    sd['one_by_one.weight'] = w
    x = torch.from_numpy(np.random.default_rng(7).random((1, 1, size, size, size), dtype=np.float32)).to(DEV)
    r = torch.from_numpy(np.random.default_rng(8).random((1, 1, size, size, size), dtype=np.float32)).to(DEV)
    out4 = (ctypes.c_ulonglong * 4)()

    def fell():
        torch.cuda.synchronize()
        assert switches.nc_h2_guard_stats(out4, 0) == 0
        return int(out4[1])
    switches.nc_set_h2_guard(2)
    res = {}
    for lean in (0, 1):
        switches.nc_set_unet_lean(lean)
        before = fell()
        res[lean] = _run(sd, x, r)
        assert fell() - before >= 1, lean
    switches.nc_set_h2_guard(1)
    ops.set_conv_split(False)
    _, _, gref = _run(sd, x, r)
    ops.set_conv_split(True)
    (y0, dx0, g0), (y1, dx1, g1) = res[0], res[1]
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        assert torch.equal(g0[k], g1[k]), k
    cat = lambda g_: torch.cat([v.reshape(-1) for k, v in g_.items() if v.dim() > 1]).double()  # noqa: E731
    d = float((cat(g1) - cat(gref)).norm() / cat(gref).norm())
    print('relative L2 difference of the weight gradients to the all-fp32 run: %.2e' % d)
    assert d < 5e-3
