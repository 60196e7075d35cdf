"""The prepared weights of the two-term Unet_deconv training step (nc_set_unet_wprep, csrc/w_prep.hip): nc_unet_deconv_train_fwd computes the
weight cells and the packed weights of blocks 1 .. 9, forward and data-gradient form, in one batched pass at its start and keeps them in
`saved`; the convolutions of the forward and the backward then launch without their three per-layer preparation launches.

Nothing about the arithmetic changes -- the batched kernels call the per-layer kernels' own device functions -- so every check is bitwise:
torch.equal with the switch on against off, the batched pass's bytes against the per-layer kernels' bytes, and `kept` bit 15 shows that the
prepared path was taken (or, under each fallback, that it was not)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neuroclear_amd import ops  # noqa: E402
from neuroclear_amd._lib import NcError, lib  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

DEV = 'cuda'
WPREP_BIT = 1 << 15
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# blocks 1 .. 9: (weight key, input channels, output channels, resolution level of the input)
BLOCKS = {1: ('double_conv1.convolution.3', 64, 64, 0), 2: ('double_conv2.convolution.0', 64, 128, 1),
          3: ('double_conv2.convolution.3', 128, 128, 1), 4: ('bottom_layer.convolution.0', 128, 256, 2),
          5: ('bottom_layer.convolution.3', 256, 256, 2), 6: ('bottom_layer.convolution.6', 256, 256, 2),
          7: ('ex_double_conv2.convolution.0', 256, 128, 1), 8: ('ex_double_conv2.convolution.3', 128, 128, 1),
          9: ('ex_conv1_1.convolution.0', 128, 64, 0)}


@pytest.fixture
def switches():
    L = lib()
    prev = L.nc_get_split_terms(), L.nc_get_unet_lean(), L.nc_get_h2_guard(), ops.set_conv_split(True), L.nc_get_unet_wprep()
    L.nc_set_split_terms(2)
    yield L
    L.nc_set_split_terms(prev[0])
    L.nc_set_unet_lean(prev[1])
    L.nc_set_h2_guard(prev[2])
    ops.set_conv_split(prev[3])
    L.nc_set_unet_wprep(prev[4])


def _run(sd, x, r):
    """One whole-network training forward + backward; returns (y, dx, gradients by name) and the forward's `kept` word."""
    net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0])
    net.load_state_dict(sd)
    xi = x.clone().requires_grad_(True)
    y = net(xi)
    kept = int(y.grad_fn.kept)
    (y * r).mean().backward()
    return (y.detach().clone(), xi.grad.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}), kept


def _same(a, b):
    (y0, dx0, g0), (y1, dx1, g1) = a, b
    assert torch.equal(y0, y1)
    assert torch.equal(dx0, dx1)
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        assert torch.equal(g0[k], g1[k]), k


def _data(shape, n, seed=5):
    sd = S.state_dict_from_seed(S.unet_deconv_spec(), seed, DEV)
    x = torch.from_numpy(np.random.default_rng(31).random((n, 1) + shape, dtype=np.float32)).to(DEV)
    r = torch.from_numpy(np.random.default_rng(32).standard_normal((n, 1) + shape).astype(np.float32)).to(DEV)
    return sd, x, r


@pytest.mark.parametrize('lean', [1, 0])
@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('shape', [(24, 24, 24), (40, 24, 32)])
def test_prepared_weights_change_no_bit(shape, n, lean, switches):
    """Switch on against off: y, dx and every parameter gradient are torch.equal; the forward reports the packs (kept bit 15) with the switch on
    and not with it off."""
    assert networks._FUSED_GEN
    sd, x, r = _data(shape, n)
    switches.nc_set_unet_lean(lean)
    switches.nc_set_unet_wprep(0)
    assert switches.nc_get_unet_wprep() == 0
    off, kept_off = _run(sd, x, r)
    switches.nc_set_unet_wprep(1)
    assert switches.nc_get_unet_wprep() == 1
    on, kept_on = _run(sd, x, r)
    print(shape, n, lean, 'kept: off %#x on %#x' % (kept_off, kept_on))
    assert kept_on & WPREP_BIT and not kept_off & WPREP_BIT
    assert kept_on & ~WPREP_BIT == kept_off
    _same(off, on)


def test_prepared_weights_under_a_guard_that_switches(switches):
    """nc_set_h2_guard(2) with block 1's dY flagged (tests/test_gpu_unet_lean.py 'dark_channels'): the flagged call runs on the three-term
    kernels, which pack their own weights; the two-term launches of every other call take the prepared packs.  On against off: torch.equal, the
    same number of calls fell back, at least one did."""
    size = 32
    sd = S.state_dict_from_seed(S.unet_deconv_spec(), 4, DEV)
    x = torch.from_numpy(np.random.default_rng(7).random((1, 1, size, size, size), dtype=np.float32)).to(DEV)
    r = torch.from_numpy(np.random.default_rng(8).random((1, 1, size, size, size), dtype=np.float32)).to(DEV)
    for k in ('double_conv2.convolution.0.weight', 'ex_conv1_1.convolution.0.weight'):
        w = sd[k].clone()
        w[:, :16] *= 2.0 ** -24
        sd[k] = w
    out4 = (ctypes.c_ulonglong * 4)()

    def fell():
        torch.cuda.synchronize()
        assert switches.nc_h2_guard_stats(out4, 0) == 0
        return int(out4[1])
    switches.nc_set_h2_guard(2)
    res, nfell, kept = {}, {}, {}
    for on in (0, 1):
        switches.nc_set_unet_wprep(on)
        before = fell()
        res[on], kept[on] = _run(sd, x, r)
        nfell[on] = fell() - before
    print('calls that fell back to the three-term kernels:', nfell, 'kept: %#x %#x' % (kept[0], kept[1]))
    assert nfell[0] == nfell[1] >= 1
    assert kept[1] & WPREP_BIT and not kept[0] & WPREP_BIT
    _same(res[0], res[1])


@pytest.mark.parametrize('fallback', ['terms3', 'split_off', 'bwd_switch_off', 'bwd_terms3'])
def test_fallbacks_launch_what_they_launched(fallback, switches):
    """nc_set_split_terms(3) and the split kernels off: nothing is prepared (bit 15 clear) and the results are those of the switch-off run under
    the same setting.  The switch, or the number of terms, moved between forward and backward: the backward ignores the packs -- the results are
    those of a run that never had them."""
    sd, x, r = _data((24, 24, 24), 1)

    def setting(on):
        switches.nc_set_unet_wprep(on)
        if fallback == 'terms3':
            switches.nc_set_split_terms(3)
        if fallback == 'split_off':
            ops.set_conv_split(False)
    if fallback in ('terms3', 'split_off'):
        setting(0)
        off, kept_off = _run(sd, x, r)
        setting(1)
        on, kept_on = _run(sd, x, r)
        assert not kept_on & WPREP_BIT and kept_on == kept_off
        _same(off, on)
        return

    def one(on_fwd, after_fwd):
        net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0])
        net.load_state_dict(sd)
        switches.nc_set_split_terms(2)
        switches.nc_set_unet_wprep(on_fwd)
        xi = x.clone().requires_grad_(True)
        y = net(xi)
        kept = int(y.grad_fn.kept)
        after_fwd()
        (y * r).mean().backward()
        return (y.detach().clone(), xi.grad.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}), kept
    move = (lambda: switches.nc_set_unet_wprep(0)) if fallback == 'bwd_switch_off' else (lambda: switches.nc_set_split_terms(3))
    off, kept_off = one(0, move)
    on, kept_on = one(1, move)
    assert kept_on & WPREP_BIT and not kept_off & WPREP_BIT
    _same(off, on)


_CHILD = r'''
import hashlib, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from neuroclear_amd._lib import lib
from neuroclear_amd.models import networks
from neuroclear_amd.util import seed as S
L = lib()
sd = S.state_dict_from_seed(S.unet_deconv_spec(), 5, 'cuda')
x = torch.from_numpy(np.random.default_rng(31).random((1, 1, 24, 24, 24), dtype=np.float32)).cuda()
r = torch.from_numpy(np.random.default_rng(32).standard_normal((1, 1, 24, 24, 24)).astype(np.float32)).cuda()
for on in (0, 1):
    if on != L.nc_get_unet_wprep():
        L.nc_set_unet_wprep(on)
    net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0])
    net.load_state_dict(sd)
    xi = x.clone().requires_grad_(True)
    y = net(xi)
    kept = int(y.grad_fn.kept)
    (y * r).mean().backward()
    h = hashlib.sha256()
    for t in [y.detach(), xi.grad] + [p.grad for p in net.parameters()]:
        h.update(t.detach().cpu().numpy().tobytes())
    print('RESULT', on, kept, h.hexdigest(), L.nc_get_unet_wprep())
'''


def _child(env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    out = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT}], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [l.split() for l in out.stdout.splitlines() if l.startswith('RESULT')]
    assert len(rows) == 2, out.stdout
    return {int(r_[1]): (int(r_[2]), r_[3]) for r_ in rows}


def test_fallbacks_set_by_the_environment():
    """The load-time switches, each in a fresh process (one at a time).  NC_S3_TRAIN_FUSE=0 and NC_CONV_SPLIT=0: nothing prepared.  NC_CONVT_H2=0:
    the transposed convolutions' halves get a measured cell -- the packs exist (bit 15), only the forward packs of blocks 7 and 9 are left to the
    per-layer launches.  NC_UNET_WPREP=0: the switch starts off.  In every one the switch-on results are the switch-off results, and all of them
    but NC_CONVT_H2=0 (another cell: other bits by design) give the default configuration's bits."""
    base = _child({})
    assert base[1][0] & WPREP_BIT and not base[0][0] & WPREP_BIT
    assert base[0][1] == base[1][1]
    for name, prepared in (('NC_S3_TRAIN_FUSE', False), ('NC_CONV_SPLIT', False), ('NC_CONVT_H2', True)):
        got = _child({name: '0'})
        print(name, '= 0: kept off %#x on %#x' % (got[0][0], got[1][0]))
        assert bool(got[1][0] & WPREP_BIT) == prepared, name
        assert not got[0][0] & WPREP_BIT
        assert got[0][1] == got[1][1], name
    env_off = subprocess.run([sys.executable, '-c', 'import sys; sys.path.insert(0, %r); from neuroclear_amd._lib import lib; '
                              'print("WPREP", lib().nc_get_unet_wprep())' % ROOT], env=dict(os.environ, NC_UNET_WPREP='0'),
                             capture_output=True, text=True, timeout=600)
    assert env_off.returncode == 0 and 'WPREP 0' in env_off.stdout, env_off.stderr[-2000:]


def test_batched_pass_writes_the_per_layer_bytes(switches):
    """Every block, both forms: the pack and the weight cell the batched pass left in `saved` equal, byte for byte, what the per-layer
    preparation (zero the cell, k_absmax_w, k_pack_w_s3x<2>) writes for the same weights and the same input cells; the two transposed
    convolutions' bounds equal the per-layer k_convT_bound's.  Blocks 7 and 9 take a concatenation whose halves have DIFFERENT powers of two
    (asserted), so the group factor is exercised."""
    L = switches
    shape = (24, 24, 24)
    sd, x, r = _data(shape, 1)
    for k in ('t_conv2.weight', 't_conv1.weight'):  # (a bound well away from the InstanceNorm bound of the other half)
        sd[k] = sd[k] * 16.0
    net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0])
    net.load_state_dict(sd)
    L.nc_set_unet_wprep(1)
    y = net(x.clone().requires_grad_(True))
    assert int(y.grad_fn.kept) & WPREP_BIT
    saved = y.grad_fn.saved_tensors[2]
    raw = saved.view(torch.uint8)
    torch.cuda.synchronize()
    vox = [shape[0] * shape[1] * shape[2] >> (3 * l) for l in range(3)]
    Z = ctypes.c_size_t

    def word(off):
        return int(raw[off:off + 4].view(torch.int32).item()) & 0xffffffff

    def dev_word(bits):
        return torch.tensor([bits if bits < 2 ** 31 else bits - 2 ** 32], dtype=torch.int32, device=DEV)

    def f32_bits(v):
        return int(np.float32(v).view(np.uint32))
    # the bounds, per layer
    bounds = {}
    for blk, key, C, K, lvl_in in ((7, 't_conv2', 256, 128, 2), (9, 't_conv1', 128, 64, 1)):
        cell = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        w, b = sd[key + '.weight'].contiguous(), sd[key + '.bias'].contiguous()
        assert L.nc_convT_h2_bound_debug(ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(b.data_ptr()), C, K,
                                         ctypes.c_float(float(np.sqrt(np.float32(vox[lvl_in])))), ctypes.c_void_p(cell.data_ptr()), None) == 0
        torch.cuda.synchronize()
        bounds[blk] = int(cell.item()) & 0xffffffff
    exp = lambda bits: bits >> 23  # noqa: E731
    for blk, (key, C, K, lvl) in BLOCKS.items():
        w = sd[key + '.weight'].contiguous()
        a_bits = f32_bits(np.sqrt(np.float32(vox[lvl])))
        b_bits = bounds.get(blk, a_bits)
        for form in (0, 1):
            po, pb, co, bo = Z(0), Z(0), Z(0), Z(0)
            assert L.nc_unet_wprep_layout(1, *shape, blk, form, ctypes.byref(po), ctypes.byref(pb), ctypes.byref(co), ctypes.byref(bo)) == 0
            assert pb.value == C * K * 27 * 4
            if blk in bounds:
                assert word(bo.value) == bounds[blk], blk
                assert exp(bounds[blk]) != exp(a_bits), (blk, hex(bounds[blk]), hex(a_bits))  # two different powers of two
            ca, cb = dev_word(a_bits), dev_word(b_bits)
            wp = torch.full((pb.value,), 0xa5, dtype=torch.uint8, device=DEV)
            wc = torch.full((1,), -1, dtype=torch.int32, device=DEV)
            assert L.nc_s3x_pack_h2_debug(ctypes.c_void_p(w.data_ptr()), C, K, form, ctypes.c_void_p(ca.data_ptr()), ctypes.c_void_p(cb.data_ptr()),
                                          ctypes.c_void_p(wp.data_ptr()), ctypes.c_void_p(wc.data_ptr()), None) == 0
            torch.cuda.synchronize()
            assert word(co.value) == int(wc.item()) & 0xffffffff, (blk, form)
            assert word(co.value) != 0
            assert torch.equal(raw[po.value:po.value + pb.value], wp), (blk, form)
    # ... and the forward left the bounds in the second cells of the concat blocks' H2 inputs, where the per-layer forward puts them
    L.nc_set_unet_wprep(0)
    y0 = net(x.clone().requires_grad_(True))
    assert torch.equal(y0, y)


def test_backward_after_a_parameter_update_raises(switches):
    """The data gradients use the weights of forward time (the packs in `saved`), the weight-space reads the live buffer: a backward after the
    parameter buffer changed in place is refused."""
    from neuroclear_amd.models.axial_to_lateral_gan_apollo_model import FlatAdam
    sd, x, r = _data((24, 24, 24), 1)
    net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0])
    net.load_state_dict(sd)
    opt = FlatAdam(net.parameters(), 1e-4, (0.5, 0.999))  # the parameters become views of one flat buffer
    for touch in (lambda: opt.flat.mul_(1.0), lambda: next(net.parameters()).mul_(1.0)):
        y = net(x.clone().requires_grad_(True))
        with torch.no_grad():
            touch()
        with pytest.raises(NcError, match='updated between'):
            (y * r).mean().backward()
    opt.zero_grad()
    y = net(x.clone().requires_grad_(True))  # (an untouched buffer: fine)
    (y * r).mean().backward()
