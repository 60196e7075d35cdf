"""The plan of the Unet_deconv training forward (csrc/gen_nets.hip u_fwd_forms): every form the forward takes is decided before its first launch,
and the `kept` word it returns is part of that plan.  nc_unet_deconv_kept_expected returns the plan's word without launching anything; the
forward checks conv_fwd_keep's own answers against it.  Here: the word the forward hands to autograd IS the planned one, under every
combination of the switches that move a bit, at the shapes where the step takes other kernels, and a query changes nothing downstream."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuroclear_amd import ops  # noqa: E402
from neuroclear_amd._lib import lib  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from test_gpu_unet_lean import moved_switch_case, moved_switch_grads  # noqa: E402

DEV = 'cuda'
DEFAULT = dict(terms=2, lean=1, wprep=1, fold=1, split=True)


@pytest.fixture
def switches():
    L = lib()
    prev = (L.nc_get_split_terms(), L.nc_get_unet_lean(), L.nc_get_unet_wprep(), L.nc_get_in_bwd_fold(), ops.set_conv_split(True))
    yield L
    L.nc_set_split_terms(prev[0])
    L.nc_set_unet_lean(prev[1])
    L.nc_set_unet_wprep(prev[2])
    L.nc_set_in_bwd_fold(prev[3])
    ops.set_conv_split(prev[4])


@pytest.fixture(scope='module')
def net():
    torch.manual_seed(3)
    return networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'normal', 0.02, [0])


def _set(L, terms, lean, wprep, fold, split):
    L.nc_set_split_terms(terms)
    L.nc_set_unet_lean(lean)
    L.nc_set_unet_wprep(wprep)
    L.nc_set_in_bwd_fold(fold)
    ops.set_conv_split(split)


def _planned_and_kept(L, net, x):
    """(the query's word just before the forward, the forward's grad_fn.kept)"""
    assert networks._FUSED_GEN
    planned = int(L.nc_unet_deconv_kept_expected(x.shape[0], *x.shape[2:]))
    y = net(x)
    return planned, int(y.grad_fn.kept)


def test_full_matrix(switches, net):
    """N = 1, 24^3: split_terms {2, 3} x unet_lean x unet_wprep x in_bwd_fold x conv-split, all 32."""
    x = torch.rand(1, 1, 24, 24, 24, device=DEV)
    words = set()
    for terms, lean, wprep, fold, split in itertools.product((2, 3), (0, 1), (0, 1), (0, 1), (True, False)):
        _set(switches, terms, lean, wprep, fold, split)
        planned, kept = _planned_and_kept(switches, net, x)
        print('terms %d lean %d wprep %d fold %d split %d: planned %08x kept %08x' % (terms, lean, wprep, fold, split, planned, kept))
        assert kept == planned, (terms, lean, wprep, fold, split, hex(planned), hex(kept))
        words.add(kept)
    assert len(words) > 8  # (the switches do move the word: the query is not a constant)


# (1; 40,24,32): the 1 x 1 layers take the flat kernels; (2; 24^3): the per-sample loops and gather_half
@pytest.mark.parametrize('n,shape', [(1, (40, 24, 32)), (1, (28, 28, 28)), (2, (24, 24, 24))])
def test_shapes(n, shape, switches, net):
    """All switches at their defaults, then each singly off."""
    x = torch.rand((n, 1) + shape, device=DEV)
    single_off = dict(terms=3, lean=0, wprep=0, fold=0, split=False)
    for off in (None,) + tuple(single_off):
        cfg = dict(DEFAULT)
        if off:
            cfg[off] = single_off[off]
        _set(switches, **cfg)
        planned, kept = _planned_and_kept(switches, net, x)
        print(n, shape, 'off:', off, 'planned %08x kept %08x' % (planned, kept))
        assert kept == planned, (off, hex(planned), hex(kept))
        if off is None:
            assert kept & (1 << 15) and kept & (1 << 26)  # (prepared weights and winner bytes: the default step)


def test_moved_switch(switches):
    """A query in front of the forward, then split_terms 2 -> 3 before the backward: the gradients of
    test_gpu_unet_lean.py::test_lean_forward_then_another_backward's ('terms', 2, 3) run, bit for bit."""
    _set(switches, **DEFAULT)
    net, x, g = moved_switch_case()
    ref = moved_switch_grads(net, x, g, lambda: switches.nc_set_split_terms(2), lambda: switches.nc_set_split_terms(3))
    planned = []

    def query_then_forward():
        switches.nc_set_split_terms(2)
        planned.append(int(switches.nc_unet_deconv_kept_expected(1, 24, 24, 24)))
    got = moved_switch_grads(net, x, g, query_then_forward, lambda: switches.nc_set_split_terms(3))
    switches.nc_set_split_terms(2)  # (the query follows the switch: three terms now would plan another word)
    assert planned[0] != 0 and planned[0] == int(switches.nc_unet_deconv_kept_expected(1, 24, 24, 24))
    assert torch.isfinite(got).all()
    assert torch.equal(got, ref)


def test_bad_shape(switches):
    """An edge that is not a multiple of 4: 0, as the other shape queries answer."""
    for n, shape in ((1, (24, 24, 26)), (1, (22, 24, 24)), (1, (24, 0, 24)), (0, (24, 24, 24))):
        assert switches.nc_unet_deconv_kept_expected(n, *shape) == 0
    assert switches.nc_unet_deconv_kept_expected(1, 24, 24, 24) != 0
