"""The plan of deep_linear_gen's two whole-network calls (csrc/gen_nets.hip l_fwd_form / l_bwd_forms): the form of each direction is decided
before its first launch, and the `kept` word the forward returns is part of the forward's plan.  nc_deep_linear_kept_expected returns the
plan's word without launching anything; the forward checks conv_fwd_keep's own answers against it.  Here: the word the forward hands to autograd
IS the planned one under every combination of the switches that move a bit, at the shapes of
tests/test_gpu_nets.py::test_deep_linear_collapsed_tail_equals_the_layered_chain; a query changes nothing downstream; and the forms behind the
environment-only switches NC_DL_K32, NC_DL_RANK_WGRAD and NC_DL_RANK_DGRAD (read when the library is loaded: one fresh child process each, the
pattern of tests/test_gpu_unet_fwd_arms.py), which no other test reaches, give the layered chain's output and gradients.

NC_DL_K32=0 and bit 30: the switch takes away "the forward without act1" (csrc/dl_tail.hip), the form of level 1 -- and of level 2 where the
position-typed form refuses.  Where the typed form runs (level 2 at both shapes of the child runs), bit 30 is set with bit 29 by the word's own
contract (include/nc_hip.h: "bit 29 implies both"), whatever the switch.  So the children assert: under NC_DL_K32=0 bit 30 is clear in every
run whose bit 29 is clear, and the level-1 runs are such runs."""
import itertools
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuroclear_amd import ops  # noqa: E402
from neuroclear_amd._lib import lib  # noqa: E402
from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402
from test_gpu_nets import load, rnd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
TOP = 7 << 29
B29, B30, B31 = 1 << 29, 1 << 30, 1 << 31
SHAPES = [(1, 1, 16, 16, 16), (2, 1, 9, 14, 21), (1, 1, 12, 20, 24), (1, 1, 36, 36, 36)]  # (2; 9,14,21): the typed form refuses it


@pytest.fixture
def switches():
    L = lib()
    prev = (L.nc_get_split_terms(), L.nc_get_dl_collapse(), ops.set_conv_split(True))
    yield L
    L.nc_set_split_terms(prev[0])
    L.nc_set_dl_collapse(prev[1])
    ops.set_conv_split(prev[2])


@pytest.fixture(scope='module')
def net():
    return load(networks.define_G(1, 1, 64, 'deep_linear_gen', 'instance', False, 'kaiming', 0.02, [0]), S.deep_linear_spec(), 32)


def _set(L, collapse, terms, split):
    L.nc_set_dl_collapse(collapse)
    L.nc_set_split_terms(terms)
    ops.set_conv_split(split)


def _planned_and_kept(L, net, x):
    """(the query's word just before the forward, the forward's grad_fn.kept)"""
    assert networks._FUSED_GEN
    planned = int(L.nc_deep_linear_kept_expected(x.shape[0], *x.shape[2:]))
    y = net(x)
    return planned, int(y.grad_fn.kept)


@pytest.mark.parametrize('shape', SHAPES)
def test_matrix(shape, switches, net):
    """dl_collapse {0, 1, 2} x split_terms {2, 3} x conv-split {on, off}: planned == kept in every cell; with the split kernels on, bit 29
    follows the rule of test_deep_linear_collapsed_tail_equals_the_layered_chain."""
    x = torch.from_numpy(rnd(41, shape)).to(DEV)
    words = {}
    for collapse, terms, split in itertools.product((0, 1, 2), (2, 3), (True, False)):
        _set(switches, collapse, terms, split)
        planned, kept = _planned_and_kept(switches, net, x)
        print('%s collapse %d terms %d split %d: planned %08x kept %08x' % (shape, collapse, terms, split, planned, kept))
        assert kept == planned, (collapse, terms, split, hex(planned), hex(kept))
        if split:
            assert bool(kept & B29) == (collapse == 2 and terms == 2 and shape != (2, 1, 9, 14, 21)), (collapse, terms, hex(kept))
        words[collapse, terms, split] = kept
    if shape == (1, 1, 16, 16, 16):  # the three levels: layered, a collapsed form, the typed form
        w0, w1, w2 = (words[c, 2, True] for c in (0, 1, 2))
        assert len({w0, w1, w2}) == 3
        assert w0 & TOP == 0 and w1 & B31 and not w1 & B29 and w2 & B29


def test_bad_shape(switches):
    """N or an extent below 1: 0, as the other shape queries answer."""
    for n, shape in ((0, (16, 16, 16)), (1, (0, 16, 16)), (1, (16, 16, -1)), (-1, (16, 16, 16))):
        assert switches.nc_deep_linear_kept_expected(n, *shape) == 0
    _set(switches, 2, 2, True)
    assert switches.nc_deep_linear_kept_expected(1, 16, 16, 16) != 0


def test_moved_switch(switches, net):
    """A query in front of the forward, then split_terms 2 -> 3 before the backward: the gradients of the same run without the query, bit for bit."""
    shape = (1, 1, 16, 16, 16)
    x, r = torch.from_numpy(rnd(41, shape)).to(DEV), torch.from_numpy(rnd(42, shape)).to(DEV)
    _set(switches, 2, 2, True)
    planned = []

    def grads(query):
        for p in net.parameters():
            p.grad = None
        switches.nc_set_split_terms(2)
        if query:
            planned.append(int(switches.nc_deep_linear_kept_expected(1, 16, 16, 16)))
        xi = x.clone().requires_grad_(True)
        y = net(xi)
        kept = int(y.grad_fn.kept)
        switches.nc_set_split_terms(3)
        (y * r).sum().backward()
        return kept, torch.cat([xi.grad.reshape(-1)] + [p.grad.reshape(-1).clone() for p in net.parameters()])
    kept_ref, ref = grads(False)
    kept_got, got = grads(True)
    assert planned[0] != 0 and planned[0] == kept_got == kept_ref
    assert torch.isfinite(got).all()
    assert torch.equal(got, ref)


_CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + '/tests')
from neuroclear_amd._lib import lib
from neuroclear_amd.models import networks
from neuroclear_amd.util import seed as S
from test_gpu_nets import load, rnd, rel2
L = lib()
L.nc_set_split_terms(2)
net = load(networks.define_G(1, 1, 64, 'deep_linear_gen', 'instance', False, 'kaiming', 0.02, [0]), S.deep_linear_spec(), 32)
out = []
for shape in ((1, 1, 16, 16, 16), (1, 1, 12, 20, 24)):
    x0 = torch.from_numpy(rnd(41, shape)).cuda()
    r = torch.from_numpy(rnd(42, shape)).cuda()
    for want_dx in (True, False):
        ref = None
        for mode in (0, 1, 2):
            L.nc_set_dl_collapse(mode)
            for p in net.parameters():
                p.grad = None
            x = x0.clone().requires_grad_(want_dx)
            planned = int(L.nc_deep_linear_kept_expected(shape[0], *shape[2:]))
            y = net(x)
            kept = int(y.grad_fn.kept)
            (y * r).sum().backward()
            res = [y.detach().cpu().numpy()] + ([x.grad.cpu().numpy()] if want_dx else []) + [p.grad.cpu().numpy() for p in net.parameters()]
            if mode == 0:
                ref = res
                continue
            out.append(dict(shape=shape, want_dx=want_dx, mode=mode, planned=planned, kept=kept,
                            y=float(np.abs(res[0] - ref[0]).max() / np.abs(ref[0]).max()),
                            grads=[rel2(a, b) for a, b in zip(res[1:], ref[1:])], finite=bool(all(np.isfinite(a).all() for a in res))))
print('RESULT ' + json.dumps(out))
'''

CONFIGS = [('default', {}), ('k32_off', {'NC_DL_K32': '0'}), ('rank_wgrad_off', {'NC_DL_RANK_WGRAD': '0'}), ('rank_dgrad_off', {'NC_DL_RANK_DGRAD': '0'})]


@pytest.mark.parametrize('name,env', CONFIGS, ids=[c[0] for c in CONFIGS])
def test_environment_forms(name, env):
    """Levels 1 and 2 with two terms at (1; 16^3) and (1; 12,20,24), dx wanted and not: planned == kept, and y, dx and the six parameter gradients
    against the layered chain of the same process within the bounds of test_deep_linear_collapsed_tail_equals_the_layered_chain (1e-5 of the
    largest |y|; relative L2 < 1e-5)."""
    child_env = {k: v for k, v in os.environ.items() if not k.startswith('NC_')}
    child_env.update(env)
    run = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT}], env=child_env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [l for l in run.stdout.splitlines() if l.startswith('RESULT ')]
    assert len(rows) == 1, run.stdout
    runs = json.loads(rows[0][7:])
    assert len(runs) == 8
    for r in runs:
        print(name, r)
        assert r['kept'] == r['planned'], (r['shape'], r['mode'], hex(r['planned']), hex(r['kept']))
        assert r['kept'] & B31
        if r['mode'] == 1:
            assert not r['kept'] & B29
        if name == 'k32_off':
            assert not r['kept'] & B30 or r['kept'] & B29, hex(r['kept'])
        assert r['finite']
        assert r['y'] <= 1e-5, r
        assert len(r['grads']) == 6 + r['want_dx'] and all(g < 1e-5 for g in r['grads']), r
