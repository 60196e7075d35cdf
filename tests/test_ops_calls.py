"""CPU: the Python side of every op in neuroclear_amd/ops.py against a stand-in library that records each C call -- name, every scalar
argument as the C side receives it, which pointers are null -- together with workspace sizes and tags, output shapes and which
parameters receive gradients.  tests/golden/ops_calls.json holds that record as taken from ops.py BEFORE the binding read the header and
the whole-network Functions shared their plumbing: the refactor must issue the same calls.  The tensors are CPU tensors and no kernel
runs; this checks call order, argument order and the gradient routing, not arithmetic."""
import ctypes
import json
import os

import torch

from neuroclear_amd import _lib, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ops_calls.json')


def _val(a, ty):
    if ty is ctypes.c_void_p:
        if a is None:
            return 'NULL'
        if isinstance(a, ctypes.c_void_p):
            return 'ptr' if a.value else 'NULL'
        return 'byref' if type(a).__name__ == 'CArgObject' else 'ptr:' + type(a).__name__
    ty.from_param(a)  # raises on a value of another type
    v = a.value if hasattr(a, 'value') else a
    return ty(v).value if ty in (ctypes.c_float, ctypes.c_double) else int(v)


class _Recorder:
    """Stands in for the loaded library: checks every call against the header's prototype, logs it, fills out-parameters with 3."""

    def __init__(self, log, npar):
        self._log, self._npar, self._protos = log, npar, _lib.prototypes()

    def __getattr__(self, name):
        ret, argtypes = self._protos[name]

        def fn(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            self._log.append([name] + [_val(a, t) for a, t in zip(args, argtypes)])
            for a in args:
                if type(a).__name__ == 'CArgObject':
                    a._obj.value = 3
            if name.endswith('_param_floats'):
                return self._npar[0]
            if ret is ctypes.c_size_t:
                return 640
            if name.endswith('_supported') or name.endswith('_active') or name in ('nc_conv_fwd_path', 'nc_conv_wgrad_path', 'nc_conv_route', 'nc_conv_path_name'):
                return 1
            return 0 if ret is ctypes.c_int else None
        fn.__name__ = name
        return fn


def test_every_op_issues_the_recorded_calls(monkeypatch):
    log, npar = [], [0]
    fake = _Recorder(log, npar)
    monkeypatch.setattr(ops, 'lib', lambda: fake)
    monkeypatch.setattr(ops, '_chk', lambda *ts: None)
    monkeypatch.setattr(ops, '_stream', lambda: ctypes.c_void_p(1))
    monkeypatch.setattr(ops, 'workspace', lambda nbytes, device, tag='ws': (
        log.append(['workspace', int(nbytes), tag]), torch.empty(max(int(nbytes), 256), dtype=torch.uint8))[1])
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a, **k: type('S', (), {'cuda_stream': 1})())
    monkeypatch.setattr(torch.Tensor, 'record_stream', lambda self, st: None)
    monkeypatch.setattr(ops, 'conv_precision', 'fp32')
    monkeypatch.setattr(ops, '_lp_cache', {})

    def params(shapes, frozen=()):
        flat = torch.zeros(sum(int(torch.tensor(s).prod()) for s in shapes))
        ps, off = [], 0
        for i, s in enumerate(shapes):
            n = int(torch.tensor(s).prod())
            ps.append(flat[off:off + n].view(s).requires_grad_(i not in frozen))
            off += n
        npar[0] = flat.numel()
        return ps

    def grads_of(ps):
        return [None if p.grad is None else list(p.grad.shape) for p in ps]

    SH = [(4, 1, 3), (4,), (2, 4), (2,)]
    for frozen in ((), (0,), (1, 3), (0, 1, 2, 3)):
        for xg in (True, False):
            if not xg and len(frozen) == 4:
                continue
            log.append(['---- frozen %s xgrad %s' % (frozen, xg)])
            # PatchGAN 2-D and 3-D
            for nd, xs in ((2, (4, 1, 36, 36)), (3, (2, 1, 20, 20, 20))):
                ps = params(SH, frozen)
                x = torch.zeros(xs).requires_grad_(xg)
                y = ops.patchgan(x, ps, 3, 64, nd)
                log.append(['y', list(y.shape)])
                y.sum().backward()
                log.append(['grads', None if x.grad is None else list(x.grad.shape), grads_of(ps)])
            # KernelGAN
            ps = params(SH, frozen)
            x = torch.zeros(4, 1, 12, 12).requires_grad_(xg)
            y = ops.kernelgan(x, ps, 2)
            log.append(['y', list(y.shape)])
            y.sum().backward()
            log.append(['grads', None if x.grad is None else list(x.grad.shape), grads_of(ps)])
            # GP
            ps = params(SH, frozen)
            x = torch.zeros(4, 1, 36, 36).requires_grad_(xg)
            pen, g = ops.patchgan_gp(x, ps, 3, 64, 2, 1.0, 10.0)
            log.append(['y', list(pen.shape), list(g.shape), g.requires_grad])
            pen.backward()
            log.append(['grads', None if x.grad is None else list(x.grad.shape), grads_of(ps)])
            # generators
            for fn in (ops.unet_deconv_train, ops.deep_linear, ops.unet_deconv_lp, ops.deep_linear_lp):
                ps = params(SH, frozen)
                x = torch.zeros(1, 1, 16, 16, 16).requires_grad_(xg)
                y = fn(x, ps)
                log.append(['y', list(y.shape)])
                y.sum().backward()
                log.append(['grads', None if x.grad is None else list(x.grad.shape), grads_of(ps)])
            # Athena pair
            ps = params(SH, (0, 1, 2, 3))
            share = ops.PatchGANShare()
            xf = torch.zeros(4, 1, 36, 36).requires_grad_(True)
            yf = ops.patchgan_fake_half(xf, ps, 3, 64, 2, share)
            log.append(['y', list(yf.shape), list(share.dims), share.cfg])
            yf.sum().backward()
            log.append(['grads', list(xf.grad.shape), grads_of(ps)])
            for i, p in enumerate(ps):
                p.requires_grad_(i not in frozen)
            x = torch.zeros(4, 1, 36, 36).requires_grad_(xg)
            y = ops.patchgan_join_real(x, ps, 3, 64, 2, share)
            log.append(['y', list(y.shape), share.saved is None])
            y.sum().backward()
            log.append(['grads', None if x.grad is None else list(x.grad.shape), grads_of(ps)])

    # no-grad forwards
    with torch.no_grad():
        ps = params(SH)
        log.append(['y', list(ops.deep_linear(torch.zeros(1, 1, 16, 16, 16), ps).shape)])

    # convolutions: fp32 and 16-bit paths
    for prec in ('fp32', 'bf16', 'fp16'):
        ops.set_conv_precision(prec)
        log.append(['---- conv ' + prec])
        for xs, ws_, b in (((1, 16, 8, 8, 8), (64, 16, 3, 3, 3), True), ((2, 1, 12, 12), (8, 1, 4, 4), False)):
            x = torch.zeros(xs).requires_grad_(True)
            w = torch.zeros(ws_).requires_grad_(True)
            bb = torch.zeros(ws_[0]).requires_grad_(True) if b else None
            y = ops.conv(x, w, bb, 1, 1)
            log.append(['y', list(y.shape)])
            y.sum().backward()
            log.append(['grads', list(x.grad.shape), list(w.grad.shape), None if bb is None else list(bb.grad.shape)])
    ops.set_conv_precision('fp32')
    # the other ops once
    x = torch.zeros(1, 2, 8, 8, 8).requires_grad_(True)
    y = ops.instance_norm_act(x, 0.2)
    y = ops.maxpool2(y)
    y = ops.leaky_relu(y, 0.1)
    y = ops.sigmoid(y)
    w = torch.zeros(2, 3, 2, 2, 2).requires_grad_(True)
    y = ops.conv_transpose_k2s2(y, w, torch.zeros(3).requires_grad_(True))
    l = ops.mse_const(y, 1.0) + ops.bce_logits_const(y, 0.0) + ops.mean(y) + ops.l1_loss(y, torch.zeros_like(y))
    l = l + ops.volume_slice(y, 1, 2).sum() + ops.volume_mip(y, 2, 0, 4).sum() + ops.volume_all_slices(y, 0).sum()
    k = torch.zeros(1, 1, 5, 5, 5).requires_grad_(True)
    l = l + ops.linear_kernel(torch.zeros(1, 1, 8, 8, 8).requires_grad_(True), k).sum()
    g, be = torch.zeros(2).requires_grad_(True), torch.zeros(2).requires_grad_(True)
    l = l + ops.batch_norm_act(torch.zeros(1, 2, 8, 8).requires_grad_(True), g, be, torch.zeros(2), torch.ones(2), True).sum()
    l.backward()
    ops.adam_step(torch.zeros(4), torch.zeros(4), torch.zeros(4), torch.zeros(4), 1e-3, 0.5, 0.999, 1e-8, 3)
    ops.set_force_direct(True)
    ops.set_conv_split(True)
    ops.to_c8(torch.zeros(1, 8, 4, 4, 4), 2)
    wsn = ops.spectral_norm_weight(torch.zeros(4, 6).requires_grad_(True), torch.zeros(4), torch.zeros(6), True)
    wsn.sum().backward()
    want = json.load(open(GOLDEN))
    got = json.loads(json.dumps(log))
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
