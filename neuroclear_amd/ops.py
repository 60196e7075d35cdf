"""torch.autograd.Function wrappers over the C ABI (include/nc_hip.h).  PyTorch provides device memory, streams and
the autograd tape only -- every forward/backward below is one or more HIP kernels from libnc_hip.so.

Each op mirrors the torch.nn call the reference makes on its hot path (models/networks.py, apollo_model.py); see the
header for the file:line of every call site."""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import I, P, check, lib

_ws_cache = {}

# Live profiler (bench.py).  Convolution launches are bracketed INSIDE the library (nc_prof_begin / nc_prof_end: HIP
# events on the launch stream around every convolution entry point, also those issued by the whole-network calls);
# `prof` additionally collects (tag, algorithmic FLOP, start, end) around the whole-network C calls themselves.
prof = None


def prof_start(min_flop=0.0):
    global prof
    prof = []
    lib().nc_prof_begin(min_flop)


_PATH = {}   # path number -> tag, read from the library (nc_conv_path_name) the first time a profile is taken


def _path_names():
    if not _PATH:
        buf = ctypes.create_string_buffer(32)
        for path in range(16):
            if lib().nc_conv_path_name(path, buf, len(buf)) > 0:
                _PATH[path] = buf.value.decode()
    return _PATH


def prof_stop():
    """-> ({tag: [launches, ms, flop, algorithmic bytes]} of the convolution launches, [(tag, flop, ms)] of the whole-network calls).  The
    caller has synchronised the device."""
    global prof
    L, names = lib(), _path_names()
    cap = 1 << 16
    cls, flop, ms, ab = (ctypes.c_int * cap)(), (ctypes.c_double * cap)(), (ctypes.c_float * cap)(), (ctypes.c_double * cap)()
    n = min(L.nc_prof_end2(cap, cls, flop, ms, ab), cap)
    stats = {}
    for i in range(n):
        c = cls[i]
        op, path, k, lp = ('fwd', 'dgrad', 'wgrad')[c & 15], (c >> 4) & 15, (c >> 8) & 255, (c >> 16) & 1
        tag = '%s_lp_k%d' % (op, k) if lp else '%s_%s_k%d' % (op, names.get(path, '?'), k)
        s = stats.setdefault(tag, [0, 0.0, 0.0, 0.0])
        s[0] += 1
        s[1] += ms[i]
        s[2] += flop[i]
        s[3] += ab[i]  # algorithmic bytes (operands once + result + weights)
    whole = [(tag, fl, e0.elapsed_time(e1)) for tag, fl, e0, e1 in (prof or [])]
    prof = None
    return stats, whole


def _prof_begin():
    if prof is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _prof_end(e0, tag, flop):
    if e0 is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        prof.append((tag, flop, e0, e1))


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.NcError('neuroclear_amd ops need CUDA(HIP) tensors; there is no CPU fallback')
        if not t.is_contiguous():
            raise _lib.NcError('tensor must be contiguous')


def _f32(*ts):
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise _lib.NcError('expected float32, got %s' % t.dtype)


def _ptr(t):
    return P(t.data_ptr()) if t is not None else P(0)


def workspace(nbytes, device, tag='ws'):
    """Grow-only scratch buffer per (device, tag, current stream): reuse is stream-ordered, and independent networks
    that run concurrently on different streams (the discriminators of the Apollo step) never share scratch."""
    key = (str(device), tag, torch.cuda.current_stream(device).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if not _ws_cache:
            # first allocation of the process: also the moment the library takes its pinned counter block of the range guard (a hipHostMalloc
            # that must not happen on the launch path, where it could land inside a stream capture: csrc/h2.hip)
            lib().nc_set_h2_guard(lib().nc_get_h2_guard())
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _dims5(shape):
    if len(shape) == 5:
        return tuple(shape)
    if len(shape) == 4:
        n, c, h, w = shape
        return n, c, 1, h, w
    raise _lib.NcError('expected NCDHW or NCHW tensor')


def _kdims(wshape):
    if len(wshape) == 5:
        return wshape[2], wshape[3], wshape[4]
    return 1, wshape[2], wshape[3]


def _conv_out_shape(xs, ws, stride, pad):
    nsp = len(xs) - 2
    return (xs[0], ws[0]) + tuple((xs[2 + i] + 2 * pad - ws[2 + i]) // stride + 1 for i in range(nsp))


# Backward runs the weight gradient of a layer on a side stream, concurrently with the data gradient of the same layer
# (they are independent given dy): the two kernels' workgroups interleave on the 256 CUs, which fills the idle tail
# each of them leaves when its tile count is not a multiple of the CU count (e.g. 1296 tiles = 5.06 rounds at 108^3).
# NC_WGRAD_STREAM=1: weight gradients of the big layers on a side stream behind the data gradient.  Off by default:
# once both kernels fill the chip by themselves (round-1 end state) running them side by side is 0.3 % slower.
overlap_wgrad = os.environ.get('NC_WGRAD_STREAM', '0') != '0'
_side_streams = {}


def _side_stream(device):
    st = _side_streams.get(device)
    if st is None:
        st = _side_streams[device] = torch.cuda.Stream(device=device)
    return st


# Arithmetic of the convolutions (BASELINE.json configs[3]): 'fp32' (default, the reference's arithmetic) or 'bf16' /
# 'fp16' = operands rounded to 16 bits, fp32 accumulation, on the layers nc_conv_lp_supported covers (3^3 / 5^3, stride
# 1, >= 16 input and >= 64 output channels); every other layer and everything between the convolutions stays fp32.
_DT = {'fp32': 0, 'fp16': 1, 'bf16': 2}
conv_precision = 'fp32'


def set_conv_split(on):
    """fp32 3^3 / 5^3 convolutions as six bf16 MFMA products of an exact three-term operand split (csrc/conv_split.hip; the
    library default) or, with on=False, on the fp32 MFMA kernels.  Returns the previous setting."""
    prev = bool(lib().nc_get_conv_split())
    lib().nc_set_conv_split(1 if on else 0)
    return prev


def set_conv_precision(name):
    global conv_precision
    if name not in _DT:
        raise _lib.NcError('conv precision must be one of %s, got %r' % (sorted(_DT), name))
    conv_precision = name


_lp_cache = {}


def _lp(what, dims, K, k3, stride, pad):
    """dtype code of the 16-bit kernel for this call, or 0 when the fp32 kernels serve it."""
    if conv_precision == 'fp32':
        return 0
    key = (what, dims, K, k3, stride, pad)
    ok = _lp_cache.get(key)
    if ok is None:
        ok = _lp_cache[key] = bool(lib().nc_conv_lp_supported(what, *dims, K, *k3, stride, pad))
    if not ok:
        return 0
    # 'fp16': forward operands in fp16 (11-bit significand); backward operands (dy, and w / x next to it) in bf16 --
    # gradients of a mean loss over 1e6..1e7 voxels sit below fp16's normal range (6e-5) and there is no loss scaling
    # in the reference's step to lean on; bf16 has fp32's exponent range (measured: tools/lp_err.py).
    if conv_precision == 'fp16' and what != 0:
        return _DT['bf16']
    return _DT[conv_precision]


def to_c8(x, dt):
    """fp32 NCDHW -> the 16-bit C8 operand layout of the *_lp kernels (include/nc_hip.h); returns a byte tensor."""
    _chk(x)
    _f32(x)
    N, C = x.shape[0], x.shape[1]
    S = x.numel() // (N * C)
    out = torch.empty(N * C * S * 2, dtype=torch.uint8, device=x.device)
    e0 = _prof_begin()
    check(lib().nc_to_c8(_ptr(x), _ptr(out), N, C, S, dt, _stream()), 'nc_to_c8')
    _prof_end(e0, 'to_c8', 0.0)
    return out


def _conv_launch(op, dt, tensors, dims, K, k3, stride, pad, device, ws_tag='ws'):
    """One convolution launch: nc_conv_<op> on the fp32 kernels, or nc_conv_<op>_lp with the 16-bit dtype code dt (_lp), on the
    workspace of that path.  The profiler brackets the launch inside the library (nc_prof_begin), not here."""
    name = 'nc_conv_' + op + ('_lp' if dt else '')
    ws_bytes = lib().nc_conv_lp_ws_bytes if dt else lib().nc_conv_ws_bytes
    ws = workspace(ws_bytes(*dims, K, *k3, stride, pad), device, ws_tag + '_lp' if dt else ws_tag)
    check(getattr(lib(), name)(*map(_ptr, tensors), *dims, K, *k3, stride, pad, *((dt,) if dt else ()), _ptr(ws), ws.numel(),
                               _stream()), name)


def conv_fwd_raw(x, w, b, stride, pad, xh=None):
    """xh: x already in the C8 layout (to_c8) for the 16-bit kernel of this call -- saves the conversion."""
    _chk(x, w, b)
    _f32(x, w, b)
    dims = _dims5(x.shape)
    k3 = _kdims(w.shape)
    K = w.shape[0]
    if w.shape[1] != dims[1]:
        raise _lib.NcError('conv: weight expects %d input channels, got %d' % (w.shape[1], dims[1]))
    y = torch.empty(_conv_out_shape(x.shape, w.shape, stride, pad), dtype=torch.float32, device=x.device)
    dt = _lp(0, dims, K, k3, stride, pad)
    _conv_launch('fwd', dt, (x, xh, w, b, y) if dt else (x, w, b, y), dims, K, k3, stride, pad, x.device)
    return y


def conv_dgrad_raw(dy, w, x_shape, stride, pad, dyh=None):
    _chk(dy, w)
    _f32(dy, w)
    dx = torch.empty(tuple(x_shape), dtype=torch.float32, device=dy.device)
    dims = _dims5(x_shape)
    k3 = _kdims(w.shape)
    K = w.shape[0]
    dt = _lp(1, dims, K, k3, stride, pad)
    _conv_launch('dgrad', dt, (dy, dyh, w, dx) if dt else (dy, w, dx), dims, K, k3, stride, pad, dy.device)
    return dx


def conv_wgrad_raw(x, dy, w_shape, stride, pad, want_bias, ws_tag='ws', xh=None, dyh=None, x_shape=None):
    """x may be None when xh (its C8 copy) and x_shape are given: the 16-bit weight gradient never reads the fp32 x."""
    _chk(x, dy)
    _f32(x, dy)
    dims = _dims5(x.shape if x is not None else x_shape)
    K = w_shape[0]
    k3 = _kdims(w_shape)
    dw = torch.empty(tuple(w_shape), dtype=torch.float32, device=dy.device)
    db = torch.empty(K, dtype=torch.float32, device=dy.device) if want_bias else None
    dt = _lp(2, dims, K, k3, stride, pad)
    if x is None and not dt:
        raise _lib.NcError('conv_wgrad: the fp32 x is needed for the fp32 kernels')
    _conv_launch('wgrad', dt, (x, xh, dy, dyh, dw, db) if dt else (x, dy, dw, db), dims, K, k3, stride, pad, dy.device, ws_tag)
    return dw, db


class BiasLink:
    """Shared by a convolution and the InstanceNorm+activation right behind it (networks.py:420-423) for one forward pass.
    The gradient at the convolution's output is the dx of the norm's backward, so the convolution's bias gradient -- the
    per-channel sum of that dx -- is taken inside the norm's backward kernel while dx is in registers
    (nc_instnorm_act_bwd_dbias) and handed over here; the convolution's backward then skips its own pass over dy.
    The same object also carries the 16-bit operand copies between the two (conv_h.hip's C8 layout), in both directions:
    * forward, norm -> NEXT convolution: `want_xh` (dtype code, set by the caller that knows the next layer) makes the
      norm's forward emit its result in C8 as well (`xh`), and that convolution skips its own conversion pass;
    * backward, norm -> the convolution in FRONT of it: `want_dyh` (set by that convolution's forward) makes the norm's
      backward emit dx in C8 (`dyh`) for the data / weight gradient kernels."""
    __slots__ = ('want', 'dbias', 'want_xh', 'xh', 'xh_dt', 'want_dyh', 'dyh', 'dyh_dt')

    def __init__(self):
        self.want = False
        self.dbias = None
        self.want_xh = 0
        self.xh = None
        self.xh_dt = 0
        self.want_dyh = 0
        self.dyh = None
        self.dyh_dt = 0


def lp_fwd_dtype(x_shape, w_shape, stride, pad):
    """dtype code of the 16-bit forward kernel a convolution with this weight would use on an input of x_shape, or 0."""
    if len(x_shape) != len(w_shape) or x_shape[1] != w_shape[1]:
        return 0
    return _lp(0, _dims5(x_shape), w_shape[0], _kdims(w_shape), int(stride), int(pad))


class _Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pad, link=None, prev=None, dead_bias=False):
        x = x.contiguous()
        bf = None if dead_bias else b   # a dead bias (conv()) stays a parameter with a gradient; only the add is skipped
        ctx.link = link
        if link is not None:
            link.want = b is not None and ctx.needs_input_grad[2]
        ctx.cfg = (stride, pad, b is not None)
        ctx.x_shape = tuple(x.shape)
        dims, K, k3 = _dims5(x.shape), w.shape[0], _kdims(w.shape)
        dt = _lp(0, dims, K, k3, stride, pad) if w.shape[1] == x.shape[1] else 0
        if dt:
            # 16-bit path: x is converted ONCE; if the weight gradient runs in the same type it reuses that copy, and the
            # copy (half the bytes) is what is kept for backward instead of the fp32 activation
            if prev is not None and prev.xh is not None and prev.xh_dt == dt:
                xh, prev.xh = prev.xh, None  # emitted by the norm in front of this layer
            else:
                xh = to_c8(x, dt)
            y = conv_fwd_raw(x, w, bf, stride, pad, xh=xh)
            keep = _lp(2, dims, K, k3, stride, pad) == dt
            if link is not None:  # backward operands: ask the norm behind this layer for dy in C8
                dd = _lp(1, dims, K, k3, stride, pad) if ctx.needs_input_grad[0] else 0
                dw_ = _lp(2, dims, K, k3, stride, pad) if (ctx.needs_input_grad[1] or link.want) else 0
                if (dd or dw_) and (not dd or not dw_ or dd == dw_):
                    link.want_dyh = dd or dw_
            ctx.x_is_c8 = keep
            ctx.save_for_backward(xh if keep else x, w)
            return y
        ctx.x_is_c8 = False
        ctx.save_for_backward(x, w)
        return conv_fwd_raw(x, w, bf, stride, pad)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, pad, has_b = ctx.cfg
        dy = dy.contiguous()
        dx = dw = db = None
        want_b = has_b and ctx.needs_input_grad[2]
        want_w = ctx.needs_input_grad[1] or want_b
        db_link = None
        if want_b and ctx.link is not None and ctx.link.dbias is not None:
            db_link, ctx.link.dbias = ctx.link.dbias, None  # taken by the norm's backward: no pass over dy for it here
            want_b = False
            want_w = ctx.needs_input_grad[1]
        dims, K, k3 = _dims5(ctx.x_shape), w.shape[0], _kdims(w.shape)
        dt_d = _lp(1, dims, K, k3, stride, pad) if ctx.needs_input_grad[0] else 0
        dt_w = _lp(2, dims, K, k3, stride, pad) if want_w else 0
        if dt_d or dt_w:  # 16-bit backward: dy is converted once for the data and the weight gradient
            lk = ctx.link
            if lk is not None and lk.dyh is not None and lk.dyh_dt == (dt_d or dt_w):
                dyh, lk.dyh = lk.dyh, None  # emitted by the backward of the norm behind this layer
            else:
                dyh = to_c8(dy, dt_d or dt_w)
            if ctx.needs_input_grad[0]:
                dx = conv_dgrad_raw(dy, w, ctx.x_shape, stride, pad, dyh=dyh if dt_d else None)
            if want_w:
                same = dt_w and (not dt_d or dt_d == dt_w)
                if ctx.x_is_c8:
                    dw, db = conv_wgrad_raw(None, dy, w.shape, stride, pad, want_b, xh=x, dyh=dyh if same else None,
                                            x_shape=ctx.x_shape)
                else:
                    dw, db = conv_wgrad_raw(x, dy, w.shape, stride, pad, want_b, dyh=dyh if same else None)
            return dx, dw, db if db_link is None else db_link, None, None, None, None, None
        big = x.numel() >= (1 << 20)  # small layers gain nothing from a second stream
        if want_w and ctx.needs_input_grad[0] and overlap_wgrad and big and prof is None:
            main = torch.cuda.current_stream()
            side = _side_stream(x.device)
            side.wait_stream(main)  # dy (and x) were produced on the main stream
            with torch.cuda.stream(side):
                dw, db = conv_wgrad_raw(x, dy, w.shape, stride, pad, want_b, 'ws_side')
            dy.record_stream(side)
            x.record_stream(side)
            dx = conv_dgrad_raw(dy, w, x.shape, stride, pad)
            main.wait_stream(side)  # dw / db are consumed (accumulated into .grad) on the main stream
            return dx, dw, db if db_link is None else db_link, None, None, None, None, None
        if ctx.needs_input_grad[0]:
            dx = conv_dgrad_raw(dy, w, x.shape, stride, pad)
        if want_w:
            dw, db = conv_wgrad_raw(x, dy, w.shape, stride, pad, want_b)
        return dx, dw, db if db_link is None else db_link, None, None, None, None, None


def conv(x, w, b=None, stride=1, padding=0, link=None, prev=None, dead_bias=False):
    """nn.Conv3d / nn.Conv2d (models/networks.py:361-369).  link / prev: BiasLink shared with the InstanceNorm behind /
    in front of this layer.  dead_bias: an InstanceNorm(affine=False) follows, so b cannot reach the output -- the add is skipped, the
    parameter keeps its (mathematically zero) gradient, taken as for every other bias (ResnetGenerator's 7 x 7 and stride-2 layers)."""
    return _Conv.apply(x, w, b, int(stride), int(padding), link, prev, bool(dead_bias))


def _lk_ok(x, w):
    """nc_lk_* cover this call: a dense fp32 CUDA x [N, 1, D, H, W] and w [1, 1, k, k, k] with odd k in 3 .. 31."""
    return (x.is_cuda and w.is_cuda and x.dim() == 5 and x.shape[1] == 1 and x.dtype == torch.float32 and w.dtype == torch.float32
            and tuple(w.shape[:2]) == (1, 1) and w.dim() == 5 and w.shape[2] == w.shape[3] == w.shape[4]
            and w.shape[2] % 2 == 1 and 3 <= w.shape[2] <= 31)


def _lk_call(fn, a, b, out, k, ws, what):
    N, _, D, H, W = out.shape
    check(fn(_ptr(a), _ptr(b), _ptr(out), N, D, H, W, k, _ptr(ws), (0 if ws is None else ws.numel()), _stream()), what)
    return out


class _LinearKernel(torch.autograd.Function):
    """Conv3d(1, 1, k, padding (k - 1) / 2, bias=False) of LinearKernel / LinearKernel_double (models/networks.py:840-871) on
    nc_lk_fwd / nc_lk_dgrad / nc_lk_wgrad.  The weight gradient goes back through autograd (never into FlatAdam's flat buffer:
    the _double form uses its weight twice and autograd adds the two contributions)."""

    @staticmethod
    def forward(ctx, x, w):
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(x, w)
        return _lk_call(lib().nc_lk_fwd, x, w, torch.empty_like(x), w.shape[2], None, 'nc_lk_fwd')

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        k = w.shape[2]
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = _lk_call(lib().nc_lk_dgrad, dy, w, torch.empty_like(dy), k, None, 'nc_lk_dgrad')
        if ctx.needs_input_grad[1]:
            N, _, D, H, W = x.shape
            ws = workspace(lib().nc_lk_ws_bytes(N, D, H, W, k), x.device, 'ws_lk')
            dw = torch.empty_like(w)
            check(lib().nc_lk_wgrad(_ptr(x), _ptr(dy), _ptr(dw), N, D, H, W, k, _ptr(ws), ws.numel(), _stream()),
                  'nc_lk_wgrad')
        return dx, dw


def linear_kernel(x, w):
    """The learned PSF: one bias-free Conv3d(1, 1, k, stride 1, padding (k - 1) // 2) (networks.py:840-854).  Always fp32, whatever
    set_conv_precision says.  Another kernel size, or a CPU tensor, goes to ops.conv (which has no CPU path either: it raises)."""
    if _lk_ok(x, w):
        return _LinearKernel.apply(x, w)
    return conv(x, w, None, 1, (w.shape[-1] - 1) // 2)


class _ConvT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        x = x.contiguous()
        _chk(x, w, b)
        _f32(x, w, b)
        if x.dim() != 5 or tuple(w.shape[2:]) != (2, 2, 2):
            raise _lib.NcError('convT_k2s2: only ConvTranspose3d(kernel 2, stride 2) is on the hot path')
        N, C, D, H, W = x.shape
        K = w.shape[1]
        y = torch.empty((N, K, 2 * D, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
        if lib().nc_convT_k2s2_split_active(1, C, D, H, W, K):
            # the split-operand kernel of csrc/convt_s3.hip, sample by sample: exactly what the whole-network calls do
            ws = workspace(lib().nc_convT_k2s2_split_ws_bytes(1, C, D, H, W, K), x.device, 'ws_convT_split')
            for n in range(N):
                check(lib().nc_convT_k2s2_fwd_split(_ptr(x[n]), None, _ptr(w), _ptr(b), _ptr(y[n]), None, 0, 0, 1, C, D, H, W,
                                                    K, _ptr(ws), ws.numel(), _stream()), 'nc_convT_k2s2_fwd_split')
        else:
            check(lib().nc_convT_k2s2_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(y), N, C, D, H, W, K,
                                          _stream()), 'nc_convT_k2s2_fwd')
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        N, C, D, H, W = x.shape
        K = w.shape[1]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            nb = lib().nc_convT_ws_bytes(N, C, D, H, W, K)
            ws = workspace(nb, x.device, 'ws_convT')
            check(lib().nc_convT_k2s2_dgrad(_ptr(dy), _ptr(w), _ptr(dx), N, C, D, H, W, K, _ptr(ws),
                                            ws.numel(), _stream()), 'nc_convT_k2s2_dgrad')
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)
            db = torch.empty(K, dtype=torch.float32, device=x.device) if ctx.has_b else None
            ws = workspace(lib().nc_convT_ws_bytes(N, C, D, H, W, K), x.device)
            check(lib().nc_convT_k2s2_wgrad(_ptr(x), _ptr(dy), _ptr(dw), _ptr(db), N, C, D, H, W, K,
                                            _ptr(ws), ws.numel(), _stream()), 'nc_convT_k2s2_wgrad')
        return dx, dw, db


class _ConvT2d(torch.autograd.Function):
    """nn.ConvTranspose2d(C, K, 2, 2) on nc_convT2d_k2s2_*: fp32 under every conv precision."""

    @staticmethod
    def forward(ctx, x, w, b):
        x = x.contiguous()
        _chk(x, w, b)
        _f32(x, w, b)
        if x.dim() != 4 or w.dim() != 4 or tuple(w.shape[2:]) != (2, 2) or w.shape[0] != x.shape[1]:
            raise _lib.NcError('convT2d_k2s2: only ConvTranspose2d(kernel 2, stride 2) with x [N,C,H,W] and w [C,K,2,2] is on the hot path')
        N, C, H, W = x.shape
        K = w.shape[1]
        y = torch.empty((N, K, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
        check(lib().nc_convT2d_k2s2_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(y), N, C, H, W, K, _stream()), 'nc_convT2d_k2s2_fwd')
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        N, C, H, W = x.shape
        K = w.shape[1]
        dx = dw = db = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            ws = workspace(lib().nc_convT2d_ws_bytes(N, C, H, W, K), x.device, 'ws_convT')
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            check(lib().nc_convT2d_k2s2_dgrad(_ptr(dy), _ptr(w), _ptr(dx), N, C, H, W, K, _ptr(ws), ws.numel(), _stream()),
                  'nc_convT2d_k2s2_dgrad')
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            dw = torch.empty_like(w)
            db = torch.empty(K, dtype=torch.float32, device=x.device) if ctx.has_b else None
            check(lib().nc_convT2d_k2s2_wgrad(_ptr(x), _ptr(dy), _ptr(dw), _ptr(db), N, C, H, W, K, _ptr(ws), ws.numel(), _stream()),
                  'nc_convT2d_k2s2_wgrad')
        return dx, dw, db


def conv_transpose_k2s2(x, w, b=None):
    """nn.ConvTranspose3d(C, K, 2, 2) / nn.ConvTranspose2d(C, K, 2, 2) (models/networks.py:382-390, 500, 503): a 5-D input takes the 3-D
    kernels, a 4-D input the 2-D ones (csrc/convt2d.hip)."""
    if x.dim() == 4:
        return _ConvT2d.apply(x, w, b)
    return _ConvT.apply(x, w, b)


def instnorm_stats(x, eps=1e-5):
    _chk(x)
    _f32(x)
    NC = x.shape[0] * x.shape[1]
    S = x.numel() // NC
    mean = torch.empty(NC, dtype=torch.float32, device=x.device)
    rstd = torch.empty(NC, dtype=torch.float32, device=x.device)
    ws = workspace(lib().nc_instnorm_ws_bytes(NC, S), x.device, 'in')
    check(lib().nc_instnorm_stats(_ptr(x), NC, S, eps, _ptr(mean), _ptr(rstd), _ptr(ws), ws.numel(),
                                  _stream()), 'nc_instnorm_stats')
    return mean, rstd


class _InstNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slope, eps, link=None, nxt=None):
        x = x.contiguous()
        ctx.link = link
        y = torch.empty_like(x)
        if nxt is not None and nxt.want_xh and x.shape[1] % 8 == 0:
            mean, rstd = instnorm_stats(x, eps)
            NC = mean.numel()
            S = x.numel() // NC
            yh = torch.empty(x.numel() * 2, dtype=torch.uint8, device=x.device)
            check(lib().nc_instnorm_act_fwd_c8(_ptr(x), _ptr(mean), _ptr(rstd), slope, _ptr(y), _ptr(yh), x.shape[0],
                                               x.shape[1], S, nxt.want_xh, _stream()), 'nc_instnorm_act_fwd_c8')
            nxt.xh, nxt.xh_dt = yh, nxt.want_xh
        else:
            _chk(x)
            _f32(x)
            NC = x.shape[0] * x.shape[1]
            S = x.numel() // NC
            mean = torch.empty(NC, dtype=torch.float32, device=x.device)
            rstd = torch.empty(NC, dtype=torch.float32, device=x.device)
            ws = workspace(lib().nc_instnorm_ws_bytes(NC, S), x.device, 'in')
            check(lib().nc_instnorm_fwd(_ptr(x), eps, slope, _ptr(mean), _ptr(rstd), _ptr(y), NC, S, _ptr(ws),
                                        ws.numel(), _stream()), 'nc_instnorm_fwd')
        ctx.save_for_backward(x, mean, rstd)
        ctx.slope = slope
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        NC = mean.numel()
        S = x.numel() // NC
        dx = torch.empty_like(x)
        link = ctx.link
        if link is not None and link.want_dyh and x.shape[1] % 8 == 0:
            N, C = x.shape[0], x.shape[1]
            db = torch.empty(C, dtype=torch.float32, device=x.device) if link.want else None
            dxh = torch.empty(x.numel() * 2, dtype=torch.uint8, device=x.device)
            ws = workspace(lib().nc_instnorm_bwd_dbias_ws_bytes(NC, S), x.device, 'in')
            check(lib().nc_instnorm_act_bwd_c8(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), ctx.slope, _ptr(dx), _ptr(dxh),
                                               _ptr(db), N, C, S, link.want_dyh, _ptr(ws), ws.numel(),
                                               _stream()), 'nc_instnorm_act_bwd_c8')
            link.dyh, link.dyh_dt, link.dbias = dxh, link.want_dyh, db
            return dx, None, None, None, None
        if link is not None and link.want:
            N, C = x.shape[0], x.shape[1]
            db = torch.empty(C, dtype=torch.float32, device=x.device)
            ws = workspace(lib().nc_instnorm_bwd_dbias_ws_bytes(NC, S), x.device, 'in')
            check(lib().nc_instnorm_act_bwd_dbias(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), ctx.slope, _ptr(dx), _ptr(db),
                                                  N, C, S, _ptr(ws), ws.numel(), _stream()),
                  'nc_instnorm_act_bwd_dbias')
            link.dbias = db
            return dx, None, None, None, None
        ws = workspace(lib().nc_instnorm_ws_bytes(NC, S), x.device, 'in')
        check(lib().nc_instnorm_act_bwd(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), ctx.slope, _ptr(dx), NC,
                                        S, _ptr(ws), ws.numel(), _stream()), 'nc_instnorm_act_bwd')
        return dx, None, None, None, None


def instance_norm_act(x, slope=0.0, eps=1e-5, link=None, nxt=None):
    """InstanceNorm{2,3}d(affine=False) followed by ReLU (slope 0) / LeakyReLU(slope) -- networks.py:33-34,422-423.
    link / nxt: BiasLink shared with the convolution in front of / behind this layer."""
    return _InstNormAct.apply(x, float(slope), float(eps), link, nxt)


class _BatchNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, slope):
        x = x.contiguous()
        _chk(x, gamma, beta)
        _f32(x, gamma, beta)
        N, C = x.shape[0], x.shape[1]
        S = x.numel() // (N * C)
        L = lib()
        mean = torch.empty(C, dtype=torch.float32, device=x.device)
        rstd = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = workspace(L.nc_instnorm_ws_bytes(N * C, S), x.device, 'bn')
        check(L.nc_batchnorm_stats(_ptr(x), N, C, S, eps, momentum, 1 if training else 0, _ptr(mean), _ptr(rstd),
                                   _ptr(running_mean), _ptr(running_var), _ptr(ws), ws.numel(), _stream()), 'nc_batchnorm_stats')
        y = torch.empty_like(x)
        check(L.nc_batchnorm_act_fwd(_ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), slope, _ptr(y), N, C, S, _stream()),
              'nc_batchnorm_act_fwd')
        ctx.save_for_backward(x, mean, rstd, gamma, beta)
        ctx.cfg = (bool(training), float(slope))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, gamma, beta = ctx.saved_tensors
        training, slope = ctx.cfg
        dy = dy.contiguous()
        N, C = x.shape[0], x.shape[1]
        S = x.numel() // (N * C)
        L = lib()
        dx = torch.empty_like(x)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        coef = torch.empty(2 * C, dtype=torch.float32, device=x.device)
        ws = workspace(L.nc_instnorm_ws_bytes(N * C, S), x.device, 'bn')
        check(L.nc_batchnorm_act_bwd(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), slope, 1 if training else 0,
                                     _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(coef), N, C, S, _ptr(ws), ws.numel(), _stream()),
              'nc_batchnorm_act_bwd')
        return dx, dgamma, dbeta, None, None, None, None, None, None


def batch_norm_act(x, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5, slope=0.0):
    """nn.BatchNorm{2,3}d(affine=True, track_running_stats=True) (models/networks.py:30-31, --norm batch) followed by ReLU (slope 0) /
    LeakyReLU(slope); running_mean / running_var are updated in place in training mode and used in evaluation mode."""
    return _BatchNormAct.apply(x, gamma, beta, running_mean, running_var, bool(training), float(momentum), float(eps), float(slope))


class _LeakyReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slope):
        x = x.contiguous()
        _chk(x)
        _f32(x)
        y = torch.empty_like(x)
        check(lib().nc_leaky_relu_fwd(_ptr(x), slope, _ptr(y), x.numel(), _stream()), 'nc_leaky_relu_fwd')
        ctx.save_for_backward(x)
        ctx.slope = slope
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        check(lib().nc_leaky_relu_bwd(_ptr(dy), _ptr(x), ctx.slope, _ptr(dx), x.numel(), _stream()),
              'nc_leaky_relu_bwd')
        return dx, None


def leaky_relu(x, slope):
    return _LeakyReLU.apply(x, float(slope))


class _Sigmoid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        _chk(x)
        _f32(x)
        y = torch.empty_like(x)
        check(lib().nc_sigmoid_fwd(_ptr(x), _ptr(y), x.numel(), _stream()), 'nc_sigmoid_fwd')
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(y)
        check(lib().nc_sigmoid_bwd(_ptr(dy), _ptr(y), _ptr(dx), y.numel(), _stream()), 'nc_sigmoid_bwd')
        return dx


def sigmoid(x):
    return _Sigmoid.apply(x)


class _MaxPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        _chk(x)
        _f32(x)
        N, C, D, H, W = _dims5(x.shape)
        wd = 2 if D > 1 else 1
        oshape = (N, C, D // wd, H // 2, W // 2) if x.dim() == 5 else (N, C, H // 2, W // 2)
        y = torch.empty(oshape, dtype=torch.float32, device=x.device)
        check(lib().nc_maxpool2_fwd(_ptr(x), _ptr(y), N * C, D, H, W, _stream()), 'nc_maxpool2_fwd')
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        N, C, D, H, W = _dims5(x.shape)
        dx = torch.empty_like(x)
        check(lib().nc_maxpool2_bwd(_ptr(dy), _ptr(x), _ptr(dx), N * C, D, H, W, _stream()),
              'nc_maxpool2_bwd')
        return dx


def maxpool2(x):
    """nn.MaxPool3d(2) (models/networks.py:491,494)."""
    return _MaxPool2.apply(x)


_PLANE = [lambda N, C, D, H, W: (N, C, H, W), lambda N, C, D, H, W: (N, C, D, W), lambda N, C, D, H, W: (N, C, D, H)]


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vol, axis, index):
        vol = vol.contiguous()
        _chk(vol)
        _f32(vol)
        N, C, D, H, W = vol.shape
        out = torch.empty(_PLANE[axis](N, C, D, H, W), dtype=torch.float32, device=vol.device)
        check(lib().nc_slice_fwd(_ptr(vol), _ptr(out), N * C, D, H, W, axis, index, _stream()),
              'nc_slice_fwd')
        ctx.cfg = (tuple(vol.shape), axis, index)
        return out

    @staticmethod
    def backward(ctx, dout):
        shape, axis, index = ctx.cfg
        dout = dout.contiguous()
        N, C, D, H, W = shape
        dvol = torch.empty(shape, dtype=torch.float32, device=dout.device)
        check(lib().nc_slice_bwd(_ptr(dout), _ptr(dvol), N * C, D, H, W, axis, index, _stream()),
              'nc_slice_bwd')
        return dvol, None, None


def volume_slice(vol, axis, index):
    """Volume.get_slice (apollo_model.py:328-337)."""
    return _Slice.apply(vol, int(axis), int(index))


class _Mip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vol, axis, start, depth):
        vol = vol.contiguous()
        _chk(vol)
        _f32(vol)
        N, C, D, H, W = vol.shape
        oshape = _PLANE[axis](N, C, D, H, W)
        out = torch.empty(oshape, dtype=torch.float32, device=vol.device)
        arg = torch.empty(oshape, dtype=torch.int32, device=vol.device)
        check(lib().nc_mip_fwd(_ptr(vol), _ptr(out), _ptr(arg), N * C, D, H, W, axis, start,
                               depth, _stream()), 'nc_mip_fwd')
        ctx.save_for_backward(arg)
        ctx.cfg = (tuple(vol.shape), axis)
        return out

    @staticmethod
    def backward(ctx, dout):
        (arg,) = ctx.saved_tensors
        shape, axis = ctx.cfg
        dout = dout.contiguous()
        N, C, D, H, W = shape
        dvol = torch.empty(shape, dtype=torch.float32, device=dout.device)
        check(lib().nc_mip_bwd(_ptr(dout), _ptr(arg), _ptr(dvol), N * C, D, H, W, axis, _stream()),
              'nc_mip_bwd')
        return dvol, None, None, None


def volume_mip(vol, axis, start, depth):
    """Volume.get_projection (apollo_model.py:339-351)."""
    return _Mip.apply(vol, int(axis), int(start), int(depth))


class _AllSlices(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vol, axis):
        vol = vol.contiguous()
        _chk(vol)
        _f32(vol)
        N, C, D, H, W = vol.shape
        L = (D, H, W)[axis]
        pn, pc, pa, pb = _PLANE[axis](N, C, D, H, W)
        out = torch.empty((N * L, C, pa, pb), dtype=torch.float32, device=vol.device)
        check(lib().nc_volume_slices(_ptr(vol), _ptr(out), N, C, D, H, W, axis, 0, _stream()),
              'nc_volume_slices')
        ctx.cfg = (tuple(vol.shape), axis)
        return out

    @staticmethod
    def backward(ctx, dout):
        shape, axis = ctx.cfg
        dout = dout.contiguous()
        N, C, D, H, W = shape
        dvol = torch.empty(shape, dtype=torch.float32, device=dout.device)
        check(lib().nc_volume_slices(_ptr(dout), _ptr(dvol), N, C, D, H, W, axis, 1, _stream()),
              'nc_volume_slices')
        return dvol, None


def volume_all_slices(vol, axis):
    """Every slice along `axis` as a batch [(n, s), C, A, B] -- the batched form of Athena's iter_f loop
    (axial_to_lateral_gan_athena_model.py:286-296)."""
    return _AllSlices.apply(vol, int(axis))


class _MseConst(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        pred = pred.contiguous()
        _chk(pred)
        _f32(pred)
        out = torch.empty((), dtype=torch.float32, device=pred.device)
        ws = workspace(lib().nc_loss_ws_bytes(pred.numel()), pred.device, 'loss')
        check(lib().nc_mse_const_fwd(_ptr(pred), pred.numel(), target, _ptr(out), _ptr(ws), ws.numel(),
                                     _stream()), 'nc_mse_const_fwd')
        ctx.save_for_backward(pred)
        ctx.target = target
        return out

    @staticmethod
    def backward(ctx, g):
        (pred,) = ctx.saved_tensors
        g = g.contiguous()
        dp = torch.empty_like(pred)
        check(lib().nc_mse_const_bwd(_ptr(pred), pred.numel(), ctx.target, _ptr(g), _ptr(dp), _stream()),
              'nc_mse_const_bwd')
        return dp, None


def mse_const(pred, target):
    """GANLoss('lsgan') (models/networks.py:276,299-313): mean((pred - target)^2), target a constant."""
    return _MseConst.apply(pred, float(target))


class _BceLogitsConst(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        pred = pred.contiguous()
        _chk(pred)
        _f32(pred)
        out = torch.empty((), dtype=torch.float32, device=pred.device)
        ws = workspace(lib().nc_loss_ws_bytes(pred.numel()), pred.device, 'loss')
        check(lib().nc_bce_logits_const_fwd(_ptr(pred), pred.numel(), target, _ptr(out), _ptr(ws), ws.numel(), _stream()),
              'nc_bce_logits_const_fwd')
        ctx.save_for_backward(pred)
        ctx.target = target
        return out

    @staticmethod
    def backward(ctx, g):
        (pred,) = ctx.saved_tensors
        g = g.contiguous()
        dp = torch.empty_like(pred)
        check(lib().nc_bce_logits_const_bwd(_ptr(pred), pred.numel(), ctx.target, _ptr(g), _ptr(dp), _stream()),
              'nc_bce_logits_const_bwd')
        return dp, None


def bce_logits_const(pred, target):
    """GANLoss('vanilla') (models/networks.py:278, 308-313): nn.BCEWithLogitsLoss of the logits against a constant label."""
    return _BceLogitsConst.apply(pred, float(target))


class _Mean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred):
        pred = pred.contiguous()
        _chk(pred)
        _f32(pred)
        out = torch.empty((), dtype=torch.float32, device=pred.device)
        ws = workspace(lib().nc_loss_ws_bytes(pred.numel()), pred.device, 'loss')
        check(lib().nc_mean_fwd(_ptr(pred), pred.numel(), _ptr(out), _ptr(ws), ws.numel(), _stream()), 'nc_mean_fwd')
        ctx.shape = pred.shape
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        dp = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        check(lib().nc_mean_bwd(dp.numel(), _ptr(g), _ptr(dp), _stream()), 'nc_mean_bwd')
        return dp


def mean(pred):
    """prediction.mean() of GANLoss('wgangp') (models/networks.py:314-318); the caller negates it for real targets."""
    return _Mean.apply(pred)


class _L1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        _chk(a, b)
        _f32(a, b)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        ws = workspace(lib().nc_loss_ws_bytes(a.numel()), a.device, 'loss')
        check(lib().nc_l1_fwd(_ptr(a), _ptr(b), a.numel(), _ptr(out), _ptr(ws), ws.numel(), _stream()),
              'nc_l1_fwd')
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        da = torch.empty_like(a)
        check(lib().nc_l1_bwd(_ptr(a), _ptr(b), a.numel(), _ptr(g), _ptr(da), _stream()), 'nc_l1_bwd')
        return da, None


def l1_loss(a, b):
    """torch.nn.L1Loss()(a, b) with b treated as a constant (apollo_model.py:128,279: rec vs real)."""
    return _L1.apply(a, b)


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step):
    """torch.optim.Adam.step over one flat buffer (apollo_model.py:131-136)."""
    _chk(p, g, m, v)
    _f32(p, g, m, v)
    check(lib().nc_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, beta1, beta2, eps,
                             step, _stream()), 'nc_adam_step')


def set_force_direct(on):
    lib().nc_set_force_direct(1 if on else 0)


# Generation counter per parameter storage: nc_adam_step (and checkpoint loads) write parameters through raw pointers,
# which autograd's version counters never see.  FlatAdam.step / BaseModel.load_networks bump it; the whole-network
# Functions, which keep a zero-copy alias of the live parameters for backward, refuse a backward across a bump.
_param_gen = {}


def bump_param_generation(t):
    k = t.untyped_storage().data_ptr()
    _param_gen[k] = _param_gen.get(k, 0) + 1


def _param_generation(t):
    return _param_gen.get(t.untyped_storage().data_ptr(), 0)


def _param_versions(packed):
    """Autograd's version counters of the packed parameters: of the view itself (it shares the first parameter's) and, when the parameters
    live in a registered flat buffer (FlatAdam: p.data are views of it, with counters of their own), of that buffer."""
    flat = _flat_bufs.get(packed.untyped_storage().data_ptr())
    return packed._version, (flat._version if flat is not None else None)


# Direct gradient destination of the whole-network calls.  FlatAdam registers its flat gradient buffer under its flat
# parameter buffer's storage; when a whole-network backward finds that its packed parameters ARE a slice of such a
# buffer, it lets the kernels write the parameter gradients straight into the matching slice of the gradient buffer
# (they overwrite, so only the first backward of a slice per optimizer step may do that) and returns views of it: with
# p.grad = None autograd's AccumulateGrad adopts them -- no per-parameter add kernels, no extra copy.
_flat_grads = {}   # storage ptr of the flat parameter buffer -> [grad buffer, set of slices written this step]
_flat_bufs = {}    # the same key -> the flat parameter buffer itself (its version counter: _param_versions)


def register_flat_grad(flat, grad):
    _flat_grads[flat.untyped_storage().data_ptr()] = [grad, set()]
    _flat_bufs[flat.untyped_storage().data_ptr()] = flat


def flat_grad_step_begin(flat):
    ent = _flat_grads.get(flat.untyped_storage().data_ptr())
    if ent is not None:
        ent[1].clear()


def _grad_destination(packed):
    """A slice of the registered flat gradient buffer for these packed parameters, or a fresh tensor."""
    ent = _flat_grads.get(packed.untyped_storage().data_ptr())
    if ent is not None and os.environ.get('NC_DIRECT_GRADS', '1') != '0':
        grad, written = ent
        off, n = packed.storage_offset(), packed.numel()
        if off + n <= grad.numel() and not any(a < off + n and off < b for a, b in written):
            written.add((off, off + n))
            return grad[off:off + n]
    return torch.empty_like(packed)


# ---- whole-network calls: one C call per direction; the plumbing the Functions below share ---------------------------------
def _pack_params(params):
    """The parameter tensors as ONE flat fp32 tensor in the given order: a zero-copy view when they already sit back
    to back in one storage (FlatAdam's flat buffer), otherwise a concatenated copy."""
    p0 = params[0]
    off = p0.storage_offset()
    same = True
    for p in params:
        if (not p.is_contiguous()) or p.untyped_storage().data_ptr() != p0.untyped_storage().data_ptr() or \
                p.storage_offset() != off:
            same = False
            break
        off += p.numel()
    total = sum(p.numel() for p in params)
    if same:
        return p0.detach().as_strided((total,), (1,), p0.storage_offset())
    return torch.cat([p.detach().reshape(-1) for p in params])


def _grad_target(ctx, first):
    """Where a whole-network backward writes its packed parameter gradients: the optimizer's flat gradient slice when EVERY parameter
    wants a gradient (the kernels OVERWRITE the whole slice), a scratch tensor otherwise -- with all parameters frozen
    (set_requires_grad(False)) nothing is handed on; with SOME frozen, autograd receives views of the scratch tensor for the others
    (FlatAdam._collect copies them into the flat buffer) and the frozen ranges of the flat gradient keep the zeros of zero_grad, so
    FlatAdam.step leaves those parameters where they are."""
    if all(ctx.needs_input_grad[first:]):
        return _grad_destination(ctx.packed)
    return torch.empty_like(ctx.packed)


def _param_grads(ctx, dpar, shapes, first):
    grads = [None] * len(shapes)
    off = 0
    for i, shp in enumerate(shapes):
        n = 1
        for s in shp:
            n *= s
        if ctx.needs_input_grad[first + i]:
            grads[i] = dpar[off:off + n].view(shp)
        off += n
    return grads


def _net_forward(ctx, x, params, *, first, dims, ws_bytes, tag, n_params=None, count_msg=None):
    """Forward side of a whole-network Function, x contiguous and `params` its inputs from position `first` on, in this order: dense fp32
    CUDA tensors; dims() -- the Function's own shape checks, returning the scalar arguments of its C calls; the parameters as one packed
    tensor of the n_params floats the library expects (NcError(count_msg) otherwise); and on ctx what the backward side needs -- among
    it the workspace query ws_bytes(*dims) with its cache tag, which _net_ws answers in both directions.  -> packed, dims"""
    _chk(x, *params)
    _f32(x, *params)
    dims = dims()
    packed = _pack_params(params)
    if n_params is not None and packed.numel() != n_params:
        raise _lib.NcError(count_msg)
    ctx.packed, ctx.packed_gen = packed, _param_generation(packed)
    ctx.shapes = [tuple(p.shape) for p in params]
    ctx.net = (first, ws_bytes, dims, tag)
    return packed, dims


def _net_ws(ctx, device):
    _, ws_bytes, dims, tag = ctx.net
    return workspace(ws_bytes(*dims), device, tag)


def _net_out_shape(out_shape, dims, nd):
    """[B, 1, (od,) oh, ow] from the library's nc_*_out_shape(*dims, &od, &oh, &ow); dims[0] is the batch."""
    od, oh, ow = I(0), I(0), I(0)
    check(out_shape(*dims, ctypes.byref(od), ctypes.byref(oh), ctypes.byref(ow)), out_shape.__name__)
    return (dims[0], 1, oh.value, ow.value) if nd == 2 else (dims[0], 1, od.value, oh.value, ow.value)


def _net_backward(ctx, device, stale_msg, always_dpar=False):
    """Backward side: refuses (NcError(stale_msg)) when the parameters were written -- optimizer step, checkpoint load -- since the forward
    packed them; -> (the tensor the packed parameter gradients go to, see _grad_target -- None when no parameter wants one, unless the
    entry point needs it regardless -- and the workspace)."""
    if _param_generation(ctx.packed) != ctx.packed_gen:
        raise _lib.NcError(stale_msg)
    first = ctx.net[0]
    dpar = _grad_target(ctx, first) if always_dpar or any(ctx.needs_input_grad[first:]) else None
    return dpar, _net_ws(ctx, device)


def _net_grads(ctx, dx, dpar):
    """What backward returns: dx, None for the non-tensor inputs in front of the parameters, then one view of dpar per parameter that wants
    a gradient."""
    first = ctx.net[0]
    grads = _param_grads(ctx, dpar, ctx.shapes, first) if dpar is not None else [None] * len(ctx.shapes)
    return (dx,) + (None,) * (first - 1) + tuple(grads)


_PG_COUNT = 'fused PatchGAN: parameter count does not match (n_layers=%d, ndf=%d)'
_UPDATED = ': the parameters were updated (optimizer step / checkpoint load) between this forward and its backward; the saved ' \
           'activations no longer match them'


def _pg_dims(x, cfg, B):
    """(B, D, H, W, n_layers, ndf, nd) of the PatchGAN calls on planes or volumes shaped like x."""
    if x.shape[1] != 1:
        raise _lib.NcError('fused PatchGAN expects one input channel')
    return (B,) + ((1, x.shape[2], x.shape[3]) if cfg[2] == 2 else tuple(x.shape[2:])) + cfg


class _PatchGAN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg, *params):
        n_layers, ndf, nd = cfg
        x = x.contiguous()
        L = lib()
        packed, dims = _net_forward(ctx, x, params, first=2, dims=lambda: _pg_dims(x, cfg, x.shape[0]), ws_bytes=L.nc_patchgan_ws_bytes,
                                    tag='patchgan', n_params=L.nc_patchgan_param_floats(*cfg), count_msg=_PG_COUNT % (n_layers, ndf))
        y = torch.empty(_net_out_shape(L.nc_patchgan_out_shape, dims, nd), dtype=torch.float32, device=x.device)
        saved = torch.empty(L.nc_patchgan_saved_floats(*dims), dtype=torch.float32, device=x.device)
        ws = _net_ws(ctx, x.device)
        check(L.nc_patchgan_fwd(_ptr(packed), _ptr(x), _ptr(y), _ptr(saved), *dims, _ptr(ws), ws.numel(), _stream()), 'nc_patchgan_fwd')
        ctx.save_for_backward(x, saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, saved = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dpar, ws = _net_backward(ctx, x.device, 'fused PatchGAN' + _UPDATED)
        check(lib().nc_patchgan_bwd(_ptr(ctx.packed), _ptr(x), _ptr(saved), _ptr(dy), _ptr(dx), _ptr(dpar), *ctx.net[2], _ptr(ws),
                                    ws.numel(), _stream()), 'nc_patchgan_bwd')
        return _net_grads(ctx, dx, dpar)


class PatchGANShare:
    """One discriminator, one optimisation step: the activations of the pass over the slices of `fake` in the generator
    loss, laid out as the SECOND half of the (real, fake) batch of the discriminator loss that follows with the same
    weights (athena_model.py:240-260 then :190-238: optimizer_D.step() comes after both).  patchgan_fake_half fills it,
    patchgan_join_real runs only the `real` half and back-propagates through the whole batch."""
    __slots__ = ('saved', 'x', 'y', 'gen', 'packed_ptr', 'cfg', 'dims', 'src', 'src_version', 'axis')

    def __init__(self):
        self.saved = None

    def matches(self, params, cfg, fake, axis):
        if self.saved is None or self.cfg != tuple(cfg) or self.src is not fake or self.src_version != fake._version \
                or self.axis != axis:
            return False
        packed = _pack_params(params)
        return packed.data_ptr() == self.packed_ptr and _param_generation(packed) == self.gen

    def release(self):
        self.saved = self.x = self.y = self.src = None


class _PatchGANFakeHalf(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg, share, *params):
        n_layers, ndf, nd = cfg
        x = x.contiguous()
        B = x.shape[0]
        L = lib()
        # (dims: of the whole (real, fake) batch)
        packed, dims = _net_forward(ctx, x, params, first=3, dims=lambda: _pg_dims(x, cfg, 2 * B), ws_bytes=L.nc_patchgan_ws_bytes,
                                    tag='patchgan', n_params=L.nc_patchgan_param_floats(*cfg), count_msg=_PG_COUNT % (n_layers, ndf))
        oshape = _net_out_shape(L.nc_patchgan_out_shape, dims, nd)
        share.saved = torch.empty(L.nc_patchgan_saved_floats(*dims), dtype=torch.float32, device=x.device)
        share.x = torch.empty((2 * B,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
        share.x[B:].copy_(x)
        share.y = torch.empty(oshape, dtype=torch.float32, device=x.device)
        ws = _net_ws(ctx, x.device)
        check(L.nc_patchgan_fwd_part(_ptr(packed), _ptr(share.x[B:]), _ptr(share.y[B:]), _ptr(share.saved), 2 * B, B, B, *dims[1:],
                                     _ptr(ws), ws.numel(), _stream()), 'nc_patchgan_fwd_part')
        share.gen, share.packed_ptr, share.cfg, share.dims = ctx.packed_gen, packed.data_ptr(), tuple(cfg), (B,) + dims[1:4]
        ctx.saved_ref = share.saved  # keeps the buffers alive for this backward even if the share is released first
        ctx.x_ref = share.x
        return share.y[B:].clone()

    @staticmethod
    def backward(ctx, dy):
        stale = 'fused PatchGAN: the parameters were updated between this forward and its backward'
        if _param_generation(ctx.packed) != ctx.packed_gen:
            raise _lib.NcError(stale)
        if any(ctx.needs_input_grad[3:]):
            raise _lib.NcError('patchgan_fake_half: the discriminator must be frozen (generator loss)')
        dims = ctx.net[2]
        B = dims[0] // 2
        dy = dy.contiguous()
        xs = ctx.x_ref[B:]
        dx = torch.empty_like(xs)
        dpar, ws = _net_backward(ctx, dy.device, stale)
        check(lib().nc_patchgan_bwd_part(_ptr(ctx.packed), _ptr(xs), _ptr(ctx.saved_ref), _ptr(dy), _ptr(dx), 2 * B, B, B, *dims[1:],
                                         _ptr(ws), ws.numel(), _stream()), 'nc_patchgan_bwd_part')
        return _net_grads(ctx, dx, dpar)


class _PatchGANJoinReal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg, share, *params):
        n_layers, ndf, nd = cfg
        x = x.contiguous()
        B = share.dims[0]

        def dims():
            if tuple(x.shape) != tuple(share.x.shape[1:]) and tuple(x.shape) != (B,) + tuple(share.x.shape[1:]):
                raise _lib.NcError('patchgan_join_real: the real planes do not have the shape of the cached fake planes')
            return (2 * B,) + share.dims[1:] + cfg

        L = lib()
        # (no parameter count here: the packed tensor must BE the one the pass over the fake planes counted)
        packed, dims = _net_forward(ctx, x, params, first=3, dims=dims, ws_bytes=L.nc_patchgan_ws_bytes, tag='patchgan')
        if packed.data_ptr() != share.packed_ptr or ctx.packed_gen != share.gen:
            raise _lib.NcError('patchgan_join_real: the parameters changed since the pass over the fake planes')
        cur = torch.cuda.current_stream()
        for t in (share.saved, share.x, share.y):
            t.record_stream(cur)
        share.x[:B].copy_(x)
        ws = _net_ws(ctx, x.device)
        check(L.nc_patchgan_fwd_part(_ptr(packed), _ptr(share.x), _ptr(share.y), _ptr(share.saved), 2 * B, 0, B, *dims[1:], _ptr(ws),
                                     ws.numel(), _stream()), 'nc_patchgan_fwd_part')
        ctx.save_for_backward(share.x, share.saved)
        y = share.y
        share.release()  # the autograd graph owns the buffers from here
        return y

    @staticmethod
    def backward(ctx, dy):
        x, saved = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dpar, ws = _net_backward(ctx, x.device, 'fused PatchGAN: the parameters were updated between this forward and its backward')
        check(lib().nc_patchgan_bwd(_ptr(ctx.packed), _ptr(x), _ptr(saved), _ptr(dy), _ptr(dx), _ptr(dpar), *ctx.net[2], _ptr(ws),
                                    ws.numel(), _stream()), 'nc_patchgan_bwd')
        return _net_grads(ctx, dx[:x.shape[0] // 2] if dx is not None else None, dpar)


def patchgan_fake_half(x, params, n_layers, ndf, dimension, share, src=None, axis=None):
    """The frozen discriminator on the slices of `fake` (generator loss), kept in `share` as the second half of the batch
    the discriminator loss runs next (see PatchGANShare).  src / axis: the volume the planes were cut from and the axis,
    which PatchGANShare.matches compares before the cached half is used."""
    y = _PatchGANFakeHalf.apply(x, (int(n_layers), int(ndf), int(dimension)), share, *params)
    share.src, share.src_version, share.axis = src, (src._version if src is not None else None), axis
    return y


def patchgan_join_real(x, params, n_layers, ndf, dimension, share):
    """Predictions for the batch (x, cached fake planes): forward of the `real` half only; backward over the whole batch."""
    return _PatchGANJoinReal.apply(x, (int(n_layers), int(ndf), int(dimension)), share, *params)


def patchgan(x, params, n_layers, ndf, dimension):
    """NLayerDiscriminator.forward (networks.py:1063-1066) with InstanceNorm, as one C call (and one for backward)."""
    return _PatchGAN.apply(x, (int(n_layers), int(ndf), int(dimension)), *params)


class _PatchGANGP(torch.autograd.Function):
    """WGAN-GP penalty of the 2-D PatchGAN (cal_gradient_penalty, networks.py:321-359) on nc_patchgan_gp_fwd / _bwd: returns
    (penalty, g = d(sum D)/dx).  g is detached; the penalty's backward is its second-order gradient with respect to the parameters
    (into the same destination as _PatchGAN's, so it accumulates with the rest of the backward) and to x."""

    @staticmethod
    def forward(ctx, x, cfg, *params):
        n_layers, ndf, nd, constant, lambda_gp = cfg
        x = x.contiguous()

        def dims():
            if nd != 2 or x.dim() != 4 or x.shape[1] != 1:
                raise _lib.NcError('patchgan_gp: the fused penalty covers 2-D inputs [B, 1, H, W], got %s (nd=%d)' % (tuple(x.shape), nd))
            return (x.shape[0], 1, x.shape[2], x.shape[3], n_layers, ndf, nd)

        L = lib()
        packed, dims = _net_forward(ctx, x, params, first=2, dims=dims, ws_bytes=L.nc_patchgan_gp_ws_bytes, tag='patchgan',
                                    n_params=L.nc_patchgan_param_floats(n_layers, ndf, nd), count_msg=_PG_COUNT % (n_layers, ndf))
        nsaved = L.nc_patchgan_gp_saved_floats(*dims)
        if nsaved == 0:
            raise _lib.NcError('patchgan_gp: shape %s not covered (n_layers=%d)' % (tuple(x.shape), n_layers))
        saved = torch.empty(nsaved, dtype=torch.float32, device=x.device)
        g = torch.empty_like(x)
        pen = torch.empty((), dtype=torch.float32, device=x.device)
        ws = _net_ws(ctx, x.device)
        check(L.nc_patchgan_gp_fwd(_ptr(packed), _ptr(x), _ptr(g), _ptr(pen), _ptr(saved), *dims, constant, lambda_gp, _ptr(ws),
                                   ws.numel(), _stream()), 'nc_patchgan_gp_fwd')
        ctx.mark_non_differentiable(g)
        ctx.save_for_backward(x, saved, g)
        ctx.gp = (constant, lambda_gp)
        return pen, g

    @staticmethod
    def backward(ctx, dpen, dg):
        x, saved, g = ctx.saved_tensors
        dpen = dpen.to(torch.float32).contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dpar, ws = _net_backward(ctx, x.device, 'fused PatchGAN gradient penalty' + _UPDATED)
        check(lib().nc_patchgan_gp_bwd(_ptr(ctx.packed), _ptr(x), _ptr(saved), _ptr(g), _ptr(dpen), _ptr(dpar), _ptr(dx), *ctx.net[2],
                                       *ctx.gp, _ptr(ws), ws.numel(), _stream()), 'nc_patchgan_gp_bwd')
        return _net_grads(ctx, dx, dpar)


def patchgan_gp(x, params, n_layers, ndf, nd, constant, lambda_gp):
    """(penalty, gradients) of cal_gradient_penalty (networks.py:321-359) for the 2-D PatchGAN with InstanceNorm on the interpolates
    x [B, 1, H, W]: penalty = lambda_gp * mean_b (||g_b + 1e-16|| - constant)^2 with g = d(sum D(x))/dx, one C call per direction.
    `gradients` (g, shape of x) is returned detached -- unlike the reference's, it carries no graph."""
    return _PatchGANGP.apply(x, (int(n_layers), int(ndf), int(nd), float(constant), float(lambda_gp)), *params)


def kgan_dims(shape, nd):
    """(B, D, H, W) of a KernelPatchDiscriminator input; ValueError, before anything is launched, for the inputs the reference's
    InstanceNorm refuses in training mode: an edge below 7 (the valid 7^nd first_layer leaves nothing) or a 7^nd input (one value per
    channel)."""
    if len(shape) != nd + 2:
        raise ValueError('kernelGAN discriminator: expected a %d-D input [B, C, spatial...], got shape %s' % (nd + 2, tuple(shape)))
    sp = tuple(int(s) for s in shape[2:])
    if min(sp) < 7:
        raise ValueError('kernelGAN discriminator: every spatial edge must be at least 7 (first_layer is a 7^%d conv with padding 0), '
                         'got %s' % (nd, sp))
    out = 1
    for s in sp:
        out *= s - 6
    if out < 2:
        raise ValueError('Expected more than 1 spatial element when training, got input size %s: the KernelGAN discriminator\'s '
                         'InstanceNorm sees one value per channel' % ((int(shape[0]), 64) + tuple(s - 6 for s in sp),))
    return (int(shape[0]), 1) + sp[-2:] if nd == 2 else (int(shape[0]),) + sp


class _KernelGAN(torch.autograd.Function):
    """KernelPatchDiscriminator.forward (networks.py:1141-1144) with InstanceNorm, 1 input channel, ndf = 64 on nc_kgan_fwd / _bwd:
    always fp32.  The parameters are packed in state-dict order (zero-copy inside FlatAdam's buffer), their gradients go straight into
    its flat gradient slice when every one of them wants one (_grad_target)."""

    @staticmethod
    def forward(ctx, x, cfg, *params):
        ndf, nd = cfg
        x = x.contiguous()

        def dims():
            if x.shape[1] != 1:
                raise _lib.NcError('fused KernelGAN discriminator expects one input channel')
            return kgan_dims(x.shape, nd) + cfg

        L = lib()
        packed, dims = _net_forward(ctx, x, params, first=2, dims=dims, ws_bytes=L.nc_kgan_ws_bytes, tag='kgan',
                                    n_params=L.nc_kgan_param_floats(ndf, nd),
                                    count_msg='fused KernelGAN discriminator: parameter count does not match (ndf=%d, nd=%d)' % (ndf, nd))
        y = torch.empty(_net_out_shape(L.nc_kgan_out_shape, dims, nd), dtype=torch.float32, device=x.device)
        saved = torch.empty(L.nc_kgan_saved_floats(*dims), dtype=torch.float32, device=x.device)
        ws = _net_ws(ctx, x.device)
        check(L.nc_kgan_fwd(_ptr(packed), _ptr(x), _ptr(y), _ptr(saved), *dims, _ptr(ws), ws.numel(), _stream()), 'nc_kgan_fwd')
        ctx.save_for_backward(x, saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, saved = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dpar, ws = _net_backward(ctx, x.device, 'fused KernelGAN discriminator' + _UPDATED)
        check(lib().nc_kgan_bwd(_ptr(ctx.packed), _ptr(x), _ptr(saved), _ptr(dy), _ptr(dx), _ptr(dpar), *ctx.net[2], _ptr(ws),
                                ws.numel(), _stream()), 'nc_kgan_bwd')
        return _net_grads(ctx, dx, dpar)


def kernelgan(x, params, nd, ndf=64):
    """KernelPatchDiscriminator.forward (networks.py:1141-1144) with InstanceNorm as one C call (and one for backward); `params` in
    state-dict order."""
    return _KernelGAN.apply(x, (int(ndf), int(nd)), *params)


# ---- whole-network generators (nc_unet_deconv_train_fwd / _bwd, nc_deep_linear_fwd / _bwd) ------------------------------------
def _gen_dims(x):
    N, _, S0, S1, S2 = x.shape
    return N, S0, S1, S2


class _UnetDeconvTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, *params):
        x = x.contiguous()
        L = lib()
        packed, dims = _net_forward(ctx, x, params, first=1, dims=lambda: _gen_dims(x), ws_bytes=L.nc_unet_deconv_train_ws_bytes,
                                    tag='unet_train', n_params=L.nc_unet_deconv_param_floats(),
                                    count_msg='fused Unet_deconv: parameter count does not match')
        nsv = L.nc_unet_deconv_saved_floats(*dims)
        if nsv == 0:
            raise _lib.NcError('fused Unet_deconv: every edge must be a positive multiple of 4, got %s' % (dims[1:],))
        saved = torch.empty(nsv, dtype=torch.float32, device=x.device)
        ws = _net_ws(ctx, x.device)
        y = torch.empty_like(x)
        e0 = _prof_begin()
        kept = ctypes.c_uint(0)  # which three-term input copies the forward left in `saved`: travels with this context
        check(L.nc_unet_deconv_train_fwd(_ptr(packed), _ptr(x), _ptr(y), _ptr(saved), *dims, _ptr(ws), ws.numel(), _stream(),
                                         ctypes.byref(kept)), 'nc_unet_deconv_train_fwd')
        ctx.kept = kept.value
        _prof_end(e0, 'unet_fwd', 2.0 * 663809 * x.numel())
        ctx.save_for_backward(x, y, saved)
        ctx.packed_version = _param_versions(packed)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, saved = ctx.saved_tensors
        stale = 'fused Unet_deconv: the parameters were updated between this forward and its backward'
        # (the backward's data gradients take the packed weights the forward prepared, its weight-space reads the live buffer: nc_hip.h)
        if _param_versions(ctx.packed) != ctx.packed_version:
            raise _lib.NcError(stale)
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dpar, ws = _net_backward(ctx, x.device, stale, always_dpar=True)
        e0 = _prof_begin()
        check(lib().nc_unet_deconv_bwd(_ptr(ctx.packed), _ptr(x), _ptr(y), _ptr(saved), _ptr(dy), _ptr(dx), _ptr(dpar), *ctx.net[2],
                                       _ptr(ws), ws.numel(), _stream(), ctx.kept), 'nc_unet_deconv_bwd')
        # dgrad + wgrad of every layer but the first one's data gradient
        _prof_end(e0, 'unet_bwd', 2.0 * (2 * 663809 - 1728) * x.numel())
        return _net_grads(ctx, dx, dpar)


def unet_deconv_train(x, params):
    """Unet_deconv.forward (networks.py:512-538) with autograd, as one C call per direction."""
    return _UnetDeconvTrain.apply(x, *params)


class _DeepLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, *params):
        x = x.contiguous()
        L = lib()
        packed, dims = _net_forward(ctx, x, params, first=1, dims=lambda: _gen_dims(x), ws_bytes=L.nc_deep_linear_ws_bytes,
                                    tag='deep_linear', n_params=L.nc_deep_linear_param_floats(),
                                    count_msg='fused DeepLinearGenerator: parameter count does not match')
        need = any(ctx.needs_input_grad)
        saved = torch.empty(L.nc_deep_linear_saved_floats(*dims), dtype=torch.float32, device=x.device) if need else None
        ws = _net_ws(ctx, x.device)
        y = torch.empty_like(x)
        e0 = _prof_begin()
        kept = ctypes.c_uint(0)
        check(L.nc_deep_linear_fwd(_ptr(packed), _ptr(x), _ptr(y), _ptr(saved), *dims, _ptr(ws), ws.numel(), _stream(),
                                   ctypes.byref(kept)), 'nc_deep_linear_fwd')
        ctx.kept = kept.value
        _prof_end(e0, 'deep_linear_fwd', 2.0 * 647120 * x.numel())
        if need:
            ctx.save_for_backward(x, saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, saved = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dpar, ws = _net_backward(ctx, x.device, 'fused DeepLinearGenerator: the parameters were updated between this forward and its '
                                 'backward', always_dpar=True)
        e0 = _prof_begin()
        check(lib().nc_deep_linear_bwd(_ptr(ctx.packed), _ptr(x), _ptr(saved), _ptr(dy), _ptr(dx), _ptr(dpar), *ctx.net[2], _ptr(ws),
                                       ws.numel(), _stream(), ctx.kept), 'nc_deep_linear_bwd')
        _prof_end(e0, 'deep_linear_bwd', 2.0 * (2 * 647120 - (0 if dx is not None else 21952)) * x.numel())
        return _net_grads(ctx, dx, dpar)


def deep_linear(x, params):
    """DeepLinearGenerator.forward (networks.py:913-917), with autograd, as one C call per direction."""
    return _DeepLinear.apply(x, *params)


# ---- the same two generators on the 16-bit end-to-end path (nc_unet_deconv_lp_* / nc_deep_linear_lp_*) ---------------
def gen_lp_supported(kind, shape):
    """True when --precision bf16 can run this generator as the whole-network 16-bit call (every layer covered)."""
    if conv_precision != 'bf16' or len(shape) != 5 or shape[1] != 1:
        return False
    N, _, S0, S1, S2 = shape
    fn = lib().nc_unet_deconv_lp_supported if kind == 'unet' else lib().nc_deep_linear_lp_supported
    return bool(fn(N, S0, S1, S2, _DT['bf16']))


class _GenLp(torch.autograd.Function):
    """kind 'unet': Unet_deconv, 'linear': DeepLinearGenerator; bf16 activations end to end, fp32 master weights."""

    @staticmethod
    def forward(ctx, x, kind, *params):
        x = x.contiguous()
        L = lib()
        net = 'unet_deconv' if kind == 'unet' else 'deep_linear'
        pre = 'nc_%s_lp' % net
        packed, dims = _net_forward(ctx, x, params, first=2, dims=lambda: _gen_dims(x), ws_bytes=getattr(L, pre + '_ws_bytes'), tag=pre,
                                    n_params=getattr(L, 'nc_%s_param_floats' % net)(), count_msg='%s: parameter count does not match' % pre)
        nsv = getattr(L, pre + '_saved_bytes')(*dims)
        if nsv == 0:
            raise _lib.NcError('%s: shape %s is not covered by the 16-bit kernels' % (pre, dims[1:]))
        saved = torch.empty(nsv, dtype=torch.uint8, device=x.device)
        ws = _net_ws(ctx, x.device)
        y = torch.empty_like(x)
        e0 = _prof_begin()
        kept = ctypes.c_uint(0)  # deep_linear_gen: the form the forward took (the backward follows it, not the switches of its own moment)
        extra = (ctypes.byref(kept),) if kind != 'unet' else ()
        check(getattr(L, pre + '_fwd')(_ptr(packed), _ptr(x), _ptr(y), _ptr(saved), *dims, _DT['bf16'], _ptr(ws), ws.numel(),
                                       _stream(), *extra), pre + '_fwd')
        ctx.kept, ctx.kind = kept.value, kind
        _prof_end(e0, ('unet' if kind == 'unet' else 'deep_linear') + '_lp_fwd', 2.0 * (663809 if kind == 'unet' else 647120) * x.numel())
        ctx.save_for_backward(x, y, saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, saved = ctx.saved_tensors
        dy = dy.contiguous()
        kind, dims, dt = ctx.kind, ctx.net[2], _DT['bf16']
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dpar, ws = _net_backward(ctx, x.device, '16-bit generator: the parameters were updated between this forward and its backward',
                                 always_dpar=True)
        L = lib()
        e0 = _prof_begin()
        if kind == 'unet':
            check(L.nc_unet_deconv_lp_bwd(_ptr(ctx.packed), _ptr(x), _ptr(y), _ptr(saved), _ptr(dy), _ptr(dx), _ptr(dpar), *dims, dt,
                                          _ptr(ws), ws.numel(), _stream()), 'nc_unet_deconv_lp_bwd')
        else:
            check(L.nc_deep_linear_lp_bwd(_ptr(ctx.packed), _ptr(x), _ptr(saved), _ptr(dy), _ptr(dx), _ptr(dpar), *dims, dt, _ptr(ws),
                                          ws.numel(), _stream(), ctx.kept), 'nc_deep_linear_lp_bwd')
        mac = (2 * 663809 - 1728) if kind == 'unet' else 2 * 647120
        _prof_end(e0, ('unet' if kind == 'unet' else 'deep_linear') + '_lp_bwd', 2.0 * mac * x.numel())
        return _net_grads(ctx, dx, dpar)


def unet_deconv_lp(x, params):
    return _GenLp.apply(x, 'unet', *params)


def deep_linear_lp(x, params):
    return _GenLp.apply(x, 'linear', *params)


# ---- torch.nn.utils.spectral_norm (NLayerDiscriminatorSN, networks.py:1069-1111) ------------------------------------
class _SpectralNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w_orig, u, v, power_iteration):
        w_orig = w_orig.contiguous()
        _chk(w_orig, u, v)
        _f32(w_orig, u, v)
        K = w_orig.shape[0]
        M = w_orig.numel() // K
        if u.numel() != K or v.numel() != M:
            raise _lib.NcError('spectral_norm: u / v do not match the weight (%d x %d)' % (K, M))
        w = torch.empty_like(w_orig)
        sigma = torch.empty(1, dtype=torch.float32, device=w_orig.device)
        scratch = torch.empty(K, dtype=torch.float32, device=w_orig.device)
        check(lib().nc_spectral_norm_fwd(_ptr(w_orig), _ptr(u), _ptr(v), _ptr(w), _ptr(sigma), _ptr(scratch), K, M,
                                         1 if power_iteration else 0, 1e-12, _stream()), 'nc_spectral_norm_fwd')
        # u, v as they stand after this forward (later forwards update the buffers in place)
        ctx.save_for_backward(w, u.clone(), v.clone(), sigma)
        return w

    @staticmethod
    def backward(ctx, g):
        w, u, v, sigma = ctx.saved_tensors
        g = g.contiguous()
        K = w.shape[0]
        M = w.numel() // K
        dw = torch.empty_like(w)
        check(lib().nc_spectral_norm_bwd(_ptr(g), _ptr(w), _ptr(u), _ptr(v), _ptr(sigma), _ptr(dw), K, M, _stream()),
              'nc_spectral_norm_bwd')
        return dw, None, None, None


def spectral_norm_weight(w_orig, u, v, power_iteration):
    """weight = w_orig / sigma with one power iteration on (u, v) (in place) when `power_iteration`."""
    return _SpectralNorm.apply(w_orig, u, v, bool(power_iteration))


# ---- the ResNet generators (ResnetGenerator / ResnetBlock, networks.py:724-837; 2-D only) -----------------------------------------------
def _nchw(x, what):
    if x.dim() != 4:
        raise _lib.NcError('%s: expected an NCHW tensor, got %s' % (what, tuple(x.shape)))
    return tuple(int(s) for s in x.shape)


class _ReflectPad2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        x = x.contiguous()
        _chk(x)
        _f32(x)
        N, C, H, W = _nchw(x, 'reflect_pad2d')
        y = torch.empty((N, C, H + 2 * p, W + 2 * p), dtype=torch.float32, device=x.device)
        check(lib().nc_reflect_pad2d_fwd(_ptr(x), _ptr(y), N * C, H, W, p, _stream()), 'nc_reflect_pad2d_fwd')
        ctx.cfg = (N, C, H, W, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W, p = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty((N, C, H, W), dtype=torch.float32, device=dy.device)
        check(lib().nc_reflect_pad2d_bwd(_ptr(dy), _ptr(dx), N * C, H, W, p, _stream()), 'nc_reflect_pad2d_bwd')
        return dx, None


def reflect_pad2d(x, p):
    """nn.ReflectionPad2d(p), p 1 or 3 (networks.py:747,772): the explicit pad in front of the 7 x 7 convolutions."""
    return _ReflectPad2d.apply(x, int(p))


class _ConvReflect3(torch.autograd.Function):
    """ReflectionPad2d(1) + Conv2d(C, K, 3) as one layer on nc_conv2d_k3_reflect_*.  dead_bias: an InstanceNorm(affine=False) follows, the bias
    cannot reach the output -- the add is skipped; its gradient (the sum of the gradient at this layer's output: mathematically zero) comes from
    the norm's backward through `link`, as for ops.conv, or from the weight-gradient call's own sum."""

    @staticmethod
    def forward(ctx, x, w, b, dead_bias, link):
        x = x.contiguous()
        _chk(x, w, b)
        _f32(x, w, b)
        N, C, H, W = _nchw(x, 'conv_reflect3')
        K = w.shape[0]
        if tuple(w.shape) != (K, C, 3, 3):
            raise _lib.NcError('conv_reflect3: weight %s does not fit %d input channels (K, C, 3, 3)' % (tuple(w.shape), C))
        ctx.link = link
        if link is not None:
            link.want = b is not None and ctx.needs_input_grad[2]
        y = torch.empty((N, K, H, W), dtype=torch.float32, device=x.device)
        ws = workspace(lib().nc_conv2d_k3_reflect_ws_bytes(N, C, H, W, K), x.device, 'ws_k3r')
        check(lib().nc_conv2d_k3_reflect_fwd(_ptr(x), _ptr(w), _ptr(None if dead_bias else b), _ptr(y), N, C, H, W, K, _ptr(ws), ws.numel(),
                                             _stream()), 'nc_conv2d_k3_reflect_fwd')
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        N, C, H, W = x.shape
        K = w.shape[0]
        L = lib()
        dx = dw = db = None
        want_b = ctx.has_b and ctx.needs_input_grad[2]
        if want_b and ctx.link is not None and ctx.link.dbias is not None:
            db, ctx.link.dbias = ctx.link.dbias, None
            want_b = False
        ws = workspace(L.nc_conv2d_k3_reflect_ws_bytes(N, C, H, W, K), x.device, 'ws_k3r')
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            check(L.nc_conv2d_k3_reflect_dgrad(_ptr(dy), _ptr(w), _ptr(dx), N, C, H, W, K, _ptr(ws), ws.numel(), _stream()),
                  'nc_conv2d_k3_reflect_dgrad')
        if ctx.needs_input_grad[1] or want_b:
            dw = torch.empty_like(w)
            if want_b:
                db = torch.empty(K, dtype=torch.float32, device=x.device)
            check(L.nc_conv2d_k3_reflect_wgrad(_ptr(x), _ptr(dy), _ptr(dw), _ptr(db if want_b else None), N, C, H, W, K, _ptr(ws), ws.numel(),
                                               _stream()), 'nc_conv2d_k3_reflect_wgrad')
        return dx, dw, db, None, None


def conv_reflect3(x, w, b=None, dead_bias=False, link=None):
    """nn.ReflectionPad2d(1) followed by nn.Conv2d(C, K, 3, padding 0) (ResnetBlock, networks.py:808-830)."""
    return _ConvReflect3.apply(x, w, b, bool(dead_bias), link)


class _ConvT2dK3S2(torch.autograd.Function):
    """nn.ConvTranspose2d(C, K, 3, stride 2, padding 1, output_padding 1) (networks.py:766-769) as the data gradient of the Conv2d(K -> C, 3 x 3,
    stride 2, padding 1) whose weight tensor IS the (C, K, 3, 3) parameter -- no flip, no copy: forward nc_conv_dgrad with the 2H x 2W image as
    its input size, data gradient nc_conv_fwd, weight gradient nc_conv_wgrad with the roles of x and dy exchanged.  Every such layer of the
    reference sits in front of a norm: its bias exists only with InstanceNorm(affine=False), where it cannot reach the output -- it is never
    added, and its gradient comes from the norm's backward through `link`."""

    @staticmethod
    def forward(ctx, x, w, b, link):
        x = x.contiguous()
        _chk(x, w, b)
        _f32(x, w, b)
        N, C, H, W = _nchw(x, 'conv_transpose_k3s2')
        if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[0] != C:
            raise _lib.NcError('conv_transpose_k3s2: weight %s does not fit x %s (C, K, 3, 3)' % (tuple(w.shape), tuple(x.shape)))
        ctx.link, ctx.has_b = link, b is not None
        if link is not None:
            link.want = b is not None and ctx.needs_input_grad[2]
        ctx.save_for_backward(x, w)
        return conv_dgrad_raw(x, w, (N, w.shape[1], 2 * H, 2 * W), 2, 1)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.link is not None and ctx.link.dbias is not None:
            db, ctx.link.dbias = ctx.link.dbias, None
        if ctx.has_b and ctx.needs_input_grad[2] and db is None:
            raise _lib.NcError('conv_transpose_k3s2: the bias gradient is taken by the InstanceNorm behind the layer (link), and none ran')
        if ctx.needs_input_grad[0]:
            dx = conv_fwd_raw(dy, w, None, 2, 1)
        if ctx.needs_input_grad[1]:
            dw, _ = conv_wgrad_raw(dy, x, w.shape, 2, 1, False)
        return dx, dw, db, None


def conv_transpose_k3s2(x, w, b=None, link=None):
    """The upsampling layers of ResnetGenerator (networks.py:766-769): x [N, C, H, W], w [C, K, 3, 3] -> [N, K, 2H, 2W].  b is a dead bias (see
    _ConvT2dK3S2): accepted, never added."""
    return _ConvT2dK3S2.apply(x, w, b, link)


class _InstNormRes(torch.autograd.Function):
    """skip + InstanceNorm2d(affine=False)(x): the tail of a ResnetBlock (networks.py:830,836) in one pass (nc_instnorm_res_fwd).  Backward: the
    skip gradient is dy itself; the other branch is the norm's backward without activation -- nc_instnorm_act_bwd with slope 1, whose
    `v > 0 ? g : g * slope` is the identity bit for bit."""

    @staticmethod
    def forward(ctx, x, skip, eps, link):
        x, skip = x.contiguous(), skip.contiguous()
        _chk(x, skip)
        _f32(x, skip)
        if x.shape != skip.shape:
            raise _lib.NcError('instance_norm_residual: x %s and skip %s differ' % (tuple(x.shape), tuple(skip.shape)))
        ctx.link = link
        mean, rstd = instnorm_stats(x, eps)
        NC = mean.numel()
        y = torch.empty_like(x)
        check(lib().nc_instnorm_res_fwd(_ptr(x), _ptr(mean), _ptr(rstd), _ptr(skip), _ptr(y), NC, x.numel() // NC, _stream()),
              'nc_instnorm_res_fwd')
        ctx.save_for_backward(x, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        NC = mean.numel()
        S = x.numel() // NC
        dx = None
        link = ctx.link
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            if link is not None and link.want:
                N, C = x.shape[0], x.shape[1]
                db = torch.empty(C, dtype=torch.float32, device=x.device)
                ws = workspace(lib().nc_instnorm_bwd_dbias_ws_bytes(NC, S), x.device, 'in')
                check(lib().nc_instnorm_act_bwd_dbias(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), 1.0, _ptr(dx), _ptr(db), N, C, S, _ptr(ws),
                                                      ws.numel(), _stream()), 'nc_instnorm_act_bwd_dbias')
                link.dbias = db
            else:
                ws = workspace(lib().nc_instnorm_ws_bytes(NC, S), x.device, 'in')
                check(lib().nc_instnorm_act_bwd(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), 1.0, _ptr(dx), NC, S, _ptr(ws), ws.numel(),
                                                _stream()), 'nc_instnorm_act_bwd')
        return dx, (dy if ctx.needs_input_grad[1] else None), None, None


def instance_norm_residual(x, skip, eps=1e-5, link=None):
    return _InstNormRes.apply(x, skip, float(eps), link)


class _ResidualAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        _chk(a, b)
        _f32(a, b)
        if a.shape != b.shape:
            raise _lib.NcError('residual_add: %s and %s differ' % (tuple(a.shape), tuple(b.shape)))
        y = torch.empty_like(a)
        check(lib().nc_residual_add(_ptr(a), _ptr(b), _ptr(y), a.numel(), _stream()), 'nc_residual_add')
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def residual_add(a, b):
    """x + conv_block(x) behind a BatchNorm (networks.py:836 with --norm batch)."""
    return _ResidualAdd.apply(a, b)


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        x = x.contiguous()
        _chk(x)
        _f32(x)
        # the mask is drawn on the device from torch's generator (torch.manual_seed governs it); matching nn.Dropout's own mask is not a goal
        mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device).bernoulli_(1.0 - p)
        ctx.mask, ctx.scale = mask, 1.0 / (1.0 - p)
        y = torch.empty_like(x)
        check(lib().nc_dropout_mul(_ptr(x), _ptr(mask), ctx.scale, _ptr(y), x.numel(), _stream()), 'nc_dropout_mul')
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        check(lib().nc_dropout_mul(_ptr(dy), _ptr(ctx.mask), ctx.scale, _ptr(dx), dy.numel(), _stream()), 'nc_dropout_mul')
        return dx, None


def dropout(x, p=0.5, training=True):
    """nn.Dropout(p) (ResnetBlock, networks.py:818-819): the identity in evaluation mode; in training mode survivors are multiplied by
    1 / (1 - p) (exactly 2 for p = 0.5) in a HIP kernel and the backward multiplies dy by the same mask."""
    if not training:
        return x
    return _Dropout.apply(x, float(p))


VIEW_KEYS = ('slice_xy', 'slice_xz', 'slice_yz', 'mip_xy', 'mip_xz', 'mip_yz')


def tensor2im(t, imtype=np.uint16):
    """util.tensor2im (util/util.py:11-39) of a dense fp32 tensor on the device: clip to [0, 1], scale by 255 / 65535 in fp32, clip, truncating
    cast.  -> numpy array of t's shape, np.uint8 or np.uint16 (the copy to the host synchronises, as the reference's .cpu() does)."""
    if imtype not in (np.uint8, np.uint16):
        raise ValueError('tensor2im: imtype must be np.uint8 or np.uint16, got %r' % (imtype,))
    t = t.detach().contiguous()
    _chk(t)
    _f32(t)
    u16 = imtype == np.uint16
    out = torch.empty(t.shape, dtype=torch.int16 if u16 else torch.uint8, device=t.device)
    if t.numel():
        check(lib().nc_tensor2im(_ptr(t), _ptr(out), 1 if u16 else 0, t.numel(), _stream()), 'nc_tensor2im')
    a = out.cpu().numpy()
    return a.view(np.uint16) if u16 else a


def progress_views(t, index=None):
    """What Visualizer.display_current_results shows of one visual (util/visualizer.py:138-144, 171-173), from one C call: the slices
    [index,:,:], [:,index,:], [:,:,index] and the maximum projections over the three axes of tensor2im(t, uint8)[0, 0], plus `hist`, the
    counts of its 256 values (int64).  index defaults to int(D / 2) for all three axes, as in the reference, whose errors are mirrored
    before any launch: a tensor that is not 5-D raises ValueError (the unpack of img_shape), an index past H or W raises IndexError."""
    if t.dim() != 5:
        raise ValueError('progress_views: expected a [N, C, D, H, W] tensor, got %d dimensions' % t.dim())
    N, C, D, H, W = t.shape
    if min(N, C, D, H, W) < 1:
        raise IndexError('progress_views: empty tensor %s' % (tuple(t.shape),))
    if index is None:
        index = int(D / 2)
    index = int(index)
    for name, ext in (('D', D), ('H', H), ('W', W)):
        if not 0 <= index < ext:
            raise IndexError('progress_views: index %d is out of bounds for axis %s with size %d' % (index, name, ext))
    t = t.detach().contiguous()
    _chk(t)
    _f32(t)
    L = lib()
    nv = int(L.nc_progress_views_bytes(D, H, W))
    hoff = (nv + 3) & ~3
    buf = torch.empty(hoff + 1024, dtype=torch.uint8, device=t.device)  # the views, then the histogram: one copy to the host
    check(L.nc_progress_views(_ptr(t), N, C, D, H, W, index, P(buf.data_ptr()), P(buf.data_ptr() + hoff), _stream()), 'nc_progress_views')
    host = buf.cpu().numpy()
    out, off = {}, 0
    for key, shape in zip(VIEW_KEYS, ((H, W), (D, W), (D, H)) * 2):
        n = shape[0] * shape[1]
        out[key] = host[off:off + n].reshape(shape)
        off += n
    out['hist'] = host[hoff:hoff + 1024].view(np.uint32).astype(np.int64)
    return out
