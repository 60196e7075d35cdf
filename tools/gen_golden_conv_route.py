"""Writes tests/golden/conv_route_parent.npz: what the host-side convolution queries of libnc_hip.so answer over a grid of layers, under four
switch settings.  Run it against a build of the commit BEFORE a change of the dispatch (NC_HIP_LIB=<that build>/libnc_hip.so); the test
tests/test_conv_route.py then holds the tree to those numbers.  Every query is host arithmetic: no GPU is needed, here or in the test.

    shapes  [n, 11] int64   N C D H W K kd kh kw stride pad
    modes   the switch settings, in the order of the second axis of `answers`
    answers [n, 4, 11] int64, per shape and mode (names in `columns`):
            nc_conv_ws_bytes | nc_conv_fwd_path | nc_conv_wgrad_path | nc_conv2d_k3_active(0 | 1) | nc_conv2d_split_active(0 | 1 | 2) |
            nc_conv_lp_supported(0 | 1 | 2)

    python tools/gen_golden_conv_route.py [--check]     (--check: compare with the committed file instead of writing it)"""
import ctypes
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT = os.path.join(ROOT, 'tests', 'golden', 'conv_route_parent.npz')

MODES = ['default', 'nc_set_conv_split(0)', 'nc_set_force_direct(1)', 'nc_set_conv2d_k3(0)']
COLUMNS = ['ws_bytes', 'fwd_path', 'wgrad_path', 'k3_active_fwd', 'k3_active_dgrad', 'split2d_active_fwd', 'split2d_active_dgrad',
           'split2d_active_wgrad', 'lp_fwd', 'lp_dgrad', 'lp_wgrad']
PROBE = {2: (32, 32), 3: (32, 32, 32)}   # the extent nc_conv_fwd_path / nc_conv_wgrad_path route at (a pointwise layer: a 256 x 256 plane)


def layer(N, C, K, sp, k, stride, pad):
    """(N, C, K, spatial, k, stride, pad) of the reference modules' case lists -> a row of `shapes`."""
    D, H, W = sp if len(sp) == 3 else (1,) + tuple(sp)
    return (N, C, D, H, W, K, k if len(sp) == 3 else 1, k, k, stride, pad)


def shapes():
    import conv2d_reference as c2
    import conv_fp32_reference as cf
    import patchgan_fp32_reference as pg
    from neuroclear_amd.util import seed as S
    rows = []
    for mod in (cf, pg):
        for op in (0, 1, 2):
            rows += [layer(*c[:7]) for c in mod.CASES[op]]
    rows += [layer(N, C, K, (H, W), 3, 1, 1) for N, C, K, H, W, _ in c2.K3_CASES + c2.K3_OUTSIDE]
    # the three models of the training step at the crops the benchmark and the smoke run use: unet_deconv (levels S, S / 2, S / 4),
    # deep_linear_gen (every layer at S; padding k / 2 and none) and the four 2-D PatchGANs, which see the crop's S slices as one batch of
    # S x S images (2 S with the fake and the real half joined, 4 S at --batch 4) or 1 .. 4 planes of it; N = 1 and 4 for the generators
    for S_ in (108, 140, 148, 16):
        for N in (1, 4):
            for key, sh in S.unet_deconv_spec():
                if key.endswith('.weight') and 't_conv' not in key:
                    e = S_ // (4 if 'bottom' in key else 2 if 'conv2' in key else 1)
                    rows.append(layer(N, sh[1], sh[0], (e, e, e), sh[2], 1, sh[2] // 2))
            for key, sh in S.deep_linear_spec():
                rows += [layer(N, sh[1], sh[0], (S_, S_, S_), sh[2], 1, p) for p in {0, sh[2] // 2}]
        for N in (1, 2, 3, 4, S_, 2 * S_, 4 * S_):
            e = S_
            spec = [sh for key, sh in S.patchgan_spec(2) if key.endswith('.weight')]
            for i, sh in enumerate(spec):
                stride = 2 if i < len(spec) - 2 else 1
                rows.append(layer(N, sh[1], sh[0], (e, e), 4, stride, 1))
                e = (e + 2 - 4) // stride + 1
    ch = (1, 2, 8, 16, 32, 64, 128)
    for nd, C, K, k, stride in itertools.product((2, 3), ch, ch, (1, 3, 4, 5, 7), (1, 2)):
        sp = (256, 256) if (nd, k) == (2, 1) else PROBE[nd]
        rows.append(layer(1, C, K, sp, k, stride, 1 if k == 4 else k // 2))   # (4: the PatchGAN's padding)
    return np.array(sorted(set(rows)), dtype=np.int64)


def load(path=None):
    L = ctypes.CDLL(path or os.environ.get('NC_HIP_LIB') or os.path.join(ROOT, 'neuroclear_amd', 'csrc', 'libnc_hip.so'))
    L.nc_conv_ws_bytes.restype = ctypes.c_size_t
    return L


def set_mode(L, m, base=(1, 1)):
    """Mode m over the switches as they were (base = nc_get_conv_split, nc_get_conv2d_k3); m = 0 puts them back."""
    L.nc_set_conv_split(0 if m == 1 else base[0])
    L.nc_set_force_direct(1 if m == 2 else 0)
    L.nc_set_conv2d_k3(0 if m == 3 else base[1])


def answers(L, sh):
    """[n, 4, 11]: COLUMNS of every shape under every mode; the switches are back at their defaults afterwards."""
    out = np.zeros((len(sh), len(MODES), len(COLUMNS)), dtype=np.int64)
    base = (L.nc_get_conv_split(), L.nc_get_conv2d_k3())
    try:
        L.nc_set_conv_split(1), L.nc_set_conv2d_k3(1)   # 'default' is the library's, whatever the environment set
        for m in range(len(MODES)):
            set_mode(L, m)
            for i, row in enumerate(sh.tolist()):
                N, C, D, H, W, K, kd, kh, kw, s, p = row
                out[i, m] = ([L.nc_conv_ws_bytes(N, C, D, H, W, K, kd, kh, kw, s, p), L.nc_conv_fwd_path(C, K, kd, kh, kw, s, p), L.nc_conv_wgrad_path(C, K, kd, kh, kw, s, p)] +
                             [L.nc_conv2d_k3_active(w, N, C, H, W, K) for w in (0, 1)] +
                             [L.nc_conv2d_split_active(w, N, C, H, W, K, kh, s, p) for w in (0, 1, 2)] +
                             [L.nc_conv_lp_supported(w, N, C, D, H, W, K, kd, kh, kw, s, p) for w in (0, 1, 2)])
    finally:
        set_mode(L, 0, base)
    return out


if __name__ == '__main__':
    sh = shapes()
    got = answers(load(), sh)
    if '--check' in sys.argv:
        want = np.load(OUT)
        assert np.array_equal(want['shapes'], sh), 'the grid changed'
        bad = np.argwhere(want['answers'] != got)
        print('%d shapes x %d modes x %d columns: %d differences' % (got.shape + (len(bad),)))
        for i, m, c in bad[:40]:
            print(sh[i].tolist(), MODES[m], COLUMNS[c], 'golden', want['answers'][i, m, c], 'now', got[i, m, c])
        sys.exit(1 if len(bad) else 0)
    np.savez_compressed(OUT, shapes=sh, modes=np.array(MODES), columns=np.array(COLUMNS), answers=got)
    print('%s: %d shapes, %d bytes' % (OUT, len(sh), os.path.getsize(OUT)))
