"""Cases, reference and yardstick of the position-typed evaluation of deep_linear_gen (csrc/dl_typed.hip, nc_set_dl_collapse(2)), type by type
(tests/test_gpu_deep_linear_types.py; checked on the CPU by tests/test_deep_linear_reference.py).  Nothing here calls the library.

REFERENCE: oracle/nets.py::deep_linear on the CPU in float64 -- y, and dx and the six weight gradients of (y * r).sum().
YARDSTICK ("fp32 oracle", as in tests/test_gpu_grad_fp64.py): the same function in float32, measured against the float64 run.
WEIGHTS: S.weights_from_seed(S.deep_linear_spec(), 32), the seed of tests/test_gpu_nets.py's deep_linear tests; x and r uniform in
[-0.5, 0.5) from fixed seeds (X_SEED, R_SEED).

POSITION TYPES, numbered as dl_typed.hip does (axis_type, :27): per axis 0 = on the low face, 1 = inside, 2 = on the high face,
tau = (tz * 3 + ty) * 3 + tx, 13 = interior.  The forward is judged per type (per_type_error: a corner type is 8 voxels of a volume and drowns
in any global norm); the backward with dy = r restricted to one type (the 27 one-type masks) or to one kernel family (GROUP_MASKS: R = the
boundary rows, types with tx == 1, lanes along x; X = the x faces, tx != 1, lanes along y through the transposed copies; the interior).

run_uncorrected is the WRONG evaluation the yardstick must tell from the right one: the interior kernel everywhere, i.e. what the product
would return if its boundary kernels did nothing (tests/test_deep_linear_reference.py holds it 100 x beyond the limits).

CASES.  Constants of dl_typed.hip the properties are computed from (restated here, checked against the source text by the CPU test):
    K_SEG = 58        voxels a wave of k_dl_bnd_fwd owns along its line (:128); lines are x = 1 .. W - 2 (rows) and y = 1 .. H - 2 (x faces)
    LANES = 64        outputs per segment of k_dl_bnd_dgrad along x (rows, :244) and along y (x faces, :275; nseg = cdiv(H, 64), :506)
    Y_LOOP = 128      threads of k_dl_gather_x, which walks y in steps of 128 (:96, :103)
    K_PITCH = 193     LDS line pitch of k_dl_bnd_wgrad (:346), dyr[192] behind it: extents up to 192
    dl_typed_supported (:473-475): N >= 1, D, H, W >= 8, H <= 192, W <= 192, W % 4 == 0
The typed form also needs the one-channel 7^3 weight gradient k_wgrad_c1 (c1w_plan, conv_c1.hip:582-598), which wants W % 4 == 0, W >= 16 and
its dY slab in at most 48 pieces of 256 floats: 64 * PAr <= 12288 with PAr = round_up(W, 16) + 8, i.e. W <= 176 (c1_wgrad_admits below).  So
W = 8, W = 12 and W = 180 .. 192 pass dl_typed_supported and still run as nc_set_dl_collapse(1): the cases that named such a width moved to the
nearest admitted one (W = 16; W = 176) and the named widths are held to the same limits in the fallback arm."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from neuroclear_amd.util import seed as S
from oracle import nets as onets

W_SEED, X_SEED, R_SEED = 32, 41, 42
K_SEG, LANES, Y_LOOP, K_PITCH = 58, 64, 128, 193
EXT_MIN, EXT_MAX = 8, 192
C1W_W_MIN, C1W_W_MAX = 16, 176
INTERIOR = 13
FACTOR, GRAD_FLOOR = 3.0, 2e-5   # tests/test_gpu_grad_fp64.py's rule: err <= 3 x the fp32 oracle's own + 2e-5
FWD_CAP = 1e-5                   # what test_deep_linear_collapsed_tail_equals_the_layered_chain grants these forms, of the output scale


def cdiv(a, b):
    return (a + b - 1) // b


def dl_typed_supported(N, D, H, W):
    """dl_typed.hip:473-475"""
    return N >= 1 and min(D, H, W) >= EXT_MIN and H <= EXT_MAX and W <= EXT_MAX and W % 4 == 0


def c1_wgrad_admits(W):
    """c1w_plan, conv_c1.hip:585-597, for the 7^3 kernel: W % 4 == 0, W >= 16, and the three fits (dY slab pieces, X ring pieces, LDS bytes)"""
    if W % 4 or W < 16:
        return False
    w16 = (W + 15) & ~15
    pa = (w16 + 7) & ~7
    if not pa & 8:
        pa += 8
    sd = (64 * pa + 255) & ~255
    prx = (4 + w16 + 7 + 2 + 31) & ~31
    lds = (8 * 8 * prx + 2 * sd) * 4
    return lds <= 160 * 1024 and sd // 256 <= 48 and 8 * prx // 256 <= 8


def typed_expected(N, D, H, W):
    """what the two-term forward of nc_set_dl_collapse(2) is expected to choose (the GPU test asserts the forward's own word, bit 29 of `kept`)"""
    return dl_typed_supported(N, D, H, W) and c1_wgrad_admits(W)


# name: (shape (N, 1, D, H, W), what it is there for).  The typed arm: bit 29 of `kept` must be set.
TYPED_CASES = {
    # (issue: 1,1,8,8,8 -- W = 8 is not admitted by k_wgrad_c1; D and H keep the property, W is the smallest the typed form takes)
    'A': ((1, 1, 8, 8, 16), 'D and H at the minimum: every voxel within three of both faces on z and y; W at the typed form\'s minimum'),
    'B': ((2, 1, 8, 12, 16), 'batch 2, three different extents (an axis swap shows)'),
    # (issue: 3,1,8,9,12 -- W = 12 is not admitted)
    'C': ((3, 1, 8, 9, 16), 'batch 3, odd H, partB\'s slot stride (gridDim.z)'),
    'D': ((1, 1, 8, 60, 60), 'H - 2 = W - 2 = 58: exactly one full forward segment'),
    'E': ((1, 1, 9, 61, 64), 'H - 2 = 59: a second y segment of one voxel; W - 2 = 62: two x segments; W = 64: exactly one 64-lane '
                             'data-gradient segment'),
    'F': ((1, 1, 10, 65, 68), 'H = 65: nseg = 2 with one live lane; W = 68: a second row segment of four lanes'),
    # (issue: 1,1,8,130,12 -- W = 12 is not admitted)
    'G': ((1, 1, 8, 130, 16), 'H > 128: second trip of k_dl_gather_x, nseg = 3'),
    # (issue: 1,1,8,192,8 -- W = 8 is not admitted)
    'H': ((1, 1, 8, 192, 16), 'the limit of H (LDS pitch 193, dyr[192])'),
    # (issue: 1,1,8,8,192 -- k_wgrad_c1 takes W <= 176)
    'I': ((1, 1, 8, 8, 176), 'the largest W the typed form takes'),
}
# The fallback arm: bit 29 must be clear.  terms: the setting of nc_set_split_terms
FALLBACK_CASES = {
    'below8': ((1, 1, 7, 9, 12), 2, 'an extent below 8'),
    'w_mod4': ((2, 1, 9, 14, 21), 2, 'W % 4 != 0'),
    'w196': ((1, 1, 8, 8, 196), 2, 'W > 192'),
    'B_terms3': ((2, 1, 8, 12, 16), 3, 'case B under nc_set_split_terms(3)'),
    # the widths the typed cases had to leave: dl_typed_supported admits them, k_wgrad_c1 does not
    'w8': ((1, 1, 8, 8, 8), 2, 'every extent at 8: admitted by dl_typed_supported, W < 16 refused by k_wgrad_c1'),
    'w12': ((3, 1, 8, 9, 12), 2, 'W = 12: the same'),
    'w192': ((1, 1, 8, 8, 192), 2, 'W = 192, the limit of dl_typed_supported: above k_wgrad_c1\'s 176'),
}
ALL_CASES = dict({k: (v[0], 2, v[1]) for k, v in TYPED_CASES.items()}, **FALLBACK_CASES)


def position_types(D, H, W):
    """int array [D, H, W] of the 27 types, (tz * 3 + ty) * 3 + tx"""
    def ax(L):
        t = np.ones(L, np.int64)
        t[L - 1] = 2
        t[0] = 0   # (in this order: axis_type asks coord == 0 first)
        return t
    tz, ty, tx = ax(D), ax(H), ax(W)
    return (tz[:, None, None] * 3 + ty[None, :, None]) * 3 + tx[None, None, :]


def type_count(tau, D, H, W):
    """closed form: an axis has one voxel of type 0, one of type 2 and L - 2 inside"""
    n = 1
    for t, L in zip((tau // 9, (tau // 3) % 3, tau % 3), (D, H, W)):
        n *= L - 2 if t == 1 else 1
    return n


def one_type_masks(D, H, W):
    """{tau: bool [D, H, W]}"""
    t = position_types(D, H, W)
    return {tau: t == tau for tau in range(27)}


GROUP_MASKS = ('R', 'X', 'interior')


def group_masks(D, H, W):
    """R: the boundary types with tx == 1 (the row kernels); X: tx != 1 (k_dl_gather_x and the XF kernels); the interior"""
    t = position_types(D, H, W)
    return {'R': (t % 3 == 1) & (t != INTERIOR), 'X': t % 3 != 1, 'interior': t == INTERIOR}


def mask_of(name, D, H, W):
    """name: None (all ones), 'R' / 'X' / 'interior', or a type number"""
    if name is None:
        return np.ones((D, H, W), bool)
    if name in GROUP_MASKS:
        return group_masks(D, H, W)[name]
    return position_types(D, H, W) == int(name)


@functools.lru_cache(maxsize=None)
def weights():
    return S.weights_from_seed(S.deep_linear_spec(), W_SEED)


def inputs(shape, mask=None):
    """x, r (float32 ndarrays), r times the mask"""
    x = np.random.default_rng(X_SEED).random(shape, dtype=np.float32) - np.float32(0.5)
    r = np.random.default_rng(R_SEED).random(shape, dtype=np.float32) - np.float32(0.5)
    return x, r * mask_of(mask, *shape[2:]).astype(np.float32)


def leaves(sd_np, x_np, dtype):
    sd = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in sd_np.items()}
    return sd, torch.from_numpy(x_np).to(dtype).requires_grad_(True)


def grads(y, x, sd, r_np):
    g = torch.autograd.grad(y, [x] + list(sd.values()), torch.from_numpy(r_np).to(y.dtype), retain_graph=True)
    return g[0], dict(zip(sd.keys(), g[1:]))


def run_oracle(sd_np, x_np, r_np, dtype):
    """y, dx and {key: weight gradient} of (y * r).sum() through oracle.nets.deep_linear on the CPU"""
    sd, x = leaves(sd_np, x_np, dtype)
    y = onets.deep_linear(sd, x)
    dx, g = grads(y, x, sd, r_np)
    return y.detach(), dx, g


def uncorrected_forward(sd, x):
    a = F.conv3d(x, sd['first_layer.weight'], padding=3)
    a = F.conv3d(a, sd['feature_block.0.weight'], padding=3)
    a = F.conv3d(a, sd['feature_block.1.weight'], padding=0)
    a = F.conv3d(a, sd['feature_block.2.weight'])
    a = F.conv3d(a, sd['feature_block.3.weight'])
    return F.conv3d(a, sd['final_layer.weight'])


def run_uncorrected(sd_np, x_np, r_np, dtype=torch.float64):
    """The same chain with act1 NOT zero-padded: layer 1 with padding 3 (act1 one voxel beyond the volume on every side, from the zero-padded
    act0), then the 3^3 layer with padding 0 -- the interior kernel H_13 at every voxel."""
    sd, x = leaves(sd_np, x_np, dtype)
    y = uncorrected_forward(sd, x)
    dx, g = grads(y, x, sd, r_np)
    return y.detach(), dx, g


def per_type_error(a, y64, types):
    """[27]: per type the maximum over its voxels and the samples of |a - y64|, over max |y64|.  a, y64: [N, 1, D, H, W] tensors or arrays"""
    a = np.asarray(torch.as_tensor(a).detach().cpu().double())
    y = np.asarray(torch.as_tensor(y64).detach().cpu().double())
    e = np.abs(a - y)[:, 0] / np.abs(y).max()
    return np.array([e[:, types == tau].max() if (types == tau).any() else 0.0 for tau in range(27)])


def rel(a, b):
    """relative L2 of a against b (tests/test_gpu_grad_fp64.py's)"""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- the oracle runs, shared: one forward graph per (shape, dtype), one backward per mask
_GRAPH, _RUNS = {}, {}


def _graph(shape, dtype):
    key = (tuple(shape), dtype)
    if key not in _GRAPH:
        sd, x = leaves(weights(), inputs(shape)[0], dtype)
        _GRAPH[key] = (sd, x, onets.deep_linear(sd, x))
    return _GRAPH[key]


def oracle(shape, mask=None):
    """((y64, dx64, g64), (y32, dx32, g32)) for r times `mask`; cached -- callers leave the tensors unchanged"""
    key = (tuple(shape), mask)
    if key not in _RUNS:
        r = inputs(shape, mask)[1]
        out = []
        for dtype in (torch.float64, torch.float32):
            sd, x, y = _graph(shape, dtype)
            dx, g = grads(y, x, sd, r)
            out.append((y.detach(), dx, g))
        _RUNS[key] = tuple(out)
    return _RUNS[key]


def clear():
    """drop the shared oracle runs and their autograd graphs (some hundred MB of host memory per large case): the test modules call it when
    they are done, so that nothing of theirs stays behind for the rest of the session"""
    _GRAPH.clear()
    _RUNS.clear()
