"""Dispatch rules and cases of the op-level tests of the PatchGAN discriminator's own 4 x 4 kernels: the image-staged kernels of
csrc/conv2d_img.hip (k_sconv forward and data gradient, k_swgrad weight gradient: api.hip's rung 7) and the first-layer kernels of
csrc/patchgan_edge.hip (C = 1, stride 2: rung 8).  tests/test_gpu_patchgan_fp32.py runs the cases; tests/test_patchgan_fp32_reference.py checks
this module on the CPU.  Nothing here calls the library.

Reference (float64 tap loops), yardstick (the one-accumulator fp32 chain), error measure and limit are tests/conv_fp32_reference.py's, imported
and not copied: rms <= FACTOR rms_chain + RMS_FLOOR and max <= FACTOR max_chain + MAX_FLOOR with FACTOR = 3, RMS_FLOOR = 2^-23, MAX_FLOOR = 2^-21.

The planners are restated below as pure functions of the layer, each naming its source.  A case is (N, C, K, (H, W), 4, stride, 1, mode, branch):
the branch states what the restated planner says the case reaches, and each case is the smallest layer found that reaches its branch with ragged
edges.  For k_sconv the floor is min_tiles = 192 workgroups: about 24 600 output columns x 64 channels, some 6 MB of output.

Not reached by any few-second case, and therefore absent instead of faked: k_swgrad with splits == 1 (the partial sums written straight into dw)
needs C / NCW * K / 128 >= 512 workgroups, i.e. C K >= 2^20 (1024 x 1024 channels)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_fp32_reference import (DGRAD, FACTOR, FWD, MAX_FLOOR, NO_SPLIT, RMS_FLOOR, WGRAD, case_id, cdiv, err, gemm_branch,  # noqa: E402,F401
                                 gemm_supported, inputs, make_dims, oracle_err, ratios, reference, within)  # noqa: F401

# ---- conv2d_img.hip: k_sconv ----------------------------------------------------------------------------------------------------------------
K_MAX_SEG = 4                 # conv2d_img.hip:38 kMaxSeg
MIN_TILES = 192               # conv2d_img.hip:273 min_tiles
LDS_CAP = 80 * 1024           # conv2d_img.hip:279 lds_cap
SCFGS = [(4, 2, 2), (8, 1, 1), (5, 2, 1), (6, 2, 1), (3, 2, 2), (4, 2, 1), (6, 1, 1), (5, 1, 1),
         (2, 2, 2), (4, 1, 2), (3, 1, 2), (2, 1, 2), (2, 2, 3), (2, 1, 3)]    # conv2d_img.hip:286 kSCfgs (WM, WN, VB)
CKS = (32, 16, 8, 4, 2)


def sconv_layer_ok(d):
    """conv2d_img.hip:435 sconv_layer_ok."""
    return (d.D == 1 and d.kd == 1 and d.kh == 4 and d.kw == 4 and d.ph == 1 and d.pw == 1 and d.sh == d.sw and d.sh in (1, 2) and
            d.N * d.C * d.H * d.W < 1 << 31 and d.N * d.K * d.Ho * d.Wo < 1 << 31)


def plan_one(g, B, C, M, Hu, Wu, si, rspan, Wp, nclass=1):
    """conv2d_img.hip:291 plan_one: the plan of one tile configuration g = (WM, WN, VB), or None where it does not apply."""
    WM, WN, VB = g
    if M % (WN * 64):
        return None
    NCT = WM * VB * 32
    HW = Hu * Wu
    if (NCT - 1) // HW + 2 > K_MAX_SEG:
        return None
    urows = cdiv(NCT, Wu) + 1
    nimg = (NCT - 1) // HW + 2
    rows = (urows - 1) * si + nimg * rspan + (nimg - 1) * si
    CS = cdiv(rows * Wp, 64) * 64
    for CK in CKS:
        if C % CK:
            continue
        nbytes = (64 + CS + 2 * CK * CS) * 4
        if nbytes > LDS_CAP:
            continue
        return dict(cfg=g, NCT=NCT, CK=CK, CS=CS, lds=nbytes, tiles=cdiv(B * HW, NCT) * (M // (64 * WN)) * nclass)
    return None


def plan_sconv(B, C, M, Hu, Wu, si, rspan, Wp, nclass=1):
    """conv2d_img.hip:314 plan_sconv: the heuristic choice -- how full the rounds of 256 workgroups are, times a mild preference for larger
    tiles; the first of equals wins."""
    best, best_eff = None, 0.0
    for g in SCFGS:
        pl = plan_one(g, B, C, M, Hu, Wu, si, rspan, Wp, nclass)
        if pl is None:
            continue
        eff = pl['tiles'] / (cdiv(pl['tiles'], 256) * 256) * (0.85 + 0.15 * (g[1] * pl['NCT']) / 512.0)
        if best is None or eff > best_eff:
            best, best_eff = pl, eff
    return best


def sconv_problem(op, d):
    """The arguments conv_fwd_sconv / conv_dgrad_sconv hand to run_tuned (conv2d_img.hip:753, 777, 802): (B, C, M, Hu, Wu, si, rspan, Wp, nclass)."""
    if op == FWD:
        return d.N, d.C, d.K, d.Ho, d.Wo, d.sh, 4, (d.Wo - 1) * d.sw + 4, 1
    if d.sh == 1:
        return d.N, d.K, d.C, d.H, d.W, 1, 4, d.W + 3, 1
    Hu, Wu = (d.H + 1) // 2, (d.W + 1) // 2
    return d.N, d.K, d.C, Hu, Wu, 1, 2, Wu + 1, 4


def sconv_supported(op, d):
    """conv2d_img.hip:714 sconv_fwd_supported and :721 sconv_dgrad_supported: the plan, or None."""
    red, out = (d.C, d.K) if op == FWD else (d.K, d.C)
    if not sconv_layer_ok(d) or red % 2 or red < 16 or out % 64:
        return None
    small = d.Ho * d.Wo if op == FWD else d.H * d.W if d.sh == 1 else (d.H // 2) * (d.W // 2)
    if small < 96:
        return None
    pl = plan_sconv(*sconv_problem(op, d))
    return pl if pl is not None and pl['tiles'] >= MIN_TILES else None


def sconv_fwd_supported(d):
    return sconv_supported(FWD, d) is not None


def sconv_dgrad_supported(d):
    return sconv_supported(DGRAD, d) is not None


def sconv_classes(op, d):
    """The output grids of a launch, (Hu, Wu) each: one, or the four parity classes (py, px) of a stride-2 data gradient
    (conv2d_img.hip:787-800): Hu = (H - py + 1) / 2, Wu = (W - px + 1) / 2."""
    if op == FWD:
        return [(d.Ho, d.Wo)]
    if d.sh == 1:
        return [(d.H, d.W)]
    return [((d.H - py + 1) // 2, (d.W - px + 1) // 2) for py in (0, 1) for px in (0, 1)]


def images_per_tile(B, Hu, Wu, NCT):
    """The most images a tile of NCT consecutive columns of the flat (image, u, v) axis touches (k_sconv's segment loop, conv2d_img.hip:101-121)."""
    HW, ncol = Hu * Wu, B * Hu * Wu
    return max(min(j0 + NCT - 1, ncol - 1) // HW - j0 // HW + 1 for j0 in range(0, ncol, NCT))


def sconv_facts(op, d, g=None):
    """What a case exercises under the heuristic plan (or under configuration g): the plan, the most images a tile touches over all classes, a
    ragged last tile in some class, classes of different sizes whose grid is cut short (the j0 >= ncol exit), staged rows wider than 64 floats."""
    prob = sconv_problem(op, d)
    pl = plan_sconv(*prob) if g is None else plan_one(g, *prob)
    cls = sconv_classes(op, d)
    ncols = [d.N * hu * wu for hu, wu in cls]
    return dict(plan=pl, images=max(images_per_tile(d.N, hu, wu, pl['NCT']) for hu, wu in cls),
                ragged=any(n % pl['NCT'] for n in ncols), early_exit=min(cdiv(n, pl['NCT']) for n in ncols) < cdiv(max(ncols), pl['NCT']),
                wide=prob[7] > 64)


def sconv_branch(op, d):
    pl = sconv_supported(op, d)
    f = sconv_facts(op, d)
    par = '/p%d%d' % (d.H % 2, d.W % 2) if op == DGRAD and d.sh == 2 else ''
    return 'sconv %s/s%d%s/CK%d/cfg(%d,%d,%d)/img%d' % (('fwd', 'dgrad')[op], d.sh, par, pl['CK'], *pl['cfg'], f['images'])


def applicable_cfgs(op, d):
    """The indices into kSCfgs nc_sconv_set_cfg may pin at a layer."""
    return [i for i, g in enumerate(SCFGS) if plan_one(g, *sconv_problem(op, d)) is not None]


# ---- conv2d_img.hip: k_swgrad ---------------------------------------------------------------------------------------------------------------
WNJ = 64                      # conv2d_img.hip:451 kWNJ: columns per stage = lanes per wave
WAP = WNJ + 1                 # conv2d_img.hip:452 kWAP
MINCOL = 4096                 # conv2d_img.hip:670 mincol


def swgrad_rows(d):
    """The input rows plan_swgrad sizes a stage of 64 columns for (conv2d_img.hip:634-635): at most two images' halos and one row step per
    started output row.  k_swgrad decodes them with ONE LANE PER ROW, so a plan exists only up to 64 of them (conv2d_img.hip:638)."""
    urows = cdiv(WNJ, d.Wo) + 1
    return (urows - 1) * d.sh + 2 * 4 + d.sh


def plan_swgrad(d, row_limit=WNJ):
    """conv2d_img.hip:626 plan_swgrad, or None.  row_limit = None: the planner as it was before it had the row limit (it then sized LDS for
    thin planes whose stages k_swgrad cannot decode: the module docstring of test_gpu_patchgan_fp32.py)."""
    s, HW = d.sh, d.Ho * d.Wo
    if HW < WNJ:
        return None
    Wp = (d.Wo - 1) * s + 4
    pitch = (Wp + 3) & ~3
    if pitch & 7 == 0:
        pitch += 4
    rows = swgrad_rows(d)
    if row_limit is not None and rows > row_limit:
        return None
    CS = rows * pitch + 16
    for NTW in (4, 2):
        NCW = 4 * NTW
        if d.C % NCW:
            continue
        nbytes = (128 + 128 * WAP + NCW * CS) * 4
        if nbytes > LDS_CAP:
            continue
        ngroups, mtiles = d.C // NCW, d.K // 128
        nst = cdiv(d.N * HW, WNJ)
        splits = min(cdiv(512, ngroups * mtiles), nst, 256)
        sps = cdiv(nst, splits)
        return dict(NTW=NTW, pitch=pitch, CS=CS, lds=nbytes, ngroups=ngroups, mtiles=mtiles, stages=nst, stages_per_split=sps,
                    splits=cdiv(nst, sps))
    return None


def sconv_wgrad_supported(d):
    """conv2d_img.hip:664 sconv_wgrad_supported."""
    if not sconv_layer_ok(d) or d.K % 128 or d.C % 8:
        return False
    if d.N * d.C * d.H * d.W >= 1 << 30 or d.N * d.K * d.Ho * d.Wo >= 1 << 30:
        return False
    return plan_swgrad(d) is not None and d.N * d.Ho * d.Wo >= MINCOL


def swgrad_facts(d):
    """The edges of k_swgrad a layer meets: 'ragged' = ncol no multiple of 64 (the last stage writes zero columns); 'short' = a last split of
    fewer stages than stages_per_split; '2img' = a stage that spans two images; 'wide' = input rows wider than one 64-lane copy (W >= 66);
    'xcd' = a grid that is a multiple of 8 (the XCD remap of the block index)."""
    w = plan_swgrad(d)
    HW, ncol = d.Ho * d.Wo, d.N * d.Ho * d.Wo
    out = []
    if ncol % WNJ:
        out.append('ragged')
    if w['stages'] % w['stages_per_split']:
        out.append('short')
    if any(js // HW != min(js + WNJ - 1, ncol - 1) // HW for js in range(0, ncol, WNJ)):
        out.append('2img')
    if d.W >= 66:
        out.append('wide')
    if (w['ngroups'] * w['mtiles'] * w['splits']) % 8 == 0:
        out.append('xcd')
    return out


def swgrad_branch(d):
    w = plan_swgrad(d)
    f = swgrad_facts(d)
    return 'swgrad<%d>/s%d/splits%d' % (w['NTW'], d.sh, w['splits']) + ('/' + '+'.join(f) if f else '')


# ---- patchgan_edge.hip ------------------------------------------------------------------------------------------------------------------------
PG1_MAX_K = 64                # patchgan_edge.hip:19 kMaxK
PG1_PIX, PG1_BLOCKS = 128, 512    # patchgan_edge.hip:69 kWgPix, kWgBlocks


def pg1_supported(d):
    """patchgan_edge.hip:289 pg1_supported."""
    return (d.C == 1 and d.D == 1 and d.kd == 1 and d.kh == 4 and d.kw == 4 and d.sh == 2 and d.sw == 2 and d.ph == 1 and d.pw == 1 and
            1 <= d.K <= PG1_MAX_K and d.N * d.K * d.Ho * d.Wo < 1 << 31)


def pg1_tiles(d):
    return cdiv(d.N * d.Ho * d.Wo, PG1_PIX)


def pg1_blocks(d):
    """patchgan_edge.hip:293 pg1_blocks: workgroups of k_pg1_wgrad; with more tiles than that a workgroup walks several."""
    return min(pg1_tiles(d), PG1_BLOCKS)


def pg1_dgrad_few(d):
    """patchgan_edge.hip:323-325 conv_dgrad_pg1: the few-planes kernel below 128 * 256 pixel blocks."""
    return d.N * cdiv(d.H, 2) * cdiv(d.W, 2) < 128 * 256


def pg1_branch(op, d):
    kk = '/K%d' % d.K
    if op == FWD:
        return 'pg1 fwd' + kk
    if op == DGRAD:
        return 'pg1 dgrad%s/p%d%d%s' % ('_few' if pg1_dgrad_few(d) else '', d.H % 2, d.W % 2, kk)
    return 'pg1 wgrad/%s%s%s' % ('walk' if pg1_tiles(d) > PG1_BLOCKS else 'one-tile', '/ragged' if d.N * d.Ho * d.Wo % PG1_PIX else '', kk)


# ---- the ladder ------------------------------------------------------------------------------------------------------------------------------
def p2d_may_take(op, d):
    """NECESSARY conditions of the two-term kernels' predicates (conv_p2d.hip:653 p2_shape: 64 | output channels, 16 | reduction channels;
    wgrad_p2d.hip:379 q_shape: stride 1, 32 | C, 64 | K), api.hip's rung 10 in front of 8 and 7 -- so False is certain.  Such a case runs under
    nc_set_conv_split(0); every other one under the default switches."""
    if op == WGRAD:
        return d.sh == 1 and d.C % 32 == 0 and d.K % 64 == 0
    red, out = (d.C, d.K) if op == FWD else (d.K, d.C)
    return out % 64 == 0 and red % 16 == 0


def dispatch(op, d):
    """(path, branch) of the rung api.hip's kRungs (conv_route) gives a 2-D 4 x 4 padding-1 layer with rung 10 out of the way
    (no other rung in front of 8 takes a 4 x 4 layer with K > 1): pg1 (8), the image-staged kernels (7), else the gather GEMM (2)."""
    assert d.D == 1 and d.kd == 1 and d.kh == 4 and d.kw == 4 and d.ph == 1 and d.K > 1
    if pg1_supported(d):
        return 8, pg1_branch(op, d)
    if op == WGRAD and sconv_wgrad_supported(d):
        return 7, swgrad_branch(d)
    if op != WGRAD and sconv_supported(op, d) is not None:
        return 7, sconv_branch(op, d)
    assert gemm_supported(op, d)
    return 2, gemm_branch(op, d)


def mode_of(op, layer):
    return NO_SPLIT if p2d_may_take(op, make_dims(*layer)) else None


# ---- the cases: (N, C, K, (H, W), 4, stride, 1, mode, branch) ---------------------------------------------------------------------------------
# mode: NO_SPLIT = under nc_set_conv_split(0), exactly where p2d_may_take() holds; None = the default switches.  branch: what dispatch() above says
# the case reaches.  k_sconv: 'sconv <op>/s<stride>[/p<H % 2><W % 2>]/CK<channels per chunk>/cfg(WM,WN,VB)/img<most images a tile touches>' under the
# HEURISTIC plan (nc_sconv_set_tune(0)); every case has a last tile of fewer than NCT columns, and in the stride-2 data gradients with an odd H or W
# the four classes differ in size, so blocks of the smaller ones leave at `j0 >= ncol`.  One image fewer falls below min_tiles
# (test_patchgan_fp32_reference.py).  CK = 32 has NO forward plan at any plane and tile (its 64 channel images of two buffers fit the 80 KiB only
# with CS <= 256 floats; the CPU file enumerates it): it is reached in the stride-2 data gradient, whose classes stage 2 rows per output row.
# k_swgrad: 'swgrad<NTW>/s<stride>/splits<n>/<edges of swgrad_facts>'.
FWD_CASES = [
    (56, 18, 64, (21, 23), 4, 1, 1, None, 'sconv fwd/s1/CK2/cfg(2,1,2)/img2'),
    (78, 20, 128, (27, 25), 4, 2, 1, None, 'sconv fwd/s2/CK4/cfg(2,1,2)/img2'),             # every configuration applies: CFG_CASES
    (171, 24, 64, (22, 26), 4, 2, 1, None, 'sconv fwd/s2/CK8/cfg(2,1,2)/img2'),
    (28, 32, 128, (23, 21), 4, 1, 1, NO_SPLIT, 'sconv fwd/s1/CK16/cfg(2,1,2)/img2'),        # the tuned case
    (223, 16, 64, (21, 23), 4, 2, 1, NO_SPLIT, 'sconv fwd/s2/CK8/cfg(2,1,2)/img3'),         # planes of 110 pixels
    (224, 16, 128, (21, 23), 4, 2, 1, NO_SPLIT, 'sconv fwd/s2/CK4/cfg(8,1,1)/img4'),        # ... under a 256-column tile: four images
    (10, 16, 128, (75, 70), 4, 2, 1, NO_SPLIT, 'sconv fwd/s2/CK4/cfg(2,1,2)/img2'),         # Wp = 72 > 64
    # patchgan_edge.hip k_pg1_fwd: three workgroups, the last one ragged; K < 64; K odd on the smallest legal plane (H = 2: ONE output row); W = 2
    (5, 1, 64, (21, 23), 4, 2, 1, None, 'pg1 fwd/K64'),
    (2, 1, 20, (13, 10), 4, 2, 1, None, 'pg1 fwd/K20'),
    (5, 1, 7, (2, 9), 4, 2, 1, None, 'pg1 fwd/K7'),
    (4, 1, 8, (11, 2), 4, 2, 1, None, 'pg1 fwd/K8'),
]

DGRAD_CASES = [
    (51, 64, 18, (21, 23), 4, 1, 1, None, 'sconv dgrad/s1/CK2/cfg(2,1,2)/img2'),            # DT = -1, one class
    (19, 128, 32, (27, 25), 4, 1, 1, NO_SPLIT, 'sconv dgrad/s1/CK16/cfg(2,1,2)/img2'),
    (47, 64, 18, (20, 26), 4, 2, 1, None, 'sconv dgrad/s2/p00/CK2/cfg(2,1,2)/img2'),        # four classes of one size
    (50, 64, 18, (22, 21), 4, 2, 1, None, 'sconv dgrad/s2/p01/CK2/cfg(2,1,2)/img3'),
    (50, 64, 16, (21, 22), 4, 2, 1, NO_SPLIT, 'sconv dgrad/s2/p10/CK16/cfg(2,1,2)/img3'),
    (17, 128, 20, (27, 25), 4, 2, 1, None, 'sconv dgrad/s2/p11/CK4/cfg(2,1,2)/img2'),       # every configuration applies: CFG_CASES
    (39, 64, 32, (23, 25), 4, 2, 1, NO_SPLIT, 'sconv dgrad/s2/p11/CK32/cfg(2,1,2)/img2'),
    (40, 64, 32, (22, 27), 4, 2, 1, NO_SPLIT, 'sconv dgrad/s2/p01/CK32/cfg(2,1,2)/img2'),
    # patchgan_edge.hip: k_pg1_dgrad_few below 128 * 256 pixel blocks (32767 here), k_pg1_dgrad from 32768 on
    (7, 1, 20, (61, 301), 4, 2, 1, None, 'pg1 dgrad_few/p11/K20'),                          # 7 x 31 x 151 = 32767; K / 8 leaves a remainder
    (2, 1, 8, (256, 256), 4, 2, 1, None, 'pg1 dgrad/p00/K8'),                               # 2 x 128 x 128 = 32768
    (3, 1, 64, (255, 257), 4, 2, 1, None, 'pg1 dgrad/p11/K64'),
    (2, 1, 20, (256, 257), 4, 2, 1, None, 'pg1 dgrad/p01/K20'),
    (2, 1, 64, (10, 12), 4, 2, 1, None, 'pg1 dgrad_few/p00/K64'),
    (3, 1, 7, (9, 12), 4, 2, 1, None, 'pg1 dgrad_few/p10/K7'),                              # fewer channels than channel groups
    (5, 1, 6, (2, 9), 4, 2, 1, None, 'pg1 dgrad_few/p01/K6'),                               # H = 2
    (4, 1, 8, (11, 2), 4, 2, 1, None, 'pg1 dgrad_few/p10/K8'),                              # W = 2
]

# every case also takes the bias gradient: rung 7 through bias_grad in a second launch, rung 8 as the 17th column of the same product
WGRAD_CASES = [
    (10, 16, 128, (21, 23), 4, 1, 1, None, 'swgrad<4>/s1/splits69/ragged+2img'),            # a grid of 69 workgroups: no XCD remap
    (10, 32, 128, (21, 23), 4, 1, 1, NO_SPLIT, 'swgrad<4>/s1/splits69/ragged+2img'),        # two channel groups
    (4, 16, 256, (23, 66), 4, 1, 1, None, 'swgrad<4>/s1/splits90/ragged+2img+wide'),        # rows of 68 dwords: two copies per row
    (8, 8, 128, (25, 23), 4, 1, 1, None, 'swgrad<2>/s1/splits66/2img'),                     # C = 8; 4224 columns = 66 whole stages
    (33, 8, 128, (25, 23), 4, 2, 1, None, 'swgrad<2>/s2/splits69/ragged+2img'),
    (31, 24, 256, (9, 70), 4, 2, 1, None, 'swgrad<2>/s2/splits68/ragged+2img+wide+xcd'),    # C = 24, K = 256, W = 70
    (20, 64, 256, (29, 31), 4, 2, 1, None, 'swgrad<4>/s2/splits33/ragged+2img+xcd'),        # two stages per split
    (21, 64, 256, (29, 31), 4, 2, 1, None, 'swgrad<4>/s2/splits35/ragged+short+2img+xcd'),  # ... and a last split of one
    # the thin planes: an output width of 2 under stride 2 and of 1 under stride 1 -- 66 .. 70 and 67 input rows per stage of 64 columns, more
    # than k_swgrad's 64 lanes decode: plan_swgrad's row limit leaves them to the gather GEMM (they pass mincol and fit LDS with NTW = 2)
    (32, 8, 128, (130, 4), 4, 2, 1, None, 'G_WGRAD/64/split-v4'),
    (32, 8, 128, (130, 5), 4, 2, 1, None, 'G_WGRAD/64/split-v4'),
    (64, 8, 128, (65, 2), 4, 1, 1, None, 'G_WGRAD/64/split-v4'),
    # patchgan_edge.hip k_pg1_wgrad: 'walk' = more tiles of 128 pixels than the 512 workgroups (524 here), 'one-tile' = fewer
    (3, 1, 64, (301, 299), 4, 2, 1, None, 'pg1 wgrad/walk/ragged/K64'),
    (3, 1, 20, (21, 23), 4, 2, 1, None, 'pg1 wgrad/one-tile/ragged/K20'),
    (2, 1, 7, (17, 19), 4, 2, 1, None, 'pg1 wgrad/one-tile/ragged/K7'),
    (4, 1, 8, (16, 16), 4, 2, 1, None, 'pg1 wgrad/one-tile/K8'),                            # 256 pixels: two whole tiles
    (5, 1, 6, (2, 9), 4, 2, 1, None, 'pg1 wgrad/one-tile/ragged/K6'),                       # H = 2
    (4, 1, 8, (11, 2), 4, 2, 1, None, 'pg1 wgrad/one-tile/ragged/K8'),                      # W = 2
]
THIN_PLANES = [c for c in WGRAD_CASES if min(c[3]) <= 5 and c[1] > 1]

CASES = {FWD: FWD_CASES, DGRAD: DGRAD_CASES, WGRAD: WGRAD_CASES}


def first_case(op, branch):
    return next(c for c in CASES[op] if c[8] == branch)


# every tile configuration applies: pinned one by one with nc_sconv_set_cfg, each against float64 and all bit-equal
CFG_CASES = [(FWD, first_case(FWD, 'sconv fwd/s2/CK4/cfg(2,1,2)/img2')), (DGRAD, first_case(DGRAD, 'sconv dgrad/s2/p11/CK4/cfg(2,1,2)/img2'))]
# tuning on (nc_sconv_set_tune(1)): the bits of the heuristic run
TUNED_CASE = (FWD, first_case(FWD, 'sconv fwd/s1/CK16/cfg(2,1,2)/img2'))
# the size check stands in front of every launch (conv2d_img.hip conv_fwd_sconv / conv_dgrad_sconv / conv_wgrad_sconv, patchgan_edge.hip
# conv_wgrad_pg1; k_pg1_fwd and the pg1 data gradients use no workspace)
UNDERSIZED = [(FWD, FWD_CASES[0], 256), (DGRAD, DGRAD_CASES[0], 256), (DGRAD, DGRAD_CASES[2], 256), (WGRAD, WGRAD_CASES[0], 256),
              (WGRAD, first_case(WGRAD, 'pg1 wgrad/one-tile/ragged/K20'), 256)]
# C = 1 with K = 65 leaves rung 8 (kMaxK = 64) for the gather GEMM
K65 = [(FWD, (3, 1, 65, (9, 11), 4, 2, 1, None, 'G_FWD/64/one')), (DGRAD, (3, 1, 65, (9, 11), 4, 2, 1, None, 'G_DGRAD_P/64/split-scalar/padded')),
       (WGRAD, (3, 1, 65, (9, 11), 4, 2, 1, None, 'G_WGRAD/64/one'))]
# a padded extent below the kernel: common.hpp make_dims refuses (N, C, K, H, W, stride)
REFUSED = [(3, 16, 64, 1, 9, 2), (3, 16, 64, 9, 1, 1), (3, 1, 8, 1, 9, 2), (3, 1, 8, 9, 1, 2)]
