"""The host-side planning of csrc/dl_bnd.hip (the boundary kernels of deep_linear_gen's position-typed path that redo dl_typed.hip's arithmetic
in the same order) restated in pure Python, and the shapes tests/test_gpu_dl_bnd.py runs.  Nothing here calls the library;
tests/test_dl_bnd_plan.py checks the constants against the source text and the plan against a brute-force walk of the volume.

dl_bnd.hip has kernels for TWO of the three boundary pieces: dL/dact0 (piece 1) and, of the type sums (piece 2), the R set's; the forward (0)
and the X set's sums run dl_typed.hip's.
Constants of dl_bnd.hip:
    REACH = 3           a 7^3 window reaches three voxels
    ROW_LANES = 64      outputs of a block along its line (x for k_dlb_dgrad_rows, y for k_dlb_dgrad_xf)
    LINE_PITCH = 70     a staged source line: ROW_LANES + 2 REACH
    ROW_SRC_MAX = 13    source rows of the R set one output row can reach (the LDS of k_dlb_dgrad_rows)
    XF_CH = 4           channels a thread of k_dlb_dgrad_xf owns; XF_GROUPS = 64 / XF_CH / 4 blocks of four waves per (uz, side, segment)
    GRP = 4             rows of a face a block of k_dlb_wgrad_rows owns
    PITCH_B = 193       its LDS line pitch; STAGE_SEG = 3 segments of 64 lanes per line (W <= 192), STAGE_CH = 10 channels per wave and line"""
import deep_linear_reference as R

REACH, ROW_LANES, LINE_PITCH, ROW_SRC_MAX, XF_CH, XF_GROUPS = 3, 64, 70, 13, 4, 4
PIECES = {'forward': 0, 'dgrad': 1, 'sums': 2}
GRP, PITCH_B, STAGE_SEG, STAGE_CH = 4, 193, 3, 10
NEW_PIECES = (1, 2)   # the pieces dl_bnd.hip has kernels for


def supported(N, D, H, W):
    """the shapes dl_bnd.hip's two pieces take: every shape dl_typed_supported admits"""
    return R.dl_typed_supported(N, D, H, W)


def variant(piece, N, D, H, W):
    """dl_bnd_variant"""
    return 1 if piece in NEW_PIECES and supported(N, D, H, W) else 0


def n_reach_rows(D, H):
    return 8 * H + 8 * (D - 8)


def reach_decode(i, D, H):
    """reach_decode of dl_bnd.hip: launch index -> output row (uz, uy)"""
    if i < 8 * H:
        p = i // H
        return (p if p < 4 else D - 8 + p), i - p * H
    j = i - 8 * H
    r = j & 7
    return 4 + (j >> 3), (r if r < 4 else H - 8 + r)


def in_reach(uz, uy, D, H):
    """the rows dl_typed.hip's k_dl_bnd_dgrad<false> does not leave at once"""
    return uz <= 3 or uz >= D - 4 or uy <= 3 or uy >= H - 4


def axis_type(c, L):
    return 0 if c == 0 else 2 if c == L - 1 else 1


def source_rows(uz, uy, D, H):
    """the rows (vz, vy) of the R set an output row reads, in the order of the walk (dz, dy ascending): [(dz, dy, tau)]"""
    out = []
    for dz in range(7):
        vz = uz - dz + 3
        if not 0 <= vz < D:
            continue
        for dy in range(7):
            vy = uy - dy + 3
            if not 0 <= vy < H:
                continue
            tz, ty = axis_type(vz, D), axis_type(vy, H)
            if tz == 1 and ty == 1:
                continue
            out.append((dz, dy, (tz * 3 + ty) * 3 + 1))
    return out


def rows_grid(N, D, H, W):
    return n_reach_rows(D, H), R.cdiv(W, ROW_LANES), N


def xf_grid(N, D, H, W):
    return D, 2 * XF_GROUPS, N * R.cdiv(H, ROW_LANES)


def xf_decode(by, wave):
    """blockIdx.y and the wave of k_dlb_dgrad_xf -> (side, first channel)"""
    return by & 1, ((by >> 1) * 4 + wave) * XF_CH


def n_bnd_rows(D, H):
    """dl_typed.hip:115"""
    return 2 * H + 2 * (D - 2)


def row_decode(r, D, H):
    """dl_typed.hip's row_decode: row number of the R set -> (z, y)"""
    if r < H:
        return 0, r
    if r < 2 * H:
        return D - 1, r - H
    k = r - 2 * H
    return 1 + (k >> 1), (H - 1 if k & 1 else 0)


def wgrad_grid(N, D, H, W):
    return 2 * R.cdiv(H, GRP) + 2 * R.cdiv(D - 2, GRP), 7, N


def wgrad_block(bx, tapf, D, H):
    """What block (bx, tapf) of k_dlb_wgrad_rows does: ([(r, d7, (zz, y2))] -- the row r of R, the tap pair d7 = dz * 7 + dy and the line of act0 it
    correlates with --, [(r, d7)] it writes as zero, the lines it stages in order)"""
    ngz, ngy = R.cdiv(H, GRP), R.cdiv(D - 2, GRP)
    zf = bx < 2 * ngz
    if zf:
        face = bx // ngz
        p0 = (bx - face * ngz) * GRP
        cnt, Lg = min(GRP, H - p0), H
        fixed, fixedL = (D - 1 if face else 0), D
        r0, rstep = face * H, 1
    else:
        g2 = bx - 2 * ngz
        face = g2 // ngy
        p0 = 1 + (g2 - face * ngy) * GRP
        cnt, Lg = min(GRP, D - 1 - p0), D
        fixed, fixedL = (H - 1 if face else 0), H
        r0, rstep = 2 * H - 2 + face, 2
    assert cnt >= 1
    fl = fixed + tapf - 3
    fixed_in = 0 <= fl < fixedL
    d7 = (lambda g: tapf * 7 + g) if zf else (lambda g: g * 7 + tapf)
    zeros = [(r0 + rstep * (p0 + f), d7(g)) for f in range(cnt) for g in range(7) if not fixed_in or not 0 <= p0 + f + g - 3 < Lg]
    work, staged = [], []
    if fixed_in:
        for t in range(max(p0 - 3, 0), min(p0 + cnt + 2, Lg - 1) + 1):
            staged.append((fl, t) if zf else (t, fl))
            glo, ghi = max(t + 4 - p0 - cnt, 0), min(t + 3 - p0, 6)
            assert 1 <= ghi - glo + 1 <= GRP
            for g in range(glo, ghi + 1):
                pos = t + 3 - g
                assert p0 <= pos < p0 + cnt
                work.append((r0 + rstep * pos, d7(g), staged[-1]))
    return work, zeros, staged


# The cases at dl_bnd.hip's own index boundaries, every extent the smallest with the property (dl_typed.hip's are R.TYPED_CASES A .. I: 58- and
# 64-wide segments, H = 130 and 192, W = 176, N = 2 and 3).  The branches of reach_decode, and the groups of GRP rows: H and D - 2 with
# remainder 0, 1 and GRP - 1 (A .. I have H % 4 in {0, 1}, (D - 2) % 4 in {0, 2, 3}); no face has fewer than GRP lines (H >= 8, D - 2 >= 6).
OWN_CASES = {
    'J': ((2, 1, 9, 8, 16), 'D = 9: ONE plane between the two sets of four (the second branch of reach_decode, eight rows); H = 8: its rows r < 4 and '
                            'r >= 4 meet; batch 2'),
    'K': ((2, 1, 12, 16, 16), 'D = 12, H = 16: four planes between with eight rows each OUT of reach -- untouched by the rows kernel; batch 2'),
    'M': ((2, 1, 11, 11, 16), 'H % GRP = GRP - 1, (D - 2) % GRP = 1: a last group of three rows and one of a single plane; batch 2'),
    'N': ((2, 1, 10, 15, 16), '(D - 2) % GRP = 0 with H % GRP = GRP - 1; batch 2'),
    'L': ((1, 1, 8, 9, 68), 'D = 8: no plane between (n_reach_rows = 8 H); odd H; W = 68: a second x segment of four lanes'),
}
CASES = dict({k: v[0] for k, v in R.TYPED_CASES.items()}, **{k: v[0] for k, v in OWN_CASES.items()})
