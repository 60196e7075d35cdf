"""CPU: the host-side planning of csrc/dl_bnd.hip, restated in tests/dl_bnd_plan.py -- its constants are the source's, the launch of
k_dlb_dgrad_rows covers every output row within reach of a source row exactly once and no other, no output row reads more source rows than the
kernel's LDS holds, every staged position lies inside its line, the x-face launch covers every (side, channel) exactly once, and the row groups of
k_dlb_wgrad_rows write every (row, dz, dy) exactly once from the line dl_typed.hip stages for it -- for every
shape tests/test_gpu_dl_bnd.py runs and the extents around the branches of reach_decode."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deep_linear_reference as R  # noqa: E402
import dl_bnd_plan as B  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'neuroclear_amd', 'csrc')
SHAPES = sorted(set(B.CASES.values()) | {(1, 1, D, H, 16) for D in (8, 9, 11, 12, 13) for H in (8, 9, 15, 16, 17)} | {(1, 1, 108, 108, 108)})


def test_restated_constants_are_the_sources():
    s = open(os.path.join(CSRC, 'dl_bnd.hip')).read()
    assert 'constexpr int kReach = %d;' % B.REACH in s
    assert 'constexpr int kRowLanes = %d;' % B.ROW_LANES in s
    assert 'constexpr int kLinePitch = kRowLanes + 2 * kReach;' in s and B.LINE_PITCH == B.ROW_LANES + 2 * B.REACH
    assert 'constexpr int kRowSrcMax = %d;' % B.ROW_SRC_MAX in s
    assert 'constexpr int kXfCh = %d;' % B.XF_CH in s
    assert 'constexpr int kXfGroups = kC / kXfCh / 4;' in s and B.XF_GROUPS == 64 // B.XF_CH // 4
    assert '__host__ inline int n_reach_rows(int D, int H) { return 8 * H + 8 * (D - 8); }' in s
    assert 'if (i < 8 * H) { const int p = i / H; uz = p < 4 ? p : D - 8 + p; uy = i - p * H; }' in s
    assert 'else { const int j = i - 8 * H, r = j & 7; uz = 4 + (j >> 3); uy = r < 4 ? r : H - 8 + r; }' in s
    assert 'int dl_bnd_variant(int piece, int N, int D, int H, int W) { return (piece == 1 || piece == 2) && dl_typed_supported(N, D, H, W) ? 1 : 0; }' in s
    assert 'constexpr int kGrp = %d;' % B.GRP in s and 'constexpr int kPitchB = %d;' % B.PITCH_B in s
    assert 'constexpr int kStageCh = %d;' % B.STAGE_CH in s and 'constexpr int kStageSeg = %d;' % B.STAGE_SEG in s
    assert B.STAGE_SEG * 64 >= R.EXT_MAX and B.PITCH_B > R.EXT_MAX and 7 * B.STAGE_CH >= 64   # a line of the widest shape, all 64 channels
    assert 'const int ngz = (int)cdiv(H, kGrp), ngy = (int)cdiv(D - 2, kGrp);' in s
    assert 'dim3((unsigned)(2 * ngz + 2 * ngy), 7, (unsigned)N), dim3(448)' in s
    assert 'const int glo = t + 4 - p0 - cnt > 0 ? t + 4 - p0 - cnt : 0, ghi = t + 3 - p0 < 6 ? t + 3 - p0 : 6;' in s
    assert 'const int t0 = p0 - 3 > 0 ? p0 - 3 : 0, t1 = p0 + cnt + 2 < Lg - 1 ? p0 + cnt + 2 : Lg - 1;' in s
    assert 'r0 = face * H; rstep = 1; d0 = tapf * 49 + k; dstep = 7;' in s and 'r0 = 2 * H - 2 + face; rstep = 2; d0 = tapf * 7 + k; dstep = 49;' in s
    assert 'dim3((unsigned)n_reach_rows(D, H), (unsigned)cdiv(W, kRowLanes), (unsigned)N), dim3(256)' in s
    assert 'dim3((unsigned)D, 2 * kXfGroups, (unsigned)(N * nseg)), dim3(256)' in s
    assert 'const int nseg = (int)cdiv(H, kRowLanes);' in s
    # the parent's kernels stay the other arm of the one branch in dl_typed.hip
    t = open(os.path.join(CSRC, 'dl_typed.hip')).read()
    assert 'if (variant < 0 ? dl_bnd_variant(1, N, D, H, W) == 1 : variant == 1) {' in t
    assert 'if (variant < 0 ? dl_bnd_variant(2, N, D, H, W) == 1 : variant == 1) {' in t
    assert t.count('hipLaunchKernelGGL(k_dl_bnd_wgrad<false>') == 1 and t.count('hipLaunchKernelGGL(k_dl_bnd_wgrad<true>') == 1
    assert t.count('hipLaunchKernelGGL(k_dl_bnd_dgrad<false>') == 1 and t.count('hipLaunchKernelGGL(k_dl_bnd_dgrad<true>') == 1
    assert ' dl_bnd.hip ' in open(os.path.join(CSRC, 'Makefile')).read()


def test_cases_are_typed_and_take_the_new_kernels():
    assert set(R.TYPED_CASES) < set(B.CASES) and len(B.CASES) == len(R.TYPED_CASES) + len(B.OWN_CASES)
    for k, (N, _, D, H, W) in B.CASES.items():
        assert R.typed_expected(N, D, H, W), k
        assert [B.variant(p, N, D, H, W) for p in range(3)] == [0, 1, 1], k
    assert B.variant(1, 1, 8, 8, 18) == 0 and B.variant(1, 1, 7, 8, 16) == 0 and B.variant(1, 1, 8, 196, 16) == 0
    # what the own cases are there for
    J, K, L = (B.CASES[k] for k in 'JKL')
    assert J[2] - 8 == 1 and J[3] == 8 and J[0] == 2
    assert K[2] - 8 == 4 and K[3] - 8 == 8 and K[0] == 2
    rem = {(H % B.GRP, (D - 2) % B.GRP) for _, _, D, H, _ in B.CASES.values()}
    assert {h for h, _ in rem} >= {0, 1, B.GRP - 1} and {d for _, d in rem} >= {0, 1, B.GRP - 1}
    assert any(N == 2 and H % B.GRP == B.GRP - 1 for N, _, D, H, _ in B.CASES.values())
    assert any(N == 2 and (D - 2) % B.GRP == 1 for N, _, D, H, _ in B.CASES.values())
    assert L[2] == 8 and L[3] % 2 == 1 and R.cdiv(L[4], B.ROW_LANES) == 2 and L[4] - B.ROW_LANES == 4


@pytest.mark.parametrize('shape', SHAPES)
def test_rows_in_reach_are_covered_exactly_once(shape):
    N, _, D, H, W = shape
    rows = [B.reach_decode(i, D, H) for i in range(B.n_reach_rows(D, H))]
    want = [(uz, uy) for uz in range(D) for uy in range(H) if B.in_reach(uz, uy, D, H)]
    assert len(rows) == len(set(rows)) and sorted(rows) == want
    assert B.rows_grid(N, D, H, W) == (len(want), R.cdiv(W, 64), N)
    # a row out of reach reads no source row (the parent leaves it at once: nothing is lost), a row in reach at most what the LDS holds
    worst = 0
    for uz in range(D):
        for uy in range(H):
            n = len(B.source_rows(uz, uy, D, H))
            if not B.in_reach(uz, uy, D, H):
                assert n == 0, (uz, uy)
            worst = max(worst, n)
    assert 0 < worst <= B.ROW_SRC_MAX
    if D >= 10 and H >= 10:
        assert worst == B.ROW_SRC_MAX   # (the bound is met: uz = 3, uy = 3)


@pytest.mark.parametrize('shape', SHAPES)
def test_staged_positions_and_segments(shape):
    N, _, D, H, W = shape
    for L, nseg in ((W, B.rows_grid(N, D, H, W)[1]), (H, B.xf_grid(N, D, H, W)[2] // N)):
        owned = []
        for seg in range(nseg):
            p0 = seg * B.ROW_LANES - B.REACH
            # the positions a block reads from memory: inside the line without its two ends, as the parent masks them
            read = [p0 + i for i in range(B.LINE_PITCH) if 1 <= p0 + i <= L - 2]
            assert all(0 <= p < L for p in read)
            for lane in range(B.ROW_LANES):
                u = seg * B.ROW_LANES + lane
                if u >= L:
                    continue
                owned.append(u)
                for d in range(7):   # the source at u - d + 3 sits at index lane - d + 2 REACH of the staged line
                    i = lane - d + 2 * B.REACH
                    assert 0 <= i < B.LINE_PITCH and p0 + i == u - d + 3
        assert owned == list(range(L))


@pytest.mark.parametrize('shape', SHAPES)
def test_row_groups_cover_every_row_and_tap_pair_once(shape):
    """every (row of R, dz, dy) is written by exactly one block of k_dlb_wgrad_rows: correlated with the line the parent stages for it
    (zz = vz + dz - 3, y2 = vy + dy - 3) where that line lies in the volume, written as zero where it does not; a block stages no line twice
    and none outside the volume"""
    N, _, D, H, W = shape
    gx, gy, gz = B.wgrad_grid(N, D, H, W)
    assert (gy, gz) == (7, N)
    seen, n_staged = {}, 0
    for bx in range(gx):
        for tapf in range(7):
            work, zeros, staged = B.wgrad_block(bx, tapf, D, H)
            assert len(set(staged)) == len(staged) and all(0 <= zz < D and 0 <= y2 < H for zz, y2 in staged)
            n_staged += len(staged)
            for r, d7, line in work:
                assert (r, d7) not in seen
                seen[r, d7] = line
            for r, d7 in zeros:
                assert (r, d7) not in seen
                seen[r, d7] = None
    nrows = B.n_bnd_rows(D, H)
    assert len(seen) == nrows * 49
    for r in range(nrows):
        vz, vy = B.row_decode(r, D, H)
        for dz in range(7):
            for dy in range(7):
                zz, y2 = vz + dz - 3, vy + dy - 3
                assert seen[r, dz * 7 + dy] == ((zz, y2) if 0 <= zz < D and 0 <= y2 < H else None), (r, dz, dy)
    # what the grouping is for: fewer stagings than the parent's one per pair inside the volume
    assert n_staged < sum(1 for v in seen.values() if v is not None)


def test_x_face_blocks_cover_every_side_and_channel_once():
    gy = B.xf_grid(1, 8, 8, 16)[1]
    got = sorted((side, c0 + c) for by in range(gy) for wave in range(4) for side, c0 in [B.xf_decode(by, wave)] for c in range(B.XF_CH))
    assert got == [(s, c) for s in range(2) for c in range(64)]
