// deep_linear_gen's position-typed path (dl_typed.hip): boundary kernels that do the arithmetic of dl_typed.hip's in the same order --
// every product, every FMA and every addition per output as there, so the same bits -- and change only where the operands come from, how many are
// in flight and which outputs share a block.  dl_typed.hip's kernels stay as the reference variant and the fallback; two of its host functions
// (dl_typed_dgrad_boundary, dl_typed_p) take these wherever dl_bnd_variant below says so.  The forward's boundary kernels are dl_typed.hip's.
//
//   dL/dact0 (k_dl_bnd_dgrad<false> / <true> of dl_typed.hip)                                                     k_dlb_dgrad_rows / k_dlb_dgrad_xf
//     rows: the launch covers the output rows within reach of a source row only (n_reach_rows / reach_decode: uz <= 3 || uz >= D - 4 || uy <= 3 ||
//       uy >= H - 4), not all D H rows; a block brings the at most kRowSrcMax source rows of dy it reads into LDS once, masked as the parent
//       masks them (x = 0 and x = W - 1 are not of the R set) with all its loads in flight together, and a thread's 343-step walk reads LDS where the parent waited for one cached
//       global load per step.
//     x faces: a thread owns kXfCh channels of its four columns where the parent's owned sixteen -- four times the waves (the parent ran 1.7
//       per SIMD at 108^3) at a quarter of the scalar weight loads each; the seven dyX lines of a block sit in LDS, masked to y = 1 .. H - 2.
//     Per output: dz, dy, dx ascending with the parent's skips, one read-modify-write of g per output and launch; the launches keep their
//     order (rows, x faces, then dl_typed.hip's k_dl_bnd_dgrad_ends).
//   type sums of the R set (k_dl_bnd_wgrad<false> of dl_typed.hip)                                                 k_dlb_wgrad_rows
//     a block owns kGrp neighbouring rows of a face and one tap across them (dz for the rows of a z face, dy for the rows y = 0 / H - 1 of
//     neighbouring planes) and walks the source lines along the group: a staged line of act0 (64 channels, LDS) serves every row of the group
//     that reads it -- up to kGrp (row, tap) pairs where the parent staged it once per pair -- and the next line's loads are in flight
//     (registers) under the correlation.  dy comes through wave-uniform loads, not LDS: one LDS read per kGrp FMAs where the parent took two
//     per FMA.  Each part[...] element is the parent's loop: m0 / m1 over x pairs from x0, the odd tail, m0 + m1; a pair whose line lies
//     outside the volume is written as zero, as there.  partA keeps its layout; the X set's sums, k_dl_bnd_reduce and k_dl_p_from_dh are
//     dl_typed.hip's.
#include "common.hpp"

namespace nc {
namespace {

constexpr int kD7 = 343, kC = 64;
constexpr int kReach = 3;                         // a 7^3 window reaches three voxels
constexpr int kRowLanes = 64;                     // outputs of a block along its line (x for the rows, y for the x faces)
constexpr int kLinePitch = kRowLanes + 2 * kReach;  // a staged source line: the block's outputs and three positions on either side
constexpr int kRowSrcMax = 13;                    // source rows of R within reach of one output row: 7 of a z face and one per other plane (D, H >= 8)
constexpr int kRowStage = (kRowSrcMax * kLinePitch + 255) / 256;  // staged elements per thread of k_dlb_dgrad_rows
constexpr int kXfCh = 4;                          // channels a thread of k_dlb_dgrad_xf owns
constexpr int kXfGroups = kC / kXfCh / 4;         // blocks per (uz, side, segment): four waves = four channel groups each
constexpr int kGrp = 4;                           // rows of a face a block of k_dlb_wgrad_rows owns
constexpr int kPitchB = 193;                      // its LDS line pitch in floats (W <= 192; odd: the 64 channels fall on different banks)
constexpr int kStageCh = 10;                      // channels a wave stages per line: wave + 7 i, i < 10 (those below 64)
constexpr int kStageSeg = 3;                      // 64-lane segments of a line: W <= 192

__host__ __device__ inline int axis_type(int coord, int L) { return coord == 0 ? 0 : coord == L - 1 ? 2 : 1; }

// the output rows (uz, uy) within reach of a row of R, numbered: the four planes next to either z face (all H rows each), then of every plane
// between the four rows next to either y face
__host__ __device__ inline void reach_decode(int i, int D, int H, int& uz, int& uy) {
  if (i < 8 * H) { const int p = i / H; uz = p < 4 ? p : D - 8 + p; uy = i - p * H; }
  else { const int j = i - 8 * H, r = j & 7; uz = 4 + (j >> 3); uy = r < 4 ? r : H - 8 + r; }
}
__host__ inline int n_reach_rows(int D, int H) { return 8 * H + 8 * (D - 8); }

__global__ void __launch_bounds__(256) k_dlb_dgrad_rows(const float* __restrict__ dysrc, const float* __restrict__ Hd, float* __restrict__ g, int D, int H, int W) {
  __shared__ float L[kRowSrcMax][kLinePitch];
  __shared__ int rowoff[kRowSrcMax], nsrc;  // vz * H + vy of the source rows, their number
  const int lane = threadIdx.x & 63, q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n = blockIdx.z;
  const long HW = (long)H * W, S = (long)D * HW;
  int uz, uy;
  reach_decode(blockIdx.x, D, H, uz, uy);
  const int x0 = blockIdx.y * kRowLanes - kReach;  // the position L[.][0] holds
  // the source rows in the order the walk below meets them: lane dz * 7 + dy of the first wave holds one candidate, its rank among the rows of R
  // is the row's slot in L
  if (threadIdx.x < 64) {
    const int dz = lane / 7, dy = lane - dz * 7, vz = uz - dz + 3, vy = uy - dy + 3;
    const bool src = lane < 49 && (unsigned)vz < (unsigned)D && (unsigned)vy < (unsigned)H && !(axis_type(vz, D) == 1 && axis_type(vy, H) == 1);
    const unsigned long long m = __ballot(src);
    if (src) rowoff[__popcll(m & ((1ull << lane) - 1))] = vz * H + vy;
    if (lane == 0) nsrc = __popcll(m);
  }
  __syncthreads();
  {
    const int ne = nsrc * kLinePitch;
    float v[kRowStage];
#pragma unroll
    for (int i = 0; i < kRowStage; ++i) {
      const int e = threadIdx.x + i * 256, j = e / kLinePitch, vx = x0 + e - j * kLinePitch;
      v[i] = (e < ne && vx >= 1 && vx <= W - 2) ? dysrc[(long)n * S + (long)rowoff[e < ne ? j : 0] * W + vx] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < kRowStage; ++i) {
      const int e = threadIdx.x + i * 256;
      if (e < ne) (&L[0][0])[e] = v[i];
    }
  }
  __syncthreads();
  const int ux = blockIdx.y * kRowLanes + lane;
  if (ux >= W) return;
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.f;
  int j = 0;
  for (int dz = 0; dz < 7; ++dz) {
    const int vz = uz - dz + 3;
    if ((unsigned)vz >= (unsigned)D) continue;
    const int tz = axis_type(vz, D);
    for (int dy = 0; dy < 7; ++dy) {
      const int vy = uy - dy + 3;
      if ((unsigned)vy >= (unsigned)H) continue;
      const int ty = axis_type(vy, H);
      if (tz == 1 && ty == 1) continue;
      const int tau = (tz * 3 + ty) * 3 + 1;
      const float* l = &L[j][lane + 2 * kReach];                                            // l[-dx]: the source at vx = ux - dx + 3
      const float* h = Hd + ((long)tau * kD7 + (dz * 7 + dy) * 7) * kC + q * 16;  // wave-uniform
#pragma unroll
      for (int dx = 0; dx < 7; ++dx) {
        const float w = l[-dx];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = __builtin_fmaf(w, h[dx * kC + c], acc[c]);
      }
      ++j;
    }
  }
  float* o = g + ((long)n * kC + q * 16) * S + (long)uz * HW + (long)uy * W + ux;
#pragma unroll
  for (int c = 0; c < 16; ++c) o[(long)c * S] += acc[c];
}

// block = (uz, side + 2 * (channel group / 4), sample * nseg + segment of y); wave = channel group
__global__ void __launch_bounds__(256) k_dlb_dgrad_xf(const float* __restrict__ dyx, const float* __restrict__ Hd, float* __restrict__ g, int D, int H, int W, int nseg) {
  __shared__ float L[7][kLinePitch];
  const int lane = threadIdx.x & 63;
  const int uz = blockIdx.x, side = blockIdx.y & 1, cg = (blockIdx.y >> 1) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = blockIdx.z / nseg, seg = blockIdx.z - n * nseg;
  const long HW = (long)H * W, S = (long)D * HW;
  const int y0 = seg * kRowLanes - kReach;
  for (int e = threadIdx.x; e < 7 * kLinePitch; e += 256) {
    const int dz = e / kLinePitch, i = e - dz * kLinePitch;
    const int vz = uz - dz + 3, vy = y0 + i;
    // (the sources at the two ends of the y line have their own types: k_dl_bnd_dgrad_ends')
    L[dz][i] = ((unsigned)vz < (unsigned)D && vy >= 1 && vy <= H - 2) ? dyx[(((long)n * 2 + side) * D + vz) * H + vy] : 0.f;
  }
  __syncthreads();
  const int uy = seg * kRowLanes + lane;
  if (uy >= H) return;
  const int tx = side ? 2 : 0;
  float acc[4][kXfCh];
#pragma unroll
  for (int xr = 0; xr < 4; ++xr)
#pragma unroll
    for (int c = 0; c < kXfCh; ++c) acc[xr][c] = 0.f;
  for (int dz = 0; dz < 7; ++dz) {
    const int vz = uz - dz + 3;
    if ((unsigned)vz >= (unsigned)D) continue;
    const int tau = (axis_type(vz, D) * 3 + 1) * 3 + tx;
    const float* l = &L[dz][lane + 2 * kReach];  // l[-dy]: the source at vy = uy - dy + 3
#pragma unroll
    for (int dy = 0; dy < 7; ++dy) {
      const float w = l[-dy];
#pragma unroll
      for (int xr = 0; xr < 4; ++xr) {
        const int dx = side ? xr : xr + 3;
        const float* h = Hd + ((long)tau * kD7 + (dz * 7 + dy) * 7 + dx) * kC + cg * kXfCh;  // wave-uniform
#pragma unroll
        for (int c = 0; c < kXfCh; ++c) acc[xr][c] = __builtin_fmaf(w, h[c], acc[xr][c]);
      }
    }
  }
  float4* o = reinterpret_cast<float4*>(g + ((long)n * kC + cg * kXfCh) * S + (long)uz * HW + (long)uy * W + (side ? W - 4 : 0));
#pragma unroll
  for (int c = 0; c < kXfCh; ++c) {
    float4 v = o[(long)c * (S / 4)];
    v.x += acc[0][c]; v.y += acc[1][c]; v.z += acc[2][c]; v.w += acc[3][c];
    o[(long)c * (S / 4)] = v;
  }
}

// NT (row, tap) pairs of one staged line: pair j reads the dy row dyrow + j * dystep and writes part0[j * pstep]
template <int NT>
__device__ __forceinline__ void dlb_corr(const float* a, const float* __restrict__ dyrow, long dystep, float* __restrict__ part0, long pstep, int sh, int W) {
  const int x0 = sh < 0 ? (1 > -sh ? 1 : -sh) : 1, x1 = sh > 0 ? (W - 2 < W - 1 - sh ? W - 2 : W - 1 - sh) : W - 2;  // 1 <= x <= W - 2, 0 <= x + sh < W
  float m0[NT], m1[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) m0[j] = m1[j] = 0.f;
  int x = x0;
#pragma unroll 4
  for (; x + 1 <= x1; x += 2) {
    const float a0 = a[x + sh], a1 = a[x + 1 + sh];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const float* d = dyrow + j * dystep;  // wave-uniform
      m0[j] = __builtin_fmaf(d[x], a0, m0[j]);
      m1[j] = __builtin_fmaf(d[x + 1], a1, m1[j]);
    }
  }
  if (x <= x1) {
    const float a0 = a[x + sh];
#pragma unroll
    for (int j = 0; j < NT; ++j) m0[j] = __builtin_fmaf((dyrow + j * dystep)[x], a0, m0[j]);
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) part0[j * pstep] = m0[j] + m1[j];
}

// block = (group, the tap across the group, sample); threads (k = dx, c) as k_dl_bnd_wgrad.  Groups: first the 2 ngz of the z faces (face, then
// kGrp rows y each; the tap is dz, the lines run along y), then the y faces' (face y = 0 / H - 1, then kGrp planes z of 1 .. D - 2 each; the tap
// is dy, the lines run along z).  part[n][r][d][c], r numbered as dl_typed.hip's row_decode does
__global__ void __launch_bounds__(448) k_dlb_wgrad_rows(const float* __restrict__ asrc, const float* __restrict__ dysrc, float* __restrict__ part, int D, int H, int W,
                                                        int nrows, int ngz, int ngy) {
  __shared__ float A[kC * kPitchB];
  const int th = threadIdx.x, c = th & 63, k = __builtin_amdgcn_readfirstlane(th >> 6);
  const int tapf = blockIdx.y, n = blockIdx.z;
  const long HW = (long)H * W, S = (long)D * HW;
  const bool zf = (int)blockIdx.x < 2 * ngz;
  int face, p0, cnt, Lg, fixed, fixedL, r0, rstep, d0, dstep;  // rows p0 .. p0 + cnt - 1 along the group's axis of extent Lg; r = r0 + rstep * pos; d = d0 + dstep * g
  if (zf) {
    face = blockIdx.x / ngz; p0 = (blockIdx.x - face * ngz) * kGrp; cnt = H - p0 < kGrp ? H - p0 : kGrp; Lg = H;
    fixed = face ? D - 1 : 0; fixedL = D;  // the rows' plane vz; the lines' plane is vz + dz - 3
    r0 = face * H; rstep = 1; d0 = tapf * 49 + k; dstep = 7;
  } else {
    const int g2 = blockIdx.x - 2 * ngz;
    face = g2 / ngy; p0 = 1 + (g2 - face * ngy) * kGrp; cnt = D - 1 - p0 < kGrp ? D - 1 - p0 : kGrp; Lg = D;
    fixed = face ? H - 1 : 0; fixedL = H;  // the rows' vy; the lines' row is vy + dy - 3
    r0 = 2 * H - 2 + face; rstep = 2; d0 = tapf * 7 + k; dstep = 49;
  }
  const int fl = fixed + tapf - 3;  // the lines' fixed coordinate
  const bool fixed_in = (unsigned)fl < (unsigned)fixedL;
  const long lstride = zf ? (long)W : HW;  // from a line / a dy row to the next along the group's axis
  float* pn = part + (long)n * nrows * kD7 * kC + c;
  // the pairs whose line lies outside the volume: zero, as the parent writes them
  for (int f = 0; f < cnt; ++f)
    for (int g = 0; g < 7; ++g) {
      const int t = p0 + f + g - 3;
      if (!fixed_in || (unsigned)t >= (unsigned)Lg) pn[((long)(r0 + rstep * (p0 + f)) * kD7 + d0 + dstep * g) * kC] = 0.f;
    }
  if (!fixed_in) return;
  const float* lines = asrc + (long)n * kC * S + (zf ? (long)fl * HW : (long)fl * W);
  const float* dyf = dysrc + (long)n * S + (zf ? (long)fixed * HW : (long)fixed * W);
  const int t0 = p0 - 3 > 0 ? p0 - 3 : 0, t1 = p0 + cnt + 2 < Lg - 1 ? p0 + cnt + 2 : Lg - 1;
  float v[kStageSeg][kStageCh];
  auto fetch = [&](int t) __attribute__((always_inline)) {
    const float* line = lines + (long)t * lstride;
#pragma unroll
    for (int sg = 0; sg < kStageSeg; ++sg)
#pragma unroll
      for (int i = 0; i < kStageCh; ++i) {
        const int cc = k + 7 * i, xx = sg * 64 + c;
        v[sg][i] = (cc < kC && xx < W) ? line[(long)cc * S + xx] : 0.f;
      }
  };
  fetch(t0);
  for (int t = t0; t <= t1; ++t) {
    __syncthreads();  // (the correlation of the line before is done with A)
#pragma unroll
    for (int sg = 0; sg < kStageSeg; ++sg)
#pragma unroll
      for (int i = 0; i < kStageCh; ++i) {
        const int cc = k + 7 * i, xx = sg * 64 + c;
        if (cc < kC && xx < W) A[cc * kPitchB + xx] = v[sg][i];
      }
    __syncthreads();
    if (t < t1) fetch(t + 1);  // in flight under the correlation
    // the rows pos = t + 3 - g of the group, g = glo .. ghi; pair j: g = glo + j
    const int glo = t + 4 - p0 - cnt > 0 ? t + 4 - p0 - cnt : 0, ghi = t + 3 - p0 < 6 ? t + 3 - p0 : 6;
    const int pos0 = t + 3 - glo;
    const float* dyrow = dyf + (long)pos0 * lstride;
    float* part0 = pn + ((long)(r0 + rstep * pos0) * kD7 + d0 + dstep * glo) * kC;
    const long pstep = ((long)-rstep * kD7 + dstep) * kC;
    const float* a = A + c * kPitchB;
    switch (ghi - glo + 1) {
      case 1: dlb_corr<1>(a, dyrow, -lstride, part0, pstep, k - 3, W); break;
      case 2: dlb_corr<2>(a, dyrow, -lstride, part0, pstep, k - 3, W); break;
      case 3: dlb_corr<3>(a, dyrow, -lstride, part0, pstep, k - 3, W); break;
      default: dlb_corr<4>(a, dyrow, -lstride, part0, pstep, k - 3, W); break;
    }
  }
}
static_assert(kGrp == 4, "k_dlb_wgrad_rows switches over 1 .. kGrp pairs per line");

}  // namespace

// Both pieces take every shape dl_typed_supported admits: reach_decode and kRowSrcMax want D, H >= 8, the float4 columns W % 4 == 0, kPitchB holds a
// line of W <= 192, and there are D - 2 >= 1 planes between the z faces.
// The pieces with kernels here: 1 = dL/dact0, 2 = the type sums (the R set's).  The forward (0) runs dl_typed.hip's kernels
int dl_bnd_variant(int piece, int N, int D, int H, int W) { return (piece == 1 || piece == 2) && dl_typed_supported(N, D, H, W) ? 1 : 0; }

// g += the difference kernels of the R set, then of the X set without the line ends (dyX: dl_typed.hip's k_dl_gather_x)
int dl_bnd_dgrad(const float* dy, const float* dyX, const float* Hd, float* g, int N, int D, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(k_dlb_dgrad_rows, dim3((unsigned)n_reach_rows(D, H), (unsigned)cdiv(W, kRowLanes), (unsigned)N), dim3(256), 0, s, dy, Hd, g, D, H, W);
  const int nseg = (int)cdiv(H, kRowLanes);
  hipLaunchKernelGGL(k_dlb_dgrad_xf, dim3((unsigned)D, 2 * kXfGroups, (unsigned)(N * nseg)), dim3(256), 0, s, dyX, Hd, g, D, H, W, nseg);
  return check_launch("deep_linear: typed data gradient, boundary");
}

// partA[n][r][d][c]: the R set's partial sums, one row r at a time
int dl_bnd_wgrad_rows(const float* act0, const float* dy, float* partA, int N, int D, int H, int W, int nrows, hipStream_t s) {
  const int ngz = (int)cdiv(H, kGrp), ngy = (int)cdiv(D - 2, kGrp);
  hipLaunchKernelGGL(k_dlb_wgrad_rows, dim3((unsigned)(2 * ngz + 2 * ngy), 7, (unsigned)N), dim3(448), 0, s, act0, dy, partA, D, H, W, nrows, ngz, ngy);
  return check_launch("deep_linear: typed parameter gradients, boundary rows");
}

}  // namespace nc

using namespace nc;

// Test exports (tests/test_gpu_dl_bnd.py): one boundary piece of the typed path alone, with dl_typed.hip's kernels (variant 0), the ones of this
// file (1) or the library's own choice (-1).  Nothing is written before every argument is checked.
extern "C" {

size_t nc_dl_typed_scratch_bytes_debug(int N, int D, int H, int W) { return dl_typed_bytes(N, D, H, W); }

int nc_dl_bnd_variant_debug(int piece, int N, int D, int H, int W) {
  if (piece < 0 || piece > 2) { set_error("dl_bnd_variant_debug: piece is 0 (forward), 1 (dL/dact0) or 2 (type sums)"); return NC_ERR_ARG; }
  if (!dl_typed_supported(N, D, H, W)) { set_error("dl_bnd_variant_debug: shape not covered by the typed form"); return NC_ERR_SHAPE; }
  return dl_bnd_variant(piece, N, D, H, W);
}

int nc_dl_bnd_piece_debug(int piece, const float* F, const float* act0, const float* dy, float* io, void* scratch, size_t scratch_bytes, int N, int D,
                          int H, int W, int variant, void* stream) {
  if (piece < 0 || piece > 2 || variant < -1 || variant > 1) { set_error("dl_bnd_piece_debug: bad piece or variant"); return NC_ERR_ARG; }
  if (!F || !act0 || !io || !scratch || (piece != 0 && !dy)) { set_error("dl_bnd_piece_debug: null pointer"); return NC_ERR_ARG; }
  if (!dl_typed_supported(N, D, H, W)) { set_error("dl_bnd_piece_debug: shape not covered by the typed form"); return NC_ERR_SHAPE; }
  if (variant == 1 && dl_bnd_variant(piece, N, D, H, W) != 1) { set_error("dl_bnd_piece_debug: no kernels of dl_bnd.hip for this piece and shape"); return NC_ERR_SHAPE; }
  if (scratch_bytes < dl_typed_bytes(N, D, H, W)) { set_error("dl_bnd_piece_debug: scratch too small"); return NC_ERR_WS; }
  hipStream_t s = (hipStream_t)stream;
  char* sc = (char*)scratch;
  NC_TRY(dl_typed_compose(F, sc, N, D, H, W, s));
  if (piece == 0) return dl_typed_fwd_boundary(act0, io, sc, N, D, H, W, s);  // (variant 1 was refused above: no forward kernels here)
  if (piece == 1) return dl_typed_dgrad_boundary(act0, dy, io, sc, N, D, H, W, s, variant);
  // the type sums read the transposed copies the data gradient's call leaves, and dWsw (the interior's correlation: zero here)
  NC_TRY(dl_typed_gather(act0, dy, sc, N, D, H, W, s));
  if (hipMemsetAsync(dl_typed_dwsw(sc, N, D, H, W), 0, (size_t)kC * kD7 * 4, s) != hipSuccess) { set_error("dl_bnd_piece_debug: hipMemsetAsync failed"); return NC_ERR_HIP; }
  return dl_typed_p(act0, dy, io, sc, N, D, H, W, s, variant);
}

}  // extern "C"
