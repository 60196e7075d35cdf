// One-channel k^3 convolution of the learned-PSF generators (models/networks.py:840-871 of the reference: LinearKernel /
// LinearKernel_double, a bias-free Conv3d(1, 1, k, padding = (k - 1) / 2), odd k = 3 .. 31) on the fp32 matrix cores.
//
// Forward (and dgrad = the forward with the kernel flipped in the weight staging): per tap row (a, b) a Toeplitz GEMM on
// v_mfma_f32_16x16x4_f32,   Y[x0 + j][row r] += sum_c' T_ab[j][c'] X[z + a - p][y0 + r + b - p][x0 - p + c'],   T_ab[j][c'] = w[a][b][c' - j]:
// M = 16 output x positions (A = the Toeplitz weights, read from a zero-padded weight row in LDS), N = 16 output rows (B = the input
// window, LDS), K = the 16 + k - 1 input x positions of the window in steps of 4.  A workgroup computes 32 x 16 x 4 outputs (x, y, z):
// wave w the plane z0 + w, two 16-wide x tiles sharing each A fragment.  Input planes stream through a five-slot LDS ring (one new plane
// per depth tap a), the weights through a double-buffered a-slab.  Issued / useful MFMA work: 4 ceil((15 + k) / 4) / k = 48/31 at k = 31,
// 24/9 at k = 9.
//
// wgrad: with b = b0 + i and y' = y + i,   dw[a][b0 + i][c0 + cc] = sum_{z, y', x} X[z + a - p][y' + b0 - p][x + c0 + cc - p] DY[z][y' - i][x]:
// A = a shifted X row window (M = 16 c), B = a shifted DY row window (N = 16 i), K = positions, 4 consecutive x per step.  One 16 x 16
// tile of (c, i) is one GEMM over all positions; k = 31 needs 2 x 2 tiles (961 / 1024 useful).  Workgroup (pc, a) sums its contiguous
// share of the position units (16 y' rows x 32 x of one plane) into per-wave registers, the four waves are added in LDS in wave order and
// the partials [pc][a][b][c] are summed over pc in index order by k_lk_wgrad_reduce: no float atomics, the same bits every run.
//
// Arithmetic: exact fp32 products, fp32 accumulation (an MFMA is a k-ordered fmaf chain).  The forward sums in three levels -- one tap
// row (a, b) as an MFMA chain of 4 ceil((15 + k) / 4) products, the k rows of a depth tap, the k depth taps -- and the weight gradient per
// position unit (128 products), then over units, waves and workgroups: error against fp64 stays ~1e-7 of sum |terms|, without the range
// guard of the 16-bit forms.
#include "common.hpp"

namespace nc {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kLkThreads = 256;  // 4 waves
constexpr int kLkRing = 5;       // forward: 4 planes in use + 1 being filled

__host__ __device__ constexpr int lk_pitch(int n) {  // smallest 4 * odd >= n: 16 lanes reading 16 rows x 4 columns hit 64 different banks
  return ((n + 3) / 4) % 2 ? (n + 3) / 4 * 4 : (n + 3) / 4 * 4 + 4;
}

template <int K>
struct LkFwdCfg {
  static constexpr int p = K / 2;
  static constexpr int S = (15 + K + 3) / 4;       // k-steps of 4 over the 16 + K - 1 window
  static constexpr int RW = 15 + 4 * S;             // weight row: 15 zeros, w[a][b][0 .. K), zeros
  static constexpr int ROWS = 15 + K;               // input rows of a 16-row output tile
  static constexpr int XC = 16 + 4 * S;             // input columns read by the two x tiles
  static constexpr int P = lk_pitch(XC);
  static constexpr int PLANE = ROWS * P;
  static constexpr int NPL = (ROWS * XC + kLkThreads - 1) / kLkThreads;  // staged plane values per thread
  static constexpr int NWL = (K * RW + kLkThreads - 1) / kLkThreads;     // staged weight values per thread
  static constexpr int LDS_FLOATS = kLkRing * PLANE + 2 * K * RW;
};

struct LkFwdParams {
  const float* x;  // [N][D][H][W]
  const float* w;  // [K][K][K]
  float* y;        // [N][D][H][W]
  int D, H, W, ZB;
  int flip;        // dgrad: w[K-1-a][K-1-b][K-1-c]
};

template <int K>
__global__ void __launch_bounds__(kLkThreads) k_lk_fwd(const LkFwdParams q) {
  using C = LkFwdCfg<K>;
  extern __shared__ float lds[];
  float* ring = lds;                         // [kLkRing][ROWS][P]
  float* wsl = lds + kLkRing * C::PLANE;     // [2][K][RW]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 16;
  const int n = blockIdx.z / q.ZB, z0 = (blockIdx.z % q.ZB) * 4;
  const long HW = (long)q.H * q.W;
  const float* xn = q.x + (long)n * q.D * HW;

  // plane `rel` of the window: input z = z0 - p + rel, rows y0 - p + [0, ROWS), columns x0 - p + [0, XC)
  auto load_plane = [&](int rel, float (&v)[C::NPL]) {
    const int iz = z0 - C::p + rel;
#pragma unroll
    for (int i = 0; i < C::NPL; ++i) {
      const int e = tid + i * kLkThreads;
      const int r = e / C::XC, c = e - r * C::XC;
      const int iy = y0 - C::p + r, ix = x0 - C::p + c;
      const bool ok = e < C::ROWS * C::XC && (unsigned)iz < (unsigned)q.D && (unsigned)iy < (unsigned)q.H && (unsigned)ix < (unsigned)q.W;
      v[i] = ok ? xn[(long)iz * HW + (long)iy * q.W + ix] : 0.f;
    }
  };
  auto store_plane = [&](int rel, const float (&v)[C::NPL]) {
    float* dst = ring + (rel % kLkRing) * C::PLANE;
#pragma unroll
    for (int i = 0; i < C::NPL; ++i) {
      const int e = tid + i * kLkThreads;
      const int r = e / C::XC, c = e - r * C::XC;
      if (e < C::ROWS * C::XC) dst[r * C::P + c] = v[i];
    }
  };
  auto load_w = [&](int a, float (&v)[C::NWL]) {
#pragma unroll
    for (int i = 0; i < C::NWL; ++i) {
      const int e = tid + i * kLkThreads;
      const int b = e / C::RW, t = e - b * C::RW - 15;
      float val = 0.f;
      if (e < K * C::RW && t >= 0 && t < K)
        val = q.flip ? q.w[((K - 1 - a) * K + (K - 1 - b)) * K + (K - 1 - t)] : q.w[(a * K + b) * K + t];
      v[i] = val;
    }
  };
  auto store_w = [&](int a, const float (&v)[C::NWL]) {
    float* dst = wsl + (a & 1) * K * C::RW;
#pragma unroll
    for (int i = 0; i < C::NWL; ++i) {
      const int e = tid + i * kLkThreads;
      if (e < K * C::RW) dst[e] = v[i];
    }
  };

  {
    float pv[C::NPL], wv[C::NWL];
    for (int rel = 0; rel < 4; ++rel) {
      load_plane(rel, pv);
      store_plane(rel, pv);
    }
    load_w(0, wv);
    store_w(0, wv);
  }
  __syncthreads();

  const int j = lane & 15, qk = lane >> 4;
  const int zo = z0 + wave;
  f32x4 tot0 = {0.f, 0.f, 0.f, 0.f}, tot1 = tot0;
  for (int a = 0; a < K; ++a) {
    const bool more = a + 1 < K;
    float pv[C::NPL], wv[C::NWL];
    if (more) {  // the next depth tap's plane and weight slab: loads in flight under this tap's MFMAs
      load_plane(a + 4, pv);
      load_w(a + 1, wv);
    }
    const int iz = zo - C::p + a;
    if (zo < q.D && (unsigned)iz < (unsigned)q.D) {
      const float* pl = ring + ((wave + a) % kLkRing) * C::PLANE;
      const float* wl = wsl + (a & 1) * K * C::RW + 15 + qk - j;
      f32x4 row0 = {0.f, 0.f, 0.f, 0.f}, row1 = row0;
      for (int b = 0; b < K; ++b) {
        float av[C::S];
#pragma unroll
        for (int s = 0; s < C::S; ++s) av[s] = wl[b * C::RW + 4 * s];
        const float* xb = pl + (j + b) * C::P + qk;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll
        for (int s = 0; s < C::S; ++s) {
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], xb[4 * s], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], xb[16 + 4 * s], acc1, 0, 0, 0);
        }
        row0 += acc0;
        row1 += acc1;
      }
      tot0 += row0;
      tot1 += row1;
    }
    if (more) {
      store_plane(a + 4, pv);
      store_w(a + 1, wv);
    }
    __syncthreads();
  }
  // D[j][r]: lane holds output row r = lane & 15, x = 4 (lane >> 4) + e of each 16-wide tile
  const int oy = y0 + j;
  if (zo < q.D && oy < q.H) {
    float* yr = q.y + ((long)n * q.D + zo) * HW + (long)oy * q.W;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ox = x0 + 4 * qk + e;
      if (ox < q.W) yr[ox] = tot0[e];
      if (ox + 16 < q.W) yr[ox + 16] = tot1[e];
    }
  }
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------
template <int K>
struct LkWgCfg {
  static constexpr int p = K / 2;
  static constexpr int NT = (K + 15) / 16;          // 16-wide tiles along b and along c
  static constexpr int DYR = 31, DYP = 36;          // DY rows y' - i of a unit (16 + 15), pitch 4 * 9
  static constexpr int XR = 16 * NT;                // X rows y' + b0 - p
  static constexpr int XCOL = 31 + 16 * NT;         // X columns x + c - p
  static constexpr int XP = (XCOL + 3) / 4 * 4;
  static constexpr int BUF = DYR * DYP + XR * XP;
  static constexpr int NDY = (DYR * 32 + kLkThreads - 1) / kLkThreads;
  static constexpr int NX = (XR * XCOL + kLkThreads - 1) / kLkThreads;
  static constexpr int TILE = 256 * NT * NT;        // partial floats per (pc, a)
};

struct LkWgParams {
  const float* x;    // [N][D][H][W]
  const float* dy;   // [N][D][H][W]
  float* part;       // [parts][K][16 NT][16 NT]
  int D, H, W, UY, UX;
  long units, per;   // position units in all, per workgroup
};

template <int K>
__global__ void __launch_bounds__(kLkThreads) k_lk_wgrad(const LkWgParams q) {
  using C = LkWgCfg<K>;
  constexpr int NT = C::NT;
  __shared__ float buf[2][C::BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int a = blockIdx.y;
  const long HW = (long)q.H * q.W;
  const long u0 = blockIdx.x * q.per, u1 = u0 + q.per < q.units ? u0 + q.per : q.units;

  struct Unit { long base; int z, Y0, X0; bool live; };
  auto unit = [&](long u) {
    Unit t;
    t.X0 = (int)(u % q.UX) * 32;
    t.Y0 = (int)((u / q.UX) % q.UY) * 16;
    const long nz = u / ((long)q.UX * q.UY);
    t.z = (int)(nz % q.D);
    t.base = (nz / q.D) * q.D * HW;  // n * D * H * W
    t.live = (unsigned)(t.z + a - C::p) < (unsigned)q.D;
    return t;
  };
  // DY rows Y0 - 15 + [0, 31) x columns X0 + [0, 32); X rows Y0 - p + [0, XR) x columns X0 - p + [0, XCOL) of plane z + a - p
  auto load = [&](const Unit& t, float (&vd)[C::NDY], float (&vx)[C::NX]) {
    const float* dyp = q.dy + t.base + (long)t.z * HW;
    const float* xp = q.x + t.base + (long)(t.z + a - C::p) * HW;
#pragma unroll
    for (int i = 0; i < C::NDY; ++i) {
      const int e = tid + i * kLkThreads;
      const int r = e >> 5, c = e & 31;
      const int iy = t.Y0 - 15 + r, ix = t.X0 + c;
      vd[i] = e < C::DYR * 32 && (unsigned)iy < (unsigned)q.H && (unsigned)ix < (unsigned)q.W ? dyp[(long)iy * q.W + ix] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < C::NX; ++i) {
      const int e = tid + i * kLkThreads;
      const int r = e / C::XCOL, c = e - r * C::XCOL;
      const int iy = t.Y0 - C::p + r, ix = t.X0 - C::p + c;
      vx[i] = e < C::XR * C::XCOL && (unsigned)iy < (unsigned)q.H && (unsigned)ix < (unsigned)q.W ? xp[(long)iy * q.W + ix] : 0.f;
    }
  };
  auto store = [&](float* bf, const float (&vd)[C::NDY], const float (&vx)[C::NX]) {
#pragma unroll
    for (int i = 0; i < C::NDY; ++i) {
      const int e = tid + i * kLkThreads;
      if (e < C::DYR * 32) bf[(e >> 5) * C::DYP + (e & 31)] = vd[i];
    }
    float* bx = bf + C::DYR * C::DYP;
#pragma unroll
    for (int i = 0; i < C::NX; ++i) {
      const int e = tid + i * kLkThreads;
      const int r = e / C::XCOL, c = e - r * C::XCOL;
      if (e < C::XR * C::XCOL) bx[r * C::XP + c] = vx[i];
    }
  };

  const int ii = lane & 15, qk = lane >> 4;
  f32x4 tot[NT][NT];
#pragma unroll
  for (int bt = 0; bt < NT; ++bt)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) tot[bt][ct] = {0.f, 0.f, 0.f, 0.f};

  // skip the units whose X plane lies in the zero padding: they add nothing (workgroup-uniform)
  long u = u0;
  while (u < u1 && !unit(u).live) ++u;
  if (u < u1) {
    float vd[C::NDY], vx[C::NX];
    load(unit(u), vd, vx);
    store(buf[0], vd, vx);
  }
  __syncthreads();
  int cur = 0;
  while (u < u1) {
    long un = u + 1;
    while (un < u1 && !unit(un).live) ++un;
    float vd[C::NDY], vx[C::NX];
    if (un < u1) load(unit(un), vd, vx);
    {
      const float* bd = buf[cur];
      const float* bx = bd + C::DYR * C::DYP;
      f32x4 acc[NT][NT];
#pragma unroll
      for (int bt = 0; bt < NT; ++bt)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) acc[bt][ct] = {0.f, 0.f, 0.f, 0.f};
      for (int rr = 0; rr < 4; ++rr) {
        const int ry = wave * 4 + rr;  // y' - Y0
        const float* dyr = bd + (ry + 15 - ii) * C::DYP + qk;  // B[pos][i] = DY[y' - i][x]
        const float* xr = bx + ry * C::XP + qk + ii;          // A[cc][pos] = X[y' + b0 - p][x + c0 + cc - p]
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const float bv = dyr[4 * t];
#pragma unroll
          for (int bt = 0; bt < NT; ++bt)
#pragma unroll
            for (int ct = 0; ct < NT; ++ct)
              acc[bt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[bt * 16 * C::XP + 4 * t + 16 * ct], bv, acc[bt][ct], 0, 0, 0);
        }
      }
#pragma unroll
      for (int bt = 0; bt < NT; ++bt)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) tot[bt][ct] += acc[bt][ct];
    }
    if (un < u1) store(buf[cur ^ 1], vd, vx);
    __syncthreads();
    cur ^= 1;
    u = un;
  }
  // the four waves' sums, added in wave order through LDS (the staging buffers are free now)
  float* red = &buf[0][0];  // [wave][tile][e][lane]
  static_assert(4 * NT * NT * 256 <= 2 * C::BUF, "reduction buffer");
#pragma unroll
  for (int bt = 0; bt < NT; ++bt)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[((wave * NT * NT + bt * NT + ct) * 4 + e) * 64 + lane] = tot[bt][ct][e];
  __syncthreads();
  float* out = q.part + ((long)blockIdx.x * K + a) * C::TILE;
  for (int o = tid; o < NT * NT * 256; o += kLkThreads) {
    const int l = o & 63, e = (o >> 6) & 3, tile = o >> 8;
    const float s = ((red[o] + red[NT * NT * 256 + o]) + red[2 * NT * NT * 256 + o]) + red[3 * NT * NT * 256 + o];
    const int bt = tile / NT, ct = tile % NT;
    // D[cc][i]: lane holds i = lane & 15 (b = 16 bt + i), cc = 4 (lane >> 4) + e (c = 16 ct + cc)
    out[(16 * bt + (l & 15)) * 16 * NT + 16 * ct + 4 * (l >> 4) + e] = s;
  }
}

// dw[a][b][c] = sum over pc in index order of part[pc][a][b][c]
__global__ void __launch_bounds__(256) k_lk_wgrad_reduce(const float* __restrict__ part, float* __restrict__ dw, int K, int NT, int parts) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= K * K * K) return;
  const int a = o / (K * K), b = (o / K) % K, c = o % K;
  const long tile = 256L * NT * NT, stride = (long)K * tile;
  const float* src = part + a * tile + b * 16 * NT + c;
  float s = 0.f;
  for (int pc = 0; pc < parts; ++pc) s += src[pc * stride];
  dw[o] = s;
}

bool lk_shape_ok(int N, int D, int H, int W, int k) {
  return N >= 1 && D >= 1 && H >= 1 && W >= 1 && k >= 3 && k <= 31 && (k & 1) && (long)N * ((D + 3) / 4) <= 65535 && (H + 15) / 16 <= 65535;
}

struct LkWgPlan { int UY, UX, parts; long units, per; };
LkWgPlan lk_wg_plan(int N, int D, int H, int W, int k) {
  LkWgPlan p;
  p.UY = (H + 15 + 15) / 16;  // y' in [0, H + 15)
  p.UX = (W + 31) / 32;
  p.units = (long)N * D * p.UY * p.UX;
  // ~1024 workgroups over (parts, a): four per CU
  long want = (1024 + k - 1) / k;
  if (want > p.units) want = p.units;
  p.per = (p.units + want - 1) / want;
  p.parts = (int)((p.units + p.per - 1) / p.per);
  return p;
}

template <int K>
int lk_fwd_launch(const float* x, const float* w, float* y, int N, int D, int H, int W, int flip, hipStream_t s) {
  using C = LkFwdCfg<K>;
  const int bytes = C::LDS_FLOATS * (int)sizeof(float);
  if (int e = raise_dyn_lds(k_lk_fwd<K>, bytes, "lk_fwd")) return e;
  LkFwdParams q{x, w, y, D, H, W, (D + 3) / 4, flip};
  hipLaunchKernelGGL(k_lk_fwd<K>, dim3((W + 31) / 32, (H + 15) / 16, N * q.ZB), dim3(kLkThreads), bytes, s, q);
  return check_launch(flip ? "lk_dgrad" : "lk_fwd");
}

template <int K>
int lk_wgrad_launch(const float* x, const float* dy, float* dw, int N, int D, int H, int W, void* ws, hipStream_t s) {
  const LkWgPlan p = lk_wg_plan(N, D, H, W, K);
  LkWgParams q{x, dy, (float*)ws, D, H, W, p.UY, p.UX, p.units, p.per};
  hipLaunchKernelGGL(k_lk_wgrad<K>, dim3(p.parts, K), dim3(kLkThreads), 0, s, q);
  if (int e = check_launch("lk_wgrad")) return e;
  hipLaunchKernelGGL(k_lk_wgrad_reduce, dim3((K * K * K + 255) / 256), dim3(256), 0, s, (const float*)ws, dw, K, LkWgCfg<K>::NT, p.parts);
  return check_launch("lk_wgrad_reduce");
}

#define NC_LK_CASES(X) X(3) X(5) X(7) X(9) X(11) X(13) X(15) X(17) X(19) X(21) X(23) X(25) X(27) X(29) X(31)

int lk_fwd_any(const float* x, const float* w, float* y, int N, int D, int H, int W, int k, int flip, hipStream_t s) {
  switch (k) {
#define X(KK) case KK: return lk_fwd_launch<KK>(x, w, y, N, D, H, W, flip, s);
    NC_LK_CASES(X)
#undef X
  }
  set_error("lk: kernel size %d", k);
  return NC_ERR_SHAPE;
}

int lk_wgrad_any(const float* x, const float* dy, float* dw, int N, int D, int H, int W, int k, void* ws, hipStream_t s) {
  switch (k) {
#define X(KK) case KK: return lk_wgrad_launch<KK>(x, dy, dw, N, D, H, W, ws, s);
    NC_LK_CASES(X)
#undef X
  }
  set_error("lk: kernel size %d", k);
  return NC_ERR_SHAPE;
}

int lk_args(const char* what, ConvDims& d, const void* a, const void* b, const void* c, int N, int D, int H, int W, int k) {
  if (!a || !b || !c) { set_error("%s: null pointer", what); return NC_ERR_ARG; }
  if (!lk_shape_ok(N, D, H, W, k)) {
    set_error("%s: bad shape N=%d D=%d H=%d W=%d k=%d (odd k in 3 .. 31, extents >= 1)", what, N, D, H, W, k);
    return NC_ERR_SHAPE;
  }
  // profiler record: a Conv3d(1, 1, k, padding (k - 1) / 2) (the geometry check of make_dims holds for every odd k and extent >= 1)
  make_dims(d, N, 1, D, H, W, 1, k, k, k, 1, k / 2);
  return NC_OK;
}

}  // namespace
}  // namespace nc

using namespace nc;

extern "C" {

size_t nc_lk_ws_bytes(int N, int D, int H, int W, int k) {
  if (!lk_shape_ok(N, D, H, W, k)) return 0;
  const LkWgPlan p = lk_wg_plan(N, D, H, W, k);
  const int nt = (k + 15) / 16;
  return (size_t)p.parts * k * 256 * nt * nt * sizeof(float);
}

// LinearKernel(_double).forward: self.convlayer(inputs) (networks.py:852-854, 868-871)
int nc_lk_fwd(const float* x, const float* w, float* y, int N, int D, int H, int W, int k, void* ws, size_t ws_bytes, void* stream) {
  (void)ws; (void)ws_bytes;
  ConvDims d;
  if (int e = lk_args("lk_fwd", d, x, w, y, N, D, H, W, k)) return e;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(0, kPathLk, d, 0, s);
  return lk_fwd_any(x, w, y, N, D, H, W, k, 0, s);
}

// its input gradient (loss.backward(), networks.py:840-871): the same kernel with the weights flipped
int nc_lk_dgrad(const float* dy, const float* w, float* dx, int N, int D, int H, int W, int k, void* ws, size_t ws_bytes, void* stream) {
  (void)ws; (void)ws_bytes;
  ConvDims d;
  if (int e = lk_args("lk_dgrad", d, dy, w, dx, N, D, H, W, k)) return e;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(1, kPathLk, d, 0, s);
  return lk_fwd_any(dy, w, dx, N, D, H, W, k, 1, s);
}

// its weight gradient (networks.py:840-871, loss.backward())
int nc_lk_wgrad(const float* x, const float* dy, float* dw, int N, int D, int H, int W, int k, void* ws, size_t ws_bytes, void* stream) {
  ConvDims d;
  if (int e = lk_args("lk_wgrad", d, x, dy, dw, N, D, H, W, k)) return e;
  const size_t need = nc_lk_ws_bytes(N, D, H, W, k);
  if (!ws || ws_bytes < need) { set_error("lk_wgrad: workspace %zu < %zu bytes", ws_bytes, need); return NC_ERR_WS; }
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(2, kPathLk, d, 0, s);
  return lk_wgrad_any(x, dy, dw, N, D, H, W, k, ws, s);
}

}  // extern "C"
