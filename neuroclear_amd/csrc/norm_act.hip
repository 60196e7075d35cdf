// InstanceNorm(affine=False) + ReLU/LeakyReLU (forward, backward), LeakyReLU, Sigmoid, MaxPool(2): the HBM-bound
// elementwise / reduction part of the hot path (reference models/networks.py:33-34,:422-423,:1042-1046,:491,:510).
// All of these are pure streams: 16-byte loads where the instance length allows it, fp64 accumulation for every
// statistic (1.26 M elements per instance at 108^3 -- fp32 sums would not hold the stated tolerance).
#include <atomic>

#include "common.hpp"
#include "s3_common.hpp"

namespace nc {

static constexpr int kMaxSplits = 64;

static int pick_splits(int NC, long S) {
  long want = cdiv(2048, NC);
  long cap = cdiv(S, 8192);
  long s = want < cap ? want : cap;
  if (s < 1) s = 1;
  if (s > kMaxSplits) s = kMaxSplits;
  return (int)s;
}

__device__ __forceinline__ void block_reduce2(double& a, double& b, double* out2) {
  __shared__ double red[2][4];
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_down(a, o);
    b += __shfl_down(b, o);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wv] = a;
    red[1][wv] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out2[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    out2[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

__device__ __forceinline__ void chunk_range(long S, int splits, int sp, long& b, long& e) {
  long chunk = (S + splits - 1) / splits;
  chunk = (chunk + 3) & ~3L;
  b = (long)sp * chunk;
  e = b + chunk < S ? b + chunk : S;
  if (b > S) b = S;
}

__global__ __launch_bounds__(256) void k_in_stats(const float* __restrict__ x, long S, int splits,
                                                  double* __restrict__ part) {
  const int inst = blockIdx.y, sp = blockIdx.x;
  long b, e;
  chunk_range(S, splits, sp, b, e);
  const float* p = x + (long)inst * S;
  double s = 0.0, q = 0.0;
  if ((S & 3) == 0 && ((uintptr_t)x & 15) == 0) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
    for (long i = b / 4 + threadIdx.x; i < e / 4; i += 256) {
      const float4 v = p4[i];
      const double a0 = v.x, a1 = v.y, a2 = v.z, a3 = v.w;
      s += (a0 + a1) + (a2 + a3);
      q = fma(a0, a0, q); q = fma(a1, a1, q); q = fma(a2, a2, q); q = fma(a3, a3, q);
    }
  } else {
    for (long i = b + threadIdx.x; i < e; i += 256) {
      const double a = p[i];
      s += a;
      q = fma(a, a, q);
    }
  }
  block_reduce2(s, q, part + ((long)inst * splits + sp) * 2);
}

__global__ void k_in_finalize(const double* __restrict__ part, int NC, int splits, long S, float eps,
                              float* __restrict__ mean, float* __restrict__ rstd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NC) return;
  double s = 0.0, q = 0.0;
  for (int k = 0; k < splits; ++k) {
    s += part[((long)i * splits + k) * 2];
    q += part[((long)i * splits + k) * 2 + 1];
  }
  const double m = s / (double)S;
  double var = q / (double)S - m * m;
  if (var < 0.0) var = 0.0;
  mean[i] = (float)m;
  rstd[i] = (float)(1.0 / sqrt(var + (double)eps));
}

__global__ __launch_bounds__(256) void k_in_act_fwd(const float* __restrict__ x, const float* __restrict__ mean,
                                                    const float* __restrict__ rstd, float slope,
                                                    float* __restrict__ y, long S) {
  const int inst = blockIdx.y;
  const float m = mean[inst], r = rstd[inst];
  const float* p = x + (long)inst * S;
  float* o = y + (long)inst * S;
  if ((S & 3) == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
    float4* o4 = reinterpret_cast<float4*>(o);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < S / 4; i += (long)gridDim.x * 256) {
      float4 v = p4[i];
      v.x = in_act(v.x, m, r, slope); v.y = in_act(v.y, m, r, slope); v.z = in_act(v.z, m, r, slope); v.w = in_act(v.w, m, r, slope);
      o4[i] = v;
    }
  } else {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < S; i += (long)gridDim.x * 256) o[i] = in_act(p[i], m, r, slope);
  }
}

// pass 1 of the backward: s1 = sum(g), s2 = sum(g * xhat), g = dy * act'(xhat)
// U (nc_set_stream_passes: 8, off: 1): the loads of U iterations are issued before the first of them is used, as in k_in_bwd_sums_h2 below.  A
// thread's element sequence i = b + tid + 256 k and the order of its additions do not depend on U: the sums have the same bits.
template <int U = 1>
__global__ __launch_bounds__(256) void k_in_bwd_sums(const float* __restrict__ dy, const float* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     float slope, long S, int splits, double* __restrict__ part) {
  const int inst = blockIdx.y, sp = blockIdx.x;
  long b, e;
  chunk_range(S, splits, sp, b, e);
  const float m = mean[inst], r = rstd[inst];
  const float* px = x + (long)inst * S;
  const float* pg = dy + (long)inst * S;
  double s1 = 0.0, s2 = 0.0;
  auto add = [&](float xv, float gy) {
    const float xh = (xv - m) * r;
    const float g = xh > 0.f ? gy : gy * slope;
    s1 += (double)g;
    s2 = fma((double)g, (double)xh, s2);
  };
  long i = b + threadIdx.x;
  if constexpr (U > 1) {
    for (; i + (long)(U - 1) * 256 < e; i += (long)U * 256) {
      float xv[U], gv[U];
#pragma unroll
      for (int k = 0; k < U; ++k) xv[k] = px[i + k * 256];
#pragma unroll
      for (int k = 0; k < U; ++k) gv[k] = pg[i + k * 256];
#pragma unroll
      for (int k = 0; k < U; ++k) add(xv[k], gv[k]);
    }
  }
  for (; i < e; i += 256) add(px[i], pg[i]);
  block_reduce2(s1, s2, part + ((long)inst * splits + sp) * 2);
}

// dx of InstanceNorm (affine = False) + (Leaky)ReLU for one element, with every rounding spelled out: the fp32, 16-bit (C8) and three-term (S3)
// forms of this backward must store the SAME value (tests compare the whole-network calls with the layer-by-layer path bit for bit),
// which the compiler's own choice of fused multiply-adds per kernel does not guarantee.
__device__ __forceinline__ float in_bwd_value(float xv, float gy, float m, float r, float m1, float m2, float slope) {
  const float xh = (xv - m) * r;
  const float g = xh > 0.f ? gy : gy * slope;
  float p = xh * m2;
  asm("" : "+v"(p));  // (keeps the backend from fusing this product into the subtraction: hipcc contracts at -ffp-contract=fast)
  return r * ((g - m1) - p);
}

// U: as in k_in_bwd_sums -- the same i = blockIdx.x * 256 + tid + k * gridDim.x * 256 per thread, the same order of the fp64 additions, plain tail.
// A workgroup of this grid lives for about five iterations, so what it does before the first load counts: the loads of the first round are
// issued BEFORE the partial sums are added up (they do not depend on them), and the partials are loaded eight at a time: the means are ready
// when the data arrives.
template <int U = 1>
__global__ __launch_bounds__(256) void k_in_bwd_apply(const float* __restrict__ dy, const float* __restrict__ x,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                      float slope, long S, int splits,
                                                      const double* __restrict__ part, float* __restrict__ dx,
                                                      double* __restrict__ rowpart) {
  const int inst = blockIdx.y;
  const float* px = x + (long)inst * S;
  const float* pg = dy + (long)inst * S;
  float* o = dx + (long)inst * S;
  const long st = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  float xv[U], gv[U];
  bool round = U > 1 && i + (U - 1) * st < S;
  if constexpr (U > 1) {
    if (round) {
#pragma unroll
      for (int k = 0; k < U; ++k) xv[k] = px[i + k * st];
#pragma unroll
      for (int k = 0; k < U; ++k) gv[k] = pg[i + k * st];
    }
  }
  double s1 = 0.0, s2 = 0.0;
  int k0 = 0;
  if constexpr (U > 1) {  // (eight partials per round of loads instead of one load waited for per partial; added in the same order)
    for (; k0 + 8 <= splits; k0 += 8) {
      double a[8], b[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { a[j] = part[((long)inst * splits + k0 + j) * 2]; b[j] = part[((long)inst * splits + k0 + j) * 2 + 1]; }
#pragma unroll
      for (int j = 0; j < 8; ++j) { s1 += a[j]; s2 += b[j]; }
    }
  }
  for (int k = k0; k < splits; ++k) {
    s1 += part[((long)inst * splits + k) * 2];
    s2 += part[((long)inst * splits + k) * 2 + 1];
  }
  const float m1 = (float)(s1 / (double)S), m2 = (float)(s2 / (double)S);
  const float m = mean[inst], r = rstd[inst];
  double rs = 0.0;
  if constexpr (U > 1) {
    // (a SECOND round needs more than 2 U iterations per thread, i.e. the grid capped at 1024 workgroups and S >= 8 x 262 144 voxels: the step's
    // 108^3 has 4.8 iterations, one round and the tail; tests/test_gpu_stream_passes.py runs the refill at 2.2 M voxels)
    while (round) {
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const float v = in_bwd_value(xv[k], gv[k], m, r, m1, m2, slope);
        o[i + k * st] = v;
        rs += (double)v;
      }
      i += U * st;
      round = i + (U - 1) * st < S;
      if (round) {
#pragma unroll
        for (int k = 0; k < U; ++k) xv[k] = px[i + k * st];
#pragma unroll
        for (int k = 0; k < U; ++k) gv[k] = pg[i + k * st];
      }
    }
  }
  for (; i < S; i += st) {
    const float v = in_bwd_value(px[i], pg[i], m, r, m1, m2, slope);
    o[i] = v;
    rs += (double)v;
  }
  // rowpart (nullable): sum of this block's share of dx -- dx is the gradient with respect to the output of the
  // convolution in front of the norm, so its per-channel sum is that convolution's bias gradient, and taking it here
  // saves the separate pass over dx (nc_conv_wgrad with dbias) that would otherwise compute it
  if (rowpart) {
    double zero = 0.0, out2[2];
    block_reduce2(rs, zero, out2);
    if (threadIdx.x == 0) rowpart[(long)inst * gridDim.x + blockIdx.x] = out2[0];
  }
}

// dbias[c] = sum over samples n and blocks b of rowpart[(n * C + c) * nb + b]: one workgroup per channel, fixed
// assignment and tree order (deterministic)
__global__ __launch_bounds__(256) void k_in_dbias_final(const double* __restrict__ rowpart, int N, int C, int nb,
                                                        float* __restrict__ dbias) {
  const int c = blockIdx.x;
  double s = 0.0, zero = 0.0;
  const int total = N * nb;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int n = i / nb, b = i - n * nb;
    s += rowpart[((long)n * C + c) * nb + b];
  }
  __shared__ double out2[2];
  block_reduce2(s, zero, out2);
  if (threadIdx.x == 0) dbias[c] = (float)out2[0];
}
// k_in_dbias_final and, in workgroup 0, the range guard's decision about the tensor the apply pass wrote (k_h2_guard_decide's, counted only:
// h2_guard_decide_one with can_flip = 0) -- one launch for the two; neither waits for the other
__global__ __launch_bounds__(256) void k_in_dbias_final_decide(const double* __restrict__ rowpart, int N, int C, int nb, float* __restrict__ dbias,
                                                               unsigned* guard, unsigned long long* stats, unsigned long long total) {
  const int c = blockIdx.x;
  double s = 0.0, zero = 0.0;
  const int tot = N * nb;
  for (int i = threadIdx.x; i < tot; i += 256) {
    const int n = i / nb, b = i - n * nb;
    s += rowpart[((long)n * C + c) * nb + b];
  }
  __shared__ double out2[2];
  block_reduce2(s, zero, out2);
  if (threadIdx.x == 0) dbias[c] = (float)out2[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) h2_guard_decide_one(guard, nullptr, nullptr, guard + kGuardFlag, 0, stats, total);
}

// ---- short instances (S <= kRowsMaxS: the 2-D PatchGAN layers, 12^2 .. 27^2 positions x tens of thousands of
//      instances, and the deepest U-Net levels): a group of G lanes owns one instance, so a workgroup covers 256 / G of
//      them, the reductions are shuffles inside the group (no LDS, no barrier, no partial-sum pass) and statistics,
//      normalisation and activation are ONE kernel -- the second sweep over the instance hits L2.
static constexpr long kRowsMaxS = 2048;

template <int G>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);  // butterfly: every lane of the group ends with the same bits
  return v;
}

// MODE 0: statistics only; 1: normalise + activation with the statistics given; 2: both
template <int G, int MODE>
__global__ __launch_bounds__(256) void k_in_fwd_rows(const float* __restrict__ x, long NC, int S, float eps, float slope,
                                                     float* __restrict__ mean, float* __restrict__ rstd,
                                                     float* __restrict__ y) {
  const int sub = threadIdx.x % G;
  const long inst = (long)blockIdx.x * (256 / G) + threadIdx.x / G;
  if (inst >= NC) return;
  const float* p = x + inst * S;
  float m, r;
  if constexpr (MODE != 1) {
    double s = 0.0, q = 0.0;
#pragma unroll 4
    for (int i = sub; i < S; i += G) {
      const double a = p[i];
      s += a;
      q = fma(a, a, q);
    }
    s = group_sum<G>(s);
    q = group_sum<G>(q);
    const double mm = s / (double)S;
    double var = q / (double)S - mm * mm;
    if (var < 0.0) var = 0.0;
    m = (float)mm;
    r = (float)(1.0 / sqrt(var + (double)eps));
    if (sub == 0) {
      mean[inst] = m;
      rstd[inst] = r;
    }
  } else {
    m = mean[inst];
    r = rstd[inst];
  }
  if constexpr (MODE != 0) {
    float* o = y + inst * S;
#pragma unroll 4
    for (int i = sub; i < S; i += G) {
      const float v = (p[i] - m) * r;
      o[i] = v > 0.f ? v : v * slope;
    }
  }
}

// backward of the same: both sums, then dx, in one kernel; rowsum (nullable) [inst] = sum of dx over the instance (the
// bias gradient of the convolution in front of the norm, see k_in_bwd_apply)
template <int G>
__global__ __launch_bounds__(256) void k_in_bwd_rows(const float* __restrict__ dy, const float* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     float slope, long NC, int S, float* __restrict__ dx,
                                                     double* __restrict__ rowsum) {
  const int sub = threadIdx.x % G;
  const long inst = (long)blockIdx.x * (256 / G) + threadIdx.x / G;
  if (inst >= NC) return;
  const float m = mean[inst], r = rstd[inst];
  const float* px = x + inst * S;
  const float* pg = dy + inst * S;
  float* o = dx + inst * S;
  double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
  for (int i = sub; i < S; i += G) {
    const float xh = (px[i] - m) * r;
    const float g = xh > 0.f ? pg[i] : pg[i] * slope;
    s1 += (double)g;
    s2 = fma((double)g, (double)xh, s2);
  }
  s1 = group_sum<G>(s1);
  s2 = group_sum<G>(s2);
  const float m1 = (float)(s1 / (double)S), m2 = (float)(s2 / (double)S);
  double rs = 0.0;
#pragma unroll 4
  for (int i = sub; i < S; i += G) {
    const float v = in_bwd_value(px[i], pg[i], m, r, m1, m2, slope);
    o[i] = v;
    rs += (double)v;
  }
  if (rowsum) {
    rs = group_sum<G>(rs);
    if (sub == 0) rowsum[inst] = rs;
  }
}

static inline bool rows_path(long S) {
  return S <= kRowsMaxS;
}

template <int MODE>
static void launch_fwd_rows(const float* x, long NC, long S, float eps, float slope, float* mean, float* rstd, float* y,
                            hipStream_t s) {
  if (S <= 256)
    hipLaunchKernelGGL((k_in_fwd_rows<16, MODE>), dim3((unsigned)cdiv(NC, 16)), dim3(256), 0, s, x, NC, (int)S, eps, slope, mean,
                       rstd, y);
  else
    hipLaunchKernelGGL((k_in_fwd_rows<64, MODE>), dim3((unsigned)cdiv(NC, 4)), dim3(256), 0, s, x, NC, (int)S, eps, slope, mean,
                       rstd, y);
}

static void launch_bwd_rows(const float* dy, const float* x, const float* mean, const float* rstd, float slope, long NC, long S,
                            float* dx, double* rowsum, hipStream_t s) {
  if (S <= 256)
    hipLaunchKernelGGL((k_in_bwd_rows<16>), dim3((unsigned)cdiv(NC, 16)), dim3(256), 0, s, dy, x, mean, rstd, slope, NC, (int)S, dx,
                       rowsum);
  else
    hipLaunchKernelGGL((k_in_bwd_rows<64>), dim3((unsigned)cdiv(NC, 4)), dim3(256), 0, s, dy, x, mean, rstd, slope, NC, (int)S, dx,
                       rowsum);
}

// ---- the same two kernels for the 16-bit convolution path (conv_h.hip): next to the fp32 result they emit it in the
//      C8 operand layout of those kernels ([N][C/8][voxels][8 channels] bf16 / fp16), so the convolution that consumes it
//      does not run a conversion pass of its own.  One thread = one voxel of 8 consecutive channels (C % 8 == 0).
template <int DT>
__device__ __forceinline__ unsigned short cvt16n(float f) {
  if constexpr (DT == NC_DT_F16) {
    const _Float16 v = (_Float16)f;
    return __builtin_bit_cast(unsigned short, v);
  } else {
    const __bf16 v = (__bf16)f;
    return __builtin_bit_cast(unsigned short, v);
  }
}
__device__ __forceinline__ uint4 pack8(const unsigned short (&e)[8]) {
  uint4 o;
  o.x = e[0] | ((unsigned)e[1] << 16); o.y = e[2] | ((unsigned)e[3] << 16);
  o.z = e[4] | ((unsigned)e[5] << 16); o.w = e[6] | ((unsigned)e[7] << 16);
  return o;
}

template <int DT>
__global__ __launch_bounds__(256) void k_in_act_fwd_c8(const float* __restrict__ x, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, float slope, float* __restrict__ y,
                                                       uint4* __restrict__ yh, long S) {
  const long ncb = blockIdx.y;  // n * (C/8) + cb: instances ncb*8 .. ncb*8+7
  float m[8], r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { m[j] = mean[ncb * 8 + j]; r[j] = rstd[ncb * 8 + j]; }
  const float* px = x + ncb * 8 * S;
  float* py = y ? y + ncb * 8 * S : nullptr;  // y == NULL: only the C8 copy is wanted (16-bit end-to-end path)
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < S; v += (long)gridDim.x * 256) {
    unsigned short e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float t = (px[j * S + v] - m[j]) * r[j];
      t = t > 0.f ? t : t * slope;
      if (py) py[j * S + v] = t;
      e[j] = cvt16n<DT>(t);
    }
    yh[ncb * S + v] = pack8(e);
  }
}

template <int DT>
__global__ __launch_bounds__(256) void k_in_bwd_apply_c8(const float* __restrict__ dy, const float* __restrict__ x,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         float slope, long S, int splits, const double* __restrict__ part,
                                                         float* __restrict__ dx, uint4* __restrict__ dxh,
                                                         double* __restrict__ rowpart) {
  __shared__ float sm[2][8];
  __shared__ double red[8][4];
  const long ncb = blockIdx.y;
  if (threadIdx.x < 8) {
    const long inst = ncb * 8 + threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < splits; ++k) {
      s1 += part[(inst * splits + k) * 2];
      s2 += part[(inst * splits + k) * 2 + 1];
    }
    sm[0][threadIdx.x] = (float)(s1 / (double)S);
    sm[1][threadIdx.x] = (float)(s2 / (double)S);
  }
  __syncthreads();
  float m[8], r[8], m1[8], m2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { m[j] = mean[ncb * 8 + j]; r[j] = rstd[ncb * 8 + j]; m1[j] = sm[0][j]; m2[j] = sm[1][j]; }
  const float* px = x + ncb * 8 * S;
  const float* pg = dy + ncb * 8 * S;
  float* o = dx + ncb * 8 * S;
  double rs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) rs[j] = 0.0;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < S; v += (long)gridDim.x * 256) {
    unsigned short e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float t = in_bwd_value(px[j * S + v], pg[j * S + v], m[j], r[j], m1[j], m2[j], slope);
      o[j * S + v] = t;
      rs[j] += (double)t;
      e[j] = cvt16n<DT>(t);
    }
    dxh[ncb * S + v] = pack8(e);
  }
  if (rowpart) {  // per-channel sums of this block's share of dx (the convolution's bias gradient, see k_in_bwd_apply)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      double a = rs[j];
      for (int of = 32; of > 0; of >>= 1) a += __shfl_down(a, of);
      if (lane == 0) red[j][wv] = a;
    }
    __syncthreads();
    if (threadIdx.x < 8)
      rowpart[(ncb * 8 + threadIdx.x) * gridDim.x + blockIdx.x] =
          (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
  }
}

// The same backward with dx written ONLY in the three-term S3 layout of the split-operand convolutions (s3_common.hpp): dx is the dY
// of the convolution in front of the norm, and when that convolution's gradients run on the split-operand kernels nothing else reads
// it -- no fp32 tensor, no separate conversion pass.  Arithmetic and partial-sum order are k_in_bwd_apply's (the same voxels per
// thread, the same reduction tree per channel): the values split here are bit for bit the values the fp32 pass would have stored.
// R1 (here and in the two H2 kernels below): the incoming gradient is RANK ONE, dy[c][v] = w1[c] * dy[v] with a one-channel dy -- the data
// gradient of a K -> 1 pointwise convolution (Unet_deconv's one_by_one behind its last block), formed on the fly instead of read as a K-channel
// tensor.  r1_product is the value the fp32 matrix kernel of that data gradient stores (one fused multiply-add onto a zero accumulator).
// (Subnormal products included as long as this file is built with fp32 denormals on, the compiler's default for gfx9: the matrix instruction
// keeps them whatever the MODE register says, a flush-to-zero build of this kernel would not -- tests/test_gpu_unet_lean.py has a tiny-w12 case.)
__device__ __forceinline__ float r1_product(float w, float s) {
  float g = __builtin_fmaf(w, s, 0.f);
  asm("" : "+v"(g));  // (a rounded value of its own: never contracted into the arithmetic that consumes it)
  return g;
}

template <bool R1 = false>
__global__ __launch_bounds__(256) void k_in_bwd_apply_s3(const float* __restrict__ dy, const float* __restrict__ x,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         float slope, long S, int splits, const double* __restrict__ part,
                                                         uint4* __restrict__ dxs, int cblocks, double* __restrict__ rowpart,
                                                         const unsigned* __restrict__ guard = nullptr, const float* __restrict__ w1 = nullptr) {
  __shared__ float sm[2][8];
  __shared__ double red[8][4];
  if (guard_skip(guard, 1)) return;  // (the range guard's fallback of k_in_bwd_apply_h2: runs only for a flagged tensor)
  const long ncb = blockIdx.y;
  if (threadIdx.x < 8) {
    const long inst = ncb * 8 + threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < splits; ++k) {
      s1 += part[(inst * splits + k) * 2];
      s2 += part[(inst * splits + k) * 2 + 1];
    }
    sm[0][threadIdx.x] = (float)(s1 / (double)S);
    sm[1][threadIdx.x] = (float)(s2 / (double)S);
  }
  __syncthreads();
  float m[8], r[8], m1[8], m2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { m[j] = mean[ncb * 8 + j]; r[j] = rstd[ncb * 8 + j]; m1[j] = sm[0][j]; m2[j] = sm[1][j]; }
  const float* px = x + ncb * 8 * S;
  const float* pg = R1 ? dy : dy + ncb * 8 * S;
  float wj[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) wj[j] = R1 ? w1[ncb * 8 + j] : 0.f;
  double rs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) rs[j] = 0.0;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < S; v += (long)gridDim.x * 256) {
    unsigned short e[8][3];
    const float sv = R1 ? pg[v] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float t = in_bwd_value(px[j * S + v], R1 ? r1_product(wj[j], sv) : pg[j * S + v], m[j], r[j], m1[j], m2[j], slope);
      rs[j] += (double)t;
      s3_split(t, e[j]);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) dxs[(ncb * 3 + t) * S + v] = s3_unit(e, t);  // [N][C/8][3][S] units: block index ncb = n * C/8 + cb
  }
  if (rowpart) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      double a = rs[j];
      for (int of = 32; of > 0; of >>= 1) a += __shfl_down(a, of);
      if (lane == 0) red[j][wv] = a;
    }
    __syncthreads();
    if (threadIdx.x < 8)
      rowpart[(ncb * 8 + threadIdx.x) * gridDim.x + blockIdx.x] =
          (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
  }
}

// ---- the same backward writing dx in the H2 form (two fp16 terms of dx * 2^k, s3_common.hpp / h2.hip).  The power of two must be known
// before the first element is written, and dx is not: pass 1 also takes max |g| and max |xhat| per instance, and
//   |dx| = r |g - mean(g) - xhat mean(g xhat)| <= r max|g| (2 + max|xhat|)      (|mean(g xhat)| <= rms(g) rms(xhat) <= max|g|)
// bounds the tensor from above within a small factor -- fp16's exponent range has room for that (s3_common.hpp).
// R1 (one sample: inst = channel): the K-channel gradient does not exist as a tensor
// POOL (k_in_bwd_sums_h2, k_in_bwd_apply_h2): the block's output feeds a MaxPool3d(2) AND a skip connection, and the gradient at it is formed per
// element instead of read from a tensor the pool's backward wrote: skip[i] + (the pooled gradient where i is its window's winner, else 0) -- the one
// fp32 add k_maxpool2_bwd<true> stores.  The winner is a byte per pooled element left by the forward (k_maxpool2_fwd<true>, pool_winner's index).
struct PoolGrad {
  const float* gp;           // dense pooled gradient [N][C][Sp]
  const unsigned char* arg;  // winner index 0..7 per pooled element, same layout
  long skip_stride;          // floats between the samples of the skip gradient (`dy`)
  long Sp;                   // Do * Ho * Wo
  int C, H, W, Ho, Wo;
};
// voxel i of a D x H x W volume (i < 2^31) -> its pooled element and its place 0..7 inside the window
__device__ __forceinline__ void pool_site(unsigned i, const PoolGrad& q, unsigned& w, unsigned& pos) {
  const unsigned x = i % (unsigned)q.W, t = i / (unsigned)q.W, y = t % (unsigned)q.H, z = t / (unsigned)q.H;
  w = ((z >> 1) * (unsigned)q.Ho + (y >> 1)) * (unsigned)q.Wo + (x >> 1);
  pos = ((z & 1u) * 2u + (y & 1u)) * 2u + (x & 1u);
}
__device__ __forceinline__ float pool_grad_value(float skip, unsigned arg, unsigned pos, float gp) {
  float g = skip + (arg == pos ? gp : 0.f);
  asm("" : "+v"(g));  // (a rounded value of its own, as the tensor element it replaces was)
  return g;
}

// U: the loads of U iterations are issued before the first of them is used (U = 1: one iteration at a time).  A thread's element sequence
// i = b + tid + 256 k and the order of its additions do not depend on U: the sums have the same bits.  The loop with U = 1 keeps 32 waves x
// 2 dwords in flight per CU, about a third of what the memory system needs to stream at full rate (k_in_stats gets there with 16-byte loads,
// which would change which thread adds what).
template <bool R1 = false, bool POOL = false, int U = 1>
__global__ __launch_bounds__(256) void k_in_bwd_sums_h2(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, float slope, long S, int splits,
                                                        double* __restrict__ part, unsigned* __restrict__ gmax, unsigned* __restrict__ xmax,
                                                        const float* __restrict__ w1, PoolGrad pq) {
  const int inst = blockIdx.y, sp = blockIdx.x;
  long b, e;
  chunk_range(S, splits, sp, b, e);
  const float m = mean[inst], r = rstd[inst];
  const float* px = x + (long)inst * S;
  const float* pg = R1 ? dy : POOL ? dy + (long)(inst / pq.C) * pq.skip_stride + (long)(inst % pq.C) * S : dy + (long)inst * S;
  const float* pp = POOL ? pq.gp + (long)inst * pq.Sp : nullptr;
  const unsigned char* pa = POOL ? pq.arg + (long)inst * pq.Sp : nullptr;
  const float w = R1 ? w1[inst] : 0.f;
  double s1 = 0.0, s2 = 0.0;
  unsigned gm = 0, xm = 0;
  auto load_g = [&](long i) -> float {
    if constexpr (POOL) {
      unsigned wi, pos;
      pool_site((unsigned)i, pq, wi, pos);
      return pool_grad_value(pg[i], pa[wi], pos, pp[wi]);
    } else {
      return pg[i];
    }
  };
  auto add = [&](float xv, float gl) {
    const float xh = (xv - m) * r;
    const float gy = R1 ? r1_product(w, gl) : gl;
    const float g = xh > 0.f ? gy : gy * slope;
    s1 += (double)g;
    s2 = fma((double)g, (double)xh, s2);
    const unsigned gb = __float_as_uint(g) & 0x7fffffffu, xb = __float_as_uint(xh) & 0x7fffffffu;
    if (gb < 0x7f800000u && gb > gm) gm = gb;
    if (xb < 0x7f800000u && xb > xm) xm = xb;
  };
  long i = b + threadIdx.x;
  if constexpr (U > 1) {
    for (; i + (long)(U - 1) * 256 < e; i += (long)U * 256) {
      float xv[U], gv[U];
#pragma unroll
      for (int k = 0; k < U; ++k) xv[k] = px[i + k * 256];
#pragma unroll
      for (int k = 0; k < U; ++k) gv[k] = load_g(i + k * 256);
#pragma unroll
      for (int k = 0; k < U; ++k) add(xv[k], gv[k]);
    }
  }
  for (; i < e; i += 256) add(px[i], load_g(i));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned q1 = (unsigned)__shfl_xor((int)gm, o), q2 = (unsigned)__shfl_xor((int)xm, o);
    gm = q1 > gm ? q1 : gm; xm = q2 > xm ? q2 : xm;
  }
  if ((threadIdx.x & 63) == 0) {
    if (gm) atomicMax(gmax + inst, gm);
    if (xm) atomicMax(xmax + inst, xm);
  }
  block_reduce2(s1, s2, part + ((long)inst * splits + sp) * 2);
}

// this thread's share of the tensor's bound (see above), reduced over its wave: max over instances of rstd max|g| (2 + max|xhat|), as float bits
__device__ __forceinline__ unsigned in_bwd_bound_wave(const float* __restrict__ rstd, const unsigned* __restrict__ gmax,
                                                      const unsigned* __restrict__ xmax, int NC) {
  unsigned m = 0;
  for (int i = threadIdx.x; i < NC; i += 256) {
    const float bnd = rstd[i] * __uint_as_float(gmax[i]) * (2.f + __uint_as_float(xmax[i]));
    const unsigned b = __float_as_uint(bnd) & 0x7fffffffu;
    if (b < 0x7f800000u && b > m) m = b;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned q = (unsigned)__shfl_xor((int)m, o);
    m = q > m ? q : m;
  }
  return m;
}

__global__ __launch_bounds__(256) void k_in_bwd_bound(const float* __restrict__ rstd, const unsigned* __restrict__ gmax,
                                                      const unsigned* __restrict__ xmax, int NC, unsigned* __restrict__ cell,
                                                      unsigned* __restrict__ cell2, unsigned* __restrict__ guard) {
  if (guard && threadIdx.x < 8) guard[threadIdx.x] = 0u;  // (the range guard's words of the tensor the apply pass is about to write)
  const unsigned m = in_bwd_bound_wave(rstd, gmax, xmax, NC);
  if ((threadIdx.x & 63) == 0 && m) {
    atomicMax(cell, m);
    atomicMax(cell2, m);
  }
}

// q (nullable): nq <= 256 more words somewhere else (the folded norm backward: the range guard's words)
__global__ void k_zero_u32(unsigned* p, int n, unsigned* q, int nq) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0u;
  if (q && blockIdx.x == 0 && (int)threadIdx.x < nq) q[threadIdx.x] = 0u;
}

// FOLD: no k_in_bwd_bound launch in front -- every workgroup takes the tensor's bound itself from rstd / gmax / xmax (a maximum over at most a few
// hundred words that sit in L2: the same bits in every workgroup, whatever the order), and workgroup (0, 0) stores it in the two cells for the
// convolution kernels behind this pass.  Nothing waits for another workgroup.
// STAGE (nc_set_stream_passes, the folded rank-one form): every load of an iteration -- the eight raw channels and the one-channel gradient -- is
// issued before the first of them is used.  Left to itself the compiler schedules that instance's loop as nine loads each waited for in turn (the
// unfolded instance of the same source and the plain forms get all of them in flight).  Same values, same additions in the same order.
template <bool R1 = false, bool POOL = false, bool FOLD = false, bool STAGE = false>
__global__ __launch_bounds__(256) void k_in_bwd_apply_h2(const float* __restrict__ dy, const float* __restrict__ x,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         float slope, long S, int splits, const double* __restrict__ part,
                                                         uint4* __restrict__ dxs, int cblocks, double* __restrict__ rowpart,
                                                         const unsigned* cell, unsigned* __restrict__ guard,
                                                         const float* __restrict__ w1, PoolGrad pq, const unsigned* gmax, const unsigned* xmax,
                                                         int NC, unsigned* cells_out) {
  __shared__ float sm[2][8];
  __shared__ double red[8][4];
  __shared__ unsigned bmax[4];
  const long ncb = blockIdx.y;
  if (threadIdx.x < 8) {
    const long inst = ncb * 8 + threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < splits; ++k) {
      s1 += part[(inst * splits + k) * 2];
      s2 += part[(inst * splits + k) * 2 + 1];
    }
    sm[0][threadIdx.x] = (float)(s1 / (double)S);
    sm[1][threadIdx.x] = (float)(s2 / (double)S);
  }
  if constexpr (FOLD) {
    const unsigned bw = in_bwd_bound_wave(rstd, gmax, xmax, NC);
    if ((threadIdx.x & 63) == 0) bmax[threadIdx.x >> 6] = bw;
  }
  __syncthreads();
  unsigned cbits_;
  if constexpr (FOLD) {
    const unsigned b01 = bmax[0] > bmax[1] ? bmax[0] : bmax[1], b23 = bmax[2] > bmax[3] ? bmax[2] : bmax[3];
    cbits_ = b01 > b23 ? b01 : b23;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { cells_out[0] = cbits_; cells_out[1] = cbits_; }
  } else {
    cbits_ = *cell;
  }
  const unsigned cbits = cbits_;
  const float sc = h2_scale(cbits);
  unsigned n_zero = 0, n_low = 0;  // (wave-uniform: every lane counts the same chunks)
  float m[8], r[8], m1[8], m2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { m[j] = mean[ncb * 8 + j]; r[j] = rstd[ncb * 8 + j]; m1[j] = sm[0][j]; m2[j] = sm[1][j]; }
  const float* px = x + ncb * 8 * S;
  // (POOL: the 8 channels of a block lie in one sample, C % 8 == 0)
  const float* pg = R1 ? dy : POOL ? dy + (ncb * 8 / pq.C) * pq.skip_stride + (ncb * 8 % pq.C) * S : dy + ncb * 8 * S;
  const float* pp = POOL ? pq.gp + ncb * 8 * pq.Sp : nullptr;
  const unsigned char* pa = POOL ? pq.arg + ncb * 8 * pq.Sp : nullptr;
  float wj[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) wj[j] = R1 ? w1[ncb * 8 + j] : 0.f;
  double rs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) rs[j] = 0.0;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < S; v += (long)gridDim.x * 256) {
    unsigned short e[8][3];
    unsigned mx = 0;
    const float sv = R1 ? pg[v] : 0.f;
    unsigned wi = 0, pos = 0;
    if constexpr (POOL) pool_site((unsigned)v, pq, wi, pos);
    float gl[8], xv[8];
    if constexpr (STAGE) {
      static_assert(!STAGE || (R1 && !POOL), "the staged loop is the rank-one form's");
#pragma unroll
      for (int j = 0; j < 8; ++j) xv[j] = px[j * S + v];
      // One statement that needs all nine: no load can sink below it, one wait for the nine.  What the backend makes of it is a property of the
      // compiler at hand (ROCm 7.2: nine global_load_dword, one s_waitcnt vmcnt(0), 71 VGPRs, no scratch): read this instance's
      // disassembly again after a compiler upgrade.
      float s0 = sv;
      asm volatile("" : "+v"(xv[0]), "+v"(xv[1]), "+v"(xv[2]), "+v"(xv[3]), "+v"(xv[4]), "+v"(xv[5]), "+v"(xv[6]), "+v"(xv[7]), "+v"(s0));
#pragma unroll
      for (int j = 0; j < 8; ++j) gl[j] = r1_product(wj[j], s0);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if constexpr (R1) gl[j] = r1_product(wj[j], sv);
        else if constexpr (POOL) gl[j] = pool_grad_value(pg[j * S + v], pa[j * pq.Sp + wi], pos, pp[j * pq.Sp + wi]);
        else gl[j] = pg[j * S + v];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float t = in_bwd_value(STAGE ? xv[j] : px[j * S + v], gl[j], m[j], r[j], m1[j], m2[j], slope);
      rs[j] += (double)t;
      asm("" : "+v"(t));
      const unsigned b = __float_as_uint(t) & 0x7fffffffu;
      if (b < 0x7f800000u && b > mx) mx = b;
      h2_split(t * sc, e[j]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) dxs[(ncb * 2 + t) * S + v] = s3_unit(e, t);  // [N][C/8][2][S] units
    // range guard (common.hpp): this wave's 64 voxels x 8 channels are one chunk.  The lanes of a wave leave the loop together except in the
    // last iteration, so the chunk's maximum is taken over the lanes that are here; zero chunks and low chunks are the rare case: atomics
    // only for those (guard[kGuardAll] counts ZERO chunks here, see k_h2_guard_decide's total_a)
    if (guard) {  // (two ballots, no cross-lane reduction: "does any lane hold a value at or above the threshold / a non-zero value")
      const unsigned thr = cbits > kGuardDrop ? cbits - kGuardDrop : 0u;
      const bool any_hi = __builtin_amdgcn_ballot_w64(mx >= thr && mx != 0) != 0;
      const bool any_nz = __builtin_amdgcn_ballot_w64(mx != 0) != 0;
      if (!any_nz) ++n_zero;
      else if (!any_hi) ++n_low;
    }
  }
  if (guard && (threadIdx.x & 63) == 0) {
    if (n_low) atomicAdd(guard + kGuardLow, n_low);
    if (n_zero) atomicAdd(guard + kGuardAll, n_zero);
  }
  if (rowpart) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      double a = rs[j];
      for (int of = 32; of > 0; of >>= 1) a += __shfl_down(a, of);
      if (lane == 0) red[j][wv] = a;
    }
    __syncthreads();
    if (threadIdx.x < 8)
      rowpart[(ncb * 8 + threadIdx.x) * gridDim.x + blockIdx.x] =
          (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
  }
}


__global__ void k_lrelu_fwd(const float* __restrict__ x, float slope, float* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = x[i];
    y[i] = v > 0.f ? v : v * slope;
  }
}
__global__ void k_lrelu_bwd(const float* __restrict__ dy, const float* __restrict__ x, float slope,
                            float* __restrict__ dx, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    dx[i] = x[i] > 0.f ? dy[i] : dy[i] * slope;
}
// The inference tail of Unet_deconv in ONE pass over the last block's raw convolution output (networks.py:533-537: InstanceNorm + ReLU,
// one_by_one 64 -> 1, one_by_one_2 1 -> 1, Sigmoid): y[v] = sigmoid(w2 * (b1 + sum_c w1[c] * relu((x[c][v] - mean[c]) * rstd[c])) + b2).  The
// separate passes wrote the 64-channel activation and read it back (1.4 GB per 140^3 cube) for one output channel.
__global__ void __launch_bounds__(256) k_in_act_tail(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                     const float* __restrict__ b2, float* __restrict__ y, long S, int C) {
  __shared__ float sm[3][256];
  for (int c = threadIdx.x; c < C; c += 256) { sm[0][c] = mean[c]; sm[1][c] = rstd[c]; sm[2][c] = w1[c]; }
  __syncthreads();
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= S) return;
  float acc = 0.f;
  for (int c = 0; c < C; ++c) {
    float t = (x[(long)c * S + v] - sm[0][c]) * sm[1][c];
    t = t > 0.f ? t : 0.f;
    acc = fmaf(sm[2][c], t, acc);
  }
  const float t1 = acc + b1[0];
  const float t2 = fmaf(w2[0], t1, b2[0]);
  y[v] = 1.f / (1.f + expf(-t2));
}

__global__ void k_sigmoid_fwd(const float* __restrict__ x, float* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    y[i] = 1.f / (1.f + expf(-x[i]));
}
__global__ void k_sigmoid_bwd(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx,
                              long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float s = y[i];
    dx[i] = dy[i] * s * (1.f - s);
  }
}

// MaxPool(2), floor mode.  H2 = 1 turns it into a 2-D pool is NOT needed: the reference only pools 3-D volumes
// in Unet_deconv; D may still be 1 for a 2-D U-Net (pool window 1x2x2).
// The window's winner, one definition for the forward (which may record it) and the backward (which recomputes it): the first element in
// (a, b, c) order that is greater than every one before it, a NaN taking over from anything.  Returns its index (a * 2 + b) * 2 + c.
__device__ __forceinline__ int pool_winner(const float* __restrict__ p, int od, int oh, int ow, int H, int W, int wd, float& best) {
  best = -INFINITY;
  int arg = 0;
  for (int a = 0; a < wd; ++a)
    for (int b = 0; b < 2; ++b)
      for (int c = 0; c < 2; ++c) pool_winner_step(p[((long)(od * wd + a) * H + (oh * 2 + b)) * W + ow * 2 + c], (a * 2 + b) * 2 + c, best, arg);
  return arg;
}

// ARG: also one byte per pooled element, the winner's index (read by the POOL form of the norm backward instead of the activation)
template <bool ARG>
__global__ void k_maxpool2_fwd(const float* __restrict__ x, float* __restrict__ y, unsigned char* __restrict__ arg, int NC, int D, int H, int W,
                               int Do, int Ho, int Wo, int wd) {
  const long total = (long)NC * Do * Ho * Wo;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ow = (int)(i % Wo), oh = (int)((i / Wo) % Ho), od = (int)((i / ((long)Wo * Ho)) % Do);
    const long nc = i / ((long)Wo * Ho * Do);
    float best;
    const int a = pool_winner(x + nc * D * H * W, od, oh, ow, H, W, wd, best);
    y[i] = best;
    if (ARG) arg[i] = (unsigned char)a;
  }
}

// SKIP: dx = skip + (the pool's gradient): the pooled tensor also feeds a skip connection (networks.py:526,531), whose
// gradient autograd would add in a separate pass
template <bool SKIP>
__global__ void k_maxpool2_bwd(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ skip,
                               float* __restrict__ dx, int NC, int D, int H, int W, int Do, int Ho, int Wo, int wd) {
  const long total = (long)NC * Do * Ho * Wo;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ow = (int)(i % Wo), oh = (int)((i / Wo) % Ho), od = (int)((i / ((long)Wo * Ho)) % Do);
    const long nc = i / ((long)Wo * Ho * Do);
    float* q = dx + nc * D * H * W;
    float best;
    const int arg = pool_winner(x + nc * D * H * W, od, oh, ow, H, W, wd, best);
    const float g = dy[i];
    for (int a = 0; a < wd; ++a)
      for (int b = 0; b < 2; ++b)
        for (int c = 0; c < 2; ++c) {
          const long o = ((long)(od * wd + a) * H + (oh * 2 + b)) * W + ow * 2 + c;
          const float v = ((a * 2 + b) * 2 + c) == arg ? g : 0.f;
          q[o] = SKIP ? skip[nc * D * H * W + o] + v : v;
        }
  }
}

// the plain sums / apply pass with the prefetch of nc_set_stream_passes (off: one iteration at a time, the kernels as they were)
static void launch_in_bwd_sums(const float* dy, const float* x, const float* mean, const float* rstd, float slope, long S, int splits, int NC,
                               double* part, hipStream_t s) {
  if (sw::get(sw::STREAM_PASSES)) hipLaunchKernelGGL(k_in_bwd_sums<8>, dim3(splits, NC), dim3(256), 0, s, dy, x, mean, rstd, slope, S, splits, part);
  else hipLaunchKernelGGL(k_in_bwd_sums<1>, dim3(splits, NC), dim3(256), 0, s, dy, x, mean, rstd, slope, S, splits, part);
}
static void launch_in_bwd_apply(const float* dy, const float* x, const float* mean, const float* rstd, float slope, long S, int splits, int NC,
                                long bx, const double* part, float* dx, double* rowpart, hipStream_t s) {
  if (sw::get(sw::STREAM_PASSES))
    hipLaunchKernelGGL(k_in_bwd_apply<4>, dim3((unsigned)bx, NC), dim3(256), 0, s, dy, x, mean, rstd, slope, S, splits, part, dx, rowpart);
  else
    hipLaunchKernelGGL(k_in_bwd_apply<1>, dim3((unsigned)bx, NC), dim3(256), 0, s, dy, x, mean, rstd, slope, S, splits, part, dx, rowpart);
}

static unsigned flat_grid(long n, int per_block = 256) {
  long b = cdiv(n, per_block);
  if (b > 16384) b = 16384;
  if (b < 1) b = 1;
  return (unsigned)b;
}

}  // namespace nc

using namespace nc;

// ---------------------------------------------------------------- BatchNorm{2,3}d(affine, running statistics) + (Leaky)ReLU
// --norm batch (reference models/networks.py:30-31: functools.partial(nn.BatchNorm3d / 2d, affine=True, track_running_stats=True); the
// reference's default --norm, although its README configuration and the north star use instance).  Statistics over (N, spatial) per
// channel from the same fp64 per-instance partial sums the instance norm takes (k_in_stats), then one fused apply pass
//   y = act((x - mean_c) * rstd_c * gamma_c + beta_c).
// Training: biased variance for the normalisation, running_mean / running_var updated with `momentum` and the UNBIASED variance, as
// torch does; evaluation: the running statistics.
__global__ void k_bn_finalize(const double* __restrict__ part, int N, int C, int splits, long S, float eps, float momentum,
                              float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ running_mean,
                              float* __restrict__ running_var) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < splits; ++k) {
      s += part[(((long)n * C + c) * splits + k) * 2];
      q += part[(((long)n * C + c) * splits + k) * 2 + 1];
    }
  const double M = (double)N * (double)S;
  const double m = s / M;
  double var = q / M - m * m;
  if (var < 0.0) var = 0.0;
  mean[c] = (float)m;
  rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * m);
  if (running_var) {
    const double unb = M > 1.0 ? var * M / (M - 1.0) : var;
    running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unb);
  }
}
// evaluation mode: mean / rstd from the running statistics
__global__ void k_bn_running(const float* __restrict__ running_mean, const float* __restrict__ running_var, int C, float eps,
                             float* __restrict__ mean, float* __restrict__ rstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  mean[c] = running_mean[c];
  rstd[c] = (float)(1.0 / sqrt((double)running_var[c] + (double)eps));
}
__device__ __forceinline__ float bn_value(float xv, float m, float r, float g, float b) {
  float xh = (xv - m) * r;
  asm("" : "+v"(xh));  // (the same rounding points in forward and backward: x-hat first, then the affine map)
  return xh * g + b;
}
__global__ __launch_bounds__(256) void k_bn_act_fwd(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
                                                    float* __restrict__ y, int C, long S) {
  const int inst = blockIdx.y, c = inst % C;
  const float m = mean[c], r = rstd[c], g = gamma[c], b = beta[c];
  const float* p = x + (long)inst * S;
  float* o = y + (long)inst * S;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < S; i += (long)gridDim.x * 256) {
    const float v = bn_value(p[i], m, r, g, b);
    o[i] = v > 0.f ? v : v * slope;
  }
}
// backward pass 1: per (instance, split) s1 = sum(gz), s2 = sum(gz * xhat), gz = dy * act'(z)
__global__ __launch_bounds__(256) void k_bn_bwd_sums(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float slope, int C, long S, int splits,
                                                     double* __restrict__ part) {
  const int inst = blockIdx.y, sp = blockIdx.x, c = inst % C;
  long b0, e;
  chunk_range(S, splits, sp, b0, e);
  const float m = mean[c], r = rstd[c], g = gamma[c], b = beta[c];
  const float* px = x + (long)inst * S;
  const float* pg = dy + (long)inst * S;
  double s1 = 0.0, s2 = 0.0;
  for (long i = b0 + threadIdx.x; i < e; i += 256) {
    float xh = (px[i] - m) * r;
    asm("" : "+v"(xh));
    const float z = xh * g + b;
    const float gz = z > 0.f ? pg[i] : pg[i] * slope;
    s1 += (double)gz;
    s2 = fma((double)gz, (double)xh, s2);
  }
  block_reduce2(s1, s2, part + ((long)inst * splits + sp) * 2);
}
// per channel: dbeta = sum gz, dgamma = sum gz xhat (over all instances and splits, fixed order); coef = (dbeta / M, dgamma / M)
__global__ void k_bn_bwd_finalize(const double* __restrict__ part, int N, int C, int splits, long S, float* __restrict__ dgamma,
                                  float* __restrict__ dbeta, float* __restrict__ coef) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < splits; ++k) {
      s1 += part[(((long)n * C + c) * splits + k) * 2];
      s2 += part[(((long)n * C + c) * splits + k) * 2 + 1];
    }
  const double M = (double)N * (double)S;
  dbeta[c] = (float)s1;
  dgamma[c] = (float)s2;
  coef[2 * c] = (float)(s1 / M);
  coef[2 * c + 1] = (float)(s2 / M);
}
// dx = gamma rstd (gz - mean(gz) - xhat mean(gz xhat))  (training);  dx = gamma rstd gz  (evaluation: the statistics are constants)
__global__ __launch_bounds__(256) void k_bn_bwd_apply(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float slope, const float* __restrict__ coef,
                                                      int training, float* __restrict__ dx, int C, long S) {
  const int inst = blockIdx.y, c = inst % C;
  const float m = mean[c], r = rstd[c], g = gamma[c], b = beta[c];
  const float m1 = training ? coef[2 * c] : 0.f, m2 = training ? coef[2 * c + 1] : 0.f;
  const float* px = x + (long)inst * S;
  const float* pg = dy + (long)inst * S;
  float* o = dx + (long)inst * S;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < S; i += (long)gridDim.x * 256) {
    float xh = (px[i] - m) * r;
    asm("" : "+v"(xh));
    const float z = xh * g + b;
    const float gz = z > 0.f ? pg[i] : pg[i] * slope;
    o[i] = (g * r) * ((gz - m1) - xh * m2);
  }
}

extern "C" {

size_t nc_instnorm_ws_bytes(int NC, long S) {
  if (S >= 1 && rows_path(S)) return (size_t)NC * 2 * sizeof(double);  // short instances: one split at most
  return (size_t)NC * kMaxSplits * 2 * sizeof(double);
}

int nc_instnorm_stats(const float* x, int NC, long S, float eps, float* mean, float* rstd, void* ws, size_t ws_bytes,
                      void* stream) {
  if (!x || !mean || !rstd) { set_error("instnorm_stats: null pointer"); return NC_ERR_ARG; }
  if (NC >= 1 && S >= 1 && rows_path(S)) {
    launch_fwd_rows<0>(x, NC, S, eps, 0.f, mean, rstd, nullptr, (hipStream_t)stream);
    return check_launch("instnorm_stats");
  }
  if (NC > 65535) {  // grid.y limit: instances in chunks (stream-ordered reuse of the workspace)
    for (int c0 = 0; c0 < NC; c0 += 65535) {
      const int n = NC - c0 < 65535 ? NC - c0 : 65535;
      if (int e = nc_instnorm_stats(x + (long)c0 * S, n, S, eps, mean + c0, rstd + c0, ws, ws_bytes, stream)) return e;
    }
    return NC_OK;
  }
  if (NC < 1 || S < 1) { set_error("instnorm_stats: bad shape NC=%d S=%ld", NC, S); return NC_ERR_SHAPE; }
  if (!ws || ws_bytes < nc_instnorm_ws_bytes(NC, S)) { set_error("instnorm_stats: workspace too small"); return NC_ERR_WS; }
  hipStream_t s = (hipStream_t)stream;
  const int splits = pick_splits(NC, S);
  hipLaunchKernelGGL(k_in_stats, dim3(splits, NC), dim3(256), 0, s, x, S, splits, (double*)ws);
  hipLaunchKernelGGL(k_in_finalize, dim3((unsigned)cdiv(NC, 128)), dim3(128), 0, s, (const double*)ws, NC, splits, S, eps,
                     mean, rstd);
  return check_launch("instnorm_stats");
}

int nc_instnorm_act_fwd(const float* x, const float* mean, const float* rstd, float slope, float* y, int NC, long S,
                        void* stream) {
  if (!x || !mean || !rstd || !y) { set_error("instnorm_act_fwd: null pointer"); return NC_ERR_ARG; }
  if (NC >= 1 && S >= 1 && rows_path(S)) {
    launch_fwd_rows<1>(x, NC, S, 0.f, slope, const_cast<float*>(mean), const_cast<float*>(rstd), y, (hipStream_t)stream);
    return check_launch("instnorm_act_fwd");
  }
  if (NC > 65535) {
    for (int c0 = 0; c0 < NC; c0 += 65535) {
      const int n = NC - c0 < 65535 ? NC - c0 : 65535;
      if (int e = nc_instnorm_act_fwd(x + (long)c0 * S, mean + c0, rstd + c0, slope, y + (long)c0 * S, n, S, stream)) return e;
    }
    return NC_OK;
  }
  if (NC < 1 || S < 1) { set_error("instnorm_act_fwd: bad shape"); return NC_ERR_SHAPE; }
  long bx = cdiv(S, 1024 * 4);
  if (bx > 1024) bx = 1024;
  hipLaunchKernelGGL(k_in_act_fwd, dim3((unsigned)bx, NC), dim3(256), 0, (hipStream_t)stream, x, mean, rstd, slope, y, S);
  return check_launch("instnorm_act_fwd");
}

int nc_instnorm_fwd(const float* x, float eps, float slope, float* mean, float* rstd, float* y, int NC, long S, void* ws,
                    size_t ws_bytes, void* stream) {
  if (!x || !mean || !rstd || !y) { set_error("instnorm_fwd: null pointer"); return NC_ERR_ARG; }
  if (NC < 1 || S < 1) { set_error("instnorm_fwd: bad shape NC=%d S=%ld", NC, S); return NC_ERR_SHAPE; }
  if (rows_path(S)) {
    launch_fwd_rows<2>(x, NC, S, eps, slope, mean, rstd, y, (hipStream_t)stream);
    return check_launch("instnorm_fwd");
  }
  if (int e = nc_instnorm_stats(x, NC, S, eps, mean, rstd, ws, ws_bytes, stream)) return e;
  return nc_instnorm_act_fwd(x, mean, rstd, slope, y, NC, S, stream);
}

int nc_instnorm_act_bwd(const float* dy, const float* x, const float* mean, const float* rstd, float slope, float* dx,
                        int NC, long S, void* ws, size_t ws_bytes, void* stream) {
  SwitchScope switches_;  // (both passes see one value of nc_set_stream_passes)
  if (!dy || !x || !mean || !rstd || !dx) { set_error("instnorm_act_bwd: null pointer"); return NC_ERR_ARG; }
  if (NC >= 1 && S >= 1 && rows_path(S)) {
    launch_bwd_rows(dy, x, mean, rstd, slope, NC, S, dx, nullptr, (hipStream_t)stream);
    return check_launch("instnorm_act_bwd");
  }
  if (NC > 65535) {
    for (int c0 = 0; c0 < NC; c0 += 65535) {
      const int n = NC - c0 < 65535 ? NC - c0 : 65535;
      if (int e = nc_instnorm_act_bwd(dy + (long)c0 * S, x + (long)c0 * S, mean + c0, rstd + c0, slope, dx + (long)c0 * S, n, S, ws,
                                      ws_bytes, stream)) return e;
    }
    return NC_OK;
  }
  if (NC < 1 || S < 1) { set_error("instnorm_act_bwd: bad shape"); return NC_ERR_SHAPE; }
  if (!ws || ws_bytes < nc_instnorm_ws_bytes(NC, S)) { set_error("instnorm_act_bwd: workspace too small"); return NC_ERR_WS; }
  hipStream_t s = (hipStream_t)stream;
  const int splits = pick_splits(NC, S);
  launch_in_bwd_sums(dy, x, mean, rstd, slope, S, splits, NC, (double*)ws, s);
  long bx = cdiv(S, 1024);
  if (bx > 1024) bx = 1024;
  launch_in_bwd_apply(dy, x, mean, rstd, slope, S, splits, NC, bx, (const double*)ws, dx, nullptr, s);
  return check_launch("instnorm_act_bwd");
}

size_t nc_instnorm_bwd_dbias_ws_bytes(int NC, long S) {
  long bx = cdiv(S, 1024);
  if (bx > 1024) bx = 1024;
  return nc_instnorm_ws_bytes(NC, S) + (size_t)NC * bx * sizeof(double);
}

int nc_instnorm_act_bwd_dbias(const float* dy, const float* x, const float* mean, const float* rstd, float slope, float* dx,
                              float* dbias, int N, int C, long S, void* ws, size_t ws_bytes, void* stream) {
  SwitchScope switches_;  // (both passes see one value of nc_set_stream_passes)
  if (!dy || !x || !mean || !rstd || !dx || !dbias) { set_error("instnorm_act_bwd_dbias: null pointer"); return NC_ERR_ARG; }
  const long NCl = (long)N * C;
  if (N < 1 || C < 1 || S < 1 || NCl > 0x7fffffffL) { set_error("instnorm_act_bwd_dbias: bad shape"); return NC_ERR_SHAPE; }
  hipStream_t s = (hipStream_t)stream;
  if (rows_path(S)) {  // one sum per instance, then one workgroup per channel over the samples
    if (!ws || ws_bytes < (size_t)NCl * sizeof(double)) { set_error("instnorm_act_bwd_dbias: workspace too small"); return NC_ERR_WS; }
    launch_bwd_rows(dy, x, mean, rstd, slope, NCl, S, dx, (double*)ws, s);
    hipLaunchKernelGGL(k_in_dbias_final, dim3(C), dim3(256), 0, s, (const double*)ws, N, C, 1, dbias);
    return check_launch("instnorm_act_bwd_dbias");
  }
  if (NCl > 65535) { set_error("instnorm_act_bwd_dbias: more than 65535 long instances"); return NC_ERR_SHAPE; }
  const int NC = (int)NCl;
  if (!ws || ws_bytes < nc_instnorm_bwd_dbias_ws_bytes(NC, S)) { set_error("instnorm_act_bwd_dbias: workspace too small"); return NC_ERR_WS; }
  const int splits = pick_splits(NC, S);
  double* rowpart = (double*)((char*)ws + nc_instnorm_ws_bytes(NC, S));
  launch_in_bwd_sums(dy, x, mean, rstd, slope, S, splits, NC, (double*)ws, s);
  long bx = cdiv(S, 1024);
  if (bx > 1024) bx = 1024;
  launch_in_bwd_apply(dy, x, mean, rstd, slope, S, splits, NC, bx, (const double*)ws, dx, rowpart, s);
  hipLaunchKernelGGL(k_in_dbias_final, dim3(C), dim3(256), 0, s, (const double*)rowpart, N, C, (int)bx, dbias);
  return check_launch("instnorm_act_bwd_dbias");
}

int nc_instnorm_act_fwd_c8(const float* x, const float* mean, const float* rstd, float slope, float* y, void* yh, int N, int C,
                           long S, int dtype, void* stream) {
  if (!x || !mean || !rstd || !yh) { set_error("instnorm_act_fwd_c8: null pointer"); return NC_ERR_ARG; }
  if (N < 1 || C < 8 || C % 8 || S < 1 || (long)N * C / 8 > 65535) { set_error("instnorm_act_fwd_c8: bad shape"); return NC_ERR_SHAPE; }
  if (dtype != NC_DT_F16 && dtype != NC_DT_BF16) { set_error("instnorm_act_fwd_c8: dtype must be NC_DT_F16 or NC_DT_BF16"); return NC_ERR_ARG; }
  long bx = cdiv(S, 256);
  if (bx > 2048) bx = 2048;
  dim3 grid((unsigned)bx, (unsigned)(N * C / 8));
  if (dtype == NC_DT_F16)
    hipLaunchKernelGGL(k_in_act_fwd_c8<NC_DT_F16>, grid, dim3(256), 0, (hipStream_t)stream, x, mean, rstd, slope, y, (uint4*)yh, S);
  else
    hipLaunchKernelGGL(k_in_act_fwd_c8<NC_DT_BF16>, grid, dim3(256), 0, (hipStream_t)stream, x, mean, rstd, slope, y, (uint4*)yh, S);
  return check_launch("instnorm_act_fwd_c8");
}

int nc_instnorm_act_bwd_c8(const float* dy, const float* x, const float* mean, const float* rstd, float slope, float* dx,
                           void* dxh, float* dbias, int N, int C, long S, int dtype, void* ws, size_t ws_bytes, void* stream) {
  SwitchScope switches_;  // (both passes see one value of nc_set_stream_passes)
  if (!dy || !x || !mean || !rstd || !dx || !dxh) { set_error("instnorm_act_bwd_c8: null pointer"); return NC_ERR_ARG; }
  const long NCl = (long)N * C;
  if (N < 1 || C < 8 || C % 8 || S < 1 || NCl > 65535) { set_error("instnorm_act_bwd_c8: bad shape"); return NC_ERR_SHAPE; }
  if (dtype != NC_DT_F16 && dtype != NC_DT_BF16) { set_error("instnorm_act_bwd_c8: dtype must be NC_DT_F16 or NC_DT_BF16"); return NC_ERR_ARG; }
  const int NC = (int)NCl;
  if (!ws || ws_bytes < nc_instnorm_bwd_dbias_ws_bytes(NC, S)) { set_error("instnorm_act_bwd_c8: workspace too small"); return NC_ERR_WS; }
  hipStream_t s = (hipStream_t)stream;
  const int splits = pick_splits(NC, S);
  launch_in_bwd_sums(dy, x, mean, rstd, slope, S, splits, NC, (double*)ws, s);
  long bx = cdiv(S, 1024);  // the same block count as nc_instnorm_bwd_dbias_ws_bytes sizes the partials for
  if (bx > 1024) bx = 1024;
  double* rowpart = dbias ? (double*)((char*)ws + nc_instnorm_ws_bytes(NC, S)) : nullptr;
  dim3 grid((unsigned)bx, (unsigned)(NC / 8));
  if (dtype == NC_DT_F16)
    hipLaunchKernelGGL(k_in_bwd_apply_c8<NC_DT_F16>, grid, dim3(256), 0, s, dy, x, mean, rstd, slope, S, splits,
                       (const double*)ws, dx, (uint4*)dxh, rowpart);
  else
    hipLaunchKernelGGL(k_in_bwd_apply_c8<NC_DT_BF16>, grid, dim3(256), 0, s, dy, x, mean, rstd, slope, S, splits,
                       (const double*)ws, dx, (uint4*)dxh, rowpart);
  if (dbias) hipLaunchKernelGGL(k_in_dbias_final, dim3(C), dim3(256), 0, s, (const double*)rowpart, N, C, (int)bx, dbias);
  return check_launch("instnorm_act_bwd_c8");
}

}  // extern "C"
namespace nc {
// nc_instnorm_act_bwd_dbias with dx delivered as an S3 tensor [N][C/8][3][S][8] bf16 (gen_nets.hip: the dY of a split-operand
// convolution).  false: this shape takes the short-instance path, which has no S3 form (the caller uses the fp32 entry point).
bool instnorm_bwd_s3_supported(int N, int C, long S) { return N >= 1 && C >= 8 && C % 8 == 0 && S >= 1 && !rows_path(S) && (long)N * C <= 65535; }
int instnorm_act_bwd_dbias_s3(const float* dy, const float* x, const float* mean, const float* rstd, float slope, void* dxs,
                              float* dbias, int N, int C, long S, void* ws, size_t ws_bytes, void* stream) {
  SwitchScope switches_;  // (both passes see one value of nc_set_stream_passes)
  if (!dy || !x || !mean || !rstd || !dxs || !dbias) { set_error("instnorm_act_bwd_dbias_s3: null pointer"); return NC_ERR_ARG; }
  if (!instnorm_bwd_s3_supported(N, C, S)) { set_error("instnorm_act_bwd_dbias_s3: bad shape"); return NC_ERR_SHAPE; }
  const int NC = N * C;
  if (!ws || ws_bytes < nc_instnorm_bwd_dbias_ws_bytes(NC, S)) { set_error("instnorm_act_bwd_dbias_s3: workspace too small"); return NC_ERR_WS; }
  hipStream_t s = (hipStream_t)stream;
  const int splits = pick_splits(NC, S);
  launch_in_bwd_sums(dy, x, mean, rstd, slope, S, splits, NC, (double*)ws, s);
  long bx = cdiv(S, 1024);
  if (bx > 1024) bx = 1024;
  double* rowpart = (double*)((char*)ws + nc_instnorm_ws_bytes(NC, S));
  hipLaunchKernelGGL(k_in_bwd_apply_s3<false>, dim3((unsigned)bx, (unsigned)(NC / 8)), dim3(256), 0, s, dy, x, mean, rstd, slope, S, splits,
                     (const double*)ws, (uint4*)dxs, C / 8, rowpart, (const unsigned*)nullptr, (const float*)nullptr);
  hipLaunchKernelGGL(k_in_dbias_final, dim3(C), dim3(256), 0, s, (const double*)rowpart, N, C, (int)bx, dbias);
  return check_launch("instnorm_act_bwd_dbias_s3");
}
// dxs: an H2 tensor [N][C/8][2][S] with its cell at byte offset h2_cells_offset(N * C * S) (cells[0] = cells[1] = the bound) and two
// arrays of N * C words of scratch behind the cells -- all inside the N * C * S * 6 bytes an S3 tensor of the same shape takes.
// w1 != NULL (the rank-one form, N == 1): dy is ONE channel and the gradient at the norm's output is w1[c] * dy[v]
// pool != NULL (the POOL form, see PoolGrad): dy is the skip gradient, the gradient at the norm's output is formed from it and the pooled one.
// Folded (nc_set_in_bwd_fold, default on; not when the range guard may switch kernels inside this call -- then every launch is the parent's):
// the sums pass keeps the loads of four iterations in flight, the bound is taken by the apply pass itself, the guard's words are zeroed with the
// cells, and the bias sums and the guard's decision are one launch -- four launches per tensor instead of six.
static int in_bwd_dbias_h2(const float* dy, const float* w1, const float* x, const float* mean, const float* rstd, float slope, void* dxs,
                           float* dbias, int N, int C, long S, void* ws, size_t ws_bytes, void* stream, unsigned* guard,
                           const PoolGrad* pool = nullptr) {
  SwitchScope switches_;  // (both passes see one value of nc_set_stream_passes)
  if (!dy || !x || !mean || !rstd || !dxs || !dbias) { set_error("instnorm_act_bwd_dbias_h2: null pointer"); return NC_ERR_ARG; }
  if (!instnorm_bwd_s3_supported(N, C, S)) { set_error("instnorm_act_bwd_dbias_h2: bad shape"); return NC_ERR_SHAPE; }
  const int NC = N * C;
  if (w1 && N != 1) { set_error("instnorm_act_bwd_dbias_h2: the rank-one form takes one sample"); return NC_ERR_ARG; }
  if (!ws || ws_bytes < nc_instnorm_bwd_dbias_ws_bytes(NC, S)) { set_error("instnorm_act_bwd_dbias_h2: workspace too small"); return NC_ERR_WS; }
  if ((size_t)NC * S * 2 < 512 + (size_t)NC * 8) { set_error("instnorm_act_bwd_dbias_h2: tensor too small"); return NC_ERR_SHAPE; }
  hipStream_t s = (hipStream_t)stream;
  unsigned* cells = (unsigned*)((char*)dxs + h2_cells_offset((size_t)NC * S));
  unsigned* gmax = cells + 64;
  unsigned* xmax = gmax + NC;
  // Range guard (common.hpp): the cell is a bound from the tensor's own per-instance maxima, i.e. data-derived like a measured one -- a block
  // of channels or a region far below the rest loses bits the same way.  guard (nullable): the words conv_bwd_s3 reads (conv_bwd_guard_words);
  // the apply pass counts its low chunks, the decision is taken on the device, and a flagged tensor is written AGAIN by the S3 twin of the
  // apply pass (same values, three exact bf16 terms, over the H2 form: the buffer has the S3 capacity) for the three-term kernels
  unsigned* g = guard && sw::get(sw::H2_GUARD) ? guard : nullptr;
  // Inside a whole-network call mode 1 (default) COUNTS a flagged tensor (nc_h2_guard_stats [2]) and leaves the switch to the caller (the
  // Python models go to the three-term form when they see it, models/base_model.py): the in-call fallback costs the training step ~65
  // near-empty launches, 0.5 ms of 35, for an event InstanceNorm networks do not produce.  Mode 2: in-call fallback here too.
  const bool flip = g && h2_guard_can_flip();
  const bool fold = sw::get(sw::IN_BWD_FOLD) && !flip;
  if (pool && (!fold || w1)) { set_error("instnorm_act_bwd_dbias_h2: the pooled form needs the folded path"); return NC_ERR_ARG; }
  const PoolGrad none{};
  hipLaunchKernelGGL(k_zero_u32, dim3((unsigned)cdiv(64 + 2 * NC, 256)), dim3(256), 0, s, cells, 64 + 2 * NC, fold ? guard : (unsigned*)nullptr, 8);
  const int splits = pick_splits(NC, S);
  const dim3 gs(splits, NC);
  // Prefetch depth of the folded sums pass: 4; with nc_set_stream_passes the rank-one form, whose one-channel gradient sits in L2, takes 8
  // (103.6 -> 100.6 us at 64 x 108^3).  The POOL and the plain form gained nothing from 8 (both grids together 117.7 -> 119.5 and 33.2 -> 34.3 us,
  // DESIGN.md 4.1): the switch does not change them.
  constexpr int U = 4, U_R1 = 8;
  const bool sp = sw::get(sw::STREAM_PASSES) != 0;
#define NC_SUMS(R1_, POOL_, U_, pq_) \
  hipLaunchKernelGGL((k_in_bwd_sums_h2<R1_, POOL_, U_>), gs, dim3(256), 0, s, dy, x, mean, rstd, slope, S, splits, (double*)ws, gmax, xmax, w1, pq_)
  if (pool) NC_SUMS(false, true, U, *pool);
  else if (fold && w1 && sp) NC_SUMS(true, false, U_R1, none);
  else if (fold && w1) NC_SUMS(true, false, U, none);
  else if (fold) NC_SUMS(false, false, U, none);
  else if (w1) NC_SUMS(true, false, 1, none);
  else NC_SUMS(false, false, 1, none);
#undef NC_SUMS
  if (!fold) hipLaunchKernelGGL(k_in_bwd_bound, dim3(1), dim3(256), 0, s, rstd, gmax, xmax, NC, cells, cells + 1, guard);
  long bx = cdiv(S, 1024);
  if (bx > 1024) bx = 1024;
  double* rowpart = (double*)((char*)ws + nc_instnorm_ws_bytes(NC, S));
  const dim3 ga((unsigned)bx, (unsigned)(NC / 8));
#define NC_APPLY(R1_, POOL_, FOLD_, pq_) NC_APPLY_(R1_, POOL_, FOLD_, false, pq_)
#define NC_APPLY_(R1_, POOL_, FOLD_, STAGE_, pq_)                                                                                            \
  hipLaunchKernelGGL((k_in_bwd_apply_h2<R1_, POOL_, FOLD_, STAGE_>), ga, dim3(256), 0, s, dy, x, mean, rstd, slope, S, splits, (const double*)ws, \
                     (uint4*)dxs, C / 8, rowpart, (const unsigned*)cells, g, w1, pq_, (const unsigned*)gmax, (const unsigned*)xmax, NC, cells)
  if (pool) NC_APPLY(false, true, true, *pool);
  else if (fold && w1 && sp) NC_APPLY_(true, false, true, true, none);
  else if (fold && w1) NC_APPLY(true, false, true, none);
  else if (fold) NC_APPLY(false, false, true, none);
  else if (w1) NC_APPLY(true, false, false, none);
  else NC_APPLY(false, false, false, none);
#undef NC_APPLY
#undef NC_APPLY_
  // chunks: one per wave and loop iteration = (NC / 8) * sum over blocks of ceil(iterations): every 64-voxel group of every 8-channel block
  const unsigned long long total = (unsigned long long)(NC / 8) * (unsigned long long)cdiv(S, 64);
  if (fold) {
    if (g) hipLaunchKernelGGL(k_in_dbias_final_decide, dim3(C), dim3(256), 0, s, (const double*)rowpart, N, C, (int)bx, dbias, g, h2_guard_stats_dev(), total);
    else hipLaunchKernelGGL(k_in_dbias_final, dim3(C), dim3(256), 0, s, (const double*)rowpart, N, C, (int)bx, dbias);
    count_in_bwd_launches(4);
    return check_launch("instnorm_act_bwd_dbias_h2");
  }
  hipLaunchKernelGGL(k_in_dbias_final, dim3(C), dim3(256), 0, s, (const double*)rowpart, N, C, (int)bx, dbias);
  count_in_bwd_launches(5);
  if (g) {
    if (int e = h2_guard_decide(g, nullptr, nullptr, g + kGuardFlag, flip, s, total)) return e;
    count_in_bwd_launches(1);
    if (!flip) return check_launch("instnorm_act_bwd_dbias_h2");
    long bx3 = bx < 128 ? bx : 128;  // (usually leaves at once; no row partials: the bias gradient is the H2 pass's)
    if (w1)  // (the rewrite takes the gradient from the same source)
      hipLaunchKernelGGL(k_in_bwd_apply_s3<true>, dim3((unsigned)bx3, (unsigned)(NC / 8)), dim3(256), 0, s, dy, x, mean, rstd, slope, S, splits,
                         (const double*)ws, (uint4*)dxs, C / 8, (double*)nullptr, (const unsigned*)g, w1);
    else
      hipLaunchKernelGGL(k_in_bwd_apply_s3<false>, dim3((unsigned)bx3, (unsigned)(NC / 8)), dim3(256), 0, s, dy, x, mean, rstd, slope, S, splits,
                         (const double*)ws, (uint4*)dxs, C / 8, (double*)nullptr, (const unsigned*)g, (const float*)nullptr);
    count_in_bwd_launches(1);
  }
  return check_launch("instnorm_act_bwd_dbias_h2");
}
// The POOL form (PoolGrad): skip = the skip half of the concat gradient, sample stride skip_stride floats; gp / arg: the dense pooled gradient
// and the forward's winner bytes [N][C][D/2 * H/2 * W/2].  false: take nc_maxpool2_bwd_add and the plain form.
bool instnorm_bwd_h2_pool_supported(int N, int C, int D, int H, int W, unsigned* guard) {
  const long S = (long)D * H * W;
  return D >= 2 && H >= 2 && W >= 2 && !((D | H | W) & 1) && S < 0x7fffffffL && instnorm_bwd_s3_supported(N, C, S) && sw::get(sw::IN_BWD_FOLD) &&
         !(guard && sw::get(sw::H2_GUARD) && h2_guard_can_flip());
}
int instnorm_act_bwd_dbias_h2_pool(const float* skip, long skip_stride, const float* gp, const unsigned char* arg, const float* x, const float* mean,
                                   const float* rstd, float slope, void* dxs, float* dbias, int N, int C, int D, int H, int W, void* ws,
                                   size_t ws_bytes, void* stream, unsigned* guard) {
  if (!gp || !arg) { set_error("instnorm_act_bwd_dbias_h2_pool: null pointer"); return NC_ERR_ARG; }
  if (!instnorm_bwd_h2_pool_supported(N, C, D, H, W, guard) || skip_stride < (long)C * D * H * W) {
    set_error("instnorm_act_bwd_dbias_h2_pool: shape or switches not covered");
    return NC_ERR_SHAPE;
  }
  const PoolGrad pq{gp, arg, skip_stride, (long)(D / 2) * (H / 2) * (W / 2), C, H, W, H / 2, W / 2};
  return in_bwd_dbias_h2(skip, nullptr, x, mean, rstd, slope, dxs, dbias, N, C, (long)D * H * W, ws, ws_bytes, stream, guard, &pq);
}
// MaxPool3d(2) forward of NC even-sized volumes that also leaves the winner bytes
int maxpool2_fwd_arg(const float* x, float* y, unsigned char* arg, int NC, int D, int H, int W, hipStream_t s) {
  if (!x || !y || !arg) { set_error("maxpool2_fwd_arg: null pointer"); return NC_ERR_ARG; }
  if (NC < 1 || D < 2 || H < 2 || W < 2 || ((D | H | W) & 1)) { set_error("maxpool2_fwd_arg: bad shape"); return NC_ERR_SHAPE; }
  const long total = (long)NC * (D / 2) * (H / 2) * (W / 2);
  hipLaunchKernelGGL(k_maxpool2_fwd<true>, dim3(flat_grid(total)), dim3(256), 0, s, x, y, arg, NC, D, H, W, D / 2, H / 2, W / 2, 2);
  return check_launch("maxpool2_fwd_arg");
}
static std::atomic<int> g_in_bwd_launches[2];  // [0] the two-term norm backward, [1] nc_maxpool2_bwd_add
void count_in_bwd_launches(int n, int which) { g_in_bwd_launches[which].fetch_add(n, std::memory_order_relaxed); }
int instnorm_act_bwd_dbias_h2(const float* dy, const float* x, const float* mean, const float* rstd, float slope, void* dxs,
                              float* dbias, int N, int C, long S, void* ws, size_t ws_bytes, void* stream, unsigned* guard) {
  return in_bwd_dbias_h2(dy, nullptr, x, mean, rstd, slope, dxs, dbias, N, C, S, ws, ws_bytes, stream, guard);
}
int instnorm_act_bwd_dbias_h2_rank1(const float* dy1, const float* w1, const float* x, const float* mean, const float* rstd, float slope, void* dxs,
                                    float* dbias, int C, long S, void* ws, size_t ws_bytes, void* stream, unsigned* guard) {
  if (!w1) { set_error("instnorm_act_bwd_dbias_h2_rank1: null pointer"); return NC_ERR_ARG; }
  return in_bwd_dbias_h2(dy1, w1, x, mean, rstd, slope, dxs, dbias, 1, C, S, ws, ws_bytes, stream, guard);
}
int instnorm_relu_tail_sigmoid(const float* x, const float* mean, const float* rstd, const float* w1, const float* b1, const float* w2,
                               const float* b2, float* y, int C, long S, hipStream_t s) {
  if (C > 256) { set_error("instnorm_relu_tail_sigmoid: at most 256 channels"); return NC_ERR_SHAPE; }
  hipLaunchKernelGGL(k_in_act_tail, dim3((unsigned)cdiv(S, 256)), dim3(256), 0, s, x, mean, rstd, w1, b1, w2, b2, y, S, C);
  return check_launch("instnorm_relu_tail_sigmoid");
}
}  // namespace nc
extern "C" {

int nc_instnorm_act_bwd_dbias_s3(const float* dy, const float* x, const float* mean, const float* rstd, float slope, void* dxs, float* dbias,
                                 int N, int C, long S, void* ws, size_t ws_bytes, void* stream) {
  return instnorm_act_bwd_dbias_s3(dy, x, mean, rstd, slope, dxs, dbias, N, C, S, ws, ws_bytes, stream);
}

int nc_in_bwd_launches(int which, int reset) {
  std::atomic<int>& c = g_in_bwd_launches[which == 1 ? 1 : 0];
  return reset ? c.exchange(0, std::memory_order_relaxed) : c.load(std::memory_order_relaxed);
}

int nc_leaky_relu_fwd(const float* x, float slope, float* y, long n, void* stream) {
  if (!x || !y) { set_error("leaky_relu_fwd: null pointer"); return NC_ERR_ARG; }
  hipLaunchKernelGGL(k_lrelu_fwd, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, x, slope, y, n);
  return check_launch("leaky_relu_fwd");
}
int nc_leaky_relu_bwd(const float* dy, const float* x, float slope, float* dx, long n, void* stream) {
  if (!dy || !x || !dx) { set_error("leaky_relu_bwd: null pointer"); return NC_ERR_ARG; }
  hipLaunchKernelGGL(k_lrelu_bwd, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, dy, x, slope, dx, n);
  return check_launch("leaky_relu_bwd");
}
int nc_sigmoid_fwd(const float* x, float* y, long n, void* stream) {
  if (!x || !y) { set_error("sigmoid_fwd: null pointer"); return NC_ERR_ARG; }
  hipLaunchKernelGGL(k_sigmoid_fwd, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, x, y, n);
  return check_launch("sigmoid_fwd");
}
int nc_sigmoid_bwd(const float* dy, const float* y, float* dx, long n, void* stream) {
  if (!dy || !y || !dx) { set_error("sigmoid_bwd: null pointer"); return NC_ERR_ARG; }
  hipLaunchKernelGGL(k_sigmoid_bwd, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, dy, y, dx, n);
  return check_launch("sigmoid_bwd");
}

int nc_maxpool2_fwd(const float* x, float* y, int NC, int D, int H, int W, void* stream) {
  if (!x || !y) { set_error("maxpool2_fwd: null pointer"); return NC_ERR_ARG; }
  const int wd = D > 1 ? 2 : 1;
  const int Do = D / wd, Ho = H / 2, Wo = W / 2;
  if (NC < 1 || Do < 1 || Ho < 1 || Wo < 1) { set_error("maxpool2_fwd: bad shape"); return NC_ERR_SHAPE; }
  const long total = (long)NC * Do * Ho * Wo;
  hipLaunchKernelGGL(k_maxpool2_fwd<false>, dim3(flat_grid(total)), dim3(256), 0, (hipStream_t)stream, x, y, (unsigned char*)nullptr, NC, D, H, W,
                     Do, Ho, Wo, wd);
  return check_launch("maxpool2_fwd");
}

int nc_maxpool2_bwd(const float* dy, const float* x, float* dx, int NC, int D, int H, int W, void* stream) {
  if (!dy || !x || !dx) { set_error("maxpool2_bwd: null pointer"); return NC_ERR_ARG; }
  const int wd = D > 1 ? 2 : 1;
  const int Do = D / wd, Ho = H / 2, Wo = W / 2;
  if (NC < 1 || Do < 1 || Ho < 1 || Wo < 1) { set_error("maxpool2_bwd: bad shape"); return NC_ERR_SHAPE; }
  hipStream_t s = (hipStream_t)stream;
  if ((D % wd) || (H & 1) || (W & 1)) {
    if (hipMemsetAsync(dx, 0, (size_t)NC * D * H * W * sizeof(float), s) != hipSuccess) {
      set_error("maxpool2_bwd: memset failed");
      return NC_ERR_HIP;
    }
  }
  const long total = (long)NC * Do * Ho * Wo;
  hipLaunchKernelGGL(k_maxpool2_bwd<false>, dim3(flat_grid(total)), dim3(256), 0, s, dy, x, nullptr, dx, NC, D, H, W, Do, Ho, Wo, wd);
  return check_launch("maxpool2_bwd");
}

int nc_maxpool2_bwd_add(const float* dy, const float* x, const float* skip, float* dx, int NC, int D, int H, int W,
                        void* stream) {
  if (!dy || !x || !skip || !dx) { set_error("maxpool2_bwd_add: null pointer"); return NC_ERR_ARG; }
  const int wd = D > 1 ? 2 : 1;
  const int Do = D / wd, Ho = H / 2, Wo = W / 2;
  if (NC < 1 || Do < 1 || Ho < 1 || Wo < 1 || (D % wd) || (H & 1) || (W & 1)) {
    set_error("maxpool2_bwd_add: even sizes expected (the skip tensor and the pooled tensor are the same tensor)");
    return NC_ERR_SHAPE;
  }
  const long total = (long)NC * Do * Ho * Wo;
  hipLaunchKernelGGL(k_maxpool2_bwd<true>, dim3(flat_grid(total)), dim3(256), 0, (hipStream_t)stream, dy, x, skip, dx, NC, D, H, W,
                     Do, Ho, Wo, wd);
  count_in_bwd_launches(1, 1);
  return check_launch("maxpool2_bwd_add");
}


// BatchNorm + activation (see the kernels above).  ws: nc_instnorm_ws_bytes(N * C, S) bytes.  mean / rstd: [C] outputs of the statistics
// call, inputs of the others.  running_mean / running_var: [C], updated in place (training) or read (evaluation); nullable in training.
int nc_batchnorm_stats(const float* x, int N, int C, long S, float eps, float momentum, int training, float* mean, float* rstd,
                       float* running_mean, float* running_var, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !mean || !rstd) { set_error("batchnorm_stats: null pointer"); return NC_ERR_ARG; }
  if (N < 1 || C < 1 || S < 1 || C > 65535 || (long)N * C > 0x7fffffffL) { set_error("batchnorm_stats: bad shape N=%d C=%d S=%ld", N, C, S); return NC_ERR_SHAPE; }
  hipStream_t s = (hipStream_t)stream;
  if (!training) {
    if (!running_mean || !running_var) { set_error("batchnorm_stats: evaluation mode needs the running statistics"); return NC_ERR_ARG; }
    hipLaunchKernelGGL(k_bn_running, dim3((unsigned)cdiv(C, 128)), dim3(128), 0, s, running_mean, running_var, C, eps, mean, rstd);
    return check_launch("batchnorm_stats");
  }
  if (!ws || ws_bytes < nc_instnorm_ws_bytes(N * C, S)) { set_error("batchnorm_stats: workspace too small"); return NC_ERR_WS; }
  const int splits = pick_splits(N * C, S);
  // (N * C is gridDim.y, at most 65535: whole samples per launch -- a 2-D PatchGAN over 148 slices x 512 channels has 75,776 instances)
  for (long i0 = 0, step = (long)(65535 / C) * C; i0 < (long)N * C; i0 += step) {
    const int ni = (long)N * C - i0 < step ? (int)((long)N * C - i0) : (int)step;
    hipLaunchKernelGGL(k_in_stats, dim3(splits, ni), dim3(256), 0, s, x + i0 * S, S, splits, (double*)ws + i0 * splits * 2);
  }
  hipLaunchKernelGGL(k_bn_finalize, dim3((unsigned)cdiv(C, 128)), dim3(128), 0, s, (const double*)ws, N, C, splits, S, eps, momentum, mean, rstd,
                     running_mean, running_var);
  return check_launch("batchnorm_stats");
}
int nc_batchnorm_act_fwd(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float slope, float* y,
                         int N, int C, long S, void* stream) {
  if (!x || !mean || !rstd || !gamma || !beta || !y) { set_error("batchnorm_act_fwd: null pointer"); return NC_ERR_ARG; }
  if (N < 1 || C < 1 || S < 1 || C > 65535 || (long)N * C > 0x7fffffffL) { set_error("batchnorm_act_fwd: bad shape"); return NC_ERR_SHAPE; }
  long bx = cdiv(S, 1024 * 4);
  if (bx > 1024) bx = 1024;
  for (long i0 = 0, step = (long)(65535 / C) * C; i0 < (long)N * C; i0 += step) {  // whole samples per launch (gridDim.y <= 65535)
    const int ni = (long)N * C - i0 < step ? (int)((long)N * C - i0) : (int)step;
    hipLaunchKernelGGL(k_bn_act_fwd, dim3((unsigned)bx, ni), dim3(256), 0, (hipStream_t)stream, x + i0 * S, mean, rstd, gamma, beta, slope, y + i0 * S, C, S);
  }
  return check_launch("batchnorm_act_fwd");
}
// dgamma / dbeta: [C] outputs (always computed); coef: 2 C floats of scratch
int nc_batchnorm_act_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         float slope, int training, float* dx, float* dgamma, float* dbeta, float* coef, int N, int C, long S, void* ws,
                         size_t ws_bytes, void* stream) {
  if (!dy || !x || !mean || !rstd || !gamma || !beta || !dx || !dgamma || !dbeta || !coef) { set_error("batchnorm_act_bwd: null pointer"); return NC_ERR_ARG; }
  if (N < 1 || C < 1 || S < 1 || C > 65535 || (long)N * C > 0x7fffffffL) { set_error("batchnorm_act_bwd: bad shape"); return NC_ERR_SHAPE; }
  if (!ws || ws_bytes < nc_instnorm_ws_bytes(N * C, S)) { set_error("batchnorm_act_bwd: workspace too small"); return NC_ERR_WS; }
  hipStream_t s = (hipStream_t)stream;
  const int splits = pick_splits(N * C, S);
  const long NCl = (long)N * C, step = (long)(65535 / C) * C;  // whole samples per launch (gridDim.y <= 65535)
  for (long i0 = 0; i0 < NCl; i0 += step) {
    const int ni = NCl - i0 < step ? (int)(NCl - i0) : (int)step;
    hipLaunchKernelGGL(k_bn_bwd_sums, dim3(splits, ni), dim3(256), 0, s, dy + i0 * S, x + i0 * S, mean, rstd, gamma, beta, slope, C, S, splits,
                       (double*)ws + i0 * splits * 2);
  }
  hipLaunchKernelGGL(k_bn_bwd_finalize, dim3((unsigned)cdiv(C, 128)), dim3(128), 0, s, (const double*)ws, N, C, splits, S, dgamma, dbeta, coef);
  long bx = cdiv(S, 1024 * 4);
  if (bx > 1024) bx = 1024;
  for (long i0 = 0; i0 < NCl; i0 += step) {
    const int ni = NCl - i0 < step ? (int)(NCl - i0) : (int)step;
    hipLaunchKernelGGL(k_bn_bwd_apply, dim3((unsigned)bx, ni), dim3(256), 0, s, dy + i0 * S, x + i0 * S, mean, rstd, gamma, beta, slope, coef, training,
                       dx + i0 * S, C, S);
  }
  return check_launch("batchnorm_act_bwd");
}
}  // extern "C"
