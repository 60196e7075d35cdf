// KernelGAN patch discriminator (KernelPatchDiscriminator, models/networks.py:1113-1145 of the reference; --netD kernelGAN,
// :243-244) with InstanceNorm, 1 input channel and ndf = 64, as one C call per direction:
//
//   z1 = W1 * x + b1     (valid 7^nd conv, 1 -> 64)        first_layer
//   z2 = W2 z1 + b2      (1x1, 64 -> 64) -> IN -> ReLU     feature_block.0 / 1 / 2      a2
//   z3 = W3 a2 + b3      (1x1)           -> IN -> ReLU     feature_block.3 / 4 / 5      a3
//   z4 = W4 a3 + b4      (1x1)           -> IN -> ReLU     feature_block.6 / 7 / 8      a4
//   y  = W5 a4 + b5      (1x1, 64 -> 1)                    final_layer
//
// Nothing nonlinear sits between the first two convolutions, so they collapse exactly: z2 = W' * x + b' with
// W' = W2 W1 (64 x 7^nd taps) and b' = W2 b1 + b2.  The 64-channel z1 is never formed.  Backward of the collapse, with
// G = sum_p dz2[p] patch(x)[p]^T (64 x taps) and s = sum_p dz2[p]:  dW2 = G W1^T + s b1^T,  dW1 = W2^T G,  db2 = s,  db1 = W2^T s,
// and dx is the full correlation of dz2 with W'.
//
// Layout: every 64-channel map is [B][64][P] (P = output pixels of one plane), so one (plane, channel) row is contiguous.
// GEMM kernels (v_mfma_f32_16x16x4_f32, exact fp32 products, fp32 accumulation): a wave owns 64 channels x 32 pixels of one
// plane (M = channels, N = pixels); the 1x1 weights sit in registers, the collapsed 7^nd weights in LDS.  The previous layer's
// InstanceNorm + ReLU is applied in the B-operand prologue from its (mean, 1/std), the InstanceNorm backward's
// g - mean(g) - n mean(g n) by a per-(plane, channel) row kernel.  Weight gradients: fixed-order split-P partials per workgroup,
// summed over workgroups in index order.  No float atomics anywhere: the same bits every run.
#include "common.hpp"

namespace nc {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kC = 64;         // ndf of the fused path
constexpr int kThreads = 256;  // 4 waves
constexpr int kTile = 128;     // pixels per GEMM workgroup (32 per wave)
constexpr int kUnit = 64;      // pixels per weight-gradient unit
constexpr int kWg = kC * kC + kC;  // one 1x1 layer's weight + bias gradient floats

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float nrm(float z, float mu, float rs) { return (z - mu) * rs; }

struct Geo {
  int B, D, H, W, nd, T, Tp, Do, Ho, Wo, nblk;
  long S, P;
};

__device__ __forceinline__ long pix_base(const Geo& g, long p) {  // input offset of output pixel p's patch origin
  const int ox = (int)(p % g.Wo);
  const long r = p / g.Wo;
  const int oy = (int)(r % g.Ho), oz = (int)(r / g.Ho);
  return ((long)oz * g.H + oy) * g.W + ox;
}
__device__ __forceinline__ long tap_off(const Geo& g, int t) {
  const int tz = t / 49, ty = (t / 7) % 7, tx = t % 7;
  return ((long)tz * g.H + ty) * g.W + tx;
}

// fixed-order block sum (256 threads); red holds 256 values; every thread gets the total
template <typename T>
__device__ T block_sum(T v, T* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// W' = W2 W1 ([64][Tp], taps T .. Tp - 1 zero) and b' = W2 b1 + b2
__global__ void __launch_bounds__(kThreads) k_kg_collapse(const float* __restrict__ w1, const float* __restrict__ b1,
                                                          const float* __restrict__ w2, const float* __restrict__ b2,
                                                          float* __restrict__ wc, float* __restrict__ bc, int T, int Tp) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < kC * Tp) {
    const int c = i / Tp, t = i - c * Tp;
    float s = 0.f;
    if (t < T)
      for (int k = 0; k < kC; ++k) s = fmaf(w2[c * kC + k], w1[k * T + t], s);
    wc[i] = s;
  } else if (i < kC * Tp + kC) {
    const int c = i - kC * Tp;
    float s = 0.f;
    for (int k = 0; k < kC; ++k) s = fmaf(w2[c * kC + k], b1[k], s);
    bc[c] = s + b2[c];
  }
}

// z2[b][c][p] = sum_t W'[c][t] x[b][base(p) + off(t)] + b'[c]: M = 64 channels (A = W' from LDS), K = taps, N = pixels (B = x gather)
__global__ void __launch_bounds__(kThreads) k_kg_conv7(const Geo g, const float* __restrict__ x, const float* __restrict__ wc,
                                                       const float* __restrict__ bc, float* __restrict__ z) {
  extern __shared__ float wl[];  // [64][Tp + 1]
  const int ld = g.Tp + 1;
  for (int i = threadIdx.x; i < kC * g.Tp; i += kThreads) {
    const int c = i / g.Tp;
    wl[c * ld + i - c * g.Tp] = wc[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
  const int b = blockIdx.y;
  const long p0 = (long)blockIdx.x * kTile + wave * 32;
  const float* xb = x + (long)b * g.S;
  long base[2];
  bool ok[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const long p = p0 + 16 * nt + m;
    ok[nt] = p < g.P;
    base[nt] = pix_base(g, ok[nt] ? p : 0);
  }
  f32x4 acc[4][2];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ks = 0; ks < g.Tp / 4; ++ks) {
    const int t = 4 * ks + kq;
    float bv[2] = {0.f, 0.f};
    if (t < g.T) {
      const long off = tap_off(g, t);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) bv[nt] = ok[nt] ? xb[base[nt] + off] : 0.f;
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const float a = wl[(16 * mt + m) * ld + 4 * ks + kq];
      acc[mt][0] = mfma4(a, bv[0], acc[mt][0]);
      acc[mt][1] = mfma4(a, bv[1], acc[mt][1]);
    }
  }
  // D[channel 16 mt + 4 kq + e][pixel m]
  float* zb = z + (long)b * kC * g.P;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    if (!ok[nt]) continue;
    const long p = p0 + 16 * nt + m;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 16 * mt + 4 * kq + e;
        zb[(long)c * g.P + p] = acc[mt][nt][e] + bc[c];
      }
  }
}

// InstanceNorm statistics of one (plane, channel) row: st = (mean, 1 / sqrt(biased var + eps)).  One pass over the values shifted by the
// row's first one, sums in fp64: the variance is exact to fp32 rounding even where it is tiny against the mean (planes of two pixels).
__global__ void __launch_bounds__(kThreads) k_kg_stats(const float* __restrict__ z, float* __restrict__ st, long P, float eps) {
  __shared__ double red[kThreads];
  const long row = blockIdx.x;
  const float* r = z + row * P;
  const double sh = r[0];
  double s1 = 0.0, s2 = 0.0;
  for (long i = threadIdx.x; i < P; i += kThreads) {
    const double d = (double)r[i] - sh;
    s1 += d;
    s2 = fma(d, d, s2);
  }
  const double m1 = block_sum(s1, red) / (double)P;
  const double m2 = block_sum(s2, red) / (double)P;
  if (threadIdx.x == 0) {
    st[2 * row] = (float)(sh + m1);
    st[2 * row + 1] = (float)(1.0 / sqrt(fmax(m2 - m1 * m1, 0.0) + (double)eps));
  }
}

// The 1x1 64 -> 64 layers, M = 64 channels (A = the weights, in registers), K = 64 channels, N = 64 pixels per wave, lane (m, kq) holding
// pixels p0 + 4 m + nt (nt = 0 .. 3): four consecutive pixels per lane, one 16-byte access per channel when V (P % 4 == 0).
//   forward (DGRAD = false): out[co][p] = sum_ci W[co][ci] relu(IN(in))[ci][p] + bias[co]      (IN from st)
//   data gradient (true):     out[ci][p] = (sum_co W[co][ci] in[co][p]) [IN(zp)[ci][p] > 0]    (in = gz; IN of the layer below from st)
constexpr int kTile1 = 256;  // pixels per 1x1 workgroup

template <bool DGRAD, bool V>
__global__ void __launch_bounds__(kThreads) k_kg_1x1(long P, const float* __restrict__ in, const float* __restrict__ st,
                                                     const float* __restrict__ w, const float* __restrict__ bias,
                                                     const float* __restrict__ zp, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
  const int b = blockIdx.y;
  const long q0 = (long)blockIdx.x * kTile1 + wave * 64 + 4 * m;  // this lane's first pixel
  const bool full = q0 + 3 < P;
  float a[4][16], mu[16], rs[16];
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
    const int k = 4 * ks + kq;
    if (!DGRAD) {
      mu[ks] = st[2 * (b * kC + k)];
      rs[ks] = st[2 * (b * kC + k) + 1];
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) a[mt][ks] = DGRAD ? w[k * kC + 16 * mt + m] : w[(16 * mt + m) * kC + k];
  }
  const float* ib = in + (long)b * kC * P;
  auto load4 = [&](const float* row, float (&v)[4]) {
    if (V && full) {
      const float4 t = *reinterpret_cast<const float4*>(row + q0);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) v[nt] = q0 + nt < P ? row[q0 + nt] : 0.f;
    }
  };
  f32x4 acc[4][4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
    float bv[4];
    load4(ib + (long)(4 * ks + kq) * P, bv);
    if (!DGRAD) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) bv[nt] = q0 + nt < P ? fmaxf(nrm(bv[nt], mu[ks], rs[ks]), 0.f) : 0.f;
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = mfma4(a[mt][ks], bv[nt], acc[mt][nt]);
  }
  // D[channel 16 mt + 4 kq + e][pixel (nt, m)]
  float* ob = out + (long)b * kC * P;
  const float* zb = DGRAD ? zp + (long)b * kC * P : nullptr;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 16 * mt + 4 * kq + e;
      float v[4];
      if (DGRAD) {
        const float cm = st[2 * (b * kC + c)], cr = st[2 * (b * kC + c) + 1];
        float zv[4];
        load4(zb + (long)c * P, zv);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) v[nt] = nrm(zv[nt], cm, cr) > 0.f ? acc[mt][nt][e] : 0.f;
      } else {
        const float bc = bias[c];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) v[nt] = acc[mt][nt][e] + bc;
      }
      float* orow = ob + (long)c * P;
      if (V && full) {
        *reinterpret_cast<float4*>(orow + q0) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          if (q0 + nt < P) orow[q0 + nt] = v[nt];
      }
    }
}

template <bool DGRAD>
void launch_1x1(const Geo& g, const float* in, const float* st, const float* w, const float* bias, const float* zp, float* out,
                hipStream_t s) {
  const dim3 grid(cdiv(g.P, kTile1), g.B);
  if (g.P % 4 == 0)
    hipLaunchKernelGGL((k_kg_1x1<DGRAD, true>), grid, dim3(kThreads), 0, s, g.P, in, st, w, bias, zp, out);
  else
    hipLaunchKernelGGL((k_kg_1x1<DGRAD, false>), grid, dim3(kThreads), 0, s, g.P, in, st, w, bias, zp, out);
}

// y[b][p] = sum_c W5[c] relu(IN(z4))[c][p] + b5
__global__ void __launch_bounds__(kThreads) k_kg_final_fwd(long P, const float* __restrict__ z4, const float* __restrict__ st4,
                                                           const float* __restrict__ w5, const float* __restrict__ b5,
                                                           float* __restrict__ y) {
  __shared__ float co[3 * kC];
  const int b = blockIdx.y;
  if (threadIdx.x < kC) {
    co[threadIdx.x] = w5[threadIdx.x];
    co[kC + threadIdx.x] = st4[2 * (b * kC + threadIdx.x)];
    co[2 * kC + threadIdx.x] = st4[2 * (b * kC + threadIdx.x) + 1];
  }
  __syncthreads();
  const long p = (long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= P) return;
  const float* zb = z4 + (long)b * kC * P + p;
  float s = 0.f;
  for (int c = 0; c < kC; ++c) s = fmaf(co[c], fmaxf(nrm(zb[(long)c * P], co[kC + c], co[2 * kC + c]), 0.f), s);
  y[(long)b * P + p] = s + b5[0];
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// InstanceNorm(affine=False) + ReLU backward of one (plane, channel) row: n = (z - mean) rstd, gn = g [n > 0] (g already masked
// when it comes from a dgrad kernel; from the final layer it is W5[c] dy[p] [n > 0]), gz = rstd (gn - mean(gn) - n mean(gn n)).
// gz may alias g.  With dy: also pw5[row] = sum_p dy a4 and, for channel 0, pb5[b] = sum_p dy.
__global__ void __launch_bounds__(kThreads) k_kg_norm_bwd(long P, const float* g, const float* __restrict__ dy,
                                                          const float* __restrict__ w5, const float* __restrict__ z,
                                                          const float* __restrict__ st, float* gz, float* __restrict__ pw5,
                                                          float* __restrict__ pb5) {
  __shared__ double red[kThreads];
  const long row = blockIdx.x;
  const int b = (int)(row / kC), c = (int)(row % kC);
  const float mu = st[2 * row], rs = st[2 * row + 1];
  const float* zr = z + row * P;
  const float* gr = g + row * P;
  const float* dr = dy ? dy + (long)b * P : nullptr;
  const float wc = dy ? w5[c] : 0.f;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
  for (long i = threadIdx.x; i < P; i += kThreads) {
    const float n = nrm(zr[i], mu, rs);
    float gn;
    if (dr) {
      const float d = dr[i];
      gn = n > 0.f ? wc * d : 0.f;
      s3 = fma((double)d, (double)fmaxf(n, 0.f), s3);
      s4 += d;
    } else {
      gn = gr[i];
    }
    s1 += gn;
    s2 = fma((double)gn, (double)n, s2);
  }
  const double m1 = block_sum(s1, red) / (double)P;
  const double m2 = block_sum(s2, red) / (double)P;
  if (dr) {
    s3 = block_sum(s3, red);
    s4 = block_sum(s4, red);
    if (threadIdx.x == 0) {
      if (pw5) pw5[row] = (float)s3;
      if (pb5 && c == 0) pb5[b] = (float)s4;
    }
  }
  float* out = gz + row * P;
  for (long i = threadIdx.x; i < P; i += kThreads) {
    const float n = nrm(zr[i], mu, rs);
    const float gn = dr ? (n > 0.f ? wc * dr[i] : 0.f) : gr[i];
    out[i] = (float)((double)rs * ((double)gn - m1 - (double)n * m2));
  }
}

// Weight-gradient partials, one slab of kWg floats per (workgroup, tap block): slab[m][n] = sum_p gz[m][p] B[n][p], slab[4096 + m] =
// sum_p gz[m][p].  M = 64 channels of gz, K = pixels, N = 64 columns of B:
//   TAPS = false: B = relu(IN(zp)) (1x1 layer: dW[co][ci], db[co]);  TAPS = true: B[t][p] = x[base(p) + off(t)], t = 64 blockIdx.y + n
//   (the collapsed first layers: G[c][t], s[c]).
// Units of 64 pixels of one plane; workgroup x takes units [x per, (x + 1) per), wave w every fourth from w; the waves' sums are added
// in LDS in wave order.
struct WgArgs {
  const float* gz;
  const float* zp;
  const float* stp;
  const float* x;
  float* part;
  long units, per;
  int cp;  // units per plane
};

template <bool TAPS>
__global__ void __launch_bounds__(kThreads) k_kg_wgrad(const Geo g, const WgArgs q) {
  __shared__ float red[kC * kC + 4 * kC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
  const int tb = blockIdx.y;
  const long u0 = (long)blockIdx.x * q.per, u1 = u0 + q.per < q.units ? u0 + q.per : q.units;
  f32x4 acc[4][4];
  float ds[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  long toff[4] = {0, 0, 0, 0};
  bool tok[4] = {false, false, false, false};
  if (TAPS) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int t = 64 * tb + 16 * nt + m;
      tok[nt] = t < g.T;
      toff[nt] = tap_off(g, tok[nt] ? t : 0);
    }
  }
  for (long u = u0 + wave; u < u1; u += 4) {
    const int b = (int)(u / q.cp);
    const long pc0 = (u % q.cp) * kUnit;
    const float* gb = q.gz + (long)b * kC * g.P;
    float mu[4], rs[4];
    if (!TAPS) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        mu[nt] = q.stp[2 * (b * kC + 16 * nt + m)];
        rs[nt] = q.stp[2 * (b * kC + 16 * nt + m) + 1];
      }
    }
    const float* zb = TAPS ? nullptr : q.zp + (long)b * kC * g.P;
    const float* xb = TAPS ? q.x + (long)b * g.S : nullptr;
#pragma unroll 4
    for (int ks = 0; ks < kUnit / 4; ++ks) {
      const long p = pc0 + 4 * ks + kq;
      const bool ok = p < g.P;
      float av[4], bv[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) av[mt] = ok ? gb[(long)(16 * mt + m) * g.P + p] : 0.f;
      if (TAPS) {
        const long base = pix_base(g, ok ? p : 0);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) bv[nt] = ok && tok[nt] ? xb[base + toff[nt]] : 0.f;
      } else {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) bv[nt] = ok ? fmaxf(nrm(zb[(long)(16 * nt + m) * g.P + p], mu[nt], rs[nt]), 0.f) : 0.f;
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        ds[mt] += av[mt];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = mfma4(av[mt], bv[nt], acc[mt][nt]);
      }
    }
  }
  // D[m = 16 mt + 4 kq + e][n = 16 nt + m]; ds[mt] belongs to row 16 mt + m, pixels of lane group kq
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int o = (16 * mt + 4 * kq + e) * kC + 16 * nt + m;
            red[o] = w == 0 ? acc[mt][nt][e] : red[o] + acc[mt][nt][e];
          }
        const int o = kC * kC + kq * kC + 16 * mt + m;
        red[o] = w == 0 ? ds[mt] : red[o] + ds[mt];
      }
    }
    __syncthreads();
  }
  float* out = q.part + ((long)blockIdx.x * gridDim.y + tb) * kWg;
  for (int o = threadIdx.x; o < kWg; o += kThreads) {
    if (o < kC * kC) {
      out[o] = red[o];
    } else {
      const int r = o - kC * kC;
      out[o] = ((red[kC * kC + r] + red[kC * kC + kC + r]) + red[kC * kC + 2 * kC + r]) + red[kC * kC + 3 * kC + r];
    }
  }
}

// out[i] = sum over parts in index order of part[pc * stride + i]; 16 loads in flight at a time, the additions in the same order
__global__ void __launch_bounds__(kThreads) k_kg_reduce(const float* __restrict__ part, float* __restrict__ out, int n, int parts,
                                                        long stride) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  int pc = 0;
  for (; pc + 16 <= parts; pc += 16) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = part[(pc + j) * stride + i];
#pragma unroll
    for (int j = 0; j < 16; ++j) s += v[j];
  }
  for (; pc < parts; ++pc) s += part[pc * stride + i];
  out[i] = s;
}

// Parameter gradients in state-dict order from the reduced slabs: r7 = [nblk][kWg] (G, s), r3 / r4 = dW, db of feature_block.3 / .6
__global__ void __launch_bounds__(kThreads) k_kg_grads(const float* __restrict__ prm, const float* __restrict__ r7,
                                                       const float* __restrict__ r3, const float* __restrict__ r4,
                                                       const float* __restrict__ pw5, const float* __restrict__ pb5,
                                                       float* __restrict__ dprm, int T, int B) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const float* w1 = prm;
  const float* b1 = w1 + kC * T;
  const float* w2 = b1 + kC;
  const long oW2 = (long)kC * T + kC, oW3 = oW2 + kWg, oW4 = oW3 + kWg, oW5 = oW4 + kWg, total = oW5 + kC + 1;
  if (i >= total) return;
  auto G = [&](int c, int t) { return r7[(long)(t / 64) * kWg + c * kC + (t % 64)]; };
  const float* s = r7 + kC * kC;
  float v = 0.f;
  if (i < (long)kC * T) {  // dW1 = W2^T G
    const int c1 = (int)(i / T), t = (int)(i % T);
    for (int c2 = 0; c2 < kC; ++c2) v = fmaf(w2[c2 * kC + c1], G(c2, t), v);
  } else if (i < oW2) {  // db1 = W2^T s
    const int c1 = (int)(i - (long)kC * T);
    for (int c2 = 0; c2 < kC; ++c2) v = fmaf(w2[c2 * kC + c1], s[c2], v);
  } else if (i < oW2 + kC * kC) {  // dW2 = G W1^T + s b1^T
    const int j = (int)(i - oW2), c2 = j / kC, c1 = j % kC;
    for (int t = 0; t < T; ++t) v = fmaf(G(c2, t), w1[c1 * T + t], v);
    v = fmaf(s[c2], b1[c1], v);
  } else if (i < oW3) {  // db2 = s
    v = s[i - oW2 - kC * kC];
  } else if (i < oW4) {
    v = r3[i - oW3];
  } else if (i < oW5) {
    v = r4[i - oW4];
  } else if (i < oW5 + kC) {  // dW5[c] = sum_b sum_p dy a4[c]
    const int c = (int)(i - oW5);
    for (int b = 0; b < B; ++b) v += pw5[b * kC + c];
  } else {  // db5 = sum dy
    for (int b = 0; b < B; ++b) v += pb5[b];
  }
  dprm[i] = v;
}

// dx[b][q] = sum_tz sum_c sum_ty sum_tx W'[c][t] gz2[b][c][q - (tz, ty, tx)] (the full correlation, 64 -> 1).  A workgroup: 16 rows x
// 64 columns of one input plane; per (tz, c) the 22 x 70 window of gz2 goes through LDS, each thread sums 4 consecutive columns.
constexpr int kDxR = 16, kDxC = 64, kDxWR = kDxR + 6, kDxWC = kDxC + 6, kDxP = 72;
__global__ void __launch_bounds__(kThreads) k_kg_dx(const Geo g, const float* __restrict__ gz, const float* __restrict__ wc,
                                                    float* __restrict__ dx) {
  __shared__ float win[kDxWR * kDxP];
  const int b = blockIdx.z / g.D, qz = blockIdx.z % g.D;
  const int y0 = blockIdx.y * kDxR, x0 = blockIdx.x * kDxC;
  const int r = threadIdx.x >> 4, c4 = (threadIdx.x & 15) * 4;
  // three-level sums (a channel's 49 taps, the 64 channels of a depth tap, the depth taps): the error of one 3136- / 21952-term fmaf chain
  // would be well above the layered path's
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int ntz = g.nd == 3 ? 7 : 1;
  for (int tz = 0; tz < ntz; ++tz) {
    const int pz = qz - tz;
    if (pz < 0 || pz >= g.Do) continue;
    float acz[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < kC; ++c) {
      const float* src = gz + ((long)b * kC + c) * g.P + (long)pz * g.Ho * g.Wo;
      __syncthreads();
      for (int i = threadIdx.x; i < kDxWR * kDxWC; i += kThreads) {
        const int rr = i / kDxWC, cc = i - rr * kDxWC;
        const int py = y0 - 6 + rr, px = x0 - 6 + cc;
        win[rr * kDxP + cc] = (unsigned)py < (unsigned)g.Ho && (unsigned)px < (unsigned)g.Wo ? src[(long)py * g.Wo + px] : 0.f;
      }
      __syncthreads();
      const float* wt = wc + c * g.Tp + tz * 49;
      float acn[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ty = 0; ty < 7; ++ty) {
        const float* wr = win + (r + 6 - ty) * kDxP + c4;
        float v[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) v[j] = wr[j];
#pragma unroll
        for (int tx = 0; tx < 7; ++tx) {
          const float w = wt[ty * 7 + tx];
#pragma unroll
          for (int j = 0; j < 4; ++j) acn[j] = fmaf(w, v[j - tx + 6], acn[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acz[j] += acn[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += acz[j];
  }
  const int qy = y0 + r;
  if (qy < g.H) {
    float* out = dx + (((long)b * g.D + qz) * g.H + qy) * g.W;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + c4 + j < g.W) out[x0 + c4 + j] = acc[j];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
int geo(const char* what, Geo& g, int B, int D, int H, int W, int ndf, int nd) {
  if (nd != 2 && nd != 3) { set_error("%s: nd = %d (2 or 3)", what, nd); return NC_ERR_ARG; }
  if (ndf != kC) { set_error("%s: ndf = %d (the fused path covers ndf = 64)", what, ndf); return NC_ERR_SHAPE; }
  if (nd == 2 && D != 1) { set_error("%s: 2-D input needs D = 1, got %d", what, D); return NC_ERR_SHAPE; }
  if (B < 1 || H < 7 || W < 7 || (nd == 3 && D < 7)) {
    set_error("%s: B=%d D=%d H=%d W=%d: every spatial edge must be >= 7 (first_layer is a valid 7^%d conv)", what, B, D, H, W, nd);
    return NC_ERR_SHAPE;
  }
  g.B = B; g.D = D; g.H = H; g.W = W; g.nd = nd;
  g.T = nd == 3 ? 343 : 49;
  g.Tp = (g.T + 3) / 4 * 4;
  g.nblk = (g.T + 63) / 64;
  g.Do = nd == 3 ? D - 6 : 1;
  g.Ho = H - 6;
  g.Wo = W - 6;
  g.S = (long)D * H * W;
  g.P = (long)g.Do * g.Ho * g.Wo;
  if (g.P < 2) {
    set_error("%s: the output plane has one element (input %dx%dx%d): InstanceNorm needs more than one value per channel", what, D, H, W);
    return NC_ERR_SHAPE;
  }
  if (B > 65535 || (long)B * D > 65535 || g.P > (1L << 30) || (long)B * kC * g.P > (1L << 40)) {
    set_error("%s: B=%d D=%d H=%d W=%d is beyond the launch geometry", what, B, D, H, W);
    return NC_ERR_SHAPE;
  }
  return NC_OK;
}

struct Plan {
  long units, per;
  int cp, p1, p7;          // weight-gradient units; workgroups of the 1x1 / first-layer weight gradients
  size_t o_wc, o_bc, o_a, o_b, o_pw5, o_pb5, o_r3, o_r4, o_r7, o_part, total;  // float offsets in the workspace
};

Plan plan(const Geo& g) {
  Plan p;
  p.cp = (int)cdiv(g.P, kUnit);
  p.units = (long)g.B * p.cp;
  // ~1024 workgroups per weight-gradient launch, the same split for both kinds (per is shared)
  long want = 1024 / g.nblk;
  if (want > p.units) want = p.units;
  p.per = cdiv(p.units, want);
  p.p1 = p.p7 = (int)cdiv(p.units, p.per);
  auto al = [](size_t n) { return (n + 63) / 64 * 64; };
  size_t o = 0;
  p.o_wc = o; o += al((size_t)kC * g.Tp);
  p.o_bc = o; o += al(kC);
  const size_t map = (size_t)g.B * kC * g.P;
  p.o_a = o; o += al(map);
  p.o_b = o; o += al(map);
  p.o_pw5 = o; o += al((size_t)g.B * kC);
  p.o_pb5 = o; o += al(g.B);
  p.o_r3 = o; o += al(kWg);
  p.o_r4 = o; o += al(kWg);
  p.o_r7 = o; o += al((size_t)g.nblk * kWg);
  p.o_part = o; o += (size_t)p.p7 * g.nblk * kWg;
  p.total = o;
  return p;
}

size_t saved_floats(const Geo& g) { return 3 * (size_t)g.B * kC * g.P + 3 * 2 * (size_t)g.B * kC; }

struct Prm {  // packed parameters in state-dict order
  const float *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4, *w5, *b5;
};
Prm unpack(const float* p, int T) {
  Prm r;
  r.w1 = p; r.b1 = r.w1 + kC * T; r.w2 = r.b1 + kC; r.b2 = r.w2 + kC * kC; r.w3 = r.b2 + kC; r.b3 = r.w3 + kC * kC;
  r.w4 = r.b3 + kC; r.b4 = r.w4 + kC * kC; r.w5 = r.b4 + kC; r.b5 = r.w5 + kC;
  return r;
}

int launch_collapse(const Geo& g, const Prm& w, float* ws, const Plan& pl, hipStream_t s) {
  hipLaunchKernelGGL(k_kg_collapse, dim3(cdiv(kC * g.Tp + kC, kThreads)), dim3(kThreads), 0, s, w.w1, w.b1, w.w2, w.b2, ws + pl.o_wc,
                     ws + pl.o_bc, g.T, g.Tp);
  return check_launch("kgan collapse");
}

int reduce(const float* part, float* out, int n, int parts, long stride, hipStream_t s) {
  hipLaunchKernelGGL(k_kg_reduce, dim3(cdiv(n, kThreads)), dim3(kThreads), 0, s, part, out, n, parts, stride);
  return check_launch("kgan reduce");
}

}  // namespace
}  // namespace nc

using namespace nc;

extern "C" {

size_t nc_kgan_param_floats(int ndf, int nd) {
  if (ndf < 1 || (nd != 2 && nd != 3)) return 0;
  const size_t T = nd == 3 ? 343 : 49;
  return (size_t)ndf * T + ndf + 3 * ((size_t)ndf * ndf + ndf) + ndf + 1;
}

size_t nc_kgan_saved_floats(int B, int D, int H, int W, int ndf, int nd) {
  Geo g;
  if (geo("kgan_saved_floats", g, B, D, H, W, ndf, nd)) return 0;
  return saved_floats(g);
}

size_t nc_kgan_ws_bytes(int B, int D, int H, int W, int ndf, int nd) {
  Geo g;
  if (geo("kgan_ws_bytes", g, B, D, H, W, ndf, nd)) return 0;
  return plan(g).total * sizeof(float);
}

int nc_kgan_out_shape(int B, int D, int H, int W, int ndf, int nd, int* oD, int* oH, int* oW) {
  Geo g;
  if (int e = geo("kgan_out_shape", g, B, D, H, W, ndf, nd)) return e;
  if (oD) *oD = g.Do;
  if (oH) *oH = g.Ho;
  if (oW) *oW = g.Wo;
  return NC_OK;
}

// KernelPatchDiscriminator.forward (networks.py:1141-1144)
int nc_kgan_fwd(const float* params, const float* x, float* y, float* saved, int B, int D, int H, int W, int ndf, int nd, void* ws,
                size_t ws_bytes, void* stream) {
  Geo g;
  if (int e = geo("kgan_fwd", g, B, D, H, W, ndf, nd)) return e;
  if (!params || !x || !y || !saved) { set_error("kgan_fwd: null pointer"); return NC_ERR_ARG; }
  const Plan pl = plan(g);
  if (!ws || ws_bytes < pl.total * sizeof(float)) { set_error("kgan_fwd: workspace %zu < %zu bytes", ws_bytes, pl.total * sizeof(float)); return NC_ERR_WS; }
  hipStream_t s = (hipStream_t)stream;
  float* wsf = (float*)ws;
  const Prm w = unpack(params, g.T);
  const size_t map = (size_t)B * kC * g.P;
  float *z2 = saved, *z3 = z2 + map, *z4 = z3 + map, *st2 = z4 + map, *st3 = st2 + 2 * B * kC, *st4 = st3 + 2 * B * kC;
  if (int e = launch_collapse(g, w, wsf, pl, s)) return e;
  const int lds = kC * (g.Tp + 1) * (int)sizeof(float);
  // raised once per device, so to the 3-D size whatever the first call is
  if (int e = raise_dyn_lds(k_kg_conv7, kC * (344 + 1) * (int)sizeof(float), "kgan conv7")) return e;
  const dim3 tiles(cdiv(g.P, kTile), B);
  hipLaunchKernelGGL(k_kg_conv7, tiles, dim3(kThreads), lds, s, g, x, wsf + pl.o_wc, wsf + pl.o_bc, z2);
  if (int e = check_launch("kgan conv7")) return e;
  const float eps = 1e-5f;
  hipLaunchKernelGGL(k_kg_stats, dim3(B * kC), dim3(kThreads), 0, s, z2, st2, g.P, eps);
  launch_1x1<false>(g, z2, st2, w.w3, w.b3, nullptr, z3, s);
  hipLaunchKernelGGL(k_kg_stats, dim3(B * kC), dim3(kThreads), 0, s, z3, st3, g.P, eps);
  launch_1x1<false>(g, z3, st3, w.w4, w.b4, nullptr, z4, s);
  hipLaunchKernelGGL(k_kg_stats, dim3(B * kC), dim3(kThreads), 0, s, z4, st4, g.P, eps);
  hipLaunchKernelGGL(k_kg_final_fwd, dim3(cdiv(g.P, kThreads), B), dim3(kThreads), 0, s, g.P, z4, st4, w.w5, w.b5, y);
  return check_launch("kgan fwd");
}

// its backward (loss.backward() through netD, e.g. apollo_model.py:195-283)
int nc_kgan_bwd(const float* params, const float* x, const float* saved, const float* dy, float* dx, float* dparams, int B, int D, int H,
                int W, int ndf, int nd, void* ws, size_t ws_bytes, void* stream) {
  Geo g;
  if (int e = geo("kgan_bwd", g, B, D, H, W, ndf, nd)) return e;
  if (!params || !x || !saved || !dy) { set_error("kgan_bwd: null pointer"); return NC_ERR_ARG; }
  const Plan pl = plan(g);
  if (!ws || ws_bytes < pl.total * sizeof(float)) { set_error("kgan_bwd: workspace %zu < %zu bytes", ws_bytes, pl.total * sizeof(float)); return NC_ERR_WS; }
  if (!dx && !dparams) return NC_OK;
  hipStream_t s = (hipStream_t)stream;
  float* wsf = (float*)ws;
  const Prm w = unpack(params, g.T);
  const size_t map = (size_t)B * kC * g.P;
  const float *z2 = saved, *z3 = z2 + map, *z4 = z3 + map, *st2 = z4 + map, *st3 = st2 + 2 * B * kC, *st4 = st3 + 2 * B * kC;
  float *A = wsf + pl.o_a, *Bf = wsf + pl.o_b;
  float *pw5 = wsf + pl.o_pw5, *pb5 = wsf + pl.o_pb5;
  const bool wg = dparams != nullptr;
  const dim3 rows(B * kC);
  WgArgs q{nullptr, nullptr, nullptr, x, wsf + pl.o_part, pl.units, pl.per, pl.cp};

  // final layer + feature_block.8 / .7: gz4 -> A
  hipLaunchKernelGGL(k_kg_norm_bwd, rows, dim3(kThreads), 0, s, g.P, (const float*)nullptr, dy, w.w5, z4, st4, A, wg ? pw5 : nullptr,
                     wg ? pb5 : nullptr);
  // feature_block.6: da3 masked by feature_block.5 -> B, dW4 / db4
  launch_1x1<true>(g, A, st3, w.w4, nullptr, z3, Bf, s);
  if (wg) {
    q.gz = A; q.zp = z3; q.stp = st3;
    hipLaunchKernelGGL(k_kg_wgrad<false>, dim3(pl.p1, 1), dim3(kThreads), 0, s, g, q);
    if (int e = check_launch("kgan wgrad 6")) return e;
    if (int e = reduce(wsf + pl.o_part, wsf + pl.o_r4, kWg, pl.p1, kWg, s)) return e;
  }
  // feature_block.4: gz3 in place in B; feature_block.3: da2 masked by feature_block.2 -> A, dW3 / db3
  hipLaunchKernelGGL(k_kg_norm_bwd, rows, dim3(kThreads), 0, s, g.P, Bf, (const float*)nullptr, w.w5, z3, st3, Bf, nullptr, nullptr);
  launch_1x1<true>(g, Bf, st2, w.w3, nullptr, z2, A, s);
  if (wg) {
    q.gz = Bf; q.zp = z2; q.stp = st2;
    hipLaunchKernelGGL(k_kg_wgrad<false>, dim3(pl.p1, 1), dim3(kThreads), 0, s, g, q);
    if (int e = check_launch("kgan wgrad 3")) return e;
    if (int e = reduce(wsf + pl.o_part, wsf + pl.o_r3, kWg, pl.p1, kWg, s)) return e;
  }
  // feature_block.1: gz2 in place in A
  hipLaunchKernelGGL(k_kg_norm_bwd, rows, dim3(kThreads), 0, s, g.P, A, (const float*)nullptr, w.w5, z2, st2, A, nullptr, nullptr);
  if (int e = check_launch("kgan bwd")) return e;
  if (int e = launch_collapse(g, w, wsf, pl, s)) return e;
  if (wg) {  // the collapsed first layers: G, s -> every parameter gradient
    q.gz = A; q.zp = nullptr; q.stp = nullptr;
    hipLaunchKernelGGL(k_kg_wgrad<true>, dim3(pl.p7, g.nblk), dim3(kThreads), 0, s, g, q);
    if (int e = check_launch("kgan wgrad 0")) return e;
    if (int e = reduce(wsf + pl.o_part, wsf + pl.o_r7, g.nblk * kWg, pl.p7, (long)g.nblk * kWg, s)) return e;
    const long total = (long)kC * g.T + kC + 3 * kWg + kC + 1;
    hipLaunchKernelGGL(k_kg_grads, dim3(cdiv(total, kThreads)), dim3(kThreads), 0, s, params, wsf + pl.o_r7, wsf + pl.o_r3,
                       wsf + pl.o_r4, pw5, pb5, dparams, g.T, B);
    if (int e = check_launch("kgan grads")) return e;
  }
  if (dx) {
    hipLaunchKernelGGL(k_kg_dx, dim3(cdiv(W, kDxC), cdiv(H, kDxR), B * D), dim3(kThreads), 0, s, g, A, wsf + pl.o_wc, dx);
    if (int e = check_launch("kgan dx")) return e;
  }
  return NC_OK;
}

}  // extern "C"
