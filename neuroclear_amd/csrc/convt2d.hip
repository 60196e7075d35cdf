// ConvTranspose2d(kernel 2, stride 2) forward / dgrad / wgrad (reference models/networks.py:382-390 with dimension == 2, used at :500,503 by
// Unet_deconv and :566-572 by Unet_vanilla: t_conv3 512->256, t_conv2 256->128, t_conv1 128->64).  With k == s every output pixel depends on
// exactly one input pixel:  y[n, k, 2u+a, 2v+b] = bias[k] + sum_c x[n, c, u, v] * w[c, k, a, b]  -- the GEMM [N H W x C] . [C x 4K] whose
// epilogue writes the 2 x 2 pixel shuffle.  The 2-D sibling of convt.hip: same structure, 4 taps instead of 8.  fp32 throughout; no atomics,
// so every result is run-to-run bit-identical.
#include "common.hpp"

namespace nc {

// VALU forward: one lane owns one INPUT pixel and KT output channels x 4 taps of accumulators; the weights are wave-uniform (scalar cache).
template <int KT>
__global__ __launch_bounds__(256) void k_convT2d_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                     float* __restrict__ y, int C, int H, int W, int K) {
  const long S = (long)H * W;
  const long pos = (long)blockIdx.x * 256 + threadIdx.x;
  const int k0 = blockIdx.y * KT, n = blockIdx.z;
  const bool valid = pos < S;
  const long p = valid ? pos : 0;
  const int iv = (int)(p % W), iu = (int)(p / W);
  float acc[KT][4];
#pragma unroll
  for (int j = 0; j < KT; ++j)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[j][t] = 0.f;
  const float* xn = x + (long)n * C * S + p;
  for (int c = 0; c < C; ++c) {
    const float xv = xn[(long)c * S];
    const float* wc = w + ((long)c * K + k0) * 4;
#pragma unroll
    for (int j = 0; j < KT; ++j)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[j][t] = fmaf(xv, wc[j * 4 + t], acc[j][t]);
  }
  if (!valid) return;
  const int W2 = 2 * W;
  const long S2 = 4 * S;
#pragma unroll
  for (int j = 0; j < KT; ++j) {
    float* yk = y + ((long)n * K + k0 + j) * S2;
    // the bias joins the finished sum (one rounding at the output's magnitude), as in convt.hip
    const float bj = bias ? bias[k0 + j] : 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      float2* dst = reinterpret_cast<float2*>(yk + (long)(2 * iu + a) * W2 + 2 * iv);
      *dst = make_float2(acc[j][a * 2] + bj, acc[j][a * 2 + 1] + bj);
    }
  }
}

// The same forward on the fp32 matrix cores (K % 32 == 0, C % 16 == 0): each tap (a, b) is a plain GEMM Y_ab[k][pixel] = sum_c W[c][k][ab] X[c][pixel].
// A wave owns one tile of 32 pixels and 32 output channels: 4 accumulator blocks (the taps), C / 2 k-steps of 4 x v_mfma_f32_32x32x2_f32.  The A
// operand of a k-step -- w[2s + h][kt * 32 + li][0..3] -- is ONE 16-byte load per lane straight from the weight tensor (its (k, tap) order is the
// operand order already; a workgroup's 32-channel slice is C * 512 bytes and stays in the caches), the B operand one dword of x.  Both are
// requested a group of 8 k-steps ahead.  No LDS, no barrier: the C == 512 layer needs no chunking of the reduction, and the sum of every output
// element is one chain over the channel pairs in ascending order whatever the grid.
typedef float f32x16 __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(256, 2) void k_convT2d_fwd_mfma(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ y, int C, int H, int W, int K, int N) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, h = lane >> 5;
  const int kt = blockIdx.y;
  const long S = (long)H * W;
  const long tiles_per_n = (S + 31) / 32, ntiles = tiles_per_n * N;
  const long tile = (long)blockIdx.x * 4 + wave;
  if (tile >= ntiles) return;  // wave-uniform; the kernel has no barrier
  const int n = (int)(tile / tiles_per_n);
  const long pos = (tile - (long)n * tiles_per_n) * 32 + li;
  const bool valid = pos < S;
  const long p = valid ? pos : S - 1;
  const float* xp = x + ((long)n * C + h) * S + p;                    // + 2 s S per k-step
  const float4* wp = reinterpret_cast<const float4*>(w) + ((long)h * K + kt * 32 + li);  // + 2 s K per k-step
  f32x16 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;
  const int CH = C / 2;
  float bc[8], bn[8];
  float4 ac[8], an[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    bc[i] = xp[(long)(2 * i) * S];
    ac[i] = wp[(long)(2 * i) * K];
  }
#pragma unroll 1
  for (int s0 = 0; s0 < CH; s0 += 8) {
    if (s0 + 8 < CH) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        bn[i] = xp[(long)(2 * (s0 + 8 + i)) * S];
        an[i] = wp[(long)(2 * (s0 + 8 + i)) * K];
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[i].x, bc[i], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[i].y, bc[i], acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[i].z, bc[i], acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[i].w, bc[i], acc[3], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      bc[i] = bn[i];
      ac[i] = an[i];
    }
  }
  if (!valid) return;
  const int iv = (int)(p % W), iu = (int)(p / W);
  const int W2 = 2 * W;
  const long S2 = 4 * S;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int k = kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;  // accumulator row of a 32 x 32 block
    const float bk = bias ? bias[k] : 0.f;
    float* yk = y + ((long)n * K + k) * S2;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      float2* dst = reinterpret_cast<float2*>(yk + (long)(2 * iu + a) * W2 + 2 * iv);
      *dst = make_float2(acc[a * 2][e] + bk, acc[a * 2 + 1][e] + bk);
    }
  }
}

template <int CT>
__global__ __launch_bounds__(256) void k_convT2d_dgrad(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx, int C,
                                                       int H, int W, int K) {
  const long S = (long)H * W;
  const long pos = (long)blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * CT, n = blockIdx.z;
  const bool valid = pos < S;
  const long p = valid ? pos : 0;
  const int iv = (int)(p % W), iu = (int)(p / W);
  const int W2 = 2 * W;
  const long S2 = 4 * S;
  float acc[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) acc[j] = 0.f;
  for (int k = 0; k < K; ++k) {
    const float* dyk = dy + ((long)n * K + k) * S2;
    float g[4];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const float2 v = *reinterpret_cast<const float2*>(dyk + (long)(2 * iu + a) * W2 + 2 * iv);
      g[a * 2] = v.x;
      g[a * 2 + 1] = v.y;
    }
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      // the 4 taps of an output channel are summed first and join the running sum as one term: K additions into acc, not one chain of 4 K
      const float* wc = w + ((long)(c0 + j) * K + k) * 4;
      float sk = g[0] * wc[0];
#pragma unroll
      for (int t = 1; t < 4; ++t) sk = fmaf(g[t], wc[t], sk);
      acc[j] += sk;
    }
  }
  if (valid) {
#pragma unroll
    for (int j = 0; j < CT; ++j) dx[((long)n * C + c0 + j) * S + pos] = acc[j];
  }
}

// dw[c][k][t] = sum_{n,pos} x[n][c][pos] * dy[n][k][2 pos + t].  Workgroup = (CB input channels) x (KB output channels); lanes stride over
// positions, CB * KB * 4 accumulators per lane, then a fixed-order reduction over lanes and waves.
template <int CB, int KB>
__global__ __launch_bounds__(256) void k_convT2d_wgrad(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dw, int N, int C,
                                                       int H, int W, int K) {
  const int c0 = blockIdx.x * CB, k0 = blockIdx.y * KB;
  const long S = (long)H * W, S2 = 4 * S;
  const int W2 = 2 * W;
  float acc[CB][KB][4];
#pragma unroll
  for (int i = 0; i < CB; ++i)
#pragma unroll
    for (int j = 0; j < KB; ++j)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[i][j][t] = 0.f;
  for (int n = 0; n < N; ++n) {
    for (long pos = threadIdx.x; pos < S; pos += 256) {
      const int iv = (int)(pos % W), iu = (int)(pos / W);
      float xv[CB];
#pragma unroll
      for (int i = 0; i < CB; ++i) xv[i] = x[((long)n * C + c0 + i) * S + pos];
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        const float* dyk = dy + ((long)n * K + k0 + j) * S2;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const float2 v = *reinterpret_cast<const float2*>(dyk + (long)(2 * iu + a) * W2 + 2 * iv);
#pragma unroll
          for (int i = 0; i < CB; ++i) {
            acc[i][j][a * 2] = fmaf(xv[i], v.x, acc[i][j][a * 2]);
            acc[i][j][a * 2 + 1] = fmaf(xv[i], v.y, acc[i][j][a * 2 + 1]);
          }
        }
      }
    }
  }
  __shared__ float red[4][CB * KB * 4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < CB; ++i)
#pragma unroll
    for (int j = 0; j < KB; ++j)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float v = acc[i][j][t];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if (lane == 0) red[wv][(i * KB + j) * 4 + t] = v;
      }
  __syncthreads();
  if (threadIdx.x < CB * KB * 4) {
    const int e = threadIdx.x, t = e & 3, j = (e >> 2) % KB, i = (e >> 2) / KB;
    dw[((long)(c0 + i) * K + k0 + j) * 4 + t] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
  }
}

static int pick(int n, int a, int b, int c) { return n % a == 0 ? a : n % b == 0 ? b : c; }

// ConvTranspose(k 2, s 2) is the adjoint of a stride-2 2 x 2 convolution with the SAME weight memory layout (w[Cin_T][Cout_T][2][2] == conv weight
// [K][C][taps] with K = Cin_T, C = Cout_T): its data gradient is that convolution's forward on dy, its weight gradient that convolution's weight
// gradient with the two tensors swapped -- both on the gather GEMM of conv_gemm.hip, as in convt.hip.
static bool convT2d_as_conv(ConvDims& d, int N, int C, int H, int W, int K) {
  return make_dims(d, N, K, 1, 2 * H, 2 * W, C, 1, 2, 2, 2, 0) && gemm_wgrad_supported(d);
}

static int convT2d_check(const char* what, int N, int C, int H, int W, int K) {
  if (N < 1 || C < 1 || H < 1 || W < 1 || K < 1 || K > 65535 || C > 65535 || N > 65535 || (long)H * W > (1L << 28)) {
    set_error("%s: bad shape N=%d C=%d H=%d W=%d K=%d", what, N, C, H, W, K);
    return NC_ERR_SHAPE;
  }
  return NC_OK;
}

// the matrix-core forward: the U-Nets' channel pairs (512, 256), (256, 128), (128, 64) and what shares their form
static bool convT2d_fwd_mfma_ok(int N, int C, int H, int W, int K) {
  return !sw::raw(sw::FORCE_DIRECT) && K % 32 == 0 && C % 16 == 0 && C >= 128 && cdiv(cdiv((long)H * W, 32) * N, 4) < (1L << 31);
}

}  // namespace nc

using namespace nc;

extern "C" {

size_t nc_convT2d_ws_bytes(int N, int C, int H, int W, int K) {
  size_t b = kBiasGradWsBytes;
  ConvDims d;
  if (convT2d_as_conv(d, N, C, H, W, K) && gemm_ws_bytes(d) > b) b = gemm_ws_bytes(d);
  return (b + 255) & ~(size_t)255;
}

int nc_convT2d_k2s2_fwd(const float* x, const float* w, const float* bias, float* y, int N, int C, int H, int W, int K, void* stream) {
  if (!x || !w || !y) { set_error("convT2d_fwd: null pointer"); return NC_ERR_ARG; }
  if (int e = convT2d_check("convT2d_fwd", N, C, H, W, K)) return e;
  const long S = (long)H * W;
  hipStream_t s = (hipStream_t)stream;
  if (convT2d_fwd_mfma_ok(N, C, H, W, K)) {
    const dim3 g((unsigned)cdiv(cdiv(S, 32) * N, 4), K / 32);
    hipLaunchKernelGGL(k_convT2d_fwd_mfma, g, dim3(256), 0, s, x, w, bias, y, C, H, W, K, N);
    return check_launch("convT2d_fwd_mfma");
  }
  const int kt = pick(K, 4, 2, 1);
  dim3 grid((unsigned)cdiv(S, 256), K / kt, N);
  if (kt == 4) hipLaunchKernelGGL(k_convT2d_fwd<4>, grid, dim3(256), 0, s, x, w, bias, y, C, H, W, K);
  else if (kt == 2) hipLaunchKernelGGL(k_convT2d_fwd<2>, grid, dim3(256), 0, s, x, w, bias, y, C, H, W, K);
  else hipLaunchKernelGGL(k_convT2d_fwd<1>, grid, dim3(256), 0, s, x, w, bias, y, C, H, W, K);
  return check_launch("convT2d_fwd");
}

int nc_convT2d_k2s2_dgrad(const float* dy, const float* w, float* dx, int N, int C, int H, int W, int K, void* ws, size_t ws_bytes, void* stream) {
  if (!dy || !w || !dx) { set_error("convT2d_dgrad: null pointer"); return NC_ERR_ARG; }
  if (int e = convT2d_check("convT2d_dgrad", N, C, H, W, K)) return e;
  ConvDims cd;
  if (!sw::raw(sw::FORCE_DIRECT) && C >= 64 && convT2d_as_conv(cd, N, C, H, W, K) && gemm_fwd_supported(cd) &&
      (gemm_ws_bytes(cd) == 0 || (ws && ws_bytes >= gemm_ws_bytes(cd)))) {
    // dx[ci][pos] = sum_(co, t) w[ci][co][t] * dy[co][2 pos + t]  ==  the FORWARD pass of Conv2d(K -> C, k 2, s 2, p 0) on dy with the
    // transposed-conv weight read as [C][K][2][2]
    return conv_fwd_gemm(dy, w, nullptr, dx, cd, ws, ws_bytes, (hipStream_t)stream);
  }
  const long S = (long)H * W;
  const int ct = pick(C, 8, 4, 1);
  dim3 grid((unsigned)cdiv(S, 256), C / ct, N);
  hipStream_t s = (hipStream_t)stream;
  if (ct == 8) hipLaunchKernelGGL(k_convT2d_dgrad<8>, grid, dim3(256), 0, s, dy, w, dx, C, H, W, K);
  else if (ct == 4) hipLaunchKernelGGL(k_convT2d_dgrad<4>, grid, dim3(256), 0, s, dy, w, dx, C, H, W, K);
  else hipLaunchKernelGGL(k_convT2d_dgrad<1>, grid, dim3(256), 0, s, dy, w, dx, C, H, W, K);
  return check_launch("convT2d_dgrad");
}

int nc_convT2d_k2s2_wgrad(const float* x, const float* dy, float* dw, float* dbias, int N, int C, int H, int W, int K, void* ws, size_t ws_bytes,
                          void* stream) {
  if (!x || !dy || !dw) { set_error("convT2d_wgrad: null pointer"); return NC_ERR_ARG; }
  if (int e = convT2d_check("convT2d_wgrad", N, C, H, W, K)) return e;
  hipStream_t s = (hipStream_t)stream;
  ConvDims cd;
  if (!sw::raw(sw::FORCE_DIRECT) && convT2d_as_conv(cd, N, C, H, W, K) && ws && ws_bytes >= gemm_ws_bytes(cd)) {
    // dW_T[ci][co][t] = sum_pos x[ci][pos] * dy[co][2 pos + t]  ==  conv_wgrad(input = dy, grad_output = x)
    if (int e = conv_wgrad_gemm(dy, x, dw, cd, ws, ws_bytes, s)) return e;
  } else if (C % 4 == 0 && K % 4 == 0) {
    hipLaunchKernelGGL((k_convT2d_wgrad<4, 4>), dim3(C / 4, K / 4), dim3(256), 0, s, x, dy, dw, N, C, H, W, K);
  } else {
    hipLaunchKernelGGL((k_convT2d_wgrad<1, 1>), dim3(C, K), dim3(256), 0, s, x, dy, dw, N, C, H, W, K);
  }
  if (int e = check_launch("convT2d_wgrad")) return e;
  if (dbias) return bias_grad(dy, dbias, N, K, 4L * H * W, ws, ws_bytes, s);
  return NC_OK;
}

}  // extern "C"
