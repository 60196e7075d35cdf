// The streaming kernels of the ResNet generators (reference models/networks.py:724-837, `--netG resnet_6blocks | resnet_9blocks`): ReflectionPad2d
// forward and backward, the tail of a ResnetBlock (skip + InstanceNorm of the second convolution), the plain residual add of the batch-norm
// blocks, and the Dropout(0.5) mask multiply.  The convolutions are in conv2d_k3.hip (reflect-padded 3 x 3 on the image-tiled kernel) and behind
// nc_conv_* (7 x 7, stride-2 3 x 3, the transposed convolutions as data gradients); the entry points that tie a reflect-padded layer together
// are in api.hip.
//
// Summation order of the fold (reflect_pad_bwd; the tests' fp32 yardstick follows it).  One padded axis of n pixels and pad p < n sends up to
// three padded positions to pixel i: the pixel's own, i + p; the mirror on the low side, p - i, for 1 <= i <= p; the mirror on the high side,
// 2 (n - 1) - i + p, for n - 1 - p <= i <= n - 2.  An output element is ONE fp32 accumulator that starts at zero and adds, rows outermost in the
// order (own, low mirror, high mirror) and inside each row the columns in the order (own, low mirror, high mirror): at most nine terms, a
// gather with a fixed order, no atomics, run-to-run identical bits.

#include "common.hpp"

namespace nc {
namespace {

unsigned stream_grid(long n) {
  const long b = cdiv(n, 256);
  return (unsigned)(b < 1 ? 1 : b > (1L << 20) ? (1L << 20) : b);
}

__device__ __forceinline__ int mirror(int i, int n) { return i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i; }

__global__ void __launch_bounds__(256) k_reflect_pad_fwd(const float* __restrict__ x, float* __restrict__ y, long total, int H, int W, int p) {
  const int Hp = H + 2 * p, Wp = W + 2 * p;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % Wp);
    const long q = i / Wp;
    const int r = (int)(q % Hp);
    const long nc = q / Hp;
    y[i] = x[(nc * H + mirror(r - p, H)) * W + mirror(c - p, W)];
  }
}

// the up-to-three padded positions of pixel i (see the header comment); -1: no such term
__device__ __forceinline__ void fold_sources(int i, int n, int p, int src[3]) {
  src[0] = i + p;
  src[1] = (i >= 1 && i <= p) ? p - i : -1;
  src[2] = (i >= n - 1 - p && i <= n - 2) ? 2 * (n - 1) - i + p : -1;
}

__global__ void __launch_bounds__(256) k_reflect_pad_bwd(const float* __restrict__ g, float* __restrict__ dx, long total, int H, int W, int p) {
  const int Hp = H + 2 * p, Wp = W + 2 * p;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % W);
    const long q = i / W;
    const int r = (int)(q % H);
    const long nc = q / H;
    int rs[3], cs[3];
    fold_sources(r, H, p, rs);
    fold_sources(c, W, p, cs);
    const float* gp = g + nc * Hp * Wp;
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        if (rs[a] >= 0 && cs[b] >= 0) acc += gp[(long)rs[a] * Wp + cs[b]];
    dx[i] = acc;
  }
}

// y = skip + (x - mean) * rstd, one (n, c) plane per blockIdx.y
__global__ void __launch_bounds__(256) k_in_res_fwd(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                    const float* __restrict__ skip, float* __restrict__ y, long S) {
  const int inst = blockIdx.y;
  const float m = mean[inst], r = rstd[inst];
  const float* px = x + (long)inst * S;
  const float* ps = skip + (long)inst * S;
  float* o = y + (long)inst * S;
  if ((S & 3) == 0 && (((uintptr_t)x | (uintptr_t)skip | (uintptr_t)y) & 15) == 0) {
    const float4* x4 = reinterpret_cast<const float4*>(px);
    const float4* s4 = reinterpret_cast<const float4*>(ps);
    float4* o4 = reinterpret_cast<float4*>(o);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < S / 4; i += (long)gridDim.x * 256) {
      const float4 v = x4[i], k = s4[i];
      float4 t;
      t.x = k.x + (v.x - m) * r; t.y = k.y + (v.y - m) * r; t.z = k.z + (v.z - m) * r; t.w = k.w + (v.w - m) * r;
      o4[i] = t;
    }
  } else {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < S; i += (long)gridDim.x * 256) o[i] = ps[i] + (px[i] - m) * r;
  }
}

__global__ void __launch_bounds__(256) k_residual_add(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = a[i] + b[i];
}

// y = mask ? scale * x : 0 (mask: one byte per element, 0 or 1)
__global__ void __launch_bounds__(256) k_dropout_mul(const float* __restrict__ x, const unsigned char* __restrict__ mask, float scale,
                                                     float* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = mask[i] ? x[i] * scale : 0.f;
}

bool pad_shape_ok(long NC, int H, int W, int p) {
  return NC >= 1 && p >= 1 && H > p && W > p && (long)(H + 2 * p) * (W + 2 * p) < (1L << 31);
}

}  // namespace

int reflect_pad_fwd(const float* x, float* y, long NC, int H, int W, int p, hipStream_t s) {
  const long total = NC * (H + 2 * p) * (W + 2 * p);
  hipLaunchKernelGGL(k_reflect_pad_fwd, dim3(stream_grid(total)), dim3(256), 0, s, x, y, total, H, W, p);
  return check_launch("reflect_pad2d_fwd");
}

int reflect_pad_bwd(const float* g, float* dx, long NC, int H, int W, int p, hipStream_t s) {
  const long total = NC * H * W;
  hipLaunchKernelGGL(k_reflect_pad_bwd, dim3(stream_grid(total)), dim3(256), 0, s, g, dx, total, H, W, p);
  return check_launch("reflect_pad2d_bwd");
}

}  // namespace nc

using namespace nc;

extern "C" {

int nc_reflect_pad2d_fwd(const float* x, float* y, int NC, int H, int W, int p, void* stream) {
  if (!x || !y) { set_error("reflect_pad2d_fwd: null pointer"); return NC_ERR_ARG; }
  if (!pad_shape_ok(NC, H, W, p) || (p != 1 && p != 3)) { set_error("reflect_pad2d_fwd: bad shape NC=%d H=%d W=%d p=%d (p 1 or 3, H and W above p)", NC, H, W, p); return NC_ERR_SHAPE; }
  return reflect_pad_fwd(x, y, NC, H, W, p, (hipStream_t)stream);
}

int nc_reflect_pad2d_bwd(const float* dy, float* dx, int NC, int H, int W, int p, void* stream) {
  if (!dy || !dx) { set_error("reflect_pad2d_bwd: null pointer"); return NC_ERR_ARG; }
  if (!pad_shape_ok(NC, H, W, p) || (p != 1 && p != 3)) { set_error("reflect_pad2d_bwd: bad shape NC=%d H=%d W=%d p=%d (p 1 or 3, H and W above p)", NC, H, W, p); return NC_ERR_SHAPE; }
  return reflect_pad_bwd(dy, dx, NC, H, W, p, (hipStream_t)stream);
}

int nc_instnorm_res_fwd(const float* x, const float* mean, const float* rstd, const float* skip, float* y, int NC, long S, void* stream) {
  if (!x || !mean || !rstd || !skip || !y) { set_error("instnorm_res_fwd: null pointer"); return NC_ERR_ARG; }
  if (NC < 1 || S < 1) { set_error("instnorm_res_fwd: bad shape"); return NC_ERR_SHAPE; }
  long bx = cdiv(S, 1024 * 4);
  if (bx > 1024) bx = 1024;
  for (int c0 = 0; c0 < NC; c0 += 65535) {  // blockIdx.y carries the plane
    const int n = NC - c0 < 65535 ? NC - c0 : 65535;
    hipLaunchKernelGGL(k_in_res_fwd, dim3((unsigned)bx, n), dim3(256), 0, (hipStream_t)stream, x + (long)c0 * S, mean + c0, rstd + c0,
                       skip + (long)c0 * S, y + (long)c0 * S, S);
  }
  return check_launch("instnorm_res_fwd");
}

int nc_residual_add(const float* a, const float* b, float* y, long n, void* stream) {
  if (!a || !b || !y) { set_error("residual_add: null pointer"); return NC_ERR_ARG; }
  if (n < 1) { set_error("residual_add: bad shape"); return NC_ERR_SHAPE; }
  hipLaunchKernelGGL(k_residual_add, dim3(stream_grid(n)), dim3(256), 0, (hipStream_t)stream, a, b, y, n);
  return check_launch("residual_add");
}

int nc_dropout_mul(const float* x, const void* mask, float scale, float* y, long n, void* stream) {
  if (!x || !mask || !y) { set_error("dropout_mul: null pointer"); return NC_ERR_ARG; }
  if (n < 1) { set_error("dropout_mul: bad shape"); return NC_ERR_SHAPE; }
  hipLaunchKernelGGL(k_dropout_mul, dim3(stream_grid(n)), dim3(256), 0, (hipStream_t)stream, x, (const unsigned char*)mask, scale, y, n);
  return check_launch("dropout_mul");
}

}  // extern "C"
