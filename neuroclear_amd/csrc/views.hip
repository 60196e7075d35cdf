// Training progress views: util.tensor2im (util/util.py:26-39) and what Visualizer.display_current_results shows of one visual
// (util/visualizer.py:138-144, 171-173): three centre slices and three maximum projections of sample 0, channel 0 as uint8, plus the
// 256-bin histogram of that sample.  Integer results only: the uint8 conversion is monotone, so every maximum is taken on the
// converted values, and the only atomics are integer adds -- the same bytes on every run and every stream.  The volume is read three
// times (rows, and the two column directions); at 108^3 that is 15 MB out of the L2 / MALL, microseconds next to a training step.
#include "common.hpp"

namespace nc {

// np.clip(x, 0, 1) * top, np.clip(., 0, top), astype: fp32 throughout, truncating cast.  NaN is outside the contract (fmaxf drops it: 0).
__device__ __forceinline__ unsigned quant(float x, float top) {
  float v = fminf(fmaxf(x, 0.f), 1.f) * top;
  v = fminf(fmaxf(v, 0.f), top);
  return (unsigned)v;
}
__device__ __forceinline__ unsigned q8(float x) { return quant(x, 255.0f); }

// vec: x is 16-byte aligned and out 4 (uint8) / 8 (uint16) byte aligned -> four elements per lane and one store; the tail and the
// unaligned case go element by element.
template <typename T>
__global__ void k_tensor2im(const float* __restrict__ x, T* __restrict__ out, long n, int vec) {
  const float top = sizeof(T) == 1 ? 255.0f : 65535.0f;
  const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x, step = (long)gridDim.x * blockDim.x;
  const long n4 = vec ? n / 4 : 0;
  for (long i = t0; i < n4; i += step) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    const unsigned a = quant(v.x, top), b = quant(v.y, top), c = quant(v.z, top), d = quant(v.w, top);
    if (sizeof(T) == 1)
      reinterpret_cast<uint32_t*>(out)[i] = a | b << 8 | c << 16 | d << 24;
    else
      reinterpret_cast<uint2*>(out)[i] = make_uint2(a | b << 16, c | d << 16);
  }
  for (long i = n4 * 4 + t0; i < n; i += step) out[i] = (T)quant(x[i], top);
}

struct ViewOffsets {
  long sxy, sxz, syz, mxy, mxz, myz, total;
};
static ViewOffsets view_offsets(long D, long H, long W) {
  ViewOffsets o;
  o.sxy = 0;
  o.sxz = o.sxy + H * W;
  o.syz = o.sxz + D * W;
  o.mxy = o.syz + D * H;
  o.mxz = o.mxy + H * W;
  o.myz = o.mxz + D * W;
  o.total = o.myz + D * H;
  return o;
}

// One wave per row (d, h) of W voxels, rows dealt round-robin to a bounded grid.  Per row: the maximum over w (mip_yz), the three
// slices where the row crosses them, and the histogram -- counted in LDS, flushed once per block with integer adds.
__global__ void __launch_bounds__(256) k_view_rows(const float* __restrict__ vol, int D, int H, int W, int index, uint8_t* __restrict__ sxy,
                                                    uint8_t* __restrict__ sxz, uint8_t* __restrict__ syz, uint8_t* __restrict__ myz,
                                                    uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (hist) {
    bins[threadIdx.x] = 0;
    __syncthreads();
  }
  const long rows = (long)D * H;
  for (long r = blockIdx.x * 4 + wave; r < rows; r += gridDim.x * 4) {
    const int d = (int)(r / H), h = (int)(r - (long)d * H);
    const float* p = vol + (size_t)r * W;
    unsigned best = 0;
    for (int w = lane; w < W; w += 64) {
      const unsigned q = q8(p[w]);
      best = max(best, q);
      if (hist) atomicAdd(&bins[q], 1u);
      if (sxy) {
        if (d == index) sxy[(size_t)h * W + w] = (uint8_t)q;
        if (h == index) sxz[(size_t)d * W + w] = (uint8_t)q;
        if (w == index) syz[r] = (uint8_t)q;
      }
    }
    if (myz) {
      for (int off = 32; off; off >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, off, 64));
      if (lane == 0) myz[r] = (uint8_t)best;
    }
  }
  if (hist) {
    __syncthreads();
    const uint32_t c = bins[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], c);
  }
}

// One lane per output pixel of mip_xy (maximum over d) and mip_xz (maximum over h); neighbouring lanes read neighbouring w.
__global__ void __launch_bounds__(256) k_view_cols(const float* __restrict__ vol, int D, int H, int W, uint8_t* __restrict__ mxy,
                                                    uint8_t* __restrict__ mxz) {
  const long nxy = (long)H * W, nxz = (long)D * W;
  const size_t HW = (size_t)H * W;
  for (long i = blockIdx.x * blockDim.x + threadIdx.x; i < nxy + nxz; i += gridDim.x * blockDim.x) {
    unsigned best = 0;
    if (i < nxy) {
      const float* p = vol + i;  // (h, w) at d = 0
      for (int d = 0; d < D; ++d) best = max(best, q8(p[d * HW]));
      mxy[i] = (uint8_t)best;
    } else {
      const long j = i - nxy, d = j / W, w = j - d * W;
      const float* p = vol + d * HW + w;
      for (int h = 0; h < H; ++h) best = max(best, q8(p[(size_t)h * W]));
      mxz[j] = (uint8_t)best;
    }
  }
}

}  // namespace nc

using namespace nc;

extern "C" {

int nc_tensor2im(const float* x, void* out, int out_is_u16, long n, void* stream) {
  if (!x || !out) { set_error("tensor2im: null pointer"); return NC_ERR_ARG; }
  if (out_is_u16 != 0 && out_is_u16 != 1) { set_error("tensor2im: out_is_u16 must be 0 or 1"); return NC_ERR_ARG; }
  if (n < 1) { set_error("tensor2im: empty input"); return NC_ERR_SHAPE; }
  const int vec = (uintptr_t)x % 16 == 0 && (uintptr_t)out % (out_is_u16 ? 8 : 4) == 0;
  long nb = cdiv(cdiv(n, 4), 256);
  if (nb > 2048) nb = 2048;
  if (out_is_u16)
    hipLaunchKernelGGL(k_tensor2im<uint16_t>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, (uint16_t*)out, n, vec);
  else
    hipLaunchKernelGGL(k_tensor2im<uint8_t>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, (uint8_t*)out, n, vec);
  return check_launch("tensor2im");
}

size_t nc_progress_views_bytes(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1) return 0;
  return (size_t)view_offsets(D, H, W).total;
}

int nc_progress_views(const float* vol, int N, int C, int D, int H, int W, int index, uint8_t* views, uint32_t* hist256, void* stream) {
  if (!vol) { set_error("progress_views: null volume"); return NC_ERR_ARG; }
  if (N < 1 || C < 1 || D < 1 || H < 1 || W < 1) {
    set_error("progress_views: bad shape [%d,%d,%d,%d,%d]", N, C, D, H, W);
    return NC_ERR_SHAPE;
  }
  const int lim = D < H ? (D < W ? D : W) : (H < W ? H : W);
  if (index < 0 || index >= lim) {
    set_error("progress_views: index %d outside [0, %d) of a %d x %d x %d volume", index, lim, D, H, W);
    return NC_ERR_SHAPE;
  }
  if ((long)D * H * W >= (1L << 31)) { set_error("progress_views: %d x %d x %d voxels do not fit 31 bits", D, H, W); return NC_ERR_SHAPE; }
  if (!views && !hist256) return NC_OK;
  hipStream_t s = (hipStream_t)stream;
  const ViewOffsets o = view_offsets(D, H, W);
  if (hist256) {
    const hipError_t e = hipMemsetAsync(hist256, 0, 256 * sizeof(uint32_t), s);
    if (e != hipSuccess) { set_error("progress_views: hipMemsetAsync: %s", hipGetErrorString(e)); return NC_ERR_HIP; }
  }
  long nb = cdiv((long)D * H, 4);
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(k_view_rows, dim3((unsigned)nb), dim3(256), 0, s, vol, D, H, W, index, views ? views + o.sxy : nullptr,
                     views ? views + o.sxz : nullptr, views ? views + o.syz : nullptr, views ? views + o.myz : nullptr, hist256);
  if (views) {
    nb = cdiv((long)H * W + (long)D * W, 256);
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(k_view_cols, dim3((unsigned)nb), dim3(256), 0, s, vol, D, H, W, views + o.mxy, views + o.mxz);
  }
  return check_launch("progress_views");
}

}  // extern "C"
