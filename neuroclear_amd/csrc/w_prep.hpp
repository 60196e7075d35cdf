// The bits of a layer's weight preparation, ONE definition for the per-layer kernels (conv_s3x.hip k_absmax_w / k_pack_w_s3x, convt_s3.hip
// k_convT_bound) and the batched pass of the U-Net training step (w_prep.hip): the largest |w'| of a weight tensor as its pack sees it, one
// element of the packed MFMA fragments, and the output bound of a transposed convolution.  Cells come BY VALUE: the per-layer kernels read
// them from memory, the batched pass knows some of them on the host.
#pragma once
#include <hip/hip_runtime.h>

#include "s3_common.hpp"

namespace nc {

// Largest finite |w'| over the elements a block walks: w' = w * 2^(kA - kB) for the input channels of the second scale group (forward layout
// [co][ci][tap]: ci = (i / T3) % C).  `bid` of `nblocks` blocks of 256 threads; the block's maximum leaves as one integer atomicMax (the
// result does not depend on the grid or the order).  wm: 4 words of LDS.
__device__ __forceinline__ void absmax_w_block(const float* __restrict__ w, long n, int T3, int C, int split_c, unsigned cell_a, unsigned cell_b,
                                               unsigned* __restrict__ out, long bid, long nblocks, unsigned* wm) {
  unsigned m = 0;
  const float gf = split_c < C ? h2_group_factor(cell_a, cell_b) : 1.f;
  for (long i = bid * 256 + threadIdx.x; i < n; i += nblocks * 256) {
    const int ci = (int)((i / T3) % C);
    const unsigned b = __float_as_uint(w[i] * (ci >= split_c ? gf : 1.f)) & 0x7fffffffu;
    if (b < 0x7f800000u && b > m) m = b;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned q = (unsigned)__shfl_xor((int)m, o);
    m = q > m ? q : m;
  }
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;  // one atomic per block (h2.hip k_absmax)
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned b = wm[0];
    for (int k = 1; k < 4; ++k) b = wm[k] > b ? wm[k] : b;
    if (b) atomicMax(out, b);
  }
}

// Element i of the packed weights of a tap-stream launch (layout: conv_s3x.hip, above k_pack_w_s3x).  NT = 3: the bf16 terms of w; NT = 2: the
// fp16 terms of w * (group factor) * 2^k, k from the weights' cell `amax`.
template <int NT>
__device__ __forceinline__ unsigned short pack_w_s3x_elem(const float* __restrict__ w, long i, int NCH, int KS, int NS, long so, long si, int flip,
                                                          unsigned amax, int split_c, unsigned cell_a, unsigned cell_b) {
  const int T2 = KS * KS, T3 = T2 * KS, NB = NCH * KS;
  const int j = (int)(i & 7);
  long q = i >> 3;
  const int lane = (int)(q & 63); q >>= 6;
  const int f = (int)(q % (2 * NT)); q /= 2 * NT;
  const int s = (int)(q % NS); q /= NS;
  const int half = (int)(q & 1);
  const int cot = (int)(q >> 1);
  const int rb = f / NT, term = f % NT;
  const int g = lane >> 4, m = lane & 15;
  const int T = 4 * s + g;
  const int bi = T / T2, tp = T % T2;
  unsigned short t[3] = {0, 0, 0};
  if (bi < NB) {
    const int chunk = bi / KS, dz = bi % KS;
#ifdef NC_S3X_B128
    const int jj = j;  // (experiment: one 16-byte read per B fragment, natural channel order)
#else
    const int jj = (g & 1) ? ((j + 4) & 7) : j;
#endif
    const long co = cot * 64 + half * 32 + rb * 16 + m, ci = chunk * 8 + jj;
    const int tap = dz * T2 + tp;
    const float v = w[co * so + ci * si + (flip ? T3 - 1 - tap : tap)];
    if constexpr (NT == 3) s3_split(v, t);
    else h2_split(v * (ci >= split_c ? h2_group_factor(cell_a, cell_b) : 1.f) * h2_scale(amax), t);
  }
  return t[term];
}

// The bound of |y| of ConvTranspose3d(k 2, s 2) (convt_s3.hip, above k_convT_bound): block `bid` takes 64 (output channel, tap) columns,
// 4 slices of the input channels; cell <- atomicMax of the float bits.  part: 4 x 64 floats of LDS, red: 64.
__device__ __forceinline__ void convT_bound_block(const float* __restrict__ w, const float* __restrict__ bias, int C, int K, float in_bound,
                                                  unsigned* __restrict__ cell, int bid, float (*part)[64], float* red) {
  const int col = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int kq = bid * 64 + col;  // one (output channel, tap) column: coalesced over the columns
  float sabs = 0.f;
  if (kq < K * 8) {
#pragma unroll 8
    for (int ci = sl; ci < C; ci += 4) sabs += fabsf(w[(long)ci * K * 8 + kq]);
  }
  part[sl][col] = sabs;
  __syncthreads();
  if (sl == 0) {
    const float t = (part[0][col] + part[1][col]) + (part[2][col] + part[3][col]);
    red[col] = kq < K * 8 ? t * in_bound + (bias ? fabsf(bias[kq >> 3]) : 0.f) : 0.f;
  }
  __syncthreads();
  for (int o = 32; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x + o] > red[threadIdx.x] ? red[threadIdx.x + o] : red[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(cell, __float_as_uint(red[0] * 1.001f) & 0x7fffffffu);  // (the cell was zeroed by the caller)
}

}  // namespace nc
