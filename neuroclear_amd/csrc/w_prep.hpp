// The bits of a layer's weight preparation, ONE definition for the per-layer kernels (conv_s3x.hip k_absmax_w / k_pack_w_s3x, convt_s3.hip
// k_convT_bound) and the batched pass of the U-Net training step (w_prep.hip): the largest |w'| of a weight tensor as its pack sees it, one
// element of the packed MFMA fragments, and the output bound of a transposed convolution.  Cells come BY VALUE: the per-layer kernels read
// them from memory, the batched pass knows some of them on the host.
#pragma once
#include <hip/hip_runtime.h>

#include "s3_common.hpp"

namespace nc {

// m <- max(m, |w * f| as float bits) over finite values: the element of every form of this maximum
__device__ __forceinline__ void absmax_w_fold(unsigned& m, float w, float f) {
  const unsigned b = __float_as_uint(w * f) & 0x7fffffffu;
  if (b < 0x7f800000u && b > m) m = b;
}
// a block's maximum leaves as one integer atomicMax (h2.hip k_absmax)
__device__ __forceinline__ void absmax_w_out(unsigned m, unsigned* __restrict__ out, unsigned* wm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned q = (unsigned)__shfl_xor((int)m, o);
    m = q > m ? q : m;
  }
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned b = wm[0];
    for (int k = 1; k < 4; ++k) b = wm[k] > b ? wm[k] : b;
    if (b) atomicMax(out, b);
  }
}
// Largest finite |w'| over the elements a block walks: w' = w * 2^(kA - kB) for the input channels of the second scale group (forward layout
// [co][ci][tap]: ci = (i / T3) % C).  `bid` of `nblocks` blocks of 256 threads; the block's maximum leaves as one integer atomicMax (the
// result does not depend on the grid or the order).  wm: 4 words of LDS.
__device__ __forceinline__ void absmax_w_block(const float* __restrict__ w, long n, int T3, int C, int split_c, unsigned cell_a, unsigned cell_b,
                                               unsigned* __restrict__ out, long bid, long nblocks, unsigned* wm) {
  unsigned m = 0;
  const float gf = split_c < C ? h2_group_factor(cell_a, cell_b) : 1.f;
  for (long i = bid * 256 + threadIdx.x; i < n; i += nblocks * 256) {
    const int ci = (int)((i / T3) % C);
    absmax_w_fold(m, w[i], ci >= split_c ? gf : 1.f);
  }
  absmax_w_out(m, out, wm);
}
// The same maximum walked by output-channel ROWS of C * T3 weights in pieces of 2048: inside a row the second scale group is the elements from
// split_c * T3 on, so no element needs a division, and a thread has eight independent coalesced loads in flight.  (A maximum does not depend on
// the order: the cell gets the same bits.)
__device__ __forceinline__ void absmax_w_rows_block(const float* __restrict__ w, long n, int T3, int C, int split_c, unsigned cell_a, unsigned cell_b,
                                                    unsigned* __restrict__ out, int bid, int nblocks, unsigned* wm) {
  unsigned m = 0;
  const float gf = split_c < C ? h2_group_factor(cell_a, cell_b) : 1.f;
  const int row = C * T3, e_split = split_c < C ? split_c * T3 : row;
  const int pieces = (row + 2047) / 2048, items = (int)(n / row) * pieces;
  for (int it = bid; it < items; it += nblocks) {
    const int co = it / pieces, e0 = (it - co * pieces) * 2048 + (int)threadIdx.x;
    const float* __restrict__ p = w + (long)co * row;
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = e0 + k * 256 < row ? p[e0 + k * 256] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) absmax_w_fold(m, v[k], e0 + k * 256 >= e_split ? gf : 1.f);
  }
  absmax_w_out(m, out, wm);
}

// The packed weights of a tap-stream launch (layout: conv_s3x.hip, above k_pack_w_s3x) are 16-byte FRAGMENTS of eight elements:
// element i = ((fr * NT + term) * 64 + lane) * 8 + j with fr = ((cot * 2 + half) * NS + s) * 2 + rb.  The terms of a weight do not depend on
// `term`: a fragment's eight weights are read and split once for all NT of its terms.
// Terms of element j of lane `lane` of fragment fr (all NT of them; zero past the last tap block).  NT = 3: the bf16 terms of w; NT = 2: the
// fp16 terms of w * (group factor) * 2^k, k from the weights' cell `amax`.
template <int NT>
__device__ __forceinline__ void pack_w_s3x_terms(const float* __restrict__ w, long fr, int lane, int j, int NCH, int KS, int NS, long so, long si,
                                                 int flip, unsigned amax, int split_c, unsigned cell_a, unsigned cell_b, unsigned short (&t)[3]) {
  const int T2 = KS * KS, T3 = T2 * KS, NB = NCH * KS;
  long q = fr;
  const int rb = (int)(q & 1); q >>= 1;
  const int s = (int)(q % NS); q /= NS;
  const int half = (int)(q & 1);
  const int cot = (int)(q >> 1);
  const int g = lane >> 4, m = lane & 15;
  const int T = 4 * s + g;
  const int bi = T / T2, tp = T % T2;
  t[0] = t[1] = t[2] = 0;
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
}

// Element i of the packed weights: term `term` of element j of its fragment (the per-layer kernels, one thread per element)
template <int NT>
__device__ __forceinline__ unsigned short pack_w_s3x_elem(const float* __restrict__ w, long i, int NCH, int KS, int NS, long so, long si, int flip,
                                                          unsigned amax, int split_c, unsigned cell_a, unsigned cell_b) {
  const int j = (int)(i & 7);
  long q = i >> 3;
  const int lane = (int)(q & 63); q >>= 6;
  const int term = (int)(q % NT);
  unsigned short t[3];
  pack_w_s3x_terms<NT>(w, q / NT, lane, j, NCH, KS, NS, so, si, flip, amax, split_c, cell_a, cell_b, t);
  return t[term];
}

// The same bits a fragment at a time (the batched pass, w_prep.hip): unit u = fr * 64 + lane; the thread reads the eight weights once and
// writes that lane's 16 bytes of both terms of the fragment (1 KB apart).  wp4: the packed weights as 16-byte units.
__device__ __forceinline__ void pack_w_s3x_frag2(const float* __restrict__ w, long u, int NCH, int KS, int NS, long so, long si, int flip,
                                                 unsigned amax, int split_c, unsigned cell_a, unsigned cell_b, uint4* __restrict__ wp4) {
  const long fr = u >> 6;
  const int lane = (int)(u & 63);
  unsigned short e[8][3];
#pragma unroll
  for (int j = 0; j < 8; ++j) pack_w_s3x_terms<2>(w, fr, lane, j, NCH, KS, NS, so, si, flip, amax, split_c, cell_a, cell_b, e[j]);
#pragma unroll
  for (int term = 0; term < 2; ++term) wp4[(fr * 2 + term) * 64 + lane] = s3_unit(e, term);
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
