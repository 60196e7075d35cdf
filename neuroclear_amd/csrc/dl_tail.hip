// deep_linear_gen (reference models/networks.py:893-917): the WEIGHT-SPACE steps of its collapsed forms -- the tail scratch, the kernels that
// compose and contract small tensors of weights, and the nc::dl_* wrappers that launch them (declared in common.hpp).  One set for the fp32
// entry points (gen_nets.hip, which plans the forms and runs the convolutions between these steps), the position-typed form (dl_typed.hip)
// and the 16-bit path (gen_nets_lp.hip).
#include "common.hpp"

using namespace nc;

namespace {

// ---- the collapsed tail ----------------------------------------------------------------------------------------------------------------
// Layers 2 .. 5 (3^3 64 -> 64, then 1 x 1: 64 -> 32 -> 16 -> 1; reference networks.py:902-911) have no bias and nothing between them, and the
// 1 x 1 layers need no padding, so with  a = W5 W4 (1 x 32),  e = a W3 (1 x 64)  and  E[c][t] = sum_k e[k] W2[k][c][t]:
//     y = E (*) act1                                   ONE 64 -> 1 convolution, 3^3, padding 1 -- exact at the borders too: the only padded
//                                                      tensor of the four layers is act1 itself
//     dL/dact1 = flip(E) (*) dy                        a 1 -> 64 convolution of the one-channel dy
//     q[c][t]  = sum_v dy[v] act1[c][v + t - 1]        64 x 27 numbers: a weight gradient with ONE "output" channel
//     dW2[k][c][t] = e[k] q[c][t];   r = sum_{c,t} W2[.][c][t] q[c][t]  (= sum_v dy[v] act2[.][v]);   dW3 = a^T r^T;   s = W3 r;
//     dW4 = W5^T s^T;   dW5 = (W4 s)^T
// -- the same output and the same six parameter gradients as the layer-by-layer evaluation (every product of the chain rule is there, the
// rank-one factors are simply never expanded over the voxels), at 2 x 27 x 64 instead of 2 x (27 x 64 x 64 + 64 x 32 + 32 x 16 + 16) MACs per
// voxel and direction, and act2 .. act4 are neither written nor read.  The weight-space products run in fp64.  Numerically this is at least
// as close to the exact result as the fp32 chain (tests/test_gpu_nets.py: against the fp64 oracle, and against the layered path).
// nc_set_dl_collapse(0) / NC_DL_COLLAPSE=0: the layered evaluation.  The forward records its choice in `kept` (bit 31): the backward of a
// collapsed forward is collapsed whatever the switch says by then (act2 .. act4 do not exist).
struct LTail {  // byte offsets into the tail scratch
  static constexpr size_t a = 0, e = 32 * 8, r = e + 64 * 8, E = r + 64 * 8, Ef = E + 1728 * 4, q = Ef + 1728 * 4, P = q + 1728 * 4 + 256,
                          Wf = P + (size_t)64 * 32 * 125 * 4 + 256, bytes = Wf + (size_t)64 * 32 * 125 * 4 + 256;
};

// ---- layer 1's weight gradient from the rank structure of its dY ---------------------------------------------------------------------------
// With the tail collapsed, dL/dact1 = g1 is 64 channels made from ONE: g1[k][v] = sum_a E[k][a] dy[v - (a - 1)] on the volume (27 shifts a).
// Write Dsh[a][v] = dy[v - (a - 1)] for v inside the volume (27 channels, padded to 32): g1 = E . Dsh, and the 5^3 layer's weight gradient
//     dW1[k][c][t] = sum_v g1[k][v] act0[c][v + t - 2] = sum_a E[k][a] P[a][c][t],   P[a][c][t] = sum_v Dsh[a][v] act0[c][v + t - 2]
// -- P is a 5^3 weight gradient between a 32- and a 64-channel tensor: HALF the matrix work of the 64 x 64 one, same kernel (k_wgrad_s3x with
// act0's kept two-term copy in the dY role, which turns P around: Pq[c][a][t'] = P[a][c][124 - t']), then 64 x 64 x 125 x 27 MACs in weight
// space.  Exact: the truncation of g1 to the volume is IN Dsh.  The data gradient of the layer still takes g1 itself.
__global__ void __launch_bounds__(256) k_dl_shift27(const float* __restrict__ dy, float* __restrict__ dsh, int D, int H, int W) {
  const long S = (long)D * H * W;
  const int a = blockIdx.y, n = blockIdx.z;
  float* out = dsh + ((long)n * 32 + a) * S;
  const float* in = dy + (long)n * S;
  const int az = a / 9 - 1, ay = (a / 3) % 3 - 1, ax = a % 3 - 1;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < S; v += (long)gridDim.x * 256) {
    float r = 0.f;
    if (a < 27) {
      const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / ((long)W * H));
      const int sx = x - ax, sy = y - ay, sz = z - az;
      if ((unsigned)sx < (unsigned)W && (unsigned)sy < (unsigned)H && (unsigned)sz < (unsigned)D) r = in[((long)sz * H + sy) * W + sx];
    }
    out[v] = r;
  }
}
// The data gradient of the same layer in the same form (used where the convolution kernel takes 32 input channels: the 16-bit path):
//     dL/dact0[c][u] = sum_{k,t} W1[k][c][t] g1[k][u - t + 2] = sum_{a,s} Wf[c][a][s] Dsh[a][u + s - 2],   Wf[c][a][s] = sum_k W1[k][c][124 - s] E[k][a]
// -- a FORWARD 5^3 convolution 32 -> 64 of Dsh with weights composed here (zero for the five padding shifts).
__global__ void __launch_bounds__(128) k_dl_w1_fold(const float* __restrict__ E, const float* __restrict__ w1, float* __restrict__ wf) {
  const int c = blockIdx.x, a = blockIdx.y, sidx = threadIdx.x;
  if (sidx >= 125) return;
  double v = 0.0;
  if (a < 27)
    for (int k = 0; k < 64; ++k) v += (double)w1[((long)k * 64 + c) * 125 + 124 - sidx] * (double)E[k * 27 + a];
  wf[((long)c * 32 + a) * 125 + sidx] = (float)v;
}
// ---- the forward without act1 ---------------------------------------------------------------------------------------------------------------
// Once the backward takes q from P, act1 is wanted by ONE consumer: y = E (*) act1.  With F_t[c][s] = sum_c' E[c'][t] W1[c'][c][s] (27 kernels
// 64 -> 1, 5^3):   y[v] = sum_t [v + t - 1 inside the volume] Z_t[v + t - 1],   Z_t = F_t (*) act0  on the volume
// -- a 5^3 convolution 64 -> 27 (padded to 32: k_conv_s3x K32, half the matrix work of 64 -> 64) and a 27-term shifted sum; the bracket IS
// the zero padding of act1.  act1 is never written; the backward (rank forms above) does not miss it.
__global__ void __launch_bounds__(128) k_dl_fold_fwd(const float* __restrict__ E, const float* __restrict__ w1, float* __restrict__ F) {
  const int t = blockIdx.x, c = blockIdx.y, sidx = threadIdx.x;
  if (sidx >= 125) return;
  double v = 0.0;
  if (t < 27)
    for (int cp = 0; cp < 64; ++cp) v += (double)E[cp * 27 + t] * (double)w1[((long)cp * 64 + c) * 125 + sidx];
  F[((long)t * 64 + c) * 125 + sidx] = (float)v;
}
__global__ void __launch_bounds__(256) k_dl_combine27(const float* __restrict__ Z, float* __restrict__ y, int D, int H, int W, int zch) {
  const long S = (long)D * H * W;
  const int n = blockIdx.y;
  const float* z = Z + (long)n * zch * S;  // (zch: channels per sample of the Z tensor, 32 or 64; the first 27 are read)
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < S; v += (long)gridDim.x * 256) {
    const int x = (int)(v % W), yy = (int)((v / W) % H), zz = (int)(v / ((long)W * H));
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < 27; ++t) {
      const int dz = t / 9 - 1, dy = (t / 3) % 3 - 1, dx = t % 3 - 1;
      if ((unsigned)(x + dx) < (unsigned)W && (unsigned)(yy + dy) < (unsigned)H && (unsigned)(zz + dz) < (unsigned)D)
        acc += z[(long)t * S + v + ((long)dz * H + dy) * W + dx];
    }
    y[(long)n * S + v] = acc;
  }
}

// q itself is a contraction of the same P: q[c'][t] = sum_{c,s} W1[c'][c][s] P[t][c][s] (act1 = W1 (*) act0, and the shift a = t of dy IS the
// mask "v + t - 1 inside the volume") -- no pass over act1.  Written tap-flipped, as k_dl_tail_w2 reads it.  Block (c', t), fixed-order tree.
__global__ void __launch_bounds__(256) k_dl_q_from_p(const float* __restrict__ w1, const float* __restrict__ Pq, float* __restrict__ qf) {
  __shared__ double red[256];
  const int cp = blockIdx.x, t = blockIdx.y, th = threadIdx.x;
  double v = 0.0;
  for (int i = th; i < 64 * 125; i += 256) {
    const int c = i / 125, sidx = i - c * 125;
    v += (double)w1[((long)cp * 64 + c) * 125 + sidx] * (double)Pq[((long)c * 32 + t) * 125 + 124 - sidx];
  }
  red[th] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (th < o) red[th] += red[th + o];
    __syncthreads();
  }
  if (th == 0) qf[cp * 27 + 26 - t] = (float)red[0];
}
// dW1[k][c][t] = sum_a E[k][a] Pq[c][a][124 - t]
__global__ void __launch_bounds__(128) k_dl_w1_contract(const float* __restrict__ E, const float* __restrict__ Pq, float* __restrict__ dw1) {
  const int k = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
  if (t >= 125) return;
  double v = 0.0;
#pragma unroll
  for (int a = 0; a < 27; ++a) v += (double)E[k * 27 + a] * (double)Pq[((long)c * 32 + a) * 125 + 124 - t];
  dw1[((long)k * 64 + c) * 125 + t] = (float)v;
}

// (8 workgroups, each derives a and e for itself and 216 of E's 1728 entries; loops unrolled so that the loads of a sum are in flight together)
__global__ void __launch_bounds__(256) k_dl_compose(const float* __restrict__ w2, const float* __restrict__ w3, const float* __restrict__ w4,
                                                    const float* __restrict__ w5, char* __restrict__ tail) {
  __shared__ double sa[32], se[64];
  const int t = threadIdx.x;
  if (t < 32) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) v += (double)w5[i] * (double)w4[i * 32 + t];
    sa[t] = v;
    if (blockIdx.x == 0) ((double*)(tail + LTail::a))[t] = v;
  }
  __syncthreads();
  if (t < 64) {
    double v = 0.0;
#pragma unroll
    for (int b = 0; b < 32; ++b) v += sa[b] * (double)w3[b * 64 + t];
    se[t] = v;
    if (blockIdx.x == 0) ((double*)(tail + LTail::e))[t] = v;
  }
  __syncthreads();
  if (t < 216) {
    const int i = blockIdx.x * 216 + t;  // i = c * 27 + tap
    double v = 0.0;
#pragma unroll 16
    for (int k = 0; k < 64; ++k) v += se[k] * (double)w2[(long)k * 1728 + i];
    const int c = i / 27, tap = i - c * 27;
    ((float*)(tail + LTail::E))[i] = (float)v;
    ((float*)(tail + LTail::Ef))[c * 27 + 26 - tap] = (float)v;
  }
}

// block k: dW2[k][.][.] and r[k].  qf = the weight gradient of the SWAPPED problem (x := dy, dY := act1): qf[c][t] = q[c][26 - t]
__global__ void __launch_bounds__(256) k_dl_tail_w2(const float* __restrict__ w2, char* __restrict__ tail, float* __restrict__ dw2) {
  __shared__ double red[256];
  const int k = blockIdx.x, t = threadIdx.x;
  const float* qf = (const float*)(tail + LTail::q);
  const double ek = ((const double*)(tail + LTail::e))[k];
  double part = 0.0;
  for (int i = t; i < 1728; i += 256) {
    const int c = i / 27, tap = i - c * 27;
    const double q = (double)qf[c * 27 + 26 - tap];
    dw2[(long)k * 1728 + i] = (float)(ek * q);
    part += (double)w2[(long)k * 1728 + i] * q;
  }
  red[t] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) ((double*)(tail + LTail::r))[k] = red[0];
}

__global__ void __launch_bounds__(256) k_dl_tail_w345(const float* __restrict__ w3, const float* __restrict__ w4, const float* __restrict__ w5,
                                                      const char* __restrict__ tail, float* __restrict__ dw3, float* __restrict__ dw4,
                                                      float* __restrict__ dw5) {
  __shared__ double ss[32];
  const int t = threadIdx.x;
  const double* a = (const double*)(tail + LTail::a);
  const double* r = (const double*)(tail + LTail::r);
  for (int i = t; i < 32 * 64; i += 256) dw3[i] = (float)(a[i / 64] * r[i % 64]);
  if (t < 32) {
    double v = 0.0;
    for (int c = 0; c < 64; ++c) v += (double)w3[t * 64 + c] * r[c];
    ss[t] = v;
  }
  __syncthreads();
  for (int i = t; i < 16 * 32; i += 256) dw4[i] = (float)((double)w5[i / 32] * ss[i % 32]);
  if (t < 16) {
    double v = 0.0;
    for (int b = 0; b < 32; ++b) v += (double)w4[t * 32 + b] * ss[b];
    dw5[t] = (float)v;
  }
}

}  // namespace

namespace nc {
size_t dl_tail_bytes() { return LTail::bytes; }
const float* dl_tail_E(const char* tail) { return (const float*)(tail + LTail::E); }
const float* dl_tail_Ef(const char* tail) { return (const float*)(tail + LTail::Ef); }
float* dl_tail_q(char* tail) { return (float*)(tail + LTail::q); }
int dl_tail_compose(const float* w2, const float* w3, const float* w4, const float* w5, char* tail, hipStream_t s) {
  hipLaunchKernelGGL(k_dl_compose, dim3(8), dim3(256), 0, s, w2, w3, w4, w5, tail);
  return check_launch("deep_linear: compose");
}
float* dl_tail_P(char* tail) { return (float*)(tail + LTail::P); }
int dl_shift27(const float* dy, float* dsh, int N, int D, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(k_dl_shift27, dim3(256, 32, (unsigned)N), dim3(256), 0, s, dy, dsh, D, H, W);
  return check_launch("deep_linear_bwd: shifted copies of dy");
}
const float* dl_w1_fold(char* tail, const float* w1, hipStream_t s) {  // composes Wf into the tail scratch and returns it (NULL: launch failed)
  hipLaunchKernelGGL(k_dl_w1_fold, dim3(64, 32), dim3(128), 0, s, (const float*)(tail + LTail::E), w1, (float*)(tail + LTail::Wf));
  return check_launch("deep_linear_bwd: composed data-gradient weights") ? nullptr : (const float*)(tail + LTail::Wf);
}
// the forward without act1: F's 32 rows [32][64][125] (27 kernels, five rows zero) in the Wf region (free in a forward; NULL: launch failed)
const float* dl_fold_fwd(char* tail, const float* w1, hipStream_t s) {
  hipLaunchKernelGGL(k_dl_fold_fwd, dim3(32, 64), dim3(128), 0, s, (const float*)(tail + LTail::E), w1, (float*)(tail + LTail::Wf));
  return check_launch("deep_linear: composed forward weights") ? nullptr : (const float*)(tail + LTail::Wf);
}
// ... for the 16-bit path: F as a [64][64][125] tensor (rows 27 .. 63 zero) in the tail scratch (the P and Wf regions, adjacent, 2 MB + 512 B;
// free in a forward), and the shifted sum over a Z tensor of `zch` channels per sample
const float* dl_fold_fwd64(char* tail, const float* w1, hipStream_t s) {
  static_assert(LTail::Wf == LTail::P + (size_t)64 * 32 * 125 * 4 + 256, "P and Wf adjacent");
  float* F = (float*)(tail + LTail::P);
  if (hipMemsetAsync(F + (size_t)32 * 64 * 125, 0, (size_t)32 * 64 * 125 * 4, s) != hipSuccess) return nullptr;
  hipLaunchKernelGGL(k_dl_fold_fwd, dim3(32, 64), dim3(128), 0, s, (const float*)(tail + LTail::E), w1, F);
  return check_launch("deep_linear_fwd: composed forward weights") ? nullptr : F;
}
int dl_combine27(const float* Z, float* y, int N, int D, int H, int W, int zch, hipStream_t s) {
  hipLaunchKernelGGL(k_dl_combine27, dim3(1024, (unsigned)N), dim3(256), 0, s, Z, y, D, H, W, zch);
  return check_launch("deep_linear_fwd: shifted sum");
}
int dl_q_from_p(char* tail, const float* w1, hipStream_t s) {
  hipLaunchKernelGGL(k_dl_q_from_p, dim3(64, 27), dim3(256), 0, s, w1, (const float*)(tail + LTail::P), (float*)(tail + LTail::q));
  return check_launch("deep_linear_bwd: q");
}
int dl_w1_contract(const char* tail, float* dw1, hipStream_t s) {
  hipLaunchKernelGGL(k_dl_w1_contract, dim3(64, 64), dim3(128), 0, s, (const float*)(tail + LTail::E), (const float*)(tail + LTail::P), dw1);
  return check_launch("deep_linear_bwd: dW1");
}
int dl_tail_grads(const float* w2, const float* w3, const float* w4, const float* w5, char* tail, float* dw2, float* dw3, float* dw4, float* dw5,
                  hipStream_t s) {
  hipLaunchKernelGGL(k_dl_tail_w2, dim3(64), dim3(256), 0, s, w2, tail, dw2);
  hipLaunchKernelGGL(k_dl_tail_w345, dim3(1), dim3(256), 0, s, w3, w4, w5, (const char*)tail, dw3, dw4, dw5);
  return check_launch("deep_linear: tail gradients");
}

}  // namespace nc
