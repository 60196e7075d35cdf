// Conv2d(kernel 3, stride 1, padding 1) forward and data gradient of the 2-D generators (reference models/networks.py:413-476 with dimension == 2:
// every 3 x 3 layer of Unet_deconv / Unet_vanilla but the one-channel first one) as ONE image-tiled implicit-GEMM kernel on the fp32 matrix
// cores (v_mfma_f32_32x32x2_f32).
//
// The operand scheme is k_sconv's (conv2d_img.hip): weights packed per (64-channel output tile, channel pair, tap) and streamed through a buffer
// descriptor; the input staged in LDS per channel chunk by LDS-DMA through a per-tile source table; the B operand of an MFMA a plain ds_read_b32
// at (lane base + scalar tap offset); one MFMA chain per output element in the order chunk -> channel pair -> tap, so the bits do not depend on
// the tile shape.  What differs is the tile: k_sconv stages whole image rows (its LDS plan stops applying a little above 500 columns), here a
// workgroup owns a 2-D spatial tile of ONE image -- TH rows x TW columns -- and stages that window with a one-pixel halo, (TH + 2) x (TW + 2)
// per channel, so the LDS need does not depend on the image width.  Pixels of the halo outside the image come from a page of zeros.
// The data gradient is the same kernel walked backwards (DT = -1) on transposed weights: dx[c][i][j] = sum_(k,ty,tx) w[k][c][ty][tx] dy[k][i+1-ty][j+1-tx].
//
// Coverage: D == 1, kd == 1, kh == kw == 3, stride 1, padding 1; reduction side (C forward, K backward) even and >= 16; output side a multiple of
// 64; any H, W, N; and enough tiles to fill the chip (k3_min_workgroups) -- smaller problems, the one-channel first layer and the weight gradient
// stay on the gather GEMM (conv_gemm.hip).

#include "common.hpp"

namespace nc {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// source of every halo lane outside the image: 256 B of zeros in the code object
__device__ __attribute__((aligned(256))) const float g_k3_zero_page[64] = {};

constexpr int kK3LdsCap = 64 * 1024;  // per workgroup: two can share a CU

struct K3Params {
  const float* x;     // input  [B][C][H][W]   (dy for the data gradient)
  const float* wp;    // packed weights [M / 64][C / 2][9][2][32][2]
  const float* bias;  // nullable
  float* y;           // output [B][M][H][W]
  int B, C, M, H, W;  // H x W: the input image (the bounds of the source table)
  int OH, OW, org;    // output image OH x OW; output pixel (oy, ox) sits at input pixel (oy + org, ox + org): H, W, 0 but for the reflect data gradient
  int reflect;        // halo slots one pixel outside the input image: 0 the zero page (Conv2d padding 1), 1 the mirrored pixel (ReflectionPad2d(1))
  int TH, TW;         // tile: TH rows x TW columns, TH * TW == WM * VB * 32
  int ntx, nty;       // tiles per image
  int CK, CS;         // channels per chunk; floats per staged channel image: (TH + 2) * (TW + 2) rounded up to 64
};

template <int DT, int WM, int WN, int VB>
__global__ void __launch_bounds__(WM* WN * 64) k_conv2d_k3(const K3Params p) {
  constexpr int NT = WM * WN * 64, NW = WM * WN, T = 9;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // LDS: [tab: CS ints][buf0: CK * CS][buf1: CK * CS]
  int* const tab = reinterpret_cast<int*>(lds);
  float* const buf0 = lds + p.CS;
  float* const buf1 = buf0 + (long)p.CK * p.CS;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % WM, wn = wave / WM;
  const int li = lane & 31, h = lane >> 5;
  const int per_img = p.ntx * p.nty;
  const int b = blockIdx.x / per_img;
  const int rt = blockIdx.x - b * per_img;
  const int ty0 = (rt / p.ntx) * p.TH, tx0 = (rt % p.ntx) * p.TW;
  const int cot = blockIdx.y * WN + wn;
  const int Wp = p.TW + 2;
  const int used = (p.TH + 2) * Wp;  // floats of a channel image actually staged (<= CS)
  const long Sin = (long)p.H * p.W, Sout = (long)p.OH * p.OW;

  // ---- per-tile source table: slot s of a staged channel image -> element offset inside a channel image, or -1 (zero).  The reflect form
  // differs only in the slots exactly one pixel outside the image: row -1 reads row 1, row H reads row H - 2, the same for the columns, the
  // corners through both (H, W >= 2); slots further out (the overhang of the last tiles) keep the zero page.
  for (int s = tid; s < used; s += NT) {
    const int r = s / Wp, c = s - r * Wp;
    int iy = ty0 + p.org - 1 + r, ix = tx0 + p.org - 1 + c;
    if (p.reflect) {
      iy = iy == -1 ? 1 : iy == p.H ? p.H - 2 : iy;
      ix = ix == -1 ? 1 : ix == p.W ? p.W - 2 : ix;
    }
    const bool ok = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    tab[s] = ok ? iy * p.W + ix : -1;
  }

  // ---- this lane's pixels: base offset into a staged channel image (the window's first tap), and the output address
  int base[VB];
  long oaddr[VB];
#pragma unroll
  for (int v = 0; v < VB; ++v) {
    const int q = (wm * VB + v) * 32 + li;
    const int pr = q / p.TW, pc = q - pr * p.TW;
    const int oy = ty0 + pr, ox = tx0 + pc;
    base[v] = DT > 0 ? pr * Wp + pc : (pr + 2) * Wp + pc + 2;
    oaddr[v] = (oy < p.OH && ox < p.OW) ? ((long)b * p.M + cot * 64) * Sout + (long)oy * p.OW + ox : -1;
  }
  __syncthreads();  // table complete

  const int nchunks = p.C / p.CK;
  auto stage = [&](int chunk, float* bd) {
    const float* xc = p.x + ((long)b * p.C + (long)chunk * p.CK) * Sin;
#pragma unroll 1
    for (int ci = 0; ci < p.CK; ++ci) {
#pragma unroll 1
      for (int s0 = wave * 64; s0 < used; s0 += NW * 64) {
        const int s = s0 + lane;
        const int o = s < used ? tab[s] : -1;
        const float* src = o >= 0 ? xc + (long)ci * Sin + o : g_k3_zero_page;
        nc_dma_lds4(src, nc_lds_addr((bd + (long)ci * p.CS + s0)));
      }
    }
  };

  f32x16 acc[2][VB];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int v = 0; v < VB; ++v)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][v][e] = 0.f;

  // weights: [cot][channel pair][tap][h][32][2]: one float2 per lane per k-step, a scalar offset walks the stream
  const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wp), 0, 0x7fffffff, 0x00020000);
  const int avoff = (h * 32 + li) * 8;  // bytes
  const int kstep_b = 64 * 2 * 4;       // bytes per k-step
  int aptr = (int)((long)cot * (p.C / 2) * T * kstep_b);
  auto wload = [&](int soff) {
    typedef int v2i __attribute__((ext_vector_type(2)));
    const v2i r = __builtin_amdgcn_raw_buffer_load_b64(wrsrc, avoff, soff, 0);
    return make_float2(__int_as_float(r.x), __int_as_float(r.y));
  };

  stage(0, buf0);
  // the weights of channel pair i + 1 are requested while pair i is multiplied (the last pair re-requests itself)
  float2 aw[T], awn[T];
#pragma unroll
  for (int t = 0; t < T; ++t) aw[t] = wload(aptr + t * kstep_b);
  const int npairs_all = p.C / 2;
  int pair_i = 0;
  for (int q = 0; q < nchunks; ++q) {
    float* cur = (q & 1) ? buf1 : buf0;
    float* nxt = (q & 1) ? buf0 : buf1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (q + 1 < nchunks) stage(q + 1, nxt);
#pragma unroll 1
    for (int cp = 0; cp < p.CK / 2; ++cp) {
      const float* cb = cur + (long)(2 * cp + h) * p.CS;
      ++pair_i;
      if (pair_i < npairs_all) aptr += T * kstep_b;
#pragma unroll
      for (int t = 0; t < T; ++t) awn[t] = wload(aptr + t * kstep_b);
#pragma unroll
      for (int ty = 0; ty < 3; ++ty)
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
          const int toff = (ty * Wp + tx) * DT;
          float bv[VB];
#pragma unroll
          for (int v = 0; v < VB; ++v) bv[v] = cb[base[v] + toff];
#pragma unroll
          for (int v = 0; v < VB; ++v) {
            acc[0][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[ty * 3 + tx].x, bv[v], acc[0][v], 0, 0, 0);
            acc[1][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[ty * 3 + tx].y, bv[v], acc[1][v], 0, 0, 0);
          }
        }
#pragma unroll
      for (int t = 0; t < T; ++t) aw[t] = awn[t];
    }
  }

  // ---- epilogue: rows = output channels, lanes = pixels
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    float bvs[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) bvs[e] = p.bias ? p.bias[cot * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * h] : 0.f;
#pragma unroll
    for (int v = 0; v < VB; ++v)
      if (oaddr[v] >= 0) {
        float* yo = p.y + oaddr[v];
#pragma unroll
        for (int e = 0; e < 16; ++e) yo[(long)(a * 32 + (e & 3) + 8 * (e >> 2) + 4 * h) * Sout] = acc[a][v][e] + bvs[e];
      }
  }
}

// A[m][c][t] = w[m * sm + c * sc + t]  ->  wp[cot][c / 2][t][c & 1][m % 32][(m / 32) % 2]
__global__ void __launch_bounds__(256) k_pack_k3(const float* __restrict__ w, float* __restrict__ wp, int C, long sm, long sc, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int a = (int)(i & 1);
  long q = i >> 1;
  const int li = (int)(q & 31); q >>= 5;
  const int h = (int)(q & 1); q >>= 1;
  const int t = (int)(q % 9); q /= 9;
  const int cp = (int)(q % (C / 2));
  const int cot = (int)(q / (C / 2));
  const int m = cot * 64 + a * 32 + li, c = 2 * cp + h;
  wp[i] = w[(long)m * sm + (long)c * sc + t];
}

// tiles: 64 * WN output channels x (WM * VB * 32) pixels.  Every configuration accumulates an output element in the same order.
struct K3Cfg { int WM, WN, VB; };
const K3Cfg kK3Cfgs[] = {{4, 1, 2}, {4, 1, 1}};
constexpr int kK3NumCfgs = (int)(sizeof(kK3Cfgs) / sizeof(kK3Cfgs[0]));

struct K3Plan {
  bool ok;
  int cfg, TH, TW, ntx, nty, CK, CS, lds;
  long wgs;
};

// the plan of ONE tile configuration for a problem with reduction side C, output side M (ok = false: not applicable)
K3Plan k3_plan_one(int ci, int B, int C, int M, int H, int W) {
  K3Plan pl{};
  const K3Cfg& g = kK3Cfgs[ci];
  if (M % (64 * g.WN)) return pl;
  const int npix = g.WM * g.VB * 32;
  pl.cfg = ci;
  pl.TW = 32;                  // column window; the rows follow from the pixel count (8 or 4)
  pl.TH = npix / pl.TW;
  pl.ntx = (int)cdiv(W, pl.TW);
  pl.nty = (int)cdiv(H, pl.TH);
  pl.CS = (int)(cdiv((long)(pl.TH + 2) * (pl.TW + 2), 64) * 64);
  for (int CK : {16, 8, 4, 2}) {
    if (C % CK) continue;
    const long bytes = ((long)pl.CS + 2L * CK * pl.CS) * 4;
    if (bytes > kK3LdsCap) continue;
    pl.CK = CK;
    pl.lds = (int)bytes;
    pl.wgs = (long)B * pl.ntx * pl.nty * (M / (64 * g.WN));
    pl.ok = (long)B * pl.ntx * pl.nty < (1L << 31);
    return pl;
  }
  return pl;
}

// Below this many workgroups of the smallest tile (128 pixels x 64 channels) the problem does not give every one of the 256 CUs a workgroup, and
// a workgroup walks its whole reduction alone where the gather GEMM splits it.  Every shape at or above the rule is measured faster than the
// gather GEMM (profiles/unet2d_k3.txt); shapes below it were not measured on this kernel and stay where they were.
long k3_min_workgroups() { return 256; }

// the heuristic: the 256-pixel tile (twice the operand reuse) once it still gives every CU two workgroups, else the 128-pixel tile
K3Plan k3_plan(int B, int C, int M, int H, int W) {
  const int forced = sw::raw(sw::CONV2D_K3_CFG);
  if (forced >= 0 && forced < kK3NumCfgs) return k3_plan_one(forced, B, C, M, H, W);
  const K3Plan big = k3_plan_one(0, B, C, M, H, W);
  if (big.ok && big.wgs >= 512) return big;
  return k3_plan_one(1, B, C, M, H, W);
}

bool k3_layer_ok(const ConvDims& d) {
  return d.D == 1 && d.kd == 1 && d.kh == 3 && d.kw == 3 && d.sh == 1 && d.sw == 1 && d.ph == 1 && d.pw == 1 &&
         (long)d.N * d.C * d.H * d.W < (1L << 31) && (long)d.N * d.K * d.H * d.W < (1L << 31) && (long)d.C * d.K * 36 < (1L << 31) &&
         (long)d.H * d.W < (1L << 30);
}
bool k3_shape_ok(const ConvDims& d, int red, int out) {
  if (!k3_layer_ok(d) || red % 2 || red < 16 || out % 64) return false;
  const K3Plan small = k3_plan_one(1, d.N, red, out, d.H, d.W);
  return small.ok && small.wgs >= k3_min_workgroups();
}

template <int DT, int WM, int WN, int VB>
int k3_launch_cfg(const K3Plan& pl, const K3Params& p, hipStream_t s) {
  auto kern = k_conv2d_k3<DT, WM, WN, VB>;
  if (int e = raise_dyn_lds(kern, kK3LdsCap, "conv2d_k3")) return e;
  const dim3 grid((unsigned)((long)p.B * pl.ntx * pl.nty), (unsigned)(p.M / (64 * WN)));
  hipLaunchKernelGGL(kern, grid, dim3(WM * WN * 64), pl.lds, s, p);
  return check_launch("conv2d_k3");
}

// H x W: the input image; OH x OW, org: the output image and its origin inside the input (K3Params); reflect: the halo mode
template <int DT>
int k3_run(const float* x, const float* w, const float* bias, float* y, int B, int C, int M, int H, int W, int OH, int OW, int org, int reflect,
           long sm, long sc, void* ws, size_t wsb, hipStream_t s) {
  const size_t need = ((size_t)C * M * 9 * sizeof(float) + 255) & ~(size_t)255;
  if (!ws || wsb < need) { set_error("conv2d_k3: workspace too small"); return NC_ERR_WS; }
  const K3Plan pl = k3_plan(B, C, M, OH, OW);
  if (!pl.ok) { set_error("conv2d_k3: tile configuration %d does not apply", sw::raw(sw::CONV2D_K3_CFG)); return NC_ERR_SHAPE; }
  float* wp = (float*)ws;
  const long total = (long)C * M * 9;
  hipLaunchKernelGGL(k_pack_k3, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, w, wp, C, sm, sc, total);
  if (int e = check_launch("pack_k3")) return e;
  K3Params p{};
  p.x = x; p.wp = wp; p.bias = bias; p.y = y;
  p.B = B; p.C = C; p.M = M; p.H = H; p.W = W;
  p.OH = OH; p.OW = OW; p.org = org; p.reflect = reflect;
  p.TH = pl.TH; p.TW = pl.TW; p.ntx = pl.ntx; p.nty = pl.nty; p.CK = pl.CK; p.CS = pl.CS;
  switch (pl.cfg) {
    case 0: return k3_launch_cfg<DT, 4, 1, 2>(pl, p, s);
    case 1: return k3_launch_cfg<DT, 4, 1, 1>(pl, p, s);
  }
  set_error("conv2d_k3: unknown tile configuration");
  return NC_ERR_SHAPE;
}

}  // namespace

int conv2d_k3_num_cfgs() { return kK3NumCfgs; }
// forward: M = K output channels, reduction over C;  data gradient: M = C, reduction over K
bool conv2d_k3_fwd_supported(const ConvDims& d) { return k3_shape_ok(d, d.C, d.K); }
bool conv2d_k3_dgrad_supported(const ConvDims& d) { return k3_shape_ok(d, d.K, d.C); }
size_t conv2d_k3_ws_bytes(const ConvDims& d) {
  if (!k3_layer_ok(d)) return 0;
  return ((size_t)d.C * d.K * 9 * sizeof(float) + 255) & ~(size_t)255;
}

int conv_fwd_k3(const float* x, const float* w, const float* bias, float* y, const ConvDims& d, void* ws, size_t wsb, hipStream_t s) {
  if (!conv2d_k3_fwd_supported(d)) { set_error("conv2d_k3_fwd: shape not covered"); return NC_ERR_SHAPE; }
  return k3_run<1>(x, w, bias, y, d.N, d.C, d.K, d.H, d.W, d.H, d.W, 0, 0, (long)d.C * 9, 9L, ws, wsb, s);
}

int conv_dgrad_k3(const float* dy, const float* w, float* dx, const ConvDims& d, void* ws, size_t wsb, hipStream_t s) {
  if (!conv2d_k3_dgrad_supported(d)) { set_error("conv2d_k3_dgrad: shape not covered"); return NC_ERR_SHAPE; }
  return k3_run<-1>(dy, w, nullptr, dx, d.N, d.K, d.C, d.H, d.W, d.H, d.W, 0, 0, 9L, (long)d.C * 9, ws, wsb, s);
}

// ---- ReflectionPad2d(1) + Conv2d(k 3, s 1, p 0) of a ResnetBlock (reference models/networks.py:808-830) on the same kernel.  d describes the
// layer as the zero-padded one (H x W image, padding 1): the coverage is that layer's rule, and H, W >= 2 (a mirror needs a second pixel).
bool conv2d_k3_reflect_ok(const ConvDims& d) { return d.H >= 2 && d.W >= 2 && (long)d.N * d.C * (d.H + 2) * (d.W + 2) < (1L << 31); }

// forward: only the source table differs (K3Params::reflect)
int conv_fwd_k3_reflect(const float* x, const float* w, const float* bias, float* y, const ConvDims& d, void* ws, size_t wsb, hipStream_t s) {
  if (!conv2d_k3_fwd_supported(d) || !conv2d_k3_reflect_ok(d)) { set_error("conv2d_k3_reflect_fwd: shape not covered"); return NC_ERR_SHAPE; }
  return k3_run<1>(x, w, bias, y, d.N, d.C, d.K, d.H, d.W, d.H, d.W, 0, 1, (long)d.C * 9, 9L, ws, wsb, s);
}

// data gradient, first half: the ZERO-padded data gradient on the (H + 2) x (W + 2) domain of the padded input -- dxe[c][i][j], i in -1 .. H,
// j in -1 .. W, with dy zero outside the image -- written densely as [N][C][H + 2][W + 2].  The caller folds the border back (reflect_pad_bwd).
int conv_dgrad_k3_reflect_ext(const float* dy, const float* w, float* dxe, const ConvDims& d, void* ws, size_t wsb, hipStream_t s) {
  if (!conv2d_k3_dgrad_supported(d) || !conv2d_k3_reflect_ok(d)) { set_error("conv2d_k3_reflect_dgrad: shape not covered"); return NC_ERR_SHAPE; }
  return k3_run<-1>(dy, w, nullptr, dxe, d.N, d.K, d.C, d.H, d.W, d.H + 2, d.W + 2, -1, 0, 9L, (long)d.C * 9, ws, wsb, s);
}

}  // namespace nc
