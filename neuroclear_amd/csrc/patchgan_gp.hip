// WGAN-GP gradient penalty of the 2-D PatchGAN (reference models/networks.py:321-359, cal_gradient_penalty) with the
// discriminator of nets.hip (NLayerDiscriminator, InstanceNorm, one input channel), as one C call per direction.
//
// Notation, conv i = 0 .. H (H = the 1-channel head): a_0 = x, z_i = W_i * a_i + b_i, a_1 = lrelu(z_0),
// n_i = (z_i - mu_i) r_i and a_{i+1} = lrelu(n_i) for the normed layers 1 .. H-1 (r = 1 / sqrt(var + eps)), y = z_H.
//
// Forward (nc_patchgan_gp_fwd): the discriminator's forward, then its backward with dy = 1:
//   delta_H = 1;  u_i = dgrad(delta_i, W_i);  delta_i = r (h - mean h - n mean(h n)) with h = lrelu'(n_i) u_{i+1}
//   (layers H-1 .. 1);  delta_0 = lrelu'(z_0) u_1;  g = u_0.   pen = lambda mean_b (||g_b + 1e-16|| - c)^2.
// `saved` keeps the forward's tensors (nets.hip layout), every delta_i, every u_{i+1} of a normed layer and ||g_b + 1e-16||.
//
// Backward (nc_patchgan_gp_bwd): the adjoint of that first backward, run in forward order, from ub_0 = v = dpen dpen/dg:
//   conv i:   db_i = W_i * ub_i (a forward conv, no bias);  dW_i += wgrad(ub_i, delta_i)
//   layer 0:  ub_1 = lrelu'(z_0) db_0                        (lrelu'' = 0 almost everywhere)
//   norm i:   ub_{i+1} = lrelu'(n_i) r (db - mean db - n mean(db n))   (the norm's backward is self-adjoint)
//             nb_i = -r (db mean(h n) + h mean(db n))         adjoint of n_i
//             rb_i = sum(db delta_i) / r                      adjoint of r_i
//   head:     dW_H += wgrad(ub_H, 1)
// then one ordinary backward through the forward network of the adjoints collected on (n_i, r_i):
//   N = nb_i + lrelu'(n_i) ab_{i+1};  zb_i = r (N - mean N - n mean(N n)) - (r^2 rb_i / S) n
//   dW_i += wgrad(a_i, zb_i);  ab_i = dgrad(zb_i, W_i);  zb_0 = lrelu'(z_0) ab_1;  db_0 = sum zb_0;  dx = dgrad(zb_0, W_0).
// zb_i has zero mean over every plane, so the bias of every conv in front of a norm gets an exact zero, and so does the head's
// bias, which g does not depend on.  Every convolution is nc_conv_fwd / _dgrad / _wgrad; the per-plane norm kernels below sum
// in fp64 in a fixed order and the weight gradients add two fixed-order products: no float atomics, the same bits every run.
#include "common.hpp"
#include "patchgan_plan.hpp"

namespace nc {
namespace {

constexpr float kSlope = 0.2f;
constexpr float kEps = 1e-16f;  // added to every element of g before the norm (networks.py:353)

size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// fixed-order sum of NV doubles over the block (NT threads); every thread gets the totals
template <int NT, int NV>
__device__ void block_sums(double (&v)[NV], double (*red)[NT]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NV; ++k) red[k][t] = v[k];
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s)
#pragma unroll
      for (int k = 0; k < NV; ++k) red[k][t] += red[k][t + s];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = red[k][0];
}

__global__ void k_gp_fill(float* __restrict__ p, float v, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

__global__ void k_gp_add(float* __restrict__ a, const float* __restrict__ b, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) a[i] += b[i];
}

// nrm[b] = ||g_b + 1e-16||_2, fp64 sum of squares; one block per sample
__global__ void __launch_bounds__(256) k_gp_norm(const float* __restrict__ g, double* __restrict__ nrm, long per) {
  __shared__ double red[1][256];
  const float* gb = g + (long)blockIdx.x * per;
  double v[1] = {0.0};
  for (long j = threadIdx.x; j < per; j += 256) {
    const double e = (double)(gb[j] + kEps);
    v[0] += e * e;
  }
  block_sums<256, 1>(v, red);
  if (threadIdx.x == 0) nrm[blockIdx.x] = sqrt(v[0]);
}

// pen = lambda mean_b (nrm_b - c)^2 in sample order
__global__ void k_gp_pen(const double* __restrict__ nrm, int B, double c, double lam, float* __restrict__ pen) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += (nrm[b] - c) * (nrm[b] - c);
  *pen = (float)(s / B * lam);
}

// v = dpen * dpen/dg = dpen lambda (2 / B) (nrm_b - c) / nrm_b (g + 1e-16); a zero norm has a zero gradient (as torch's norm)
__global__ void k_gp_v(const float* __restrict__ g, const double* __restrict__ nrm, const float* __restrict__ dpen, float* __restrict__ v,
                       long per, long n, int B, double c, double lam) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double nb = nrm[i / per];
  const float k = nb > 0.0 ? (float)((double)dpen[0] * lam * 2.0 / B * (nb - c) / nb) : 0.f;
  v[i] = k * (g[i] + kEps);
}

// Adjoint of one norm layer's backward (forward order), one block per (sample, channel) plane of S elements:
// db = W * ub (this conv's adjoint), u = dL/da_{i+1} and delta = dL/dz_i of the first backward.
// Writes ub_next = lrelu'(n) r (db - mean db - n mean(db n)), nb = -r (db mean(h n) + h mean(db n)), rb = sum(db delta) / r.
template <int NT>
__global__ void __launch_bounds__(NT) k_gp_in_adj(const float* __restrict__ db, const float* __restrict__ u, const float* __restrict__ z,
                                                  const float* __restrict__ mean, const float* __restrict__ rstd,
                                                  const float* __restrict__ delta, float* __restrict__ ub_next, float* __restrict__ nb,
                                                  float* __restrict__ rb, long S) {
  __shared__ double red[4][NT];
  const long o = (long)blockIdx.x * S;
  const float mu = mean[blockIdx.x], r = rstd[blockIdx.x];
  double v[4] = {0.0, 0.0, 0.0, 0.0};  // sum db, sum db n, sum h n, sum db delta
  for (long j = threadIdx.x; j < S; j += NT) {
    const float n = (z[o + j] - mu) * r;
    const float h = (n > 0.f ? 1.f : kSlope) * u[o + j];
    const float d = db[o + j];
    v[0] += d;
    v[1] += (double)d * n;
    v[2] += (double)h * n;
    v[3] += (double)d * delta[o + j];
  }
  block_sums<NT, 4>(v, red);
  const float m_d = (float)(v[0] / S), m_dn = (float)(v[1] / S), m_hn = (float)(v[2] / S);
  for (long j = threadIdx.x; j < S; j += NT) {
    const float n = (z[o + j] - mu) * r;
    const float mk = n > 0.f ? 1.f : kSlope;
    const float h = mk * u[o + j];
    const float d = db[o + j];
    ub_next[o + j] = mk * (r * (d - m_d - n * m_dn));
    nb[o + j] = -r * (d * m_hn + h * m_dn);
  }
  if (threadIdx.x == 0) rb[blockIdx.x] = (float)(v[3] / r);
}

// Ordinary backward of one norm layer with the extra adjoints: N = nb + lrelu'(n) ab (ab nullable: the layer under the head),
// zb = r (N - mean N - n mean(N n)) - (r^2 rb / S) n.  zb may alias nb.
template <int NT>
__global__ void __launch_bounds__(NT) k_gp_in_zbar(const float* nb, const float* __restrict__ ab, const float* __restrict__ z,
                                                   const float* __restrict__ mean, const float* __restrict__ rstd,
                                                   const float* __restrict__ rb, float* zb, long S) {
  __shared__ double red[2][NT];
  const long o = (long)blockIdx.x * S;
  const float mu = mean[blockIdx.x], r = rstd[blockIdx.x];
  double v[2] = {0.0, 0.0};  // sum N, sum N n
  for (long j = threadIdx.x; j < S; j += NT) {
    const float n = (z[o + j] - mu) * r;
    const float N = ab ? nb[o + j] + (n > 0.f ? 1.f : kSlope) * ab[o + j] : nb[o + j];
    v[0] += N;
    v[1] += (double)N * n;
  }
  block_sums<NT, 2>(v, red);
  const float m_N = (float)(v[0] / S), m_Nn = (float)(v[1] / S);
  const float kr = (float)((double)r * r * rb[blockIdx.x] / S);
  for (long j = threadIdx.x; j < S; j += NT) {
    const float n = (z[o + j] - mu) * r;
    const float N = ab ? nb[o + j] + (n > 0.f ? 1.f : kSlope) * ab[o + j] : nb[o + j];
    zb[o + j] = r * (N - m_N - n * m_Nn) - kr * n;
  }
}

// the penalty's own layout on top of the discriminator's plan
struct GpPlan {
  PgPlan P;
  size_t d_off[8], u_off[8];  // floats into `saved`: delta_i (i < H); u_{i+1} of normed layer i
  size_t nrm_off;             // B doubles
  size_t saved;               // floats
  size_t nb_off[8], rb_off[8];  // floats into the adjoint region of the workspace
  size_t nb_total, rb_total, max_w, head_n;
  size_t pg_ws, o_gc, o_nb, o_rb, o_tw, o_ones, o_y, ws;  // bytes
};

bool gp_plan(GpPlan& G, int B, int D, int H, int W, int n_layers, int ndf, int nd) {
  if (nd != 2 || D != 1 || !pg_plan(G.P, B, D, H, W, n_layers, ndf, nd)) return false;
  const PgPlan& P = G.P;
  size_t so = P.saved, nb = 0, rb = 0;
  G.max_w = 0;
  for (int i = 0; i < P.nl; ++i) {
    const PgLayer& l = P.L[i];
    const size_t on = (size_t)B * l.K * l.oH * l.oW;
    const size_t wn = (size_t)l.K * l.C * 16;
    if (wn > G.max_w) G.max_w = wn;
    if (i == P.nl - 1) { G.head_n = on; break; }
    G.d_off[i] = so; so += on;
    if (l.norm) {
      G.u_off[i] = so; so += on;
      G.nb_off[i] = nb; nb += on;
      G.rb_off[i] = rb; rb += (size_t)B * l.K;
    }
  }
  so = (so + 1) & ~(size_t)1;  // 8-byte alignment of the norms
  G.nrm_off = so; so += 2 * (size_t)B;
  G.saved = so;
  G.nb_total = nb; G.rb_total = rb;
  G.pg_ws = nc_patchgan_ws_bytes(B, D, H, W, n_layers, ndf, nd);
  size_t o = G.pg_ws;
  G.o_gc = o; o += al256(P.max_act * sizeof(float));
  G.o_nb = o; o += al256(nb * sizeof(float));
  G.o_rb = o; o += al256(rb * sizeof(float));
  G.o_tw = o; o += al256(G.max_w * sizeof(float));
  G.o_ones = o; o += al256(G.head_n * sizeof(float));
  G.o_y = o; o += al256(G.head_n * sizeof(float));
  G.ws = o;
  return true;
}

int gp_check(const char* what, GpPlan& G, int B, int D, int H, int W, int n_layers, int ndf, int nd, size_t ws_bytes, const void* ws) {
  if (!gp_plan(G, B, D, H, W, n_layers, ndf, nd)) {
    set_error("%s: B=%d D=%d H=%d W=%d n_layers=%d ndf=%d nd=%d not covered (2-D, D = 1, instance norm, 1 <= n_layers <= 6)", what, B, D,
              H, W, n_layers, ndf, nd);
    return NC_ERR_SHAPE;
  }
  if (!ws || ws_bytes < G.ws) { set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, G.ws); return NC_ERR_WS; }
  return NC_OK;
}

int zero(float* p, long n, hipStream_t s) {
  hipLaunchKernelGGL(k_gp_fill, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, p, 0.f, n);
  return check_launch("patchgan_gp zero");
}

template <typename K, typename... A>
int plane_launch(K k64, K k256, long planes, long S, hipStream_t s, const char* what, A... a) {
  if (S >= 1024) hipLaunchKernelGGL(k256, dim3((unsigned)planes), dim3(256), 0, s, a...);
  else hipLaunchKernelGGL(k64, dim3((unsigned)planes), dim3(64), 0, s, a...);
  return check_launch(what);
}

}  // namespace
}  // namespace nc

using namespace nc;

extern "C" {

size_t nc_patchgan_gp_saved_floats(int B, int D, int H, int W, int n_layers, int ndf, int nd) {
  GpPlan G;
  return gp_plan(G, B, D, H, W, n_layers, ndf, nd) ? G.saved : 0;
}

size_t nc_patchgan_gp_ws_bytes(int B, int D, int H, int W, int n_layers, int ndf, int nd) {
  GpPlan G;
  return gp_plan(G, B, D, H, W, n_layers, ndf, nd) ? G.ws : 0;
}

int nc_patchgan_gp_fwd(const float* params, const float* x, float* g, float* pen, float* saved, int B, int D, int H, int W, int n_layers,
                       int ndf, int nd, float constant, float lambda_gp, void* ws, size_t ws_bytes, void* stream) {
  GpPlan G;
  NC_TRY(gp_check("patchgan_gp_fwd", G, B, D, H, W, n_layers, ndf, nd, ws_bytes, ws));
  if (!params || !x || !g || !pen || !saved) { set_error("patchgan_gp_fwd: null pointer"); return NC_ERR_ARG; }
  const PgPlan& P = G.P;
  hipStream_t s = (hipStream_t)stream;
  char* wb = (char*)ws;
  void* cws = ws;
  void* iws = wb + al256(P.conv_ws);
  float* ga = (float*)(wb + al256(P.conv_ws) + al256(P.in_ws));
  float* ones = (float*)(wb + G.o_ones);
  NC_TRY(nc_patchgan_fwd(params, x, (float*)(wb + G.o_y), saved, B, 1, H, W, n_layers, ndf, nd, ws, G.pg_ws, stream));
  hipLaunchKernelGGL(k_gp_fill, dim3((unsigned)cdiv((long)G.head_n, 256)), dim3(256), 0, s, ones, 1.f, (long)G.head_n);
  NC_TRY(check_launch("patchgan_gp fill"));
  // backward of sum(D(x)): delta_H = 1
  const float* delta = ones;
  for (int i = P.nl - 1; i >= 0; --i) {
    const PgLayer& l = P.L[i];
    float* u = i == 0 ? g : i == 1 ? ga : saved + G.u_off[i - 1];  // dL/da_i
    NC_TRY(nc_conv_dgrad(delta, params + l.w_off, u, B, l.C, 1, l.iH, l.iW, l.K, 1, 4, 4, l.stride, 1, cws, P.conv_ws, stream));
    if (i == 0) break;
    const PgLayer& q = P.L[i - 1];
    const long S = (long)q.oH * q.oW;
    float* dq = saved + G.d_off[i - 1];
    if (q.norm) {
      const float* mean = saved + q.stat_off;
      NC_TRY(nc_instnorm_act_bwd(u, saved + q.raw_off, mean, mean + (size_t)B * q.K, kSlope, dq, B * q.K, S, iws, P.in_ws, stream));
    } else {  // layer 0: the sign of the stored activation is the sign of z_0
      NC_TRY(nc_leaky_relu_bwd(u, saved + q.act_off, kSlope, dq, (long)B * q.K * S, stream));
    }
    delta = dq;
  }
  double* nrm = (double*)(saved + G.nrm_off);
  hipLaunchKernelGGL(k_gp_norm, dim3(B), dim3(256), 0, s, (const float*)g, nrm, (long)H * W);
  hipLaunchKernelGGL(k_gp_pen, dim3(1), dim3(64), 0, s, (const double*)nrm, B, (double)constant, (double)lambda_gp, pen);
  return check_launch("patchgan_gp pen");
}

int nc_patchgan_gp_bwd(const float* params, const float* x, const float* saved, const float* g, const float* dpen, float* dparams, float* dx,
                       int B, int D, int H, int W, int n_layers, int ndf, int nd, float constant, float lambda_gp, void* ws, size_t ws_bytes,
                       void* stream) {
  GpPlan G;
  NC_TRY(gp_check("patchgan_gp_bwd", G, B, D, H, W, n_layers, ndf, nd, ws_bytes, ws));
  if (!params || !x || !saved || !g || !dpen) { set_error("patchgan_gp_bwd: null pointer"); return NC_ERR_ARG; }
  if (!dparams && !dx) return NC_OK;
  const PgPlan& P = G.P;
  hipStream_t s = (hipStream_t)stream;
  char* wb = (char*)ws;
  void* cws = ws;
  float* ga = (float*)(wb + al256(P.conv_ws) + al256(P.in_ws));
  float* gb = (float*)((char*)ga + al256(P.max_act * sizeof(float)));
  float* gc = (float*)(wb + G.o_gc);
  float* nbar = (float*)(wb + G.o_nb);
  float* rbar = (float*)(wb + G.o_rb);
  float* tw = (float*)(wb + G.o_tw);
  const float* ones = (const float*)(wb + G.o_ones);
  hipLaunchKernelGGL(k_gp_fill, dim3((unsigned)cdiv((long)G.head_n, 256)), dim3(256), 0, s, (float*)ones, 1.f, (long)G.head_n);
  const long nx = (long)B * H * W;
  hipLaunchKernelGGL(k_gp_v, dim3((unsigned)cdiv(nx, 256)), dim3(256), 0, s, g, (const double*)(saved + G.nrm_off), dpen, ga, (long)H * W,
                     nx, B, (double)constant, (double)lambda_gp);
  NC_TRY(check_launch("patchgan_gp v"));

  // adjoint of the first backward, in forward order: ga = ub_i, gb = db_i
  for (int i = 0; i < P.nl; ++i) {
    const PgLayer& l = P.L[i];
    const bool head = i == P.nl - 1;
    if (dparams)
      NC_TRY(nc_conv_wgrad(ga, head ? ones : saved + G.d_off[i], dparams + l.w_off, nullptr, B, l.C, 1, l.iH, l.iW, l.K, 1, 4, 4, l.stride,
                           1, cws, P.conv_ws, stream));
    if (head) break;
    NC_TRY(nc_conv_fwd(ga, params + l.w_off, nullptr, gb, B, l.C, 1, l.iH, l.iW, l.K, 1, 4, 4, l.stride, 1, cws, P.conv_ws, stream));
    const long S = (long)l.oH * l.oW;
    if (!l.norm) {
      NC_TRY(nc_leaky_relu_bwd(gb, saved + l.act_off, kSlope, ga, (long)B * l.K * S, stream));
      continue;
    }
    const float* mean = saved + l.stat_off;
    NC_TRY(plane_launch(k_gp_in_adj<64>, k_gp_in_adj<256>, (long)B * l.K, S, s, "patchgan_gp in_adj", (const float*)gb,
                        saved + G.u_off[i], saved + l.raw_off, mean, mean + (size_t)B * l.K, saved + G.d_off[i], ga, nbar + G.nb_off[i],
                        rbar + G.rb_off[i], S));
  }
  if (dparams) NC_TRY(zero(dparams + P.L[P.nl - 1].b_off, P.L[P.nl - 1].K, s));  // the head's bias does not reach g

  // ordinary backward through the forward network of the adjoints of (n_i, r_i)
  const float* ab = nullptr;  // dL/da_{i+1}
  float* abuf[2] = {ga, gb};
  int ping = 0;
  for (int i = P.nl - 2; i >= 0; --i) {
    const PgLayer& l = P.L[i];
    const long S = (long)l.oH * l.oW;
    const float* in = i == 0 ? x : saved + P.L[i - 1].act_off;
    float* zb;
    if (l.norm) {
      zb = nbar + G.nb_off[i];
      const float* mean = saved + l.stat_off;
      NC_TRY(plane_launch(k_gp_in_zbar<64>, k_gp_in_zbar<256>, (long)B * l.K, S, s, "patchgan_gp in_zbar", (const float*)zb, ab,
                          saved + l.raw_off, mean, mean + (size_t)B * l.K, (const float*)(rbar + G.rb_off[i]), zb, S));
    } else {
      zb = gc;
      NC_TRY(nc_leaky_relu_bwd(ab, saved + l.act_off, kSlope, zb, (long)B * l.K * S, stream));
    }
    if (dparams) {
      const size_t wn = (size_t)l.K * l.C * 16;
      NC_TRY(nc_conv_wgrad(in, zb, tw, l.norm ? nullptr : dparams + l.b_off, B, l.C, 1, l.iH, l.iW, l.K, 1, 4, 4, l.stride, 1, cws,
                           P.conv_ws, stream));
      hipLaunchKernelGGL(k_gp_add, dim3((unsigned)cdiv((long)wn, 256)), dim3(256), 0, s, dparams + l.w_off, (const float*)tw, (long)wn);
      NC_TRY(check_launch("patchgan_gp add"));
      if (l.norm) NC_TRY(zero(dparams + l.b_off, l.K, s));
    }
    if (i == 0) {
      if (dx) NC_TRY(nc_conv_dgrad(zb, params + l.w_off, dx, B, l.C, 1, l.iH, l.iW, l.K, 1, 4, 4, l.stride, 1, cws, P.conv_ws, stream));
      break;
    }
    float* an = abuf[ping];
    ping ^= 1;
    NC_TRY(nc_conv_dgrad(zb, params + l.w_off, an, B, l.C, 1, l.iH, l.iW, l.K, 1, 4, 4, l.stride, 1, cws, P.conv_ws, stream));
    ab = an;
  }
  return NC_OK;
}

}  // extern "C"
