// Layer plan of the whole-network PatchGAN entry points (nets.hip: nc_patchgan_*; patchgan_gp.hip: nc_patchgan_gp_*):
// per-conv shapes, offsets of every parameter tensor in the packed blob and of every stored tensor in `saved`.
#pragma once

#include "common.hpp"

namespace nc {

struct PgLayer {
  int C, K, stride;   // channels in / out, stride
  int iD, iH, iW;     // input spatial size (iD = 1 for 2-D)
  int oD, oH, oW;
  bool norm;          // InstanceNorm + LeakyReLU after the conv (else: LeakyReLU only for layer 0, nothing for the head)
  size_t w_off, b_off;        // floats into the parameter blob
  size_t raw_off, act_off;    // floats into `saved`: raw conv output; activation that feeds the NEXT conv
  size_t stat_off;            // mean [B*K] then rstd [B*K]
};

struct PgPlan {
  int nl;            // number of convs = n_layers + 2
  PgLayer L[8];
  size_t params, saved;       // floats
  bool fused0;                // first layer = conv + LeakyReLU in one kernel (patchgan_edge.hip): only its activation is stored
  size_t max_act;             // largest per-layer tensor (floats), for the gradient ping-pong buffers
  size_t conv_ws, in_ws;      // bytes
  int oD, oH, oW;
};

inline bool pg_plan(PgPlan& P, int B, int D, int H, int W, int n_layers, int ndf, int nd) {
  if (B < 1 || H < 4 || W < 4 || n_layers < 1 || n_layers > 6 || ndf < 1 || (nd != 2 && nd != 3)) return false;
  if (nd == 2 && D != 1) return false;
  if (nd == 3 && D < 4) return false;
  P = PgPlan{};
  P.nl = n_layers + 2;
  int cin = 1, mult = 1;
  int d = D, h = H, w = W;
  size_t po = 0, so = 0;
  const int k3 = nd == 3 ? 64 : 16;
  for (int i = 0; i < P.nl; ++i) {
    PgLayer& l = P.L[i];
    const bool head = i == P.nl - 1;
    if (i == 0) {
      mult = 1;
      const bool pg1 = sw::raw(sw::PG1) != 0;
      ConvDims c0;
      P.fused0 = pg1 && nd == 2 && make_dims(c0, B, 1, 1, h, w, ndf, 1, 4, 4, 2, 1) && pg1_supported(c0);
    }
    else if (!head) mult = (1 << i) < 8 ? (1 << i) : 8;
    l.C = cin;
    l.K = head ? 1 : ndf * mult;
    l.stride = (i < n_layers) ? 2 : 1;
    l.norm = i > 0 && !head;
    l.iD = d; l.iH = h; l.iW = w;
    ConvDims cd;
    if (!make_dims(cd, B, l.C, d, h, w, l.K, nd == 3 ? 4 : 1, 4, 4, l.stride, 1)) return false;
    l.oD = cd.Do; l.oH = cd.Ho; l.oW = cd.Wo;
    l.w_off = po; po += (size_t)l.K * l.C * k3;
    l.b_off = po; po += (size_t)l.K;
    const size_t on = (size_t)B * l.K * l.oD * l.oH * l.oW;
    l.raw_off = so; so += on;
    l.act_off = so;
    if (!head) so += on;
    l.stat_off = so;
    if (l.norm) so += 2 * (size_t)B * l.K;
    if (on > P.max_act) P.max_act = on;
    const size_t in_n = (size_t)B * l.C * d * h * w;
    if (in_n > P.max_act) P.max_act = in_n;
    const size_t cw = nc_conv_ws_bytes(B, l.C, d, h, w, l.K, nd == 3 ? 4 : 1, 4, 4, l.stride, 1);
    if (cw > P.conv_ws) P.conv_ws = cw;
    if (l.norm) {
      const size_t iw = nc_instnorm_bwd_dbias_ws_bytes(B * l.K, (long)l.oD * l.oH * l.oW);
      if (iw > P.in_ws) P.in_ws = iw;
    }
    cin = l.K; d = l.oD; h = l.oH; w = l.oW;
  }
  P.params = po; P.saved = so;
  P.oD = d; P.oH = h; P.oW = w;
  return true;
}

}  // namespace nc
