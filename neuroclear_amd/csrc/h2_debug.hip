// Test exports of the writers of the H2 operand form (h2.hip, norm_act.hip, convt_s3.hip; tests/test_gpu_h2_writers.py): each entry validates
// its arguments and forwards to the internal function the whole-network calls use, unchanged -- no kernel of its own.
#include <cmath>

#include "common.hpp"

using namespace nc;

extern "C" {

// an H2 tensor of N * C * S elements: the units, 256 bytes of cells behind them (common.hpp h2_cells_offset)
size_t nc_h2_bytes(int N, int C, long S) {
  if (N < 1 || C < 1 || S < 1) return 0;
  return h2_cells_offset((size_t)N * C * S) + 256;
}
size_t nc_h2_cells_offset(size_t elems) { return h2_cells_offset(elems); }

static bool h2_part_ok(int N, int C, long S, int ctot, int c0) {
  return N >= 1 && C >= 8 && S >= 1 && C % 8 == 0 && ctot % 8 == 0 && c0 % 8 == 0 && c0 >= 0 && c0 + C <= ctot && (long)N * C / 8 <= 65535;
}

int nc_to_h2_debug(const float* x, long xstride, void* xs, int N, int C, long S, int ctot, int c0, unsigned* cell, float bound, unsigned* guard,
                   void* stream) {
  if (!x || !xs || !cell) { set_error("to_h2_debug: null pointer"); return NC_ERR_ARG; }
  if (!h2_part_ok(N, C, S, ctot, c0) || xstride < (long)C * S) { set_error("to_h2_debug: bad shape"); return NC_ERR_SHAPE; }
  hipStream_t s = (hipStream_t)stream;
  if (bound > 0.f) {
    if (int e = h2_set_cell(cell, bound, s)) return e;
  } else {  // measured, sample by sample (conv_split.hip operand_into)
    if (int e = h2_zero_cells(cell, 1, s)) return e;
    for (int n = 0; n < N; ++n)
      if (int e = h2_absmax(x + (long)n * xstride, (long)C * S, cell, s)) return e;
  }
  if (guard)
    if (int e = h2_guard_zero(guard, s)) return e;
  return split2h_into(x, xstride, xs, N, C, S, ctot, c0, cell, s, guard);
}

int nc_act_split2h_debug(const float* x, const float* mean, const float* rstd, float slope, float* y, long ystride, void* ys, int N, int C, long S,
                         int ctot, int c0, float bound, unsigned* cell, unsigned* cell2, void* stream) {
  if (!x || !mean || !rstd || !ys) { set_error("act_split2h_debug: null pointer"); return NC_ERR_ARG; }
  if (!h2_part_ok(N, C, S, ctot, c0) || (y && ystride < (long)C * S) || !(bound > 0.f)) { set_error("act_split2h_debug: bad shape"); return NC_ERR_SHAPE; }
  return act_split2h(x, mean, rstd, slope, y, ystride, ys, N, C, S, ctot, c0, bound, cell, cell2, (hipStream_t)stream);
}

int nc_act_split2h_pool_debug(const float* x, const float* mean, const float* rstd, float slope, void* ys, void* pooled, int N, int C, int D, int H,
                              int W, int ctot, int c0, float bound, unsigned* cell, void* stream) {
  if (!x || !mean || !rstd || !ys || !pooled) { set_error("act_split2h_pool_debug: null pointer"); return NC_ERR_ARG; }
  if (D < 2 || H < 2 || W < 2 || !h2_part_ok(N, C, (long)D * H * W, ctot, c0) || !(bound > 0.f)) { set_error("act_split2h_pool_debug: bad shape"); return NC_ERR_SHAPE; }
  return act_split2h_pool(x, mean, rstd, slope, ys, pooled, N, C, D, H, W, ctot, c0, bound, cell, (hipStream_t)stream);
}

// the training form (h2.hip k_act_split2h_pool<true>): pooled fp32 and the winner bytes; pointers and shape are checked by the internal function
int nc_act_split2h_pool_arg_debug(const float* x, const float* mean, const float* rstd, float slope, void* ys, float* pooled, unsigned char* arg, int N,
                                  int C, int D, int H, int W, int ctot, int c0, float bound, unsigned* cell, void* stream) {
  if (!(bound > 0.f)) { set_error("act_split2h_pool_arg_debug: bad shape"); return NC_ERR_SHAPE; }
  return act_split2h_pool_arg(x, mean, rstd, slope, ys, pooled, arg, N, C, D, H, W, ctot, c0, bound, cell, (hipStream_t)stream);
}

int nc_maxpool2_h2_debug(const void* in, void* out, int N, int C, int ctot, int D, int H, int W, void* stream) {
  if (!in || !out) { set_error("maxpool2_h2_debug: null pointer"); return NC_ERR_ARG; }
  if (D < 2 || H < 2 || W < 2 || !h2_part_ok(N, C, (long)D * H * W, ctot, 0)) { set_error("maxpool2_h2_debug: bad shape"); return NC_ERR_SHAPE; }
  return maxpool2_h2(in, out, N, C, ctot, D, H, W, (hipStream_t)stream);
}

int nc_h2_to_s3_if_debug(const void* xh, void* xs, int N, int C, long S, const unsigned* cells, const unsigned* guard, void* stream) {
  if (!xh || !xs || !cells) { set_error("h2_to_s3_if_debug: null pointer"); return NC_ERR_ARG; }
  if (!h2_part_ok(N, C, S, C, 0)) { set_error("h2_to_s3_if_debug: bad shape"); return NC_ERR_SHAPE; }
  return h2_to_s3_if(xh, xs, N, C, S, cells, guard, (hipStream_t)stream);
}

int nc_instnorm_act_bwd_dbias_h2_debug(const float* dy, const float* w1, const float* x, const float* mean, const float* rstd, float slope, void* dxs,
                                       float* dbias, int N, int C, long S, void* ws, size_t ws_bytes, unsigned* guard, void* stream) {
  // (pointers, shape and workspace: checked by the internal function)
  if (w1) {
    if (N != 1) { set_error("instnorm_act_bwd_dbias_h2_debug: the rank-one form takes one sample"); return NC_ERR_ARG; }
    return instnorm_act_bwd_dbias_h2_rank1(dy, w1, x, mean, rstd, slope, dxs, dbias, C, S, ws, ws_bytes, stream, guard);
  }
  return instnorm_act_bwd_dbias_h2(dy, x, mean, rstd, slope, dxs, dbias, N, C, S, ws, ws_bytes, stream, guard);
}

// The same inside a whole-network scope (guard mode 1 counts a flagged tensor and switches nothing, as in nc_unet_deconv_bwd), and with gp / arg
// != NULL the POOL form: dy is the skip gradient with sample stride dy_stride.  nc_maxpool2_fwd_arg_debug: the pool forward that leaves the
// winner bytes.
int nc_instnorm_act_bwd_dbias_h2_pool_debug(const float* dy, long dy_stride, const float* gp, const unsigned char* arg, const float* x, const float* mean,
                                            const float* rstd, float slope, void* dxs, float* dbias, int N, int C, int D, int H, int W, void* ws,
                                            size_t ws_bytes, unsigned* guard, void* stream) {
  NetworkScope net_scope;
  if (D < 1 || H < 1 || W < 1) { set_error("instnorm_act_bwd_dbias_h2_pool_debug: bad shape"); return NC_ERR_SHAPE; }
  if (!gp && !arg) {
    if (dy_stride != (long)C * D * H * W) { set_error("instnorm_act_bwd_dbias_h2_pool_debug: the plain form takes a dense gradient"); return NC_ERR_ARG; }
    return instnorm_act_bwd_dbias_h2(dy, x, mean, rstd, slope, dxs, dbias, N, C, (long)D * H * W, ws, ws_bytes, stream, guard);
  }
  return instnorm_act_bwd_dbias_h2_pool(dy, dy_stride, gp, arg, x, mean, rstd, slope, dxs, dbias, N, C, D, H, W, ws, ws_bytes, stream, guard);
}
int nc_maxpool2_fwd_arg_debug(const float* x, float* y, unsigned char* arg, int NC, int D, int H, int W, void* stream) {
  return maxpool2_fwd_arg(x, y, arg, NC, D, H, W, (hipStream_t)stream);
}

static size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
size_t nc_convT_k2s2_split_h2_ws_bytes(int N, int C, int D, int H, int W, int K) {
  if (!convT_s3x_supported(N, C, D, H, W, K)) return 0;
  return al256(convT_s3x_ws_bytes(C, K)) + h2_cells_offset((size_t)N * C * D * H * W) + 256;
}
int nc_convT_k2s2_fwd_split_h2_debug(const float* x, const float* w, const float* bias, float* y, void* ys, int ys_ctot, int ys_c0, int N, int C,
                                     int D, int H, int W, int K, unsigned* out_cell, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !w || !ys || !out_cell || !ws) { set_error("convT_k2s2_fwd_split_h2_debug: null pointer"); return NC_ERR_ARG; }
  if (!convT_s3x_supported(N, C, D, H, W, K) || ys_ctot % 8 || ys_c0 % 8 || ys_c0 < 0 || ys_c0 + K > ys_ctot) {
    set_error("convT_k2s2_fwd_split_h2_debug: shape not covered");
    return NC_ERR_SHAPE;
  }
  hipStream_t s = (hipStream_t)stream;
  if (int e = h2_zero_cells(out_cell, 1, s)) return e;
  // (the input bound is the one convT_fwd_split_h2 converts x with: an InstanceNorm + ReLU output)
  if (int e = convT_h2_bound(w, bias, C, K, sqrtf((float)((long)D * H * W)), out_cell, s)) return e;
  return convT_fwd_split_h2(x, w, bias, y, ys, ys_ctot, ys_c0, N, C, D, H, W, K, out_cell, ws, ws_bytes, s);
}

// the three-term (S3) output of the fp32 matrix-core kernel (convt.hip convT_fwd_s3; tests/test_gpu_convt.py): pointers and coverage
// (convT_fwd_s3_supported) are checked by the internal function, the slice [ys_c0, ys_c0 + K) of the ys_ctot channels here
int nc_convT_k2s2_fwd_s3_debug(const float* x, const float* w, const float* bias, float* y, void* ys, int ys_ctot, int ys_c0, int N, int C, int D,
                               int H, int W, int K, void* stream) {
  if (N < 1 || C < 1 || D < 1 || H < 1 || W < 1 || K < 1 || ys_ctot < 8 || ys_ctot % 8 || ys_c0 % 8 || ys_c0 < 0 || (long)ys_c0 + K > ys_ctot) {
    set_error("convT_k2s2_fwd_s3_debug: shape not covered");
    return NC_ERR_SHAPE;
  }
  return convT_fwd_s3(x, w, bias, y, ys, ys_ctot, ys_c0, N, C, D, H, W, K, stream);
}

// the one-pass inference tail of Unet_deconv (norm_act.hip k_in_act_tail; tests/test_gpu_norm.py): the channel limit is the internal function's
int nc_instnorm_relu_tail_sigmoid_debug(const float* x, const float* mean, const float* rstd, const float* w1, const float* b1, const float* w2,
                                        const float* b2, float* y, int C, long S, void* stream) {
  if (!x || !mean || !rstd || !w1 || !b1 || !w2 || !b2 || !y) { set_error("instnorm_relu_tail_sigmoid_debug: null pointer"); return NC_ERR_ARG; }
  if (C < 1 || S < 1) { set_error("instnorm_relu_tail_sigmoid_debug: bad shape"); return NC_ERR_SHAPE; }
  return instnorm_relu_tail_sigmoid(x, mean, rstd, w1, b1, w2, b2, y, C, S, (hipStream_t)stream);
}

}  // extern "C"
