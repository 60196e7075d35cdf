// Whole-network inference forward of Unet_deconv, the call behind diced inference (reference models/networks.py:512-538 via
// models/test_model.py:60-62).  Host code only: which kernels run, in which order, on which buffers.  Two forwards over one context:
//   two_term    every 3^3 layer on the two-term (H2) tap-stream kernel, the whole batch through every launch (the default)
//   one_sample  everything else -- three-term operands, the fp32 kernels, the VALU kernels -- one sample per pass
// A block is a convolution step (conv_h2 / conv_s3 / conv_f32; each leaves the raw output and its InstanceNorm statistics) and a finish step that
// normalises, applies the ReLU and writes the form the consumer takes (to_h2_pool / to_h2 / to_s3 / to_f32); every call site names both.
#include "common.hpp"
#include "unet_desc.hpp"

using namespace nc;

namespace {

struct UnetWs {
  size_t raw, cat1, a1, p1, cat2, a2, a2b, p2, b1, b2, t1, t2, mean, rstd, in_ws, conv_ws, total;
  size_t s_a1, s_cat1, s_a2, s_cat2, s_b1, s_b2;  // S3 (three-term bf16) forms of the convolution inputs, conv_split.hip
  size_t cells;  // H2 mode (nc_set_split_terms(2)): scale cells of the convolution inputs, h2.hip
  size_t stats;  // H2 mode: partial InstanceNorm sums written by the convolutions' own epilogues (conv_s3x.hip ST), largest layer
  size_t in_ws_bytes, conv_ws_bytes;
};
// NB samples per pass: the two-term (H2) forward runs a whole batch through every launch (round 6: three 140^3 cubes per call fill the
// persistent 256-workgroup launches of the 70^3 / 35^3 levels -- 1.64 rounds of tiles become 4.92 -- 5 % of the convolution time); the other
// forms walk the samples one by one through buffers of one sample (NB = 1).
UnetWs unet_ws(int S0, int S1, int S2, int NB = 1) {
  int d[3][3]; long Sl[3];
  u_level_dims(S0, S1, S2, d, Sl);
  const size_t S = (size_t)Sl[0] * NB, Sh = S / 8, Sq = S / 64;  // (per-batch element counts: every activation buffer holds NB samples)
  UnetWs u{};
  size_t off = 0;
  auto take = [&](size_t n) { size_t r = off; off += up64(n); return r; };
  u.raw = take(64 * S); u.cat1 = take(128 * S); u.a1 = take(64 * S); u.p1 = take(64 * Sh); u.cat2 = take(256 * Sh);
  u.a2 = take(128 * Sh); u.a2b = take(128 * Sh); u.p2 = take(128 * Sq); u.b1 = take(256 * Sq); u.b2 = take(256 * Sq);
  u.t1 = take(S); u.t2 = take(S); u.mean = take(256 * (size_t)NB); u.rstd = take(256 * (size_t)NB);
  u.in_ws_bytes = nc_instnorm_ws_bytes(256, Sl[0]);
  u.in_ws = take(u.in_ws_bytes / 4);
  // one sample's convolution workspace and the batch's epilogue sums, the largest of blocks 1 .. 9 (and the first block's own kernel's sums)
  size_t sb = 0;
  for (int i = 1; i < 10; ++i) {
    const UBlock& b = kUB[i];
    const int* e = d[b.lvl];
    const size_t cw = nc_conv_ws_bytes(1, b.C, e[0], e[1], e[2], b.K, 3, 3, 3, 1, 1), st = s3x_stats_bytes(NB, e[0], e[1], e[2], b.K, 3);
    if (cw > u.conv_ws_bytes) u.conv_ws_bytes = cw;
    if (st > sb) sb = st;
  }
  ConvDims d0;
  if (make_dims(d0, 1, 1, S0, S1, S2, 64, 3, 3, 3, 1, 1) && c1k3_stats_bytes(d0) > sb) sb = c1k3_stats_bytes(d0);
  u.conv_ws = take(u.conv_ws_bytes / 4 + 64);
  auto take3 = [&](size_t elems) { return take((elems * 6 + 3) / 4); };  // 6 bytes per element
  u.s_a1 = take3(64 * S); u.s_cat1 = take3(128 * S); u.s_a2 = take3(128 * Sh); u.s_cat2 = take3(256 * Sh);
  u.s_b1 = take3(256 * Sq); u.s_b2 = take3(256 * Sq);
  u.cells = take(64);
  u.stats = take(sb / 4 + 64);
  u.total = off;
  return u;
}

// H2 mode of the whole-network forward: every 3^3 layer must be one the tap-stream kernel covers, its packed weights must fit the workspace
bool unet_h2_ok(int S0, int S1, int S2, size_t conv_ws_bytes) {
  if (!sw::raw(sw::CONV_SPLIT) || !sw::raw(sw::S3_FUSE) || sw::get(sw::SPLIT_TERMS) == 3) return false;
  int d[3][3]; long Sl[3];
  u_level_dims(S0, S1, S2, d, Sl);
  size_t packed = 0;
  for (int i = 1; i < 10; ++i) {
    const UBlock& b = kUB[i];
    if (!s3x_supported(1, b.C, d[b.lvl][0], d[b.lvl][1], d[b.lvl][2], b.K, 3)) return false;
    if (s3x_packed_bytes(b.C, b.K, 3, 2) > packed) packed = s3x_packed_bytes(b.C, b.K, 3, 2);
  }
  return conv_ws_bytes >= 256 + packed + 256;
}

// samples per pass of the whole-network forward: the whole batch in the two-term mode (NC_INFER_BATCHED=0: one by one, A/B), else one
int unet_fwd_batch(int N, int S0, int S1, int S2) {
  return N > 1 && sw::raw(sw::INFER_BATCHED) && nc_unet_deconv_fwd_terms(S0, S1, S2) == 2 ? N : 1;
}

// the two transposed convolutions: block `from` -> ConvTranspose3d(C, K, 2, 2) `id` at level lvl -> the upper K channels of block `to`'s input
struct UUp { int id, from, to, C, K, lvl; };
constexpr UUp kUT[2] = {{10, 6, 7, 256, 128, 2}, {11, 8, 9, 128, 64, 1}};

// One call's context: parameters, workspace, level sizes, the stream; bn = samples per pass of every step below
struct Fwd {
  const float* P; UOff o;  // the parameter blob and its offsets
  float* W; UnetWs u;      // the workspace and its layout
  int d[3][3]; long S[3];
  void* stream; hipStream_t hs;
  int bn;
  bool epi;       // InstanceNorm sums from the convolutions' own epilogues (see conv_h2)
  bool s3in[10];  // block i runs on the split-operand kernels: its producer writes its input in operand form (see nc_unet_deconv_fwd)

  const float* w(int id) const { return P + o.w[id]; }
  const float* b(int id) const { return P + o.b[id]; }
  float* raw() const { return W + u.raw; }
  float* mean() const { return W + u.mean; }
  float* rstd() const { return W + u.rstd; }
  float* stats() const { return W + u.stats; }
  void* cws() const { return W + u.conv_ws; }
  unsigned* cells() const { return (unsigned*)(W + u.cells); }
  const int* dims(int i) const { return d[kUB[i].lvl]; }
  long vox(int i) const { return S[kUB[i].lvl]; }

  // ---- statistics of sample n of block i's raw output in a pass of their own (mean / rstd are [sample][channel])
  int stats_sample(int i, int n) const {
    const long K = kUB[i].K;
    return nc_instnorm_stats(raw() + n * K * vox(i), (int)K, vox(i), 1e-5f, mean() + n * K, rstd() + n * K, W + u.in_ws, u.in_ws_bytes, stream);
  }

  // ---- the convolution step, three forms: 3^3, pad 1, block i's input -> raw, then mean / rstd
  // Two-term: in3 is an H2 tensor (two fp16 terms of the tensor times a power of two, h2.hip) of bn samples; in_a / in_b: the cells of the
  // input's channels [0, split_c) / [split_c, C) (a concatenation; in_b NULL: one cell).
  // Epilogue statistics (default; NC_EPI_STATS=0 / nc_set_epi_stats(0): off): the two-term convolution leaves the partial InstanceNorm sums of
  // its output itself (conv_s3x.hip, ST) and k_in_stats' pass over the raw output goes away: -1.8 % per 140^3 cube, mean / rstd equal to 4e-8
  int conv_h2_launch(int i, const void* in3, const unsigned* in_a, const unsigned* in_b, int split_c) const {
    const UBlock& k = kUB[i];
    const int* e = dims(i);
    ConvDims cd;
    make_dims(cd, bn, k.C, e[0], e[1], e[2], k.K, 3, 3, 3, 1, 1);
    {
      ProfScope ps(0, kPathSplit, cd, 0, hs);
      NC_TRY(conv_s3x_h2(in3, in_a, in_b, in_b ? split_c : k.C, w(i), b(i), raw(), bn, k.C, e[0], e[1], e[2], k.K, 3, (long)k.C * 27, 27, 0,
                         (unsigned*)cws(), (char*)cws() + 256, hs, nullptr, epi ? stats() : nullptr));
    }
    return epi ? s3x_stats_finalize(stats(), b(i), bn, e[0], e[1], e[2], k.K, 3, 1e-5f, mean(), rstd(), hs) : NC_OK;
  }
  int conv_h2(int i, const void* in3, const unsigned* in_a, const unsigned* in_b = nullptr, int split_c = 0) const {
    NC_TRY(conv_h2_launch(i, in3, in_a, in_b, split_c));
    for (int n = 0; !epi && n < bn; ++n) NC_TRY(stats_sample(i, n));
    return NC_OK;
  }
  // Three-term: in3 is the S3 tensor of ONE sample
  int conv_s3(int i, const void* in3) const {
    const UBlock& k = kUB[i];
    const int* e = dims(i);
    ConvDims cd;
    make_dims(cd, 1, k.C, e[0], e[1], e[2], k.K, 3, 3, 3, 1, 1);
    {
      ProfScope ps(0, kPathSplit, cd, 0, hs);
      NC_TRY(conv_fwd_s3(nullptr, in3, w(i), b(i), raw(), cd, cws(), u.conv_ws_bytes, hs));
    }
    return stats_sample(i, 0);
  }
  // From fp32, whatever nc_conv_fwd dispatches to, one sample per launch with its statistics behind it
  int conv_f32(int i, const float* in) const {
    const UBlock& k = kUB[i];
    const int* e = dims(i);
    const long Sl = vox(i);
    ConvDims d1;
    // the first block: the one-channel kernel leaves its InstanceNorm sums too (conv_c1k3.hip ST) -- one sample per launch, then ONE
    // normalise + convert pass over the batch
    const bool c1k3 = epi && k.C == 1 && !sw::raw(sw::FORCE_DIRECT) && make_dims(d1, 1, k.C, e[0], e[1], e[2], k.K, 3, 3, 3, 1, 1) && c1k3_stats_bytes(d1);
    for (int n = 0; n < bn; ++n) {
      const float* xn = in + n * k.C * Sl;
      float* yn = raw() + n * k.K * Sl;
      if (c1k3) {
        NC_TRY(conv_fwd_c1k3(xn, w(i), b(i), yn, d1, hs, stats()));
        NC_TRY(c1k3_stats_finalize(stats(), b(i), d1, 1e-5f, mean() + n * k.K, rstd() + n * k.K, hs));
      } else {
        NC_TRY(nc_conv_fwd(xn, w(i), b(i), yn, 1, k.C, e[0], e[1], e[2], k.K, 3, 3, 3, 1, 1, cws(), u.conv_ws_bytes, stream));
        NC_TRY(stats_sample(i, n));
      }
    }
    return NC_OK;
  }

  // ---- the finish step, four forms: normalise + ReLU of raw, written as ...
  // ... channels [0, K) of the ctot-channel H2 tensor out3 (cell: the bound sqrt(voxels) of an InstanceNorm output), bn samples
  int to_h2(int i, void* out3, int ctot) const {
    const long K = kUB[i].K, Sl = vox(i);
    return act_split2h(raw(), mean(), rstd(), 0.f, nullptr, K * Sl, out3, bn, (int)K, Sl, ctot, 0, sqrtf((float)Sl), nullptr, nullptr, hs);
  }
  // ... the same and, in the same pass, its 2 x 2 x 2 max-pool as a dense H2 tensor (same cell)
  int to_h2_pool(int i, void* out3, int ctot, void* pooled) const {
    const int* e = dims(i);
    return act_split2h_pool(raw(), mean(), rstd(), 0.f, out3, pooled, bn, kUB[i].K, e[0], e[1], e[2], ctot, 0, sqrtf((float)vox(i)), nullptr, hs);
  }
  // ... fp32 `out` (nullable) and channels [0, K) of the ctot-channel S3 tensor out3, ONE sample
  int to_s3(int i, float* out, void* out3, int ctot) const {
    const long K = kUB[i].K, Sl = vox(i);
    return act_split3(raw(), mean(), rstd(), 0.f, out, K * Sl, out3, 1, (int)K, Sl, ctot, 0, hs);
  }
  // ... fp32, ONE sample
  int to_f32(int i, float* out) const { return nc_instnorm_act_fwd(raw(), mean(), rstd(), 0.f, out, kUB[i].K, vox(i), stream); }

  int up_two_term(const UUp& t, void* src_op, float* src_f32, float* cat_f32, void* cat_op) const;
  int up_one_sample(const UUp& t, void* src_op, float* src_f32, float* cat_f32, void* cat_op) const;
  int two_term(const float* xn, float* yn) const;
  int one_sample(const float* xn, float* yn) const;
};

// Two-term: normalise block t.from, the transposed convolution t.id, its output as the upper K channels of the H2 concatenation cat_op with a cell
// of its own (cells 3, 4).  On the matrix cores (convt_s3.hip) where they cover the layer, else the fp32 kernel.  NC_CONVT_H2 (default): H2 in (the
// block's output, bound sqrt(voxels)), H2 out -- the kernel writes the H2 form of its half itself, with a BOUND for its power of two (every output
// voxel gets one tap per input channel); the ratio of the two halves' powers of two goes into the consumer's weights.  NC_CONVT_H2=0 (A/B) and
// the fp32 kernel: a three-term / fp32 input, the fp32 output as a dense [bn][K] tensor in the upper half of cat_f32, measured and converted.
// (In those two arms the block in front is normalised for ONE sample whatever bn is: tests/test_gpu_unet_fwd_arms.py.)
int Fwd::up_two_term(const UUp& t, void* src_op, float* src_f32, float* cat_f32, void* cat_op) const {
  const int* e = d[t.lvl];
  const long Si = S[t.lvl], So = S[t.lvl - 1];
  unsigned* cell = cells() + (t.id == 10 ? 3 : 4);
  const bool mc = convT_s3x_supported(bn, t.C, e[0], e[1], e[2], t.K) && u.conv_ws_bytes >= convT_s3x_ws_bytes(t.C, t.K);
  if (mc && sw::raw(sw::CONVT_H2) != 0) {
    NC_TRY(to_h2(t.from, src_op, t.C));
    NC_TRY(convT_h2_bound(w(t.id), b(t.id), t.C, t.K, sqrtf((float)Si), cell, hs));
    return convT_fwd_s3x(src_op, w(t.id), b(t.id), nullptr, cat_op, 2 * t.K, t.K, bn, t.C, e[0], e[1], e[2], t.K, cws(), u.conv_ws_bytes, hs, cell,
                         cells() + t.lvl);
  }
  float* up = cat_f32 + t.K * So * bn;
  if (mc) {
    NC_TRY(to_s3(t.from, nullptr, src_op, t.C));
    NC_TRY(convT_fwd_s3x(src_op, w(t.id), b(t.id), up, nullptr, t.K, 0, bn, t.C, e[0], e[1], e[2], t.K, cws(), u.conv_ws_bytes, hs));
  } else {
    NC_TRY(to_f32(t.from, src_f32));
    NC_TRY(nc_convT_k2s2_fwd(src_f32, w(t.id), b(t.id), up, bn, t.C, e[0], e[1], e[2], t.K, stream));
  }
  NC_TRY(h2_absmax(up, t.K * So * bn, cell, hs));
  return split2h_into(up, t.K * So, cat_op, bn, t.K, So, 2 * t.K, t.K, cell, hs);
}

// The two-term forward of bn samples: every 3^3 layer on k_conv_s3x<3, NCB, 2>.  Every activation buffer is [bn][channels][voxels], the pooled /
// half-resolution offsets scale with bn.  The outputs of InstanceNorm + ReLU are bounded by sqrt(voxels) by construction (cells 0..2, one per
// level, set by the caller).
int Fwd::two_term(const float* xn, float* yn) const {
  const unsigned *c0 = cells(), *c1 = cells() + 1, *c2 = cells() + 2, *c3 = cells() + 3, *c4 = cells() + 4;
  NC_TRY(h2_zero_cells(cells() + 3, 2, hs));
  NC_TRY(conv_f32(0, xn));
  NC_TRY(to_h2(0, W + u.s_a1, 64));
  // The max-pools work on the H2 tensors themselves (the winner's two terms are the pooled element's terms, same cell: h2.hip), in the pass
  // that converts: blocks 1 and 3 write NO fp32 activation.  The pooled tensors go into slots nobody needs yet (the upper half of s_cat2 until
  // the transposed convolution's output arrives; s_b2 until block 5 writes it).
  void* p1h = W + u.s_cat2 + 128 * S[1] * bn;
  NC_TRY(conv_h2(1, W + u.s_a1, c0));
  NC_TRY(to_h2_pool(1, W + u.s_cat1, 128, p1h));
  NC_TRY(conv_h2(2, p1h, c0));
  NC_TRY(to_h2(2, W + u.s_a2, 128));
  NC_TRY(conv_h2(3, W + u.s_a2, c1));
  NC_TRY(to_h2_pool(3, W + u.s_cat2, 256, W + u.s_b2));
  NC_TRY(conv_h2(4, W + u.s_b2, c1));
  NC_TRY(to_h2(4, W + u.s_b1, 256));
  NC_TRY(conv_h2(5, W + u.s_b1, c2));
  NC_TRY(to_h2(5, W + u.s_b2, 256));
  NC_TRY(conv_h2(6, W + u.s_b2, c2));
  NC_TRY(up_two_term(kUT[0], W + u.s_b1, W + u.b1, W + u.cat2, W + u.s_cat2));
  NC_TRY(conv_h2(7, W + u.s_cat2, c1, c3, 128));
  NC_TRY(to_h2(7, W + u.s_a2, 128));
  NC_TRY(conv_h2(8, W + u.s_a2, c1));
  NC_TRY(up_two_term(kUT[1], W + u.s_cat2, W + u.a2b, W + u.cat1, W + u.s_cat1));
  // the last block's normalisation, the two pointwise layers and the sigmoid in one pass over its raw output
  NC_TRY(conv_h2_launch(9, W + u.s_cat1, c0, c4, 64));
  for (int n = 0; n < bn; ++n) {  // (the fused tail is a per-sample pass: 0.13 ms per 140^3 cube)
    if (!epi) NC_TRY(stats_sample(9, n));
    NC_TRY(instnorm_relu_tail_sigmoid(raw() + n * 64 * S[0], mean() + n * 64, rstd() + n * 64, w(12), b(12), w(13), b(13), yn + n * S[0], 64, S[0], hs));
  }
  return NC_OK;
}

// One sample: normalise block t.from, the transposed convolution t.id, its output as the upper K channels of block t.to's input.  On the bf16
// matrix cores (convt_s3.hip; with the split-operand kernels switched on) it takes its input in S3 form: the block in front leaves its
// output ONLY in that form (in a slot that is free by then: s_b1 after block 5, s_cat2 after block 7) -- or, with the fusion switched off, in
// fp32 and a separate pass converts it (the same bits) -- and it writes the S3 form of the upper half of the concatenation itself when the
// next convolution takes it (in the inference forward nothing else reads it, so no fp32 copy is written), fp32 otherwise.
int Fwd::up_one_sample(const UUp& t, void* src_op, float* src_f32, float* cat_f32, void* cat_op) const {
  const int* e = d[t.lvl];
  const long Si = S[t.lvl], So = S[t.lvl - 1];
  const bool fuse = sw::raw(sw::S3_FUSE) != 0, op = s3in[t.to];
  const bool mc = sw::raw(sw::CONV_SPLIT) && convT_s3x_supported(1, t.C, e[0], e[1], e[2], t.K) && u.conv_ws_bytes >= convT_s3x_ws_bytes(t.C, t.K);
  float* up = cat_f32 + t.K * So;
  NC_TRY(mc && fuse ? to_s3(t.from, nullptr, src_op, t.C) : to_f32(t.from, src_f32));
  if (mc) {
    if (!fuse) NC_TRY(split3_into(src_f32, t.C * Si, src_op, 1, t.C, Si, t.C, 0, hs));
    return convT_fwd_s3x(src_op, w(t.id), b(t.id), op ? nullptr : up, op ? cat_op : nullptr, 2 * t.K, t.K, 1, t.C, e[0], e[1], e[2], t.K, cws(),
                         u.conv_ws_bytes, hs);
  }
  // convt.hip's matrix-core kernel (128 input channels: t_conv1) writes the consumer's operand form itself; the fp32 half is not written at all
  if (op && convT_fwd_s3_supported(1, t.C, e[0], e[1], e[2], t.K))
    return convT_fwd_s3(src_f32, w(t.id), b(t.id), nullptr, cat_op, 2 * t.K, t.K, 1, t.C, e[0], e[1], e[2], t.K, stream);
  NC_TRY(nc_convT_k2s2_fwd(src_f32, w(t.id), b(t.id), up, 1, t.C, e[0], e[1], e[2], t.K, stream));
  return op ? split3_into(up, t.K * So, cat_op, 1, t.K, So, 2 * t.K, t.K, hs) : NC_OK;
}

// The forward of one sample in every other form: a block takes its input in S3 form when it runs on the split-operand kernels (s3in) and
// its producer is a normalisation pass or a transposed convolution -- the blocks behind a max-pool (2, 4) and the first one convert for
// themselves inside nc_conv_fwd.
int Fwd::one_sample(const float* xn, float* yn) const {
  const int *e = d[0], *h = d[1];
  NC_TRY(conv_f32(0, xn));
  NC_TRY(s3in[1] ? to_s3(0, nullptr, W + u.s_a1, 64) : to_f32(0, W + u.a1));
  NC_TRY(s3in[1] ? conv_s3(1, W + u.s_a1) : conv_f32(1, W + u.a1));
  NC_TRY(s3in[9] ? to_s3(1, W + u.cat1, W + u.s_cat1, 128) : to_f32(1, W + u.cat1));
  NC_TRY(nc_maxpool2_fwd(W + u.cat1, W + u.p1, 64, e[0], e[1], e[2], stream));
  NC_TRY(conv_f32(2, W + u.p1));
  NC_TRY(s3in[3] ? to_s3(2, nullptr, W + u.s_a2, 128) : to_f32(2, W + u.a2));
  NC_TRY(s3in[3] ? conv_s3(3, W + u.s_a2) : conv_f32(3, W + u.a2));
  NC_TRY(s3in[7] ? to_s3(3, W + u.cat2, W + u.s_cat2, 256) : to_f32(3, W + u.cat2));
  NC_TRY(nc_maxpool2_fwd(W + u.cat2, W + u.p2, 128, h[0], h[1], h[2], stream));
  NC_TRY(conv_f32(4, W + u.p2));
  NC_TRY(s3in[5] ? to_s3(4, nullptr, W + u.s_b1, 256) : to_f32(4, W + u.b1));
  NC_TRY(s3in[5] ? conv_s3(5, W + u.s_b1) : conv_f32(5, W + u.b1));
  NC_TRY(s3in[6] ? to_s3(5, nullptr, W + u.s_b2, 256) : to_f32(5, W + u.b2));
  NC_TRY(s3in[6] ? conv_s3(6, W + u.s_b2) : conv_f32(6, W + u.b2));
  NC_TRY(up_one_sample(kUT[0], W + u.s_b1, W + u.b1, W + u.cat2, W + u.s_cat2));
  NC_TRY(s3in[7] ? conv_s3(7, W + u.s_cat2) : conv_f32(7, W + u.cat2));
  NC_TRY(s3in[8] ? to_s3(7, nullptr, W + u.s_a2, 128) : to_f32(7, W + u.a2));
  NC_TRY(s3in[8] ? conv_s3(8, W + u.s_a2) : conv_f32(8, W + u.a2));
  NC_TRY(up_one_sample(kUT[1], W + u.s_cat2, W + u.a2b, W + u.cat1, W + u.s_cat1));
  NC_TRY(s3in[9] ? conv_s3(9, W + u.s_cat1) : conv_f32(9, W + u.cat1));
  NC_TRY(to_f32(9, W + u.a1));
  NC_TRY(nc_conv_fwd(W + u.a1, w(12), b(12), W + u.t1, 1, 64, e[0], e[1], e[2], 1, 1, 1, 1, 1, 0, cws(), u.conv_ws_bytes, stream));
  NC_TRY(nc_conv_fwd(W + u.t1, w(13), b(13), W + u.t2, 1, 1, e[0], e[1], e[2], 1, 1, 1, 1, 1, 0, cws(), u.conv_ws_bytes, stream));
  return nc_sigmoid_fwd(W + u.t2, yn, S[0], stream);
}

}  // namespace

extern "C" {

int nc_unet_deconv_fwd_terms(int S0, int S1, int S2) {
  if (!u_edges_ok(S0, S1, S2)) return 0;
  // (asked of the full-resolution and of the quarter-resolution level)
  const bool f = conv_fwd_on_split(1, 64, S0, S1, S2, 64, 3) && conv_fwd_on_split(1, 256, S0 / 4, S1 / 4, S2 / 4, 256, 3);
  return f && unet_h2_ok(S0, S1, S2, unet_ws(S0, S1, S2).conv_ws_bytes) ? 2 : 3;
}

size_t nc_unet_deconv_fwd_ws_bytes(int N, int S0, int S1, int S2) {
  if (N < 1 || !u_edges_ok(S0, S1, S2)) return 0;
  return unet_ws(S0, S1, S2, unet_fwd_batch(N, S0, S1, S2)).total * sizeof(float);
}

// Parameter blob = state-dict order (unet_desc.hpp), fp32, back to back
int nc_unet_deconv_fwd(const float* params, const float* x, float* y, int N, int S0, int S1, int S2, void* ws, size_t ws_bytes, void* stream) {
  NetworkScope net_scope;
  if (!params || !x || !y) { set_error("unet_deconv_fwd: null pointer"); return NC_ERR_ARG; }
  if (N < 1 || !u_edges_ok(S0, S1, S2)) {
    set_error("unet_deconv_fwd: every edge must be a positive multiple of 4 (got %d,%d,%d): MaxPool3d floors and the "
              "skip concat would not line up (reference networks.py:526,531)", S0, S1, S2);
    return NC_ERR_SHAPE;
  }
  const int NB = unet_fwd_batch(N, S0, S1, S2);  // NB = N: the two-term forward takes the whole batch through every launch
  Fwd f{};
  f.u = unet_ws(S0, S1, S2, NB);
  if (!ws || ws_bytes < f.u.total * sizeof(float)) { set_error("unet_deconv_fwd: workspace too small"); return NC_ERR_WS; }
  f.P = params;
  f.o = u_offsets();
  f.W = (float*)ws;
  u_level_dims(S0, S1, S2, f.d, f.S);
  f.stream = stream;
  f.hs = (hipStream_t)stream;
  f.epi = sw::raw(sw::EPI_STATS) != 0;
  // Does block i's 3^3 convolution run on the split-operand kernels?  Then its input is wanted in operand form, and the layer in front writes
  // that form from its normalisation pass (k_act_split3 / k_act_split2h) instead of a separate conversion pass.
  bool all = true;
  for (int i = 1; i < 10; ++i) {
    const int* e = f.dims(i);
    f.s3in[i] = sw::raw(sw::S3_FUSE) && conv_fwd_on_split(1, kUB[i].C, e[0], e[1], e[2], kUB[i].K, 3);
    all = all && f.s3in[i];
  }
  const bool use_h2 = all && unet_h2_ok(S0, S1, S2, f.u.conv_ws_bytes);
  if (use_h2)
    for (int l = 0; l < 3; ++l) NC_TRY(h2_set_cell(f.cells() + l, sqrtf((float)f.S[l]), f.hs));
  f.bn = use_h2 ? NB : 1;
  for (int n = 0; n < N; n += f.bn) NC_TRY(use_h2 ? f.two_term(x + n * f.S[0], y + n * f.S[0]) : f.one_sample(x + n * f.S[0], y + n * f.S[0]));
  return NC_OK;
}

}  // extern "C"
