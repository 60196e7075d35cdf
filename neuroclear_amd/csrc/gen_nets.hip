// Whole-network TRAINING entry points of the two generators: one C call per direction, as nets.hip does for the PatchGAN.
//   Unet_deconv          reference models/networks.py:478-538   (forward at :512-538; backward = autograd of it, driven
//                        by loss_G.backward() at models/axial_to_lateral_gan_apollo_model.py:283)
//   DeepLinearGenerator  reference models/networks.py:893-917   (bias-free linear chain 7^3 / 5^3 / 3^3 / 1 / 1 / 1)
// Same kernels in the same order as the layer-by-layer Python path (neuroclear_amd/models/networks.py), so outputs and
// gradients are bit-identical to it (DeepLinearGenerator: with nc_set_dl_collapse(0); its default evaluation exploits the chain's linearity,
// see "the collapsed tail" below); what the single call removes is ~60 autograd nodes per direction on the host, the
// torch.cat copies of the two skip connections (the producers write straight into halves of the concat buffers) and the
// at::native adds that merge the two gradients of a skip tensor (the max-pool backward adds the skip gradient itself).
//
// Parameter blob = the tensors in state-dict order, packed back to back.  `saved` receives what the
// backward needs (raw conv outputs, activations, InstanceNorm statistics); sizes from the *_saved_floats queries.


#include "common.hpp"
#include "unet_desc.hpp"

using namespace nc;

namespace {

// `kept`: what a training forward left in (or out of) its `saved` buffer.  A host word that the forward RETURNS and the caller hands to the backward
// of the same buffer: every decision behind it (library switches, shape coverage) is host state, so the word travels with the autograd context
// that owns `saved`, not with a table keyed by its address.  The backward decides from these bits, never from the switches of forward time.
// Unet_deconv: u_fwd_forms composes the word and u_bwd_forms reads it.  DeepLinearGenerator: the operand bits and its own flags (kKeptCollapsed ..).
struct Kept {
  unsigned w = 0;
  // bit i (1 .. 9): layer i's input in split-operand form is in saved (xs3[i]) -- its weight gradient takes that instead of converting x again
  bool operand(int i) const { return bit(i); }
  // bit 16 + i: that copy is a two-term (H2) tensor -- a backward under another setting of nc_set_split_terms ignores it
  bool operand_h2(int i) const { return bit(16 + i); }
  // ... so the kept copy is usable now: it exists, in the form the layer has under the switches of this call
  bool operand_usable(int i, bool now_h2) const { return operand(i) && operand_h2(i) == now_h2; }
  // bits 10 .. 14 (nc_set_unet_lean): the fp32 input of block 1 / 3 / 5 / 6 / 8 (a1, a2, b1, b2, e2a) was not written -- only that block's H2 operand
  bool lean_input(int consumer) const { return lean_bit(consumer) && bit(lean_bit(consumer)); }
  // bit 15 (nc_set_unet_wprep; w_prep.hip): cells and packed weights of the two-term blocks, forward AND data-gradient form, are in saved
  // (UPlan::wprep), from one batched pass at the forward's start -- the data gradients see the weights of FORWARD time
  bool wprep() const { return bit(15); }
  // bit 26 (the only bit nc_set_in_bwd_fold moves; norm_act.hip PoolGrad): one winner byte per pooled element of both max-pools is in saved (UPlan::parg)
  bool pool_arg() const { return bit(26); }
  // bit 27: e1 (block 9's output) was not written -- one_by_one ran on the two flat 1 x 1 kernels (conv_1x1.hip), which normalise raw[9] as they read
  bool lean_e1() const { return bit(27); }
  // bits 28, 29: the fp32 upper half of cat1 / cat2 was not written -- the transposed convolution wrote the H2 half of block 9 / 7's operand alone
  bool lean_up(int level) const { return bit(27 + level); }
  // bits 30, 31: block 1 / 3 normalises, converts and POOLS in one pass (h2.hip k_act_split2h_pool) -- the fp32 lower half of cat1 / cat2 was not
  // written IF pool_arg() too: the pass is taken when the forward writes winner bytes, and only then
  bool lean_lo(int level) const { return bit(29 + level); }
  bool has(unsigned flags) const { return (w & flags) == flags; }  // (the deep-linear flags below)

  void set_operand(int i, bool h2) { put(i); if (h2) put(16 + i); }
  void set_lean_input(int consumer) { if (lean_bit(consumer)) put(lean_bit(consumer)); }
  void set_wprep() { put(15); }
  void set_pool_arg() { put(26); }
  void set_lean_e1() { put(27); }
  void set_lean_up(int level) { put(27 + level); }
  void set_lean_lo(int level) { put(29 + level); }
  void set(unsigned flags) { w |= flags; }

 private:
  bool bit(int b) const { return (w >> b) & 1; }
  void put(int b) { w |= 1u << b; }
  static int lean_bit(int c) { return c == 1 ? 10 : c == 3 ? 11 : c == 5 ? 12 : c == 6 ? 13 : c == 8 ? 14 : 0; }  // 0: not a lean input
};

size_t s3_floats(size_t elems) { return up64((elems * 6 + 3) / 4); }
// are the layer's operands in the two-term form under the switches of now (nc_set_split_terms(2); conv_split.hip s3_layer_h2)?
bool layer_h2_now(int N, int C, const int* d, int K, int k) {
  ConvDims cd;
  return make_dims(cd, N, C, d[0], d[1], d[2], K, k, k, k, 1, k / 2) && conv_layer_h2(cd);
}

// ---- Unet_deconv ---------------------------------------------------------------------------------------------------
// segment 2 (i - 1) + form of block i's prepared weights (form 0: forward, 1: data gradient); all 18 have their place in the region whichever of
// them a call prepares
void wprep_segs(WPrepSeg (&sg)[18]) {
  for (int i = 1; i < 10; ++i) {
    sg[2 * (i - 1)] = WPrepSeg{nullptr, kUB[i].C, kUB[i].K, 0, 0u, -1, nullptr};
    sg[2 * (i - 1) + 1] = WPrepSeg{nullptr, kUB[i].K, kUB[i].C, 1, 0u, -1, nullptr};
  }
}
unsigned f32_bits(float f) { unsigned b; __builtin_memcpy(&b, &f, 4); return b; }

struct UPlan {
  int N, d[3][3];      // spatial size per level
  long S[3];           // voxels per level
  // saved (floats): activations, raw conv outputs, statistics
  size_t a1, cat1, p1, a2, cat2, p2, b1, b2, b3, e2a, e2b, e1, t1, raw[10], mean[10], rstd[10], saved;
  size_t xs3[10];      // the split-operand copy of block i's input (i >= 1), see Kept::operand
  size_t wprep;        // the prepared weights (w_prep.hip wprep_run's region), see Kept::wprep
  size_t parg[2];      // the winner bytes of pool 1 (behind block 1) and pool 2 (behind block 3), see Kept::pool_arg
  // backward scratch (floats)
  size_t G1, G2, G3, H1, H2, H3, Q1, Q2, s1, s2, T, grads;
  size_t conv_ws, in_ws, convT_ws;  // bytes
};

bool u_plan(UPlan& p, int N, int S0, int S1, int S2) {
  if (N < 1 || !u_edges_ok(S0, S1, S2)) return false;
  p = UPlan{};
  p.N = N;
  u_level_dims(S0, S1, S2, p.d, p.S);
  const size_t n = (size_t)N, S = (size_t)p.S[0], Sh = (size_t)p.S[1], Sq = (size_t)p.S[2];
  size_t off = 0;
  auto take = [&](size_t k) { size_t r = off; off += up64(k); return r; };
  p.a1 = take(n * 64 * S); p.cat1 = take(n * 128 * S); p.p1 = take(n * 64 * Sh); p.a2 = take(n * 128 * Sh);
  p.cat2 = take(n * 256 * Sh); p.p2 = take(n * 128 * Sq); p.b1 = take(n * 256 * Sq); p.b2 = take(n * 256 * Sq);
  p.b3 = take(n * 256 * Sq); p.e2a = take(n * 128 * Sh); p.e2b = take(n * 128 * Sh); p.e1 = take(n * 64 * S);
  p.t1 = take(n * S);
  for (int i = 0; i < 10; ++i) {
    p.raw[i] = take(n * kUB[i].K * (size_t)p.S[kUB[i].lvl]);
    p.mean[i] = take(n * kUB[i].K);
    p.rstd[i] = take(n * kUB[i].K);
  }
  for (int i = 1; i < 10; ++i) { p.xs3[i] = off; off += s3_floats(n * kUB[i].C * (size_t)p.S[kUB[i].lvl]); }
  {
    WPrepSeg sg[18];
    wprep_segs(sg);
    p.wprep = off;
    off += up64((wprep_bytes(sg, 18) + 3) / 4);
  }
  p.parg[0] = off; off += up64((n * 64 * Sh + 3) / 4);
  p.parg[1] = off; off += up64((n * 128 * Sq + 3) / 4);
  p.saved = off;
  off = 0;
  p.G1 = take(n * 64 * S); p.G2 = take(n * 64 * S); p.G3 = take(n * 128 * S);
  p.H1 = take(n * 128 * Sh); p.H2 = take(n * 128 * Sh); p.H3 = take(n * 256 * Sh);
  p.Q1 = take(n * 256 * Sq); p.Q2 = take(n * 256 * Sq); p.s1 = take(n * S); p.s2 = take(n * S);
  p.T = take(n * 64 * S);  // dense copy of a concat half's gradient when N > 1
  p.grads = off;
  auto upd = [&](int C, int K, int l, int k) {
    const size_t b = nc_conv_ws_bytes(N, C, p.d[l][0], p.d[l][1], p.d[l][2], K, k, k, k, 1, k / 2);
    if (b > p.conv_ws) p.conv_ws = b;
  };
  for (int i = 0; i < 10; ++i) upd(kUB[i].C, kUB[i].K, kUB[i].lvl, 3);
  upd(64, 1, 0, 1); upd(1, 1, 0, 1);
  p.in_ws = nc_instnorm_bwd_dbias_ws_bytes(N * 256, (long)S);
  for (int i = 1; i < 10; ++i) {  // the same region holds the partial sums of a block whose convolution takes its InstanceNorm statistics itself
    const size_t b = s3x_stats_bytes(N, p.d[kUB[i].lvl][0], p.d[kUB[i].lvl][1], p.d[kUB[i].lvl][2], kUB[i].K, 3);
    if (b > p.in_ws) p.in_ws = b;
  }
  p.convT_ws = nc_convT_ws_bytes(N, 256, p.d[2][0], p.d[2][1], p.d[2][2], 128);
  const size_t c2 = nc_convT_ws_bytes(N, 128, p.d[1][0], p.d[1][1], p.d[1][2], 64);
  if (c2 > p.convT_ws) p.convT_ws = c2;
  return true;
}

// dst[n][0..C) <- src[n][c0..c0+C) of a [N][Ctot][S] tensor (dense result); N == 1 needs no copy
int gather_half(const float* src, float* dst, int N, int Ctot, int c0, int C, long S, hipStream_t s) {
  if (hipMemcpy2DAsync(dst, (size_t)C * S * 4, src + (size_t)c0 * S, (size_t)Ctot * S * 4, (size_t)C * S * 4, N,
                       hipMemcpyDeviceToDevice, s) != hipSuccess) {
    set_error("gather_half: hipMemcpy2DAsync failed");
    return NC_ERR_HIP;
  }
  return NC_OK;
}

size_t u_ws_bytes(const UPlan& p, bool bwd) {
  return align256(p.conv_ws) + align256(p.in_ws) + align256(p.convT_ws) + (bwd ? p.grads * sizeof(float) : 0) + 256;
}

// The two skip levels.  Level L (1, 2): block `lo` writes the lower K channels of the concat buffer `cat` (resolution level L - 1) and is pooled into
// `pooled`; transposed convolution `tw` (parameter id) takes `tin` (2 K channels, level L) to the upper K channels; block `cons` reads the concat.
struct ULevel { int lo, cons, tw, K; size_t UPlan::*cat, UPlan::*pooled, UPlan::*tin; };
constexpr ULevel kUL[3] = {{}, {1, 9, 11, 64, &UPlan::cat1, &UPlan::p1, &UPlan::e2b}, {3, 7, 10, 128, &UPlan::cat2, &UPlan::p2, &UPlan::b3}};

// EVERY FORM OF THE FORWARD, decided before its first launch (all of it host state).  The forward reads these fields and launches.
// use: the block runs forward and weight gradient on the split-operand kernels, NC_S3_TRAIN_FUSE on: its input is wanted in operand form.  pre: the
//   PRODUCER of that input (the block in front's normalisation pass, the transposed convolution) writes it straight into xs3[i]; a block behind a
//   max-pool (2, 4), or any block with the fusion off, converts inside conv_fwd_keep.
// lean (nc_set_unet_lean): fp32 tensors that only a fallback path reads are not written -- behind two-term blocks only.  Kept says which.
enum CtArm { kCtPlain, kCtSplit, kCtH2, kCtS3 };
struct UFwdForms {
  bool use[10], h2l[10], pre[10];  // h2l: the block's operands in the two-term form
  bool epi[10];                    // the convolution's epilogue leaves the partial InstanceNorm sums (nc_set_epi_stats(2); conv_s3x.hip ST)
  ConvDims cd[10];
  // the transposed convolution of level L: ct on the bf16 matrix cores from an S3 copy of its input (convt_s3.hip; the layer-by-layer path makes
  // the same choice), cth writing the H2 half of the consumer's operand itself, its power of two from a BOUND -- nothing measured (NC_CONVT_H2=0:
  // fp32 output, measured and converted); ct_s3 writing the three-term half itself.  Level 1 alone has an arm for that without ct (convT_fwd_s3).
  bool ct[3], cth[3], ct_s3[3];
  bool bound[3];         // the prepared-weights pass leaves cth's bound in the consumer's second cell
  bool lean, pool_arg;   // pool_arg: the pools also write their winner bytes
  bool pool_in_norm[3];  // block lo of level L normalises, converts and pools in one pass: no full-resolution fp32, no pool launch
  bool tail_flat;        // no e1: block 9 stops at its statistics and one_by_one's flat kernel normalises raw[9] as it reads it
  bool seg[18];          // the prepared-weight segments of this call (wprep_segs' numbering)
  Kept kept;
  CtArm arm(int L) const { return cth[L] ? kCtH2 : ct[L] ? kCtSplit : ct_s3[L] ? kCtS3 : kCtPlain; }
};

UFwdForms u_fwd_forms(const UPlan& p) {
  UFwdForms f{};
  const int N = p.N;
  const bool fuse_on = sw::raw(sw::S3_TRAIN_FUSE) != 0, ct_h2 = sw::raw(sw::CONVT_H2) != 0, wprep = sw::raw(sw::UNET_WPREP) != 0;
  const bool epi_on = sw::raw(sw::EPI_STATS) == 2;  // an option, not the default (no measurable gain in the training step)
  f.lean = sw::raw(sw::UNET_LEAN) != 0;
  f.pool_arg = sw::get(sw::IN_BWD_FOLD) != 0;
  if (f.pool_arg) f.kept.set_pool_arg();
  for (int i = 0; i < 10; ++i) {
    const UBlock& b = kUB[i];
    const int* d = p.d[b.lvl];
    const bool keep = i >= 1 && conv_keep_supported(N, b.C, d[0], d[1], d[2], b.K, 3);  // (conv_fwd_keep's *kept)
    const bool h2 = make_dims(f.cd[i], N, b.C, d[0], d[1], d[2], b.K, 3, 3, 3, 1, 1) && keep && conv_layer_h2(f.cd[i]);
    f.use[i] = fuse_on && keep;
    f.h2l[i] = f.use[i] && h2;
    f.pre[i] = f.use[i] && i != 2 && i != 4;
    const size_t sb = f.pre[i] && f.h2l[i] && epi_on ? s3x_stats_bytes(N, d[0], d[1], d[2], b.K, 3) : 0;
    f.epi[i] = sb && sb <= p.in_ws;
    if (keep) f.kept.set_operand(i, h2);
    if (f.lean && f.h2l[i]) f.kept.set_lean_input(i);  // (the block in front writes no fp32 output: the backward takes the H2 copy)
    if (wprep && f.h2l[i]) { f.seg[2 * (i - 1)] = f.seg[2 * (i - 1) + 1] = true; f.kept.set_wprep(); }
  }
  for (int L = 1; L <= 2; ++L) {
    const ULevel& u = kUL[L];
    const int* d = p.d[L];
    f.ct[L] = nc_convT_k2s2_split_active(1, 2 * u.K, d[0], d[1], d[2], u.K) &&
              p.conv_ws >= nc_convT_k2s2_split_ws_bytes(1, 2 * u.K, d[0], d[1], d[2], u.K);
    f.cth[L] = f.ct[L] && f.h2l[u.cons] && ct_h2;
    f.ct_s3[L] = f.use[u.cons] && !f.h2l[u.cons] && (f.ct[L] || (L == 1 && convT_fwd_s3_supported(1, 2 * u.K, d[0], d[1], d[2], u.K)));
    f.bound[L] = wprep && f.cth[L];
    if (f.seg[2 * (u.cons - 1)] && !f.cth[L]) f.seg[2 * (u.cons - 1)] = false;  // (a measured second cell: that forward pack stays per-layer)
    f.pool_in_norm[L] = f.pool_arg && f.lean && f.h2l[u.cons];
    if (f.lean && f.h2l[u.cons]) f.kept.set_lean_lo(L);
    if (f.lean && f.cth[L]) f.kept.set_lean_up(L);  // (the H2 half is all block 9 / 7 reads of the transposed convolution's output)
  }
  f.tail_flat = f.lean && norm_1x1_taken(N, 64, p.d[0][0], p.d[0][1], p.d[0][2], 1);
  if (f.tail_flat) f.kept.set_lean_e1();
  return f;
}

// EVERY FORM OF THE BACKWARD, decided at its top from `kept`, the switches of NOW and the shape.  A tensor the lean forward left out is written
// again wherever this backward reads it after all, with the bits the full forward stores: a block's fp32 input (rewrite_in: the block in front's
// normalisation + ReLU, into scratch) unless the block leaves it alone (input_unread); the halves of the concat buffers (rebuild_lo / rebuild_up,
// into their own slots of `saved`: the lower half is block 1 / 3's normalisation + ReLU, the upper half the transposed convolution's forward
// again with its fp32 output alone) for block 9 / 7's weight gradient without the kept H2 copy and, the lower half, for a pool backward outside
// the norm backward; e1 (rebuild_e1, into scratch) for one_by_one off the flat kernels.
enum NormBwd { kNormFp32, kNormS3, kNormH2, kNormH2Pool, kNormRank1 };
struct UBwdForms {
  bool now_h2[10];        // the block is in the two-term form now
  bool xs[10];            // its kept operand is usable (Kept::operand_usable)
  bool pack[10];          // its data gradient takes the pack the forward prepared: same test, and nc_set_unet_wprep still on
  bool input_unread[10];  // its backward leaves its fp32 input alone: the kept copy AND the split weight gradient AND a range guard that cannot
                          // switch inside this call (a flagged call builds its three-term x operand from the fp32 tensor, conv_split.hip run_ws_h2)
  bool rewrite_in[10];
  // the InstanceNorm backward.  S3 / H2: it writes the convolution's dY straight in operand form at the head of the convolution workspace -- no fp32
  // tensor, no conversion pass.  H2Pool (blocks 1, 3): it also takes skip half + pool backward from the winner bytes, and nc_maxpool2_bwd_add
  // with its 64- / 128-channel tensor is not launched.  Rank1 (block 9, one sample): it forms w12[c] * s2[v] from the one-channel s2 -- no
  // 64-channel data gradient of one_by_one is written or read.  Fp32: the fallback, then conv_bwd_keep.
  NormBwd norm[10];
  bool dy_guarded[10];    // the range guard may rewrite that dY as three terms inside the call
  bool tail_flat, rebuild_e1, rebuild_lo[3], rebuild_up[3];
  bool pool_folds(int L) const { return norm[kUL[L].lo] == kNormH2Pool; }
  bool r1() const { return norm[9] == kNormRank1; }
};

UBwdForms u_bwd_forms(const UPlan& p, Kept k, bool want_dx0) {
  UBwdForms f{};
  const int N = p.N;
  const bool fuse = sw::raw(sw::S3_TRAIN_FUSE) != 0, wprep_now = sw::raw(sw::UNET_WPREP) != 0, lean_now = sw::raw(sw::UNET_LEAN) != 0;
  const bool flip = h2_guard_can_flip();
  for (int i = 0; i < 10; ++i) {
    const UBlock& b = kUB[i];
    const int* d = p.d[b.lvl];
    const bool pre_ok = conv_bwd_pre_supported(N, b.C, d[0], d[1], d[2], b.K, 3, i >= 1 || want_dx0, p.conv_ws);
    f.now_h2[i] = layer_h2_now(N, b.C, d, b.K, 3);
    f.xs[i] = k.operand_usable(i, f.now_h2[i]);
    f.pack[i] = i >= 1 && f.now_h2[i] && k.wprep() && k.operand_h2(i) && wprep_now;
    f.input_unread[i] = f.xs[i] && !flip && pre_ok;
    f.rewrite_in[i] = k.lean_input(i) && !f.input_unread[i];
    f.norm[i] = !(fuse && i >= 1 && pre_ok && instnorm_bwd_s3_supported(N, b.K, p.S[b.lvl])) ? kNormFp32 : f.now_h2[i] ? kNormH2 : kNormS3;
    f.dy_guarded[i] = f.now_h2[i] && flip;
  }
  if (lean_now && N == 1 && f.norm[9] == kNormH2) f.norm[9] = kNormRank1;  // (dW12 / db12 stay with the matrix kernel: their summation order is part of the step)
  for (int L = 1; L <= 2; ++L) {
    const ULevel& u = kUL[L];
    const int* d = p.d[L - 1];
    unsigned guard;  // (block_bwd always passes the guard's words: only their presence counts here)
    if (k.pool_arg() && f.norm[u.lo] == kNormH2 && instnorm_bwd_h2_pool_supported(N, u.K, d[0], d[1], d[2], &guard)) f.norm[u.lo] = kNormH2Pool;
    const bool cat_read = !f.input_unread[u.cons];
    f.rebuild_lo[L] = k.lean_lo(L) && k.pool_arg() && (cat_read || f.norm[u.lo] != kNormH2Pool);
    f.rebuild_up[L] = k.lean_up(L) && cat_read;
  }
  f.tail_flat = k.lean_e1() && norm_1x1_taken(N, 64, p.d[0][0], p.d[0][1], p.d[0][2], 1);
  f.rebuild_e1 = k.lean_e1() && !f.tail_flat;
  return f;
}

}  // namespace

extern "C" {

size_t nc_unet_deconv_param_floats(void) { return u_offsets().total; }

int nc_unet_wprep_layout(int N, int S0, int S1, int S2, int block, int form, size_t* pack_off, size_t* pack_bytes, size_t* cell_off,
                         size_t* bound_off) {
  UPlan p;
  if (!u_plan(p, N, S0, S1, S2) || block < 1 || block > 9 || form < 0 || form > 1) { set_error("unet_wprep_layout: bad argument"); return NC_ERR_ARG; }
  WPrepSeg sg[18];
  wprep_segs(sg);
  const int k = 2 * (block - 1) + form;
  size_t off = kWPrepCellBytes;
  for (int j = 0; j < k; ++j) off += s3x_packed_bytes(sg[j].Cin, sg[j].Kout, 3, 2);
  if (pack_off) *pack_off = p.wprep * 4 + off;
  if (pack_bytes) *pack_bytes = s3x_packed_bytes(sg[k].Cin, sg[k].Kout, 3, 2);
  if (cell_off) *cell_off = p.wprep * 4 + (size_t)k * 4;
  // (bounds are numbered in block order: 7 first when both are computed -- the default configuration)
  if (bound_off) *bound_off = block == 7 ? p.wprep * 4 + (size_t)kWPrepBoundCell0 * 4 : block == 9 ? p.wprep * 4 + (size_t)(kWPrepBoundCell0 + 1) * 4 : 0;
  return NC_OK;
}
int nc_s3x_pack_h2_debug(const float* w, int C, int K, int form, const unsigned* cell_a, const unsigned* cell_b, void* wp, unsigned* wcell,
                         void* stream) {
  if (!w || !cell_a || !cell_b || !wp || !wcell || C % 64 || K % 64) { set_error("s3x_pack_h2_debug: bad argument"); return NC_ERR_ARG; }
  if (form) return s3x_pack_h2(w, K, C, 3, 27, (long)C * 27, 1, K, cell_a, cell_a, wcell, wp, (hipStream_t)stream);
  return s3x_pack_h2(w, C, K, 3, (long)C * 27, 27, 0, C / 2, cell_a, cell_b, wcell, wp, (hipStream_t)stream);
}
int nc_convT_h2_bound_debug(const float* w, const float* bias, int C, int K, float in_bound, unsigned* cell, void* stream) {
  if (!w || !cell) { set_error("convT_h2_bound_debug: null pointer"); return NC_ERR_ARG; }
  NC_TRY(h2_zero_cells(cell, 1, (hipStream_t)stream));
  return convT_h2_bound(w, bias, C, K, in_bound, cell, (hipStream_t)stream);
}

size_t nc_unet_deconv_saved_floats(int N, int S0, int S1, int S2) {
  UPlan p;
  return u_plan(p, N, S0, S1, S2) ? p.saved : 0;
}

size_t nc_unet_deconv_train_ws_bytes(int N, int S0, int S1, int S2) {
  UPlan p;
  return u_plan(p, N, S0, S1, S2) ? u_ws_bytes(p, true) : 0;
}

unsigned nc_unet_deconv_kept_expected(int N, int S0, int S1, int S2) {
  NetworkScope net_scope;
  UPlan p;
  return u_plan(p, N, S0, S1, S2) ? u_fwd_forms(p).kept.w : 0;
}

int nc_unet_deconv_train_fwd(const float* params, const float* x, float* y, float* saved, int N, int S0, int S1, int S2,
                             void* ws, size_t ws_bytes, void* stream, unsigned* kept) {
  NetworkScope net_scope;
  if (!params || !x || !y || !saved) { set_error("unet_deconv_train_fwd: null pointer"); return NC_ERR_ARG; }
  UPlan p;
  if (!u_plan(p, N, S0, S1, S2)) {
    set_error("unet_deconv_train_fwd: every edge must be a positive multiple of 4 (got %d,%d,%d)", S0, S1, S2);
    return NC_ERR_SHAPE;
  }
  if (!ws || ws_bytes < u_ws_bytes(p, false)) { set_error("unet_deconv_train_fwd: workspace too small"); return NC_ERR_WS; }
  const UFwdForms f = u_fwd_forms(p);
  const UOff o = u_offsets();
  void* cws = ws;
  void* iws = (char*)ws + align256(p.conv_ws);
  float* V = saved;
  const float* P = params;
  if (kept) *kept = 0;
  hipStream_t hs = (hipStream_t)stream;
  const long S = p.S[0];
  const int* d0 = p.d[0];
  // the second cell of block 9 / 7's H2 operand: the upper half's, written by level 1 / 2's transposed convolution
  unsigned* cell[3] = {nullptr, h2_cells_of(V + p.xs3[9], (size_t)N * 128 * S) + 1, h2_cells_of(V + p.xs3[7], (size_t)N * 256 * p.S[1]) + 1};
  // the prepared weights (Kept::wprep): every two-term block's cells and packs, both forms, before the first convolution
  S3xPrepared prep[18] = {};
  if (f.kept.wprep()) {
    WPrepSeg sg[18];
    wprep_segs(sg);
    WPrepBound wb[2];
    int nb = 0;  // (bounds are numbered in block order)
    for (int i = 1; i < 10; ++i) {
      if (!f.seg[2 * (i - 1) + 1]) continue;
      WPrepSeg& fw = sg[2 * (i - 1)];
      // the input's first cell: the InstanceNorm bound of its level (h2.hip act_split2h) -- or, behind a max-pool, a measured cell that both
      // halves share: the ratio is 1 whatever the value
      fw.a_bits = f32_bits(sqrtf((float)p.S[kUB[i].lvl]));
      if (f.seg[2 * (i - 1)]) fw.w = P + o.w[i];
      const int L = i == 7 ? 2 : i == 9 ? 1 : 0;
      if (L && f.bound[L]) {
        fw.b_cell = kWPrepBoundCell0 + nb;
        fw.ext_cell = cell[L];
        wb[nb++] = WPrepBound{P + o.w[kUL[L].tw], P + o.b[kUL[L].tw], 2 * kUL[L].K, kUL[L].K, sqrtf((float)p.S[L]), 0};
      }
      sg[2 * (i - 1) + 1].w = P + o.w[i];
    }
    NC_TRY(wprep_run(sg, 18, wb, nb, V + p.wprep, prep, hs));
  }
  // conv (3^3, pad 1) -> raw; statistics; normalise + ReLU into `out`, where sample n's K planes start at
  // out + n * out_stride (out_stride = K * S for a dense tensor, Ctot * S for a half of a concat buffer).
  // to >= 0: block `to` consumes this output as channels [0, K) of its `to_ctot`-channel input; to == -2: the consumer normalises for itself.
  // skip = L: the block is level L's `lo`, a max-pool follows
  auto block = [&](int i, const float* in, float* out, size_t out_stride, int to, int to_ctot, int skip = 0) -> int {
    const UBlock& b = kUB[i];
    const int* d = p.d[b.lvl];
    const long S = p.S[b.lvl];
    const S3xPrepared* pw = i >= 1 && prep[2 * (i - 1)].wp ? &prep[2 * (i - 1)] : nullptr;
    if (f.pre[i]) {  // the producers left the operand form of the input in saved
      NC_TRY(conv_fwd_pre(V + p.xs3[i], P + o.w[i], P + o.b[i], V + p.raw[i], N, b.C, d[0], d[1], d[2], b.K, 3, cws, p.conv_ws, stream,
                          f.epi[i] ? (float*)iws : nullptr, pw));
    } else {
      bool kept1 = false;
      NC_TRY(conv_fwd_keep(in, P + o.w[i], P + o.b[i], V + p.raw[i], N, b.C, d[0], d[1], d[2], b.K, 3, cws, p.conv_ws, stream,
                           i >= 1 ? (void*)(V + p.xs3[i]) : nullptr, &kept1, pw));
      if (kept1 != f.kept.operand(i)) { set_error("unet_deconv_train_fwd: block %d %s its converted input, against the plan", i, kept1 ? "kept" : "did not keep"); return NC_ERR_ARG; }
    }
    if (f.epi[i]) NC_TRY(s3x_stats_finalize((const float*)iws, P + o.b[i], N, d[0], d[1], d[2], b.K, 3, 1e-5f, V + p.mean[i], V + p.rstd[i], hs));
    else NC_TRY(nc_instnorm_stats(V + p.raw[i], N * b.K, S, 1e-5f, V + p.mean[i], V + p.rstd[i], iws, p.in_ws, stream));
    if (skip && f.pool_in_norm[skip])  // the H2 half, the fp32 POOLED tensor and the winner bytes in one pass (act_operand's cell and bound)
      return act_split2h_pool_arg(V + p.raw[i], V + p.mean[i], V + p.rstd[i], 0.f, V + p.xs3[to], V + p.*kUL[skip].pooled,
                                  (unsigned char*)(V + p.parg[skip - 1]), N, b.K, d[0], d[1], d[2], to_ctot, 0, sqrtf((float)S),
                                  h2_cells_of(V + p.xs3[to], (size_t)N * to_ctot * S), hs);
    if (to >= 0 && f.use[to]) {  // fp32 (the backward of the pool / the fallback paths read it) AND the consumer's operand in one pass
      if (f.kept.lean_input(to)) out = nullptr;  // (its only regular reader is the two-term block behind it)
      return act_operand(f.cd[to], V + p.raw[i], V + p.mean[i], V + p.rstd[i], 0.f, out, (long)out_stride, V + p.xs3[to], N, b.K, S, to_ctot, 0, hs);
    }
    if (to == -2) return NC_OK;
    if (out_stride == (size_t)b.K * S || N == 1)
      return nc_instnorm_act_fwd(V + p.raw[i], V + p.mean[i], V + p.rstd[i], 0.f, out, N * b.K, S, stream);
    for (int n = 0; n < N; ++n)
      NC_TRY(nc_instnorm_act_fwd(V + p.raw[i] + (size_t)n * b.K * S, V + p.mean[i] + n * b.K, V + p.rstd[i] + n * b.K, 0.f,
                                 out + n * out_stride, b.K, S, stream));
    return NC_OK;
  };
  // level L's max-pool, unless its block pooled in its normalisation pass
  auto pool = [&](int L) -> int {
    const ULevel& u = kUL[L];
    const int* d = p.d[L - 1];
    const long Sc = p.S[L - 1], Sp = p.S[L];
    for (int n = 0; n < N && !f.pool_in_norm[L]; ++n) {
      const float* src = V + p.*u.cat + (size_t)n * 2 * u.K * Sc;
      float* dst = V + p.*u.pooled + (size_t)n * u.K * Sp;
      if (f.pool_arg) NC_TRY(maxpool2_fwd_arg(src, dst, (unsigned char*)(V + p.parg[L - 1]) + (size_t)n * u.K * Sp, u.K, d[0], d[1], d[2], hs));
      else NC_TRY(nc_maxpool2_fwd(src, dst, u.K, d[0], d[1], d[2], stream));
    }
    return NC_OK;
  };
  // level L's transposed convolution writes the second half of the concat buffer, on the plan's arm, and the consumer's operand is completed (its
  // first half came from block lo's normalisation pass).  A half in the two-term form that the arm did not write (kCtSplit under NC_CONVT_H2=0) is
  // measured after the fact: its power of two cannot be known while it is written.
  auto t_conv = [&](int L) -> int {
    const ULevel& u = kUL[L];
    const int C = 2 * u.K, *d = p.d[L];
    const long Si = p.S[L], So = p.S[L - 1];
    const float *w = P + o.w[u.tw], *bias = P + o.b[u.tw];
    const CtArm arm = f.arm(L);
    if (arm == kCtH2 && !f.bound[L]) {  // (the prepared pass leaves the bound in the cell itself)
      NC_TRY(h2_zero_cells(cell[L], 1, hs));
      NC_TRY(convT_h2_bound(w, bias, C, u.K, sqrtf((float)Si), cell[L], hs));
    }
    for (int n = 0; n < N; ++n) {
      const float* tin = V + p.*u.tin + (size_t)n * C * Si;
      float* half = V + p.*u.cat + ((size_t)n * C + u.K) * So;
      char* xs = (char*)(V + p.xs3[u.cons]) + (size_t)n * C * So * (arm == kCtH2 ? 4 : 6);
      if (arm == kCtH2)
        NC_TRY(convT_fwd_split_h2(tin, w, bias, f.kept.lean_up(L) ? nullptr : half, xs, C, u.K, 1, C, d[0], d[1], d[2], u.K, cell[L], cws, p.conv_ws, hs));
      else if (arm == kCtSplit)
        NC_TRY(nc_convT_k2s2_fwd_split(tin, nullptr, w, bias, half, f.ct_s3[L] ? xs : nullptr, C, u.K, 1, C, d[0], d[1], d[2], u.K, cws, p.conv_ws, stream));
      else if (arm == kCtS3)  // (level 1 only: u_fwd_forms)
        NC_TRY(convT_fwd_s3(tin, w, bias, half, xs, C, u.K, 1, C, d[0], d[1], d[2], u.K, stream));
      else
        NC_TRY(nc_convT_k2s2_fwd(tin, w, bias, half, 1, C, d[0], d[1], d[2], u.K, stream));
    }
    if (f.use[u.cons] && !f.ct_s3[L] && arm != kCtH2)
      NC_TRY(operand_into(f.cd[u.cons], V + p.*u.cat + (size_t)u.K * So, (long)C * So, V + p.xs3[u.cons], N, u.K, So, C, u.K, hs));
    return NC_OK;
  };
  NC_TRY(block(0, x, V + p.a1, (size_t)64 * S, 1, 64));
  NC_TRY(block(1, V + p.a1, V + p.cat1, (size_t)128 * S, 9, 128, 1));
  NC_TRY(pool(1));
  NC_TRY(block(2, V + p.p1, V + p.a2, (size_t)128 * p.S[1], 3, 128));
  NC_TRY(block(3, V + p.a2, V + p.cat2, (size_t)256 * p.S[1], 7, 256, 2));
  NC_TRY(pool(2));
  NC_TRY(block(4, V + p.p2, V + p.b1, (size_t)256 * p.S[2], 5, 256));
  NC_TRY(block(5, V + p.b1, V + p.b2, (size_t)256 * p.S[2], 6, 256));
  NC_TRY(block(6, V + p.b2, V + p.b3, (size_t)256 * p.S[2], -1, 0));
  NC_TRY(t_conv(2));
  NC_TRY(block(7, V + p.cat2, V + p.e2a, (size_t)128 * p.S[1], 8, 128));
  NC_TRY(block(8, V + p.e2a, V + p.e2b, (size_t)128 * p.S[1], -1, 0));
  NC_TRY(t_conv(1));
  // the 1x1 tail
  if (f.tail_flat) {
    NC_TRY(block(9, V + p.cat1, nullptr, (size_t)64 * S, -2, 0));
    NC_TRY(conv_fwd_norm_1x1(V + p.raw[9], V + p.mean[9], V + p.rstd[9], 0.f, P + o.w[12], P + o.b[12], V + p.t1, N, 64, d0[0], d0[1], d0[2], 1, cws,
                             p.conv_ws, stream));
  } else {
    NC_TRY(block(9, V + p.cat1, V + p.e1, (size_t)64 * S, -1, 0));
    NC_TRY(nc_conv_fwd(V + p.e1, P + o.w[12], P + o.b[12], V + p.t1, N, 64, d0[0], d0[1], d0[2], 1, 1, 1, 1, 1, 0, cws, p.conv_ws, stream));
  }
  // one_by_one_2 + sigmoid: y doubles as the buffer of the pre-sigmoid value (the sigmoid kernel is elementwise in place)
  NC_TRY(nc_conv_fwd(V + p.t1, P + o.w[13], P + o.b[13], y, N, 1, d0[0], d0[1], d0[2], 1, 1, 1, 1, 1, 0, cws, p.conv_ws, stream));
  if (kept) *kept = f.kept.w;
  return nc_sigmoid_fwd(y, y, (long)N * S, stream);
}

// dparams: packed like params, OVERWRITTEN with this call's parameter gradients.  dx nullable (the U-Net's input is the
// real volume in the Apollo / Athena steps: its gradient -- the data gradient of the first convolution -- is skipped).
int nc_unet_deconv_bwd(const float* params, const float* x, const float* y, const float* saved, const float* dy, float* dx,
                       float* dparams, int N, int S0, int S1, int S2, void* ws, size_t ws_bytes, void* stream, unsigned kept) {
  NetworkScope net_scope;
  if (!params || !x || !y || !saved || !dy || !dparams) { set_error("unet_deconv_bwd: null pointer"); return NC_ERR_ARG; }
  UPlan p;
  if (!u_plan(p, N, S0, S1, S2)) { set_error("unet_deconv_bwd: bad shape"); return NC_ERR_SHAPE; }
  if (!ws || ws_bytes < u_ws_bytes(p, true)) { set_error("unet_deconv_bwd: workspace too small"); return NC_ERR_WS; }
  const UBwdForms f = u_bwd_forms(p, Kept{kept}, dx != nullptr);
  const UOff o = u_offsets();
  hipStream_t hs = (hipStream_t)stream;
  void* cws = ws;
  void* iws = (char*)ws + align256(p.conv_ws);
  void* tws = (char*)iws + align256(p.in_ws);
  float* G = (float*)((char*)tws + align256(p.convT_ws));
  const float* V = saved;
  const float* P = params;
  float* DP = dparams;
  const long S = p.S[0];
  const int* d0 = p.d[0];
  S3xPrepared prepd[10] = {};  // block i's data-gradient pack in `saved` (wprep_run's layout: cells, then the segments in order)
  {
    WPrepSeg sg[18];
    wprep_segs(sg);
    const char* region = (const char*)(V + p.wprep);
    size_t off = kWPrepCellBytes;
    for (int k = 0; k < 18; ++k) {
      if (k & 1) prepd[k / 2 + 1] = S3xPrepared{region + off, (const unsigned*)region + k};
      off += s3x_packed_bytes(sg[k].Cin, sg[k].Kout, 3, 2);
    }
  }
  // backward of block i: g = gradient at the block's (post-ReLU) output, dense [N][K][S]; `in` = the block's input.
  // draw <- InstanceNorm/ReLU backward (+ the conv's bias gradient); dW <- wgrad; gin (nullable) <- dgrad
  // kNormH2Pool: g is the skip half of the concat gradient (sample stride 2 K Sl), pool the dense pooled gradient; kNormRank1: g is the one-channel s2
  auto block_bwd = [&](int i, const float* g, const float* in, float* draw, float* gin, const float* pool = nullptr) -> int {
    const UBlock& b = kUB[i];
    const int* d = p.d[b.lvl];
    const long Sl = p.S[b.lvl];
    const void* xs = f.xs[i] ? (const void*)(V + p.xs3[i]) : nullptr;
    if (f.rewrite_in[i]) {  // (into scratch no block's backward uses)
      NC_TRY(nc_instnorm_act_fwd(V + p.raw[i - 1], V + p.mean[i - 1], V + p.rstd[i - 1], 0.f, G + p.T, N * b.C, Sl, stream));
      in = G + p.T;
    }
    const float *raw = V + p.raw[i], *mean = V + p.mean[i], *rstd = V + p.rstd[i];
    unsigned* gw = conv_bwd_guard_words(cws, N, b.K, Sl);  // (the norm backward counts, decides and -- flagged -- rewrites its dY as S3)
    const NormBwd nf = f.norm[i];
    if (nf == kNormFp32) {
      NC_TRY(nc_instnorm_act_bwd_dbias(g, raw, mean, rstd, 0.f, draw, DP + o.b[i], N, b.K, Sl, iws, p.in_ws, stream));
      return conv_bwd_keep(in, xs, draw, P + o.w[i], gin, DP + o.w[i], N, b.C, d[0], d[1], d[2], b.K, 3, cws, p.conv_ws, stream);
    }
    if (nf == kNormRank1)
      NC_TRY(instnorm_act_bwd_dbias_h2_rank1(g, P + o.w[12], raw, mean, rstd, 0.f, cws, DP + o.b[i], b.K, Sl, iws, p.in_ws, stream, gw));
    else if (nf == kNormH2Pool)
      NC_TRY(instnorm_act_bwd_dbias_h2_pool(g, (long)2 * b.K * Sl, pool, (const unsigned char*)(V + p.parg[i == 1 ? 0 : 1]), raw, mean, rstd, 0.f, cws,
                                            DP + o.b[i], N, b.K, d[0], d[1], d[2], iws, p.in_ws, stream, gw));
    else if (nf == kNormH2)
      NC_TRY(instnorm_act_bwd_dbias_h2(g, raw, mean, rstd, 0.f, cws, DP + o.b[i], N, b.K, Sl, iws, p.in_ws, stream, gw));
    else
      NC_TRY(instnorm_act_bwd_dbias_s3(g, raw, mean, rstd, 0.f, cws, DP + o.b[i], N, b.K, Sl, iws, p.in_ws, stream));
    return conv_bwd_pre(in, xs, P + o.w[i], gin, DP + o.w[i], N, b.C, d[0], d[1], d[2], b.K, 3, cws, p.conv_ws, stream, f.dy_guarded[i],
                        f.pack[i] ? &prepd[i] : nullptr);
  };
  // backward of level L's transposed convolution, from the gradient of the concat buffer's second half as a dense tensor (N == 1 needs no copy)
  auto t_conv_bwd = [&](int L, const float* dcat, float* gin) -> int {
    const ULevel& u = kUL[L];
    const int* d = p.d[L];
    const float* g = dcat + (size_t)u.K * p.S[L - 1];
    if (N > 1) { NC_TRY(gather_half(dcat, G + p.T, N, 2 * u.K, u.K, u.K, p.S[L - 1], hs)); g = G + p.T; }
    NC_TRY(nc_convT_k2s2_dgrad(g, P + o.w[u.tw], gin, N, 2 * u.K, d[0], d[1], d[2], u.K, tws, p.convT_ws, stream));
    return nc_convT_k2s2_wgrad(V + p.*u.tin, g, DP + o.w[u.tw], DP + o.b[u.tw], N, 2 * u.K, d[0], d[1], d[2], u.K, tws, p.convT_ws, stream);
  };
  // level L's halves of the concat buffer that a lean forward left out and this backward reads (UBwdForms), before anything of this call lives
  // in the convolution workspace
  auto rebuild = [&](int L) -> int {
    const ULevel& u = kUL[L];
    const int C = u.K, *td = p.d[L];
    const long Sl = p.S[L - 1];
    float* cat = const_cast<float*>(saved) + p.*u.cat;
    for (int n = 0; n < N && f.rebuild_lo[L]; ++n)
      NC_TRY(nc_instnorm_act_fwd(V + p.raw[u.lo] + (size_t)n * C * Sl, V + p.mean[u.lo] + n * C, V + p.rstd[u.lo] + n * C, 0.f,
                                 cat + (size_t)n * 2 * C * Sl, C, Sl, stream));
    for (int n = 0; n < N && f.rebuild_up[L]; ++n)
      NC_TRY(convT_fwd_split_h2(V + p.*u.tin + (size_t)n * 2 * C * p.S[L], P + o.w[u.tw], P + o.b[u.tw], cat + ((size_t)n * 2 + 1) * C * Sl, nullptr, 2 * C,
                                C, 1, 2 * C, td[0], td[1], td[2], C, nullptr, cws, p.conv_ws, hs));
    return NC_OK;
  };
  // block lo of level L feeds the pool AND the skip: gradient = pool backward (of gpool) + the first half of dcat, formed inside the block's norm
  // backward (no K-channel tensor) or by nc_maxpool2_bwd_add into gsum; then the block's backward, its data gradient into gsum
  auto skip_bwd = [&](int L, const float* gpool, const float* dcat, float* gsum, const float* in, float* draw) -> int {
    const ULevel& u = kUL[L];
    const int* d = p.d[L - 1];
    const long Sc = p.S[L - 1], Sp = p.S[L];
    if (f.pool_folds(L)) return block_bwd(u.lo, dcat, in, draw, gsum, gpool);
    for (int n = 0; n < N; ++n)
      NC_TRY(nc_maxpool2_bwd_add(gpool + (size_t)n * u.K * Sp, V + p.*u.cat + (size_t)n * 2 * u.K * Sc, dcat + (size_t)n * 2 * u.K * Sc,
                                 gsum + (size_t)n * u.K * Sc, u.K, d[0], d[1], d[2], stream));
    return block_bwd(u.lo, gsum, in, draw, gsum);
  };
  NC_TRY(rebuild(1));
  NC_TRY(rebuild(2));
  // 1x1 tail
  NC_TRY(nc_sigmoid_bwd(dy, y, G + p.s1, (long)N * S, stream));
  NC_TRY(nc_conv_wgrad(V + p.t1, G + p.s1, DP + o.w[13], DP + o.b[13], N, 1, d0[0], d0[1], d0[2], 1, 1, 1, 1, 1, 0, cws, p.conv_ws, stream));
  NC_TRY(nc_conv_dgrad(G + p.s1, P + o.w[13], G + p.s2, N, 1, d0[0], d0[1], d0[2], 1, 1, 1, 1, 1, 0, cws, p.conv_ws, stream));
  if (f.tail_flat) {  // (no e1: the weight gradient normalises raw[9] as it reads it)
    NC_TRY(conv_wgrad_norm_1x1(V + p.raw[9], V + p.mean[9], V + p.rstd[9], 0.f, G + p.s2, DP + o.w[12], DP + o.b[12], N, 64, d0[0], d0[1], d0[2], 1, cws,
                               p.conv_ws, stream));
  } else {
    const float* e1 = V + p.e1;
    if (f.rebuild_e1) {  // (T is free until block 9's backward)
      NC_TRY(nc_instnorm_act_fwd(V + p.raw[9], V + p.mean[9], V + p.rstd[9], 0.f, G + p.T, N * 64, S, stream));
      e1 = G + p.T;
    }
    NC_TRY(nc_conv_wgrad(e1, G + p.s2, DP + o.w[12], DP + o.b[12], N, 64, d0[0], d0[1], d0[2], 1, 1, 1, 1, 1, 0, cws, p.conv_ws, stream));
  }
  if (!f.r1()) NC_TRY(nc_conv_dgrad(G + p.s2, P + o.w[12], G + p.G1, N, 64, d0[0], d0[1], d0[2], 1, 1, 1, 1, 1, 0, cws, p.conv_ws, stream));
  // ex_conv1_1 (cat1 -> e1)
  NC_TRY(block_bwd(9, f.r1() ? G + p.s2 : G + p.G1, V + p.cat1, G + p.G2, G + p.G3));
  NC_TRY(t_conv_bwd(1, G + p.G3, G + p.H1));  // t_conv1 (e2b -> cat1[:, 64:])
  // ex_double_conv2 (cat2 -> e2a -> e2b)
  NC_TRY(block_bwd(8, G + p.H1, V + p.e2a, G + p.H2, G + p.H1));
  NC_TRY(block_bwd(7, G + p.H1, V + p.cat2, G + p.H2, G + p.H3));
  NC_TRY(t_conv_bwd(2, G + p.H3, G + p.Q1));  // t_conv2 (b3 -> cat2[:, 128:])
  // bottom_layer (p2 -> b1 -> b2 -> b3)
  NC_TRY(block_bwd(6, G + p.Q1, V + p.b2, G + p.Q2, G + p.Q1));
  NC_TRY(block_bwd(5, G + p.Q1, V + p.b1, G + p.Q2, G + p.Q1));
  NC_TRY(block_bwd(4, G + p.Q1, V + p.p2, G + p.Q2, G + p.Q1));
  // double_conv2 (p1 -> a2 -> conv2 = cat2[:, :128]), double_conv1 (x -> a1 -> conv1 = cat1[:, :64])
  NC_TRY(skip_bwd(2, G + p.Q1, G + p.H3, G + p.H1, V + p.a2, G + p.H2));
  NC_TRY(block_bwd(2, G + p.H1, V + p.p1, G + p.H2, G + p.H1));
  NC_TRY(skip_bwd(1, G + p.H1, G + p.G3, G + p.G1, V + p.a1, G + p.G2));
  return block_bwd(0, G + p.G1, x, G + p.G2, dx);
}


}  // extern "C"

// ---- DeepLinearGenerator ------------------------------------------------------------------------------------------
// The layer table kLL is common.hpp's.  The weight-space steps of the collapsed forms (their algebra, kernels and scratch) are dl_tail.hip's
// nc::dl_*; the position-typed kernels are dl_typed.hip's.  Here: the plan of each direction, and the launches it names.
namespace {

struct LPlan {
  int N, d[3];
  long S;
  size_t w[6], params;        // floats into the packed blob
  size_t act[5], saved;       // outputs of layers 0..4 (inputs of layers 1..5)
  size_t xs3[6];              // S3 copy of the input of layer i (the 5^3 and 3^3 layers), see `kept`
  size_t g[2], grads;         // gradient ping-pong
  size_t conv_ws;
};

bool l_plan(LPlan& p, int N, int S0, int S1, int S2) {
  if (N < 1 || S0 < 1 || S1 < 1 || S2 < 1) return false;
  p = LPlan{};
  p.N = N; p.d[0] = S0; p.d[1] = S1; p.d[2] = S2;
  p.S = (long)S0 * S1 * S2;
  size_t off = 0;
  for (int i = 0; i < 6; ++i) { p.w[i] = off; off += (size_t)kLL[i].K * kLL[i].C * kLL[i].k * kLL[i].k * kLL[i].k; }
  p.params = off;
  off = 0;
  for (int i = 0; i < 5; ++i) { p.act[i] = off; off += up64((size_t)N * kLL[i].K * p.S); }
  for (int i = 0; i < 6; ++i) {
    p.xs3[i] = off;
    if (kLL[i].k > 1 && kLL[i].C % 8 == 0) off += s3_floats((size_t)N * kLL[i].C * p.S);
  }
  p.saved = off;
  p.g[0] = 0; p.g[1] = up64((size_t)N * 64 * p.S);
  p.grads = 2 * up64((size_t)N * 64 * p.S);
  for (int i = 0; i < 6; ++i) {
    const size_t b = nc_conv_ws_bytes(N, kLL[i].C, S0, S1, S2, kLL[i].K, kLL[i].k, kLL[i].k, kLL[i].k, 1, kLL[i].k / 2);
    if (b > p.conv_ws) p.conv_ws = b;
  }
  const size_t b1 = nc_conv_ws_bytes(N, 1, S0, S1, S2, 64, 3, 3, 3, 1, 1);  // the collapsed tail's two one-channel problems
  if (b1 > p.conv_ws) p.conv_ws = b1;
  if (conv_fwd_to1_k3_ws_bytes(N, S0, S1, S2) > p.conv_ws) p.conv_ws = conv_fwd_to1_k3_ws_bytes(N, S0, S1, S2);
  return true;
}

// THE WORKSPACE of both directions: convolution scratch | the gradient ping-pong (inference: the activations') | the tail scratch of the
// weight-space steps | the typed form's scratch.  ws == NULL: the size alone.
struct LWs { void* cws; float* G; char* tail; char* typed; size_t bytes; };
LWs l_ws(const LPlan& p, void* ws) {
  uintptr_t at = (uintptr_t)ws;
  auto take = [&](size_t bytes) { const uintptr_t r = at; at += bytes; return r; };
  LWs v;
  v.cws = (void*)take(align256(p.conv_ws));
  v.G = (float*)take(p.grads * sizeof(float) + 256);
  v.tail = (char*)take(align256(dl_tail_bytes()));
  v.typed = (char*)take(dl_typed_bytes(p.N, p.d[0], p.d[1], p.d[2]));
  v.bytes = at - (uintptr_t)ws;
  return v;
}

// the deep-linear flags of `kept` (Kept::has / Kept::set)
constexpr unsigned kKeptCollapsed = 1u << 31;  // layers 2 .. 5 ran in the collapsed form: act2 .. act4 do not exist ("the collapsed tail")
constexpr unsigned kKeptNoAct1 = 1u << 30;     // ... and layer 1 ran in its 64 -> 27 form: act1 was never written ("the forward without act1")
constexpr unsigned kKeptTyped = 1u << 29;      // ... layers 1 .. 5 ran as ONE position-typed 7^3 kernel (dl_typed.hip): neither act1 nor a two-term copy of act0 exists

// THE FORM OF THE FORWARD, decided before its first launch (all of it host state).  The forward reads these fields and launches.
// sw::DL_COLLAPSE 0: layer by layer; 1: the collapsed tail + the rank forms of the 5^3 layer (round 5); 2 (default): layers 1 .. 5 as one
// position-typed 7^3 kernel where the shape admits it (dl_typed.hip), else as 1.
//   kLTyped    layers 1 .. 5 as ONE position-typed 7^3 convolution 64 -> 1 of act0 (dl_typed.hip): the interior kernel on the
//              two-term pseudo-channel kernel of Conv3d(1, 64, 7)'s data gradient, the voxels on a face recomputed with their own kernels
//   kLNoAct1   layers 1 .. 5 without act1 (dl_tail.hip, "the forward without act1"): Z = the 64 -> 27 convolution of act0, which leaves the
//              two-term copy of act0, and y = its shifted sum
//   kLTail     layers 2 .. 5 as one 64 -> 1 convolution of act1 (dl_tail.hip, "the collapsed tail")
//   kLLayered  all six layers
// The first two are training forms (they pay off through their backward): inference, saved == NULL, takes kLTail under levels 1 and 2.
// A layer that runs layer by layer keeps its converted input where conv_fwd_keep does (Kept::operand, training only).
enum LForm { kLLayered, kLTail, kLNoAct1, kLTyped };
struct LFwdForms {
  LForm form;
  int layered;  // layers 0 .. layered - 1 run layer by layer, in front of the form's own launches
  ConvDims cd;  // kLTyped: Conv3d(1, 64, 7)'s problem; kLNoAct1: the 64 -> 32 one, 5^3
  Kept kept;
};

LFwdForms l_fwd_form(const LPlan& p, bool training) {
  LFwdForms f{};
  const int N = p.N, *d = p.d;
  const int level = sw::raw(sw::DL_COLLAPSE);
  if (level == 2 && training && dl_typed_supported(N, d[0], d[1], d[2]) && make_dims(f.cd, N, 1, d[0], d[1], d[2], 64, 7, 7, 7, 1, 3) &&
      c1k7_h2_supported(f.cd) && c1_wgrad_supported(f.cd) && c1k7_h2_dgrad_ws_bytes(f.cd) <= p.conv_ws && c1k7_h2_ws_bytes(f.cd) <= p.conv_ws &&
      c1_wgrad_ws_bytes(f.cd) <= p.conv_ws) {
    f.form = kLTyped;
    f.kept.set(kKeptCollapsed | kKeptNoAct1 | kKeptTyped);
  } else if (level && training && sw::raw(sw::DL_K32) != 0 && make_dims(f.cd, N, 64, d[0], d[1], d[2], 32, 5, 5, 5, 1, 2) &&
             conv_fwd_h2_k32_supported(f.cd) && (size_t)256 + s3x_packed_bytes(64, 32, 5, 2) + 512 <= p.conv_ws) {
    f.form = kLNoAct1;
    f.kept.set(kKeptCollapsed | kKeptNoAct1);
    f.kept.set_operand(1, true);
  } else if (level) {
    f.form = kLTail;
    f.kept.set(kKeptCollapsed);
  } else {
    f.form = kLLayered;
  }
  f.layered = f.form == kLLayered ? 6 : f.form == kLTail ? 2 : 1;
  for (int i = 0; i < f.layered; ++i) {
    const LLayer& l = kLL[i];
    if (training && l.k > 1 && l.C % 8 == 0 && conv_keep_supported(N, l.C, d[0], d[1], d[2], l.K, l.k))  // (conv_fwd_keep's *kept)
      f.kept.set_operand(i, layer_h2_now(N, l.C, d, l.K, l.k));
  }
  return f;
}

// THE FORM OF THE BACKWARD, decided at its top from `kept`, the switches of NOW and the shape.
// top: where it starts.  kLTopTyped (kKeptTyped): layers 1 .. 5 from dy, act0 and the weights, then layer 0.  kLTopTail (kKeptCollapsed): layers
// 2 .. 5 from dy, act1 and the weights alone, then layer 1 in the form below, then layer 0.  kLTopLayered: layers 5 .. 0.
// Layer 1 behind a collapsed tail (dl_tail.hip, "layer 1's weight gradient from the rank structure of its dY"):
//   rank_w      dW1 and q from P, the 32 x 64 weight gradient between the 27 shifted copies of dy and act0's kept two-term copy -- act1 is not read
//   rank_dgrad  ... and dL/dact0 as a forward 32 -> 64 convolution of the shifted copies with composed weights: dL/dact1 is never formed (!g1)
//   neither     q from dy and act1, dL/dact1 = flip(E) (*) dy, then the layer's ordinary backward in the loop.  remake_act1: the forward never
//               wrote act1 (kKeptNoAct1) and the switches moved since -- it is formed now, in a gradient buffer
// Whether dx is wanted is no input: layer 1's data gradient feeds layer 0's weight gradient either way, and layer 0 skips its own on a NULL dx.
enum LTop { kLTopLayered, kLTopTail, kLTopTyped };
struct LBwdForms {
  LTop top;
  int first;         // the layer loop runs first .. 0
  bool xs[6];        // the layer's kept operand is usable (Kept::operand_usable)
  bool rank_w, rank_dgrad, remake_act1, g1;
  ConvDims cd;       // kLTopTyped: Conv3d(1, 64, 7)'s problem; rank_w: the 32 x 64 one, 5^3
  const char* error; // `kept` names a form that this shape does not admit
};

LBwdForms l_bwd_forms(const LPlan& p, Kept k) {
  LBwdForms f{};
  const int N = p.N, *d = p.d;
  bool now_h2[6] = {};
  for (int i = 0; i < 6; ++i) {
    const LLayer& l = kLL[i];
    now_h2[i] = l.k > 1 && layer_h2_now(N, l.C, d, l.K, l.k);
    f.xs[i] = l.k > 1 && k.operand_usable(i, now_h2[i]);
  }
  if (k.has(kKeptTyped)) {
    // (its kernels exist in the two-term form only and convert their fp32 operands themselves: a caller who moved nc_set_split_terms after the
    // forward still gets this form's backward)
    ForceTwoTerm two_;
    f.top = kLTopTyped;
    f.first = 0;
    if (!dl_typed_supported(N, d[0], d[1], d[2]) || !make_dims(f.cd, N, 1, d[0], d[1], d[2], 64, 7, 7, 7, 1, 3) || !c1k7_h2_supported(f.cd) ||
        !c1_wgrad_supported(f.cd))
      f.error = "deep_linear_bwd: the forward ran the position-typed form, which this shape does not admit";
  } else if (k.has(kKeptCollapsed)) {
    f.top = kLTopTail;
    // now_h2[1] && xs[1]: the layer is two-term now AND its kept copy is there in that form -- so a rank form never needs a second look at either
    f.rank_w = sw::raw(sw::DL_RANK_WGRAD) != 0 && now_h2[1] && f.xs[1] && make_dims(f.cd, N, 32, d[0], d[1], d[2], 64, 5, 5, 5, 1, 2) &&
               wgrad_h2_supported(f.cd) && s3_wgrad_ws_bytes(f.cd) <= p.conv_ws;
    f.rank_dgrad = f.rank_w && sw::raw(sw::DL_RANK_DGRAD) != 0 && conv_fwd_h2_c32_supported(f.cd) && conv_fwd_h2_c32_ws_bytes(f.cd) <= p.conv_ws;
    f.remake_act1 = !f.rank_w && k.has(kKeptNoAct1);
    f.g1 = !f.rank_dgrad;
    f.first = f.rank_w ? 0 : 1;
  } else {
    f.top = kLTopLayered;
    f.first = 5;
  }
  return f;
}

}  // namespace

extern "C" {

size_t nc_deep_linear_param_floats(void) {
  LPlan p;
  l_plan(p, 1, 8, 8, 8);
  return p.params;
}

size_t nc_deep_linear_saved_floats(int N, int S0, int S1, int S2) {
  LPlan p;
  return l_plan(p, N, S0, S1, S2) ? p.saved : 0;
}

size_t nc_deep_linear_ws_bytes(int N, int S0, int S1, int S2) {
  LPlan p;
  return l_plan(p, N, S0, S1, S2) ? l_ws(p, nullptr).bytes : 0;
}

unsigned nc_deep_linear_kept_expected(int N, int S0, int S1, int S2) {
  NetworkScope net_scope;
  LPlan p;
  return l_plan(p, N, S0, S1, S2) ? l_fwd_form(p, true).kept.w : 0;
}

// saved == NULL: inference -- the intermediate activations ping-pong through the workspace instead
int nc_deep_linear_fwd(const float* params, const float* x, float* y, float* saved, int N, int S0, int S1, int S2, void* ws,
                       size_t ws_bytes, void* stream, unsigned* kept) {
  NetworkScope net_scope;
  if (!params || !x || !y) { set_error("deep_linear_fwd: null pointer"); return NC_ERR_ARG; }
  LPlan p;
  if (!l_plan(p, N, S0, S1, S2)) { set_error("deep_linear_fwd: bad shape"); return NC_ERR_SHAPE; }
  const LWs w = l_ws(p, ws);
  if (!ws || ws_bytes < w.bytes) { set_error("deep_linear_fwd: workspace too small"); return NC_ERR_WS; }
  const LFwdForms f = l_fwd_form(p, saved != nullptr);
  const float* P = params;
  hipStream_t hs = (hipStream_t)stream;
  if (kept) *kept = 0;
  const float* in = x;
  for (int i = 0; i < f.layered; ++i) {
    const LLayer& l = kLL[i];
    float* out = i == 5 ? y : (saved ? saved + p.act[i] : w.G + p.g[i & 1]);
    if (l.k > 1) {
      bool kept1 = false;
      void* keep = saved && l.C % 8 == 0 ? (void*)(saved + p.xs3[i]) : nullptr;
      NC_TRY(conv_fwd_keep(in, P + p.w[i], nullptr, out, N, l.C, S0, S1, S2, l.K, l.k, w.cws, p.conv_ws, stream, keep, &kept1));
      if (kept1 != f.kept.operand(i)) { set_error("deep_linear_fwd: layer %d %s its converted input, against the plan", i, kept1 ? "kept" : "did not keep"); return NC_ERR_ARG; }
    } else {
      NC_TRY(nc_conv_fwd(in, P + p.w[i], nullptr, out, N, l.C, S0, S1, S2, l.K, l.k, l.k, l.k, 1, l.k / 2, w.cws, p.conv_ws, stream));
    }
    in = out;
  }
  switch (f.form) {
    case kLTyped: {
      NC_TRY(dl_tail_compose(P + p.w[2], P + p.w[3], P + p.w[4], P + p.w[5], w.tail, hs));
      const float* F = dl_fold_fwd(w.tail, P + p.w[1], hs);
      if (!F) return NC_ERR_HIP;
      NC_TRY(dl_typed_compose(F, w.typed, N, S0, S1, S2, hs));
      NC_TRY(conv_c1k7_h2_dgrad(in, dl_typed_wp(w.typed, N, S0, S1, S2), y, f.cd, w.cws, p.conv_ws, hs));
      NC_TRY(dl_typed_fwd_boundary(in, y, w.typed, N, S0, S1, S2, hs));
      break;
    }
    case kLNoAct1: {
      NC_TRY(dl_tail_compose(P + p.w[2], P + p.w[3], P + p.w[4], P + p.w[5], w.tail, hs));
      const float* F = dl_fold_fwd(w.tail, P + p.w[1], hs);
      if (!F) return NC_ERR_HIP;
      float* Z = saved + p.act[1];  // (the slot act1 would take: 32 of its 64 channels)
      NC_TRY(conv_fwd_h2_k32_keep(in, F, Z, f.cd, w.cws, p.conv_ws, hs, saved + p.xs3[1]));
      NC_TRY(dl_combine27(Z, y, N, S0, S1, S2, 32, hs));
      break;
    }
    case kLTail:
      NC_TRY(dl_tail_compose(P + p.w[2], P + p.w[3], P + p.w[4], P + p.w[5], w.tail, hs));
      NC_TRY(conv_fwd_to1_k3(in, dl_tail_E(w.tail), y, N, 64, S0, S1, S2, w.cws, p.conv_ws, hs));
      break;
    case kLLayered:
      break;
  }
  if (kept) *kept = f.kept.w;
  return NC_OK;
}

// dx nullable; dparams overwritten
int nc_deep_linear_bwd(const float* params, const float* x, const float* saved, const float* dy, float* dx, float* dparams,
                       int N, int S0, int S1, int S2, void* ws, size_t ws_bytes, void* stream, unsigned kept) {
  NetworkScope net_scope;
  if (!params || !x || !saved || !dy || !dparams) { set_error("deep_linear_bwd: null pointer"); return NC_ERR_ARG; }
  LPlan p;
  if (!l_plan(p, N, S0, S1, S2)) { set_error("deep_linear_bwd: bad shape"); return NC_ERR_SHAPE; }
  const LWs w = l_ws(p, ws);
  if (!ws || ws_bytes < w.bytes) { set_error("deep_linear_bwd: workspace too small"); return NC_ERR_WS; }
  const LBwdForms f = l_bwd_forms(p, Kept{kept});
  if (f.error) { set_error("%s", f.error); return NC_ERR_ARG; }
  const float *P = params, *act0 = saved + p.act[0];
  float *DP = dparams, *g0 = w.G + p.g[0], *g1 = w.G + p.g[1];
  hipStream_t hs = (hipStream_t)stream;
  const float* g = dy;  // the gradient at the output of layer f.first
  switch (f.top) {
    case kLTopTyped: {
      ForceTwoTerm two_;
      NC_TRY(dl_tail_compose(P + p.w[2], P + p.w[3], P + p.w[4], P + p.w[5], w.tail, hs));
      const float* F = dl_fold_fwd(w.tail, P + p.w[1], hs);
      if (!F) return NC_ERR_HIP;
      NC_TRY(dl_typed_compose(F, w.typed, N, S0, S1, S2, hs));
      // dL/dact0: the 1 -> 64 convolution of dy with the interior kernel (the pseudo-channel forward kernel), then the boundary voxels' differences
      NC_TRY(conv_c1k7_h2(dy, dl_typed_wp(w.typed, N, S0, S1, S2), nullptr, g1, f.cd, w.cws, p.conv_ws, hs));
      NC_TRY(dl_typed_dgrad_boundary(act0, dy, g1, w.typed, N, S0, S1, S2, hs));
      // every parameter gradient through dH: the full correlation of dy and act0 (the one-channel 7^3 weight gradient with the operands' roles swapped)
      // and the boundary types' sums -> P, then weight space as in the rank forms
      NC_TRY(conv_wgrad_c1(dy, act0, dl_typed_dwsw(w.typed, N, S0, S1, S2), f.cd, w.cws, p.conv_ws, hs));
      NC_TRY(dl_typed_p(act0, dy, dl_tail_P(w.tail), w.typed, N, S0, S1, S2, hs));
      NC_TRY(dl_q_from_p(w.tail, P + p.w[1], hs));
      NC_TRY(dl_w1_contract(w.tail, DP + p.w[1], hs));
      NC_TRY(dl_tail_grads(P + p.w[2], P + p.w[3], P + p.w[4], P + p.w[5], w.tail, DP + p.w[2], DP + p.w[3], DP + p.w[4], DP + p.w[5], hs));
      g = g1;
      break;
    }
    case kLTopTail: {
      NC_TRY(dl_tail_compose(P + p.w[2], P + p.w[3], P + p.w[4], P + p.w[5], w.tail, hs));
      if (f.rank_w) {  // the shifted copies of dy in g1: free until layer 1's data gradient is written there, below
        NC_TRY(dl_shift27(dy, g1, N, S0, S1, S2, hs));
        NC_TRY(conv_wgrad_h2(g1, nullptr, nullptr, saved + p.xs3[1], dl_tail_P(w.tail), f.cd, w.cws, p.conv_ws, hs));
        NC_TRY(dl_q_from_p(w.tail, P + p.w[1], hs));
        NC_TRY(dl_w1_contract(w.tail, DP + p.w[1], hs));
      } else {
        const float* act1 = saved + p.act[1];
        if (f.remake_act1) {
          NC_TRY(nc_conv_fwd(act0, P + p.w[1], nullptr, g1, N, 64, S0, S1, S2, 64, 5, 5, 5, 1, 2, w.cws, p.conv_ws, stream));
          act1 = g1;
        }
        // q (tap-flipped): the weight gradient of Conv3d(1, 64, 3) with x := dy and dY := act1
        NC_TRY(nc_conv_wgrad(dy, act1, dl_tail_q(w.tail), nullptr, N, 1, S0, S1, S2, 64, 3, 3, 3, 1, 1, w.cws, p.conv_ws, stream));
      }
      NC_TRY(dl_tail_grads(P + p.w[2], P + p.w[3], P + p.w[4], P + p.w[5], w.tail, DP + p.w[2], DP + p.w[3], DP + p.w[4], DP + p.w[5], hs));
      if (f.g1) NC_TRY(nc_conv_fwd(dy, dl_tail_Ef(w.tail), nullptr, g0, N, 1, S0, S1, S2, 64, 3, 3, 3, 1, 1, w.cws, p.conv_ws, stream));
      g = g0;
      if (f.rank_w) {  // layer 1's data gradient (dW1 came out of P above); layer 0 needs it whether or not dx is wanted
        if (f.rank_dgrad) {
          const float* Wf = dl_w1_fold(w.tail, P + p.w[1], hs);
          if (!Wf) return NC_ERR_HIP;
          NC_TRY(conv_fwd_h2_c32(g1, Wf, g1, f.cd, w.cws, p.conv_ws, hs));  // (converts the shifted copies into cws first: the output is their buffer)
        } else {
          NC_TRY(nc_conv_dgrad(g0, P + p.w[1], g1, N, 64, S0, S1, S2, 64, 5, 5, 5, 1, 2, w.cws, p.conv_ws, stream));
        }
        g = g1;
      }
      break;
    }
    case kLTopLayered:
      break;
  }
  for (int i = f.first; i >= 0; --i) {
    const LLayer& l = kLL[i];
    const float* in = i == 0 ? x : saved + p.act[i - 1];
    float* gin = i == 0 ? dx : w.G + p.g[i & 1];
    if (l.k > 1)
      NC_TRY(conv_bwd_keep(in, f.xs[i] ? (const void*)(saved + p.xs3[i]) : nullptr, g, P + p.w[i], gin, DP + p.w[i], N, l.C, S0, S1, S2, l.K, l.k,
                           w.cws, p.conv_ws, stream));
    else
      NC_TRY(nc_conv_bwd(in, g, P + p.w[i], gin, DP + p.w[i], nullptr, N, l.C, S0, S1, S2, l.K, l.k, l.k, l.k, 1, l.k / 2, w.cws, p.conv_ws, stream));
    g = gin;
  }
  return NC_OK;
}

}  // extern "C"
