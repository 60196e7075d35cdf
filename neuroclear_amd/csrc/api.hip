// C-ABI glue: error reporting, the switches' setters and the convolution dispatch (MFMA implicit GEMM vs direct).
#include <cstring>
#include <vector>

#include <atomic>
#include <mutex>
#include <set>
#include <utility>

#include "common.hpp"

namespace nc {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int raise_dyn_lds(const void* kernel, int bytes, const char* who) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { set_error("%s: hipGetDevice failed", who); return NC_ERR_HIP; }
  std::lock_guard<std::mutex> g(mu);
  if (done.count({kernel, dev})) return NC_OK;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot raise dynamic LDS limit to %d bytes", who, bytes);
    return NC_ERR_HIP;
  }
  done.insert({kernel, dev});
  return NC_OK;
}


// ---- live launch profiler (bench.py): HIP events on the launch stream around every convolution entry point --------
struct ProfRec { int cls; double flop, abytes; hipEvent_t e0, e1; };
static std::mutex g_prof_mu;  // launches come from the main thread (forward) and the autograd engine's thread (backward)
static std::vector<ProfRec> g_prof;
static std::vector<hipEvent_t> g_prof_pool;
static std::atomic<bool> g_prof_on{false};
static double g_prof_min_flop = 0.0;

ProfScope::ProfScope(int op, int path, const ConvDims& d, int lp, hipStream_t stream) : idx(-1), s(stream) {
  if (!g_prof_on) return;
  const double flop = 2.0 * d.C * d.K * d.kd * d.kh * d.kw * ((double)d.N * d.Do * d.Ho * d.Wo);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (flop < g_prof_min_flop) return;
  auto get = [&]() {
    hipEvent_t e;
    if (!g_prof_pool.empty()) { e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
    if (hipEventCreate(&e) != hipSuccess) return (hipEvent_t) nullptr;
    return e;
  };
  // algorithmic bytes of the launch: every operand element once (4 B: fp32, or the two-term H2 form; 2 B on the 16-bit path; the three-term
  // form's 6 B is not the algorithm's doing) + the result + the weights
  const double xin = (double)d.N * d.C * d.D * d.H * d.W, yout = (double)d.N * d.K * d.Do * d.Ho * d.Wo, wts = (double)d.K * d.C * d.kd * d.kh * d.kw;
  const double eb = lp ? 2.0 : 4.0;
  const double abytes = op == 2 ? (xin + yout) * eb + wts * 4.0 : (op == 0 ? xin * eb + yout * 4.0 : yout * eb + xin * 4.0) + wts * 4.0;
  ProfRec r{op | (path << 4) | (d.kh << 8) | (lp ? 1 << 16 : 0), flop, abytes, get(), get()};
  if (!r.e0 || !r.e1) return;
  (void)hipEventRecord(r.e0, s);
  g_prof.push_back(r);
  idx = (int)g_prof.size() - 1;
}
ProfScope::~ProfScope() {
  if (idx < 0) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (idx < (int)g_prof.size()) (void)hipEventRecord(g_prof[idx].e1, s);
}

// ---- the layer dispatch (conv_route.hpp): ONE ordered list of rungs.  conv_route walks it, nc_conv_ws_bytes takes the maximum of its workspace
// column, and the `switch` of an entry point is the only other place a family is named.  gate: the switches that must be on.  pred / ws: per op
// (forward, data gradient, weight gradient); no predicate = no kernel for that op.  when: nc_conv_ws_bytes counts the row's workspace always, only
// where its predicate holds, only while its gate is open (kWsGated); kWsRequired: the CALL must bring it for the rung to be taken at all.
enum { kOnSplit = 1, kOnK3 = 2, kOnPg1 = 4, kOnImg = 8, kOnImgWgrad = 16 };
enum { kWsAlways = 0, kWsIfPred = 1, kWsGated = 2, kWsRequired = 4 };
struct Rung { ConvRung rung; int path; unsigned gate; bool (*pred[3])(const ConvDims&); size_t (*ws[3])(const ConvDims&); int when; };
static unsigned switches_on() {  // every switch of the dispatch but FORCE_DIRECT, read once
  return (sw::raw(sw::CONV_SPLIT) ? kOnSplit : 0) | (sw::raw(sw::CONV2D_K3) ? kOnK3 : 0) | (sw::raw(sw::PG1) ? kOnPg1 : 0) |
         (sw::raw(sw::SCONV) ? kOnImg : 0) | (sw::raw(sw::SCONV_WGRAD) ? kOnImgWgrad : 0);
}
static size_t s3_wgrad_bwd_ws_bytes(const ConvDims& d) {  // the weight gradient alone, or fused with the data gradient (nc_conv_bwd)
  return s3_wgrad_ws_bytes(d) > s3_bwd_ws_bytes(d) ? s3_wgrad_ws_bytes(d) : s3_bwd_ws_bytes(d);
}
static constexpr Rung kRungs[kRungCount] = {  // (in the order of enum ConvRung: the route tries them top down)
    // Split-operand kernels (conv_split.hip): the fp32 3^3 / 5^3 convolutions they cover as six bf16 MFMA products of an exact three-term operand
    // split, fp32 accumulation (tests/test_gpu_split.py).  nc_set_conv_split(0) / NC_CONV_SPLIT=0: these three rungs back on the fp32 kernels.
    {kRungS3, kPathSplit, kOnSplit, {s3_fwd_supported, s3_dgrad_supported, s3_wgrad_supported}, {s3_ws_bytes, s3_ws_bytes, s3_wgrad_bwd_ws_bytes}, kWsIfPred | kWsGated},
    {kRungP2d, kPathSplit2d, kOnSplit, {p2d_fwd_supported, p2d_dgrad_supported, p2d_wgrad_supported}, {p2d_ws_bytes, p2d_ws_bytes, p2d_wgrad_ws_bytes}, kWsGated},
    // Conv3d(1, 64, 7) in pseudo-channel form on the two-term kernels (conv_s3x.hip; data gradient: + fold); a call without its workspace moves on
    {kRungC1k7, kPathC1k7, kOnSplit, {c1k7_h2_supported, c1k7_h2_supported, nullptr}, {c1k7_h2_ws_bytes, c1k7_h2_dgrad_ws_bytes, nullptr}, kWsGated | kWsRequired},
    // Conv2d 3 x 3 of the 2-D generators, image-tiled (conv2d_k3.hip); nc_set_conv2d_k3(0): the gather GEMM (the packed weights stay counted)
    {kRungK3Img, kPathK3Img, kOnK3, {conv2d_k3_fwd_supported, conv2d_k3_dgrad_supported, nullptr}, {conv2d_k3_ws_bytes, conv2d_k3_ws_bytes, nullptr}, kWsAlways},
    {kRungC1k3, kPathMfma, 0, {c1k3_fwd_supported, nullptr, nullptr}, {}, kWsAlways},  // 1 -> K channels, 3^3: its own fp32 MFMA kernel
    {kRungBrick, kPathMfma, 0, {mfma_fwd_supported, mfma_dgrad_supported, mfma_wgrad_supported}, {mfma_ws_bytes, mfma_ws_bytes, mfma_ws_bytes}, kWsAlways},
    {kRungFlat, kPathFlat, 0, {flat_1x1_supported, flat_1x1_supported, wgrad_1x1_supported}, {nullptr, nullptr, wgrad_1x1_ws_bytes}, kWsAlways},
    {kRungTaps, kPathTaps, 0, {nullptr, nullptr, c1_wgrad_supported}, {nullptr, nullptr, c1_wgrad_ws_bytes}, kWsAlways},
    {kRungK1, kPathK1, 0, {k1_fwd_supported, nullptr, k1_wgrad_supported}, {}, kWsAlways},
    {kRungTo1Mfma, kPathTo1, 0, {nullptr, to1_mfma_supported, nullptr}, {nullptr, to1_mfma_ws_bytes, nullptr}, kWsAlways},
    {kRungTo1, kPathDirect, 0, {nullptr, to1_dgrad_supported, nullptr}, {}, kWsAlways},  // k_conv_to1: VALU, but not the direct kernel
    // NC_PG1=0: the PatchGAN's first layer back on the generic kernels (A/B runs)
    {kRungPg1, kPathPg1, kOnPg1, {pg1_supported, pg1_supported, pg1_supported}, {pg1_ws_bytes, pg1_ws_bytes, pg1_ws_bytes}, kWsIfPred},
    // NC_SCONV=0: the image-staged kernels of the PatchGAN layers off (A/B runs against the gather GEMM); NC_SCONV_WGRAD=0: the weight gradient's
    {kRungImg, kPathImg, kOnImg, {sconv_fwd_supported, sconv_dgrad_supported, nullptr}, {sconv_ws_bytes, sconv_ws_bytes, nullptr}, kWsIfPred},
    {kRungImgWgrad, kPathImg, kOnImg | kOnImgWgrad, {nullptr, nullptr, sconv_wgrad_supported}, {nullptr, nullptr, sconv_wgrad_ws_bytes}, kWsIfPred},
    {kRungGemm, kPathGemm, 0, {gemm_fwd_supported, gemm_dgrad_supported, gemm_wgrad_supported}, {gemm_ws_bytes, gemm_ws_bytes, gemm_ws_bytes}, kWsAlways},
    {kRungDirect, kPathDirect, 0, {}, {}, kWsAlways},  // what is left, and everything under nc_set_force_direct(1)
};
static_assert([] { for (int i = 0; i < kRungCount; ++i) if (kRungs[i].rung != i) return false; return true; }(), "kRungs follows enum ConvRung");
static const char* const kPathNames[16] = {"direct", "mfma", "gemm", "flat", "taps", "k1", "to1", "img", "pg1", "split", "split2d", "split", "lk", "k3img"};
static const char kWsGranted = 0;  // the host queries' workspace: (&kWsGranted, SIZE_MAX) is "whatever the rung needs is there"
int path_of(ConvRung r) { return kRungs[r].path; }
ConvRung conv_route(int op, const ConvDims& d, const void* ws, size_t ws_bytes, unsigned skip) {
  const unsigned on = switches_on();
  if (!sw::raw(sw::FORCE_DIRECT))
    for (const Rung& r : kRungs) {
      if (!r.pred[op] || (on & r.gate) != r.gate || (skip >> r.rung & 1) || !r.pred[op](d)) continue;
      if (!(r.when & kWsRequired) || (ws && ws_bytes >= r.ws[op](d))) return r.rung;
    }
  return kRungDirect;
}

}  // namespace nc

using namespace nc;

extern "C" {

void nc_prof_begin(double min_flop) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (ProfRec& r : g_prof) { g_prof_pool.push_back(r.e0); g_prof_pool.push_back(r.e1); }
  g_prof.clear();
  g_prof_min_flop = min_flop;
  g_prof_on = true;
}

// Stops recording, waits for the recorded launches and returns how many there were; the first `max` are written to
// cls / flop / ms (cls encoding: see ProfScope).  The caller synchronises the device first.
int nc_prof_end(int max, int* cls, double* flop, float* ms) { return nc_prof_end2(max, cls, flop, ms, nullptr); }
int nc_prof_end2(int max, int* cls, double* flop, float* ms, double* abytes) {
  g_prof_on = false;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  const int n = (int)g_prof.size();
  for (int i = 0; i < n && i < max; ++i) {
    float t = 0.f;
    (void)hipEventSynchronize(g_prof[i].e1);
    (void)hipEventElapsedTime(&t, g_prof[i].e0, g_prof[i].e1);
    cls[i] = g_prof[i].cls; flop[i] = g_prof[i].flop; ms[i] = t;
    if (abytes) abytes[i] = g_prof[i].abytes;
  }
  return n;
}

const char* nc_last_error(void) { return g_err; }
int nc_version(void) { return 100; }
// the switches of the C ABI over the one table (switches.hpp): a setter clamps by its row; the two frozen getters answer as the call sees them
void nc_set_force_direct(int on) { sw::set(sw::FORCE_DIRECT, on); }
void nc_sconv_set_cfg(int cfg) { sw::set(sw::SCONV_CFG_PIN, cfg); }
void nc_sconv_set_tune(int on) { sw::set(sw::SCONV_TUNE_MODE, on); }
void nc_set_conv_split(int on) { sw::set(sw::CONV_SPLIT, on); }
int nc_get_conv_split(void) { return sw::raw(sw::CONV_SPLIT); }
void nc_set_s3_fusion(int on) { sw::set(sw::S3_FUSE, on); }
void nc_set_split_terms(int terms) { sw::set(sw::SPLIT_TERMS, terms); }
int nc_get_split_terms(void) { return sw::get(sw::SPLIT_TERMS); }
void nc_set_epi_stats(int on) { sw::set(sw::EPI_STATS, on); }
int nc_get_epi_stats(void) { return sw::raw(sw::EPI_STATS); }
void nc_set_s3x_w64(int on) { sw::set(sw::S3X_W64, on); }
int nc_get_s3x_w64(void) { return sw::raw(sw::S3X_W64); }
void nc_set_p2d_terms(int mode) { sw::set(sw::P2D_TERMS, mode); }
int nc_get_p2d_terms(void) { return sw::raw(sw::P2D_TERMS); }
// (allocates the pinned counter block HERE, off the launch path: a first allocation inside h2_guard_decide could invalidate a stream capture)
void nc_set_h2_guard(int on) { sw::set(sw::H2_GUARD, on); if (on) (void)h2_guard_stats_dev(); }
int nc_get_h2_guard(void) { return sw::get(sw::H2_GUARD); }
void nc_set_c8x_mode(int mode) { sw::set(sw::C8X, mode); }
int nc_get_c8x_mode(void) { return sw::raw(sw::C8X); }
void nc_set_unet_wprep(int on) { sw::set(sw::UNET_WPREP, on); }
int nc_get_unet_wprep(void) { return sw::raw(sw::UNET_WPREP); }
void nc_set_unet_lean(int on) { sw::set(sw::UNET_LEAN, on); }
int nc_get_unet_lean(void) { return sw::raw(sw::UNET_LEAN); }
void nc_set_dl_collapse(int on) { sw::set(sw::DL_COLLAPSE, on); }
int nc_get_dl_collapse(void) { return sw::raw(sw::DL_COLLAPSE); }
int nc_set_in_bwd_fold(int on) { return sw::set(sw::IN_BWD_FOLD, on); }
int nc_get_in_bwd_fold(void) { return sw::raw(sw::IN_BWD_FOLD); }
int nc_set_stream_passes(int on) { return sw::set(sw::STREAM_PASSES, on); }
int nc_get_stream_passes(void) { return sw::raw(sw::STREAM_PASSES); }
int nc_set_conv2d_k3(int on) { return sw::set(sw::CONV2D_K3, on); }
int nc_get_conv2d_k3(void) { return sw::raw(sw::CONV2D_K3); }
int nc_conv2d_k3_set_cfg(int cfg) { return sw::set(sw::CONV2D_K3_CFG, cfg); }
int nc_h2_guard_stats(unsigned long long* out4, int reset) {
  if (!out4) { set_error("h2_guard_stats: null pointer"); return NC_ERR_ARG; }
  return h2_guard_read(out4, reset);
}

// Views of the route for callers that plan ahead.  Host arithmetic only.
int nc_conv2d_split_active(int what, int N, int C, int H, int W, int K, int k, int stride, int pad) {
  ConvDims d;
  return what >= 0 && what <= 2 && make_dims(d, N, C, 1, H, W, K, 1, k, k, stride, pad) && conv_route(what, d) == kRungP2d;
}
int nc_conv2d_k3_num_cfgs(void) { return conv2d_k3_num_cfgs(); }
int nc_conv2d_k3_active(int what, int N, int C, int H, int W, int K) {
  ConvDims d;
  return what >= 0 && what <= 2 && make_dims(d, N, C, 1, H, W, K, 1, 3, 3, 1, 1) && conv_route(what, d) == kRungK3Img;
}
// The path of a layer at a probe extent with batch 1 and every workspace granted.  The rungs that depend on the batch or the image, which these
// queries do not take, are not reported: such a layer answers with the rung behind them.
static int probe_path(int op, int C, int K, int kd, int kh, int kw, int stride, int pad, unsigned skip) {
  ConvDims d;
  const int e = (kd == 1 && kh == 1 && kw == 1) ? 256 : 32;  // pointwise: a plane large enough for the flat kernel
  return make_dims(d, 1, C, kd > 1 ? 32 : 1, e, e, K, kd, kh, kw, stride, pad) ? path_of(conv_route(op, d, &kWsGranted, SIZE_MAX, skip)) : -1;
}
int nc_conv_fwd_path(int C, int K, int kd, int kh, int kw, int stride, int pad) {
  return probe_path(0, C, K, kd, kh, kw, stride, pad, 1u << kRungP2d | 1u << kRungK3Img | 1u << kRungC1k3 | 1u << kRungK1 | 1u << kRungImg);
}
int nc_conv_wgrad_path(int C, int K, int kd, int kh, int kw, int stride, int pad) {
  return probe_path(2, C, K, kd, kh, kw, stride, pad, 1u << kRungP2d | 1u << kRungK1 | 1u << kRungPg1 | 1u << kRungImgWgrad);
}
int nc_conv_route(int op, int N, int C, int D, int H, int W, int K, int kd, int kh, int kw, int stride, int pad, size_t ws_bytes) {
  ConvDims d;
  if (op < 0 || op > 2 || !make_dims(d, N, C, D, H, W, K, kd, kh, kw, stride, pad)) return -1;
  const ConvRung r = conv_route(op, d, ws_bytes ? &kWsGranted : nullptr, ws_bytes);
  return path_of(r) | r << 8;
}
int nc_conv_path_name(int path, char* buf, int cap) {
  const char* name = (path >= 0 && path < 16) ? kPathNames[path] : nullptr;
  return (name && buf && cap > 0) ? snprintf(buf, (size_t)cap, "%s", name) : 0;  // (its length, also where cap cuts it)
}

int nc_conv_mfma_plan_debug(int what, int N, int C, int D, int H, int W, int K, int k, int* out) {
  ConvDims d;
  if (!out) { set_error("conv_mfma_plan_debug: null pointer"); return NC_ERR_ARG; }
  if (what < 0 || what > 2 || !make_dims(d, N, C, D, H, W, K, k, k, k, 1, k / 2)) { set_error("conv_mfma_plan_debug: bad arguments"); return NC_ERR_SHAPE; }
  if (what == 2 ? mfma_wgrad_plan_debug(d, out) : mfma_fwd_plan_debug(d, what, out)) return NC_OK;
  set_error("conv_mfma_plan_debug: the brick kernels do not take this layer");
  return NC_ERR_SHAPE;
}

size_t nc_conv_ws_bytes(int N, int C, int D, int H, int W, int K, int kd, int kh, int kw, int stride, int pad) {
  ConvDims d;
  if (!make_dims(d, N, C, D, H, W, K, kd, kh, kw, stride, pad)) return 0;
  const unsigned on = switches_on();
  size_t b = kBiasGradWsBytes;
  for (const Rung& r : kRungs)
    for (int op = 0; op < 3; ++op) {
      if (!r.ws[op] || ((r.when & kWsGated) && (on & r.gate) != r.gate) || ((r.when & kWsIfPred) && !r.pred[op](d))) continue;
      const size_t n = r.ws[op](d);
      if (n > b) b = n;
    }
  return (b + 255) & ~(size_t)255;
}

static int conv_args(const char* what, ConvDims& d, const void* a, const void* b, const void* c, int N, int C, int D,
                     int H, int W, int K, int kd, int kh, int kw, int stride, int pad) {
  if (!a || !b || !c) { set_error("%s: null pointer", what); return NC_ERR_ARG; }
  if (!make_dims(d, N, C, D, H, W, K, kd, kh, kw, stride, pad) || N > 65535) {
    set_error("%s: bad shape N=%d C=%d D=%d H=%d W=%d K=%d k=(%d,%d,%d) s=%d p=%d", what, N, C, D, H, W, K, kd, kh, kw,
              stride, pad);
    return NC_ERR_SHAPE;
  }
  return NC_OK;
}

int nc_conv_fwd(const float* x, const float* w, const float* bias, float* y, int N, int C, int D, int H, int W, int K,
                int kd, int kh, int kw, int stride, int pad, void* ws, size_t ws_bytes, void* stream) {
  ConvDims d;
  if (int e = conv_args("conv_fwd", d, x, w, y, N, C, D, H, W, K, kd, kh, kw, stride, pad)) return e;
  hipStream_t s = (hipStream_t)stream;
  const ConvRung rung = conv_route(0, d, ws, ws_bytes);
  ProfScope ps(0, path_of(rung), d, 0, s);
  switch (rung) {
    case kRungS3: return conv_fwd_s3(x, nullptr, w, bias, y, d, ws, ws_bytes, s);
    case kRungP2d: return conv_fwd_p2d(x, w, bias, y, d, ws, ws_bytes, s);
    case kRungC1k7: return conv_c1k7_h2(x, w, bias, y, d, ws, ws_bytes, s);
    case kRungK3Img: return conv_fwd_k3(x, w, bias, y, d, ws, ws_bytes, s);
    case kRungC1k3: return conv_fwd_c1k3(x, w, bias, y, d, s);
    case kRungBrick: return conv_fwd_mfma(x, w, bias, y, d, ws, ws_bytes, s);
    case kRungFlat: return conv_fwd_1x1(x, w, bias, y, d, ws, ws_bytes, s);
    case kRungK1: return conv_fwd_k1(x, w, bias, y, d, s);
    case kRungPg1: return conv_fwd_pg1(x, w, bias, y, d, 1.f, s);
    case kRungImg: return conv_fwd_sconv(x, w, bias, y, d, ws, ws_bytes, s);
    case kRungGemm: return conv_fwd_gemm(x, w, bias, y, d, ws, ws_bytes, s);
    default: return conv_fwd_direct(x, w, bias, y, d, s);
  }
}

int nc_conv_dgrad(const float* dy, const float* w, float* dx, int N, int C, int D, int H, int W, int K, int kd, int kh,
                  int kw, int stride, int pad, void* ws, size_t ws_bytes, void* stream) {
  ConvDims d;
  if (int e = conv_args("conv_dgrad", d, dy, w, dx, N, C, D, H, W, K, kd, kh, kw, stride, pad)) return e;
  hipStream_t s = (hipStream_t)stream;
  const ConvRung rung = conv_route(1, d, ws, ws_bytes);
  ProfScope ps(1, path_of(rung), d, 0, s);
  switch (rung) {
    case kRungS3: return conv_dgrad_s3(dy, nullptr, w, dx, d, ws, ws_bytes, s);
    case kRungP2d: return conv_dgrad_p2d(dy, w, dx, d, ws, ws_bytes, s);
    case kRungC1k7: return conv_c1k7_h2_dgrad(dy, w, dx, d, ws, ws_bytes, s);
    case kRungK3Img: return conv_dgrad_k3(dy, w, dx, d, ws, ws_bytes, s);
    case kRungBrick: return conv_dgrad_mfma(dy, w, dx, d, ws, ws_bytes, s);
    case kRungFlat: return conv_dgrad_1x1(dy, w, dx, d, ws, ws_bytes, s);
    case kRungTo1Mfma: return conv_dgrad_to1_mfma(dy, w, dx, d, ws, ws_bytes, s);
    case kRungTo1: return conv_dgrad_to1(dy, w, dx, d, s);
    case kRungPg1: return conv_dgrad_pg1(dy, nullptr, 1.f, w, dx, d, s);
    case kRungImg: return conv_dgrad_sconv(dy, w, dx, d, ws, ws_bytes, s);
    case kRungGemm: return conv_dgrad_gemm(dy, w, dx, d, ws, ws_bytes, s);
    default: return conv_dgrad_direct(dy, w, dx, d, s);
  }
}

int nc_conv_lp_supported(int what, int N, int C, int D, int H, int W, int K, int kd, int kh, int kw, int stride, int pad) {
  ConvDims d;
  if (!make_dims(d, N, C, D, H, W, K, kd, kh, kw, stride, pad)) return 0;
  return what == 0 ? h_fwd_supported(d) : what == 1 ? h_dgrad_supported(d) : what == 2 ? h_wgrad_supported(d) : 0;
}

size_t nc_conv_lp_ws_bytes(int N, int C, int D, int H, int W, int K, int kd, int kh, int kw, int stride, int pad) {
  ConvDims d;
  if (!make_dims(d, N, C, D, H, W, K, kd, kh, kw, stride, pad)) return 0;
  return h_ws_bytes(d);
}

static int lp_args(const char* what, ConvDims& d, const void* a, const void* ah, const void* b, const void* o, int N, int C,
                   int D, int H, int W, int K, int kd, int kh, int kw, int stride, int pad, int dtype) {
  if ((!a && !ah) || !b || !o) { set_error("%s: null pointer", what); return NC_ERR_ARG; }
  if (!make_dims(d, N, C, D, H, W, K, kd, kh, kw, stride, pad)) { set_error("%s: bad shape", what); return NC_ERR_SHAPE; }
  if (dtype != NC_DT_F16 && dtype != NC_DT_BF16) { set_error("%s: dtype must be NC_DT_F16 or NC_DT_BF16", what); return NC_ERR_ARG; }
  return NC_OK;
}

size_t nc_c8_bytes(int N, int C, long S) { return (C % 8 || N < 1 || S < 1) ? 0 : (size_t)N * C * S * 2; }

int nc_to_c8(const float* x, void* xh, int N, int C, long S, int dtype, void* stream) {
  if (!x || !xh) { set_error("to_c8: null pointer"); return NC_ERR_ARG; }
  if (N < 1 || C < 8 || C % 8 || S < 1) { set_error("to_c8: channels must be a multiple of 8"); return NC_ERR_SHAPE; }
  if (dtype != NC_DT_F16 && dtype != NC_DT_BF16) { set_error("to_c8: dtype must be NC_DT_F16 or NC_DT_BF16"); return NC_ERR_ARG; }
  return to_c8(x, xh, N, C, S, dtype, (hipStream_t)stream);
}

int nc_conv_fwd_lp(const float* x, const void* xh, const float* w, const float* bias, float* y, int N, int C, int D, int H,
                   int W, int K, int kd, int kh, int kw, int stride, int pad, int dtype, void* ws, size_t ws_bytes,
                   void* stream) {
  ConvDims d;
  if (int e = lp_args("conv_fwd_lp", d, x, xh, w, y, N, C, D, H, W, K, kd, kh, kw, stride, pad, dtype)) return e;
  if (!h_fwd_supported(d)) { set_error("conv_fwd_lp: shape not covered by the 16-bit kernels"); return NC_ERR_SHAPE; }
  ProfScope ps(0, kPathMfma, d, 1, (hipStream_t)stream);
  return conv_fwd_h(x, xh, w, bias, y, d, dtype, ws, ws_bytes, (hipStream_t)stream);
}

int nc_conv_dgrad_lp(const float* dy, const void* dyh, const float* w, float* dx, int N, int C, int D, int H, int W, int K,
                     int kd, int kh, int kw, int stride, int pad, int dtype, void* ws, size_t ws_bytes, void* stream) {
  ConvDims d;
  if (int e = lp_args("conv_dgrad_lp", d, dy, dyh, w, dx, N, C, D, H, W, K, kd, kh, kw, stride, pad, dtype)) return e;
  if (!h_dgrad_supported(d)) { set_error("conv_dgrad_lp: shape not covered by the 16-bit kernels"); return NC_ERR_SHAPE; }
  ProfScope ps(1, kPathMfma, d, 1, (hipStream_t)stream);
  return conv_dgrad_h(dy, dyh, w, dx, d, dtype, ws, ws_bytes, (hipStream_t)stream);
}

int nc_conv_wgrad_lp(const float* x, const void* xh, const float* dy, const void* dyh, float* dw, float* dbias, int N, int C,
                     int D, int H, int W, int K, int kd, int kh, int kw, int stride, int pad, int dtype, void* ws,
                     size_t ws_bytes, void* stream) {
  ConvDims d;
  if (int e = lp_args("conv_wgrad_lp", d, x, xh, dw, dw, N, C, D, H, W, K, kd, kh, kw, stride, pad, dtype)) return e;
  if (!dy && !dyh) { set_error("conv_wgrad_lp: null pointer"); return NC_ERR_ARG; }
  if (dbias && !dy) { set_error("conv_wgrad_lp: the bias gradient needs the fp32 dy"); return NC_ERR_ARG; }
  if (!h_wgrad_supported(d)) { set_error("conv_wgrad_lp: shape not covered by the 16-bit kernels"); return NC_ERR_SHAPE; }
  hipStream_t s = (hipStream_t)stream;
  {
    ProfScope ps(2, kPathMfma, d, 1, s);
    if (int e = conv_wgrad_h(x, xh, dy, dyh, dw, d, dtype, ws, ws_bytes, s)) return e;
  }
  if (dbias) return bias_grad(dy, dbias, d.N, d.K, (long)d.Do * d.Ho * d.Wo, ws, ws_bytes, s);  // fp32, from the fp32 dy
  return NC_OK;
}

int nc_conv_wgrad(const float* x, const float* dy, float* dw, float* dbias, int N, int C, int D, int H, int W, int K,
                  int kd, int kh, int kw, int stride, int pad, void* ws, size_t ws_bytes, void* stream) {
  ConvDims d;
  if (int e = conv_args("conv_wgrad", d, x, dy, dw, N, C, D, H, W, K, kd, kh, kw, stride, pad)) return e;
  hipStream_t s = (hipStream_t)stream;
  int e;
  {
    const ConvRung rung = conv_route(2, d, ws, ws_bytes);
    ProfScope ps(2, path_of(rung), d, 0, s);
    switch (rung) {
      case kRungS3: e = conv_wgrad_s3(x, nullptr, dy, nullptr, dw, d, ws, ws_bytes, s); break;
      case kRungP2d: e = conv_wgrad_p2d(x, dy, dw, d, ws, ws_bytes, s); break;
      case kRungBrick: e = conv_wgrad_mfma(x, dy, dw, d, ws, ws_bytes, s); break;
      case kRungFlat: e = conv_wgrad_1x1(x, dy, dw, d, ws, ws_bytes, s); break;
      case kRungTaps: e = conv_wgrad_c1(x, dy, dw, d, ws, ws_bytes, s); break;
      case kRungK1: e = conv_wgrad_k1(x, dy, dw, d, s); break;
      case kRungPg1: e = conv_wgrad_pg1(x, dy, nullptr, 1.f, dw, dbias, d, ws, ws_bytes, s); dbias = nullptr; break;  // (a column of the same product)
      case kRungImgWgrad: e = conv_wgrad_sconv(x, dy, dw, d, ws, ws_bytes, s); break;
      case kRungGemm: e = conv_wgrad_gemm(x, dy, dw, d, ws, ws_bytes, s); break;
      default: e = conv_wgrad_direct(x, dy, dw, d, s);
    }
  }
  if (e) return e;
  return dbias ? bias_grad(dy, dbias, d.N, d.K, (long)d.Do * d.Ho * d.Wo, ws, ws_bytes, s) : NC_OK;
}

// ---- ReflectionPad2d(1) + Conv2d(C, K, 3) of a ResnetBlock (reference models/networks.py:808-830) as one layer.  Workspace:
// [the padded input / the extended data gradient, N C (H + 2)(W + 2) floats][the convolution's own workspace].
static size_t k3r_pad_bytes(int N, int C, int H, int W) { return ((size_t)N * C * (H + 2) * (W + 2) * sizeof(float) + 255) & ~(size_t)255; }
static int k3r_args(const char* what, ConvDims& d, const void* a, const void* b, const void* c, int N, int C, int H, int W, int K, void* ws,
                    size_t ws_bytes) {
  if (int e = conv_args(what, d, a, b, c, N, C, 1, H, W, K, 1, 3, 3, 1, 1)) return e;
  if (!conv2d_k3_reflect_ok(d)) { set_error("%s: bad shape N=%d C=%d H=%d W=%d K=%d (a mirror needs H, W >= 2)", what, N, C, H, W, K); return NC_ERR_SHAPE; }
  if (!ws || ws_bytes < nc_conv2d_k3_reflect_ws_bytes(N, C, H, W, K)) { set_error("%s: workspace too small", what); return NC_ERR_WS; }
  return NC_OK;
}

size_t nc_conv2d_k3_reflect_ws_bytes(int N, int C, int H, int W, int K) {
  ConvDims d;
  if (!make_dims(d, N, C, 1, H, W, K, 1, 3, 3, 1, 1) || !conv2d_k3_reflect_ok(d)) return 0;
  size_t b = nc_conv_ws_bytes(N, C, 1, H + 2, W + 2, K, 1, 3, 3, 1, 0);  // the fallback: the explicitly padded image, padding 0
  if (conv2d_k3_ws_bytes(d) > b) b = conv2d_k3_ws_bytes(d);               // the tiled kernel's packed weights
  return k3r_pad_bytes(N, C, H, W) + b;
}

// the zero-padded layer's coverage rule and switches (nc_conv2d_k3_active), and a second pixel to mirror
int nc_conv2d_k3_reflect_active(int what, int N, int C, int H, int W, int K) {
  return (H >= 2 && W >= 2 && (what == 0 || what == 1)) ? nc_conv2d_k3_active(what, N, C, H, W, K) : 0;
}

int nc_conv2d_k3_reflect_fwd(const float* x, const float* w, const float* bias, float* y, int N, int C, int H, int W, int K, void* ws,
                             size_t ws_bytes, void* stream) {
  ConvDims d;
  if (int e = k3r_args("conv2d_k3_reflect_fwd", d, x, w, y, N, C, H, W, K, ws, ws_bytes)) return e;
  hipStream_t s = (hipStream_t)stream;
  const size_t pb = k3r_pad_bytes(N, C, H, W);
  if (nc_conv2d_k3_reflect_active(0, N, C, H, W, K)) {
    ProfScope ps(0, kPathK3Img, d, 0, s);
    return conv_fwd_k3_reflect(x, w, bias, y, d, (char*)ws + pb, ws_bytes - pb, s);
  }
  if (int e = reflect_pad_fwd(x, (float*)ws, (long)N * C, H, W, 1, s)) return e;
  return nc_conv_fwd((const float*)ws, w, bias, y, N, C, 1, H + 2, W + 2, K, 1, 3, 3, 1, 0, (char*)ws + pb, ws_bytes - pb, stream);
}

int nc_conv2d_k3_reflect_dgrad(const float* dy, const float* w, float* dx, int N, int C, int H, int W, int K, void* ws, size_t ws_bytes,
                               void* stream) {
  ConvDims d;
  if (int e = k3r_args("conv2d_k3_reflect_dgrad", d, dy, w, dx, N, C, H, W, K, ws, ws_bytes)) return e;
  hipStream_t s = (hipStream_t)stream;
  const size_t pb = k3r_pad_bytes(N, C, H, W);
  float* dxe = (float*)ws;  // the gradient at the padded input, [N][C][H + 2][W + 2]
  if (nc_conv2d_k3_reflect_active(1, N, C, H, W, K)) {
    ProfScope ps(1, kPathK3Img, d, 0, s);
    if (int e = conv_dgrad_k3_reflect_ext(dy, w, dxe, d, (char*)ws + pb, ws_bytes - pb, s)) return e;
  } else {
    if (int e = nc_conv_dgrad(dy, w, dxe, N, C, 1, H + 2, W + 2, K, 1, 3, 3, 1, 0, (char*)ws + pb, ws_bytes - pb, stream)) return e;
  }
  return reflect_pad_bwd(dxe, dx, (long)N * C, H, W, 1, s);
}

int nc_conv2d_k3_reflect_wgrad(const float* x, const float* dy, float* dw, float* dbias, int N, int C, int H, int W, int K, void* ws,
                               size_t ws_bytes, void* stream) {
  ConvDims d;
  if (int e = k3r_args("conv2d_k3_reflect_wgrad", d, x, dy, dw, N, C, H, W, K, ws, ws_bytes)) return e;
  const size_t pb = k3r_pad_bytes(N, C, H, W);
  if (int e = reflect_pad_fwd(x, (float*)ws, (long)N * C, H, W, 1, (hipStream_t)stream)) return e;
  return nc_conv_wgrad((const float*)ws, dy, dw, dbias, N, C, 1, H + 2, W + 2, K, 1, 3, 3, 1, 0, (char*)ws + pb, ws_bytes - pb, stream);
}

// dY to S3 form once, then the data gradient (dx nullable) and the weight gradient (xs nullable: the input already in S3 form) from it
static int bwd_s3_fused(const float* x, const void* xs, const float* dy, const float* w, float* dx, float* dw, const ConvDims& d, void* ws,
                        size_t ws_bytes, hipStream_t s) {
  {
    ProfScope ps(1, kPathSplit, d, 0, s);
    if (int e = conv_bwd_s3(x, dy, w, dx, dw, d, ws, ws_bytes, s, 0)) return e;
    if (dx)
      if (int e = conv_bwd_s3(x, dy, w, dx, dw, d, ws, ws_bytes, s, 1)) return e;
  }
  ProfScope ps(2, kPathSplit, d, 0, s);
  return conv_bwd_s3(x, dy, w, dx, dw, d, ws, ws_bytes, s, 2, xs);
}

// Backward of one convolution layer: dx (nullable) and dw (+ dbias) from x, dy, w.  The same results as nc_conv_dgrad followed
// by nc_conv_wgrad; on the split-operand kernels dY is converted to its three-term form once for both.
int nc_conv_bwd(const float* x, const float* dy, const float* w, float* dx, float* dw, float* dbias, int N, int C, int D, int H, int W,
                int K, int kd, int kh, int kw, int stride, int pad, void* ws, size_t ws_bytes, void* stream) {
  ConvDims d;
  if (int e = conv_args("conv_bwd", d, x, dy, dw, N, C, D, H, W, K, kd, kh, kw, stride, pad)) return e;
  if (!w) { set_error("conv_bwd: null pointer"); return NC_ERR_ARG; }
  hipStream_t s = (hipStream_t)stream;
  SwitchScope switches_;  // the three phases below see ONE value of every arithmetic switch
  if (dx && conv_route(1, d) == kRungS3 && conv_route(2, d) == kRungS3 && ws && s3_bwd_ws_bytes(d) && ws_bytes >= s3_bwd_ws_bytes(d)) {
    if (int e = bwd_s3_fused(x, nullptr, dy, w, dx, dw, d, ws, ws_bytes, s)) return e;
    return dbias ? bias_grad(dy, dbias, d.N, d.K, (long)d.Do * d.Ho * d.Wo, ws, ws_bytes, s) : NC_OK;
  }
  if (dx)
    if (int e = nc_conv_dgrad(dy, w, dx, N, C, D, H, W, K, kd, kh, kw, stride, pad, ws, ws_bytes, stream)) return e;
  return nc_conv_wgrad(x, dy, dw, dbias, N, C, D, H, W, K, kd, kh, kw, stride, pad, ws, ws_bytes, stream);
}

}  // extern "C"

namespace nc {
int conv_fwd_keep(const float* x, const float* w, const float* bias, float* y, int N, int C, int D, int H, int W, int K, int ks,
                  void* ws, size_t ws_bytes, void* stream, void* xs_keep, bool* kept, const S3xPrepared* prep) {
  ConvDims d;
  *kept = false;
  if (xs_keep && make_dims(d, N, C, D, H, W, K, ks, ks, ks, 1, ks / 2) && conv_route(0, d) == kRungS3 && conv_route(2, d) == kRungS3) {
    if (!x || !w || !y) { set_error("conv_fwd: null pointer"); return NC_ERR_ARG; }
    ProfScope ps(0, kPathSplit, d, 0, (hipStream_t)stream);
    *kept = true;
    return conv_fwd_s3(x, nullptr, w, bias, y, d, ws, ws_bytes, (hipStream_t)stream, xs_keep, nullptr, prep);
  }
  return nc_conv_fwd(x, w, bias, y, N, C, D, H, W, K, ks, ks, ks, 1, ks / 2, ws, ws_bytes, stream);
}

// Does the 3^3 / 5^3 layer run forward AND weight gradient on the split-operand kernels (then producers may hand it its input in S3 form)?
bool conv_keep_supported(int N, int C, int D, int H, int W, int K, int ks) {
  ConvDims d;
  return make_dims(d, N, C, D, H, W, K, ks, ks, ks, 1, ks / 2) && conv_route(0, d) == kRungS3 && conv_route(2, d) == kRungS3;
}
// ... the forward alone (the inference forward, unet_fwd.hip)?
bool conv_fwd_on_split(int N, int C, int D, int H, int W, int K, int ks) {
  ConvDims d;
  return make_dims(d, N, C, D, H, W, K, ks, ks, ks, 1, ks / 2) && conv_route(0, d) == kRungS3;
}

// The 1 x 1 layer behind an InstanceNorm + (Leaky)ReLU without the stored activation (conv_1x1.hip, the NORM forms): taken only where nc_conv_fwd
// AND nc_conv_wgrad would put the layer on the two flat kernels now, whose products and order the forms keep.
bool norm_1x1_taken(int N, int C, int D, int H, int W, int K) {
  ConvDims d;
  return make_dims(d, N, C, D, H, W, K, 1, 1, 1, 1, 0) && conv_route(0, d) == kRungFlat && conv_route(2, d) == kRungFlat && norm_1x1_supported(d);
}
int conv_fwd_norm_1x1(const float* raw, const float* mean, const float* rstd, float slope, const float* w, const float* bias, float* y, int N, int C,
                      int D, int H, int W, int K, void* ws, size_t ws_bytes, void* stream) {
  ConvDims d;
  if (int e = conv_args("conv_fwd_norm_1x1", d, raw, w, y, N, C, D, H, W, K, 1, 1, 1, 1, 0)) return e;
  if (!mean || !rstd) { set_error("conv_fwd_norm_1x1: null pointer"); return NC_ERR_ARG; }
  ProfScope ps(0, kPathFlat, d, 0, (hipStream_t)stream);
  return conv_fwd_1x1_norm(raw, mean, rstd, slope, w, bias, y, d, ws, ws_bytes, (hipStream_t)stream);
}
int conv_wgrad_norm_1x1(const float* raw, const float* mean, const float* rstd, float slope, const float* dy, float* dw, float* dbias, int N, int C,
                        int D, int H, int W, int K, void* ws, size_t ws_bytes, void* stream) {
  ConvDims d;
  if (int e = conv_args("conv_wgrad_norm_1x1", d, raw, dy, dw, N, C, D, H, W, K, 1, 1, 1, 1, 0)) return e;
  if (!mean || !rstd) { set_error("conv_wgrad_norm_1x1: null pointer"); return NC_ERR_ARG; }
  hipStream_t s = (hipStream_t)stream;
  {
    ProfScope ps(2, kPathFlat, d, 0, s);
    if (int e = conv_wgrad_1x1_norm(raw, mean, rstd, slope, dy, dw, d, ws, ws_bytes, s)) return e;
  }
  if (dbias) return bias_grad(dy, dbias, d.N, d.K, (long)d.Do * d.Ho * d.Wo, ws, ws_bytes, s);  // (as nc_conv_wgrad)
  return NC_OK;
}

// forward of such a layer whose input already exists in S3 form (written by the producer: act_split3 / split3_into)
int conv_fwd_pre(const void* xs, const float* w, const float* bias, float* y, int N, int C, int D, int H, int W, int K, int ks, void* ws,
                 size_t ws_bytes, void* stream, float* stats_part, const S3xPrepared* prep) {
  ConvDims d;
  if (!xs || !w || !y) { set_error("conv_fwd_pre: null pointer"); return NC_ERR_ARG; }
  if (!make_dims(d, N, C, D, H, W, K, ks, ks, ks, 1, ks / 2) || conv_route(0, d) != kRungS3) { set_error("conv_fwd_pre: layer not on the split-operand kernels"); return NC_ERR_SHAPE; }
  ProfScope ps(0, kPathSplit, d, 0, (hipStream_t)stream);
  if (stats_part && !(conv_layer_h2(d) && ks == 3)) { set_error("conv_fwd_pre: epilogue statistics exist for the two-term 3^3 layers only"); return NC_ERR_ARG; }
  return conv_fwd_s3(nullptr, xs, w, bias, y, d, ws, ws_bytes, (hipStream_t)stream, nullptr, stats_part, prep);
}

// Can the backward of the layer take dY in S3 form at the head of its workspace (conv_bwd_pre)?  want_dx: the data gradient is needed too
bool conv_bwd_pre_supported(int N, int C, int D, int H, int W, int K, int ks, bool want_dx, size_t ws_bytes) {
  ConvDims d;
  return make_dims(d, N, C, D, H, W, K, ks, ks, ks, 1, ks / 2) && conv_route(2, d) == kRungS3 && s3_bwd_ws_bytes(d) && ws_bytes >= s3_bwd_ws_bytes(d) &&
         (!want_dx || conv_route(1, d) == kRungS3);
}
// data (dx nullable) + weight gradient with dY ALREADY in S3 form at the start of ws (where conv_bwd_s3's conversion phase puts it);
// xs (nullable): the layer's input in S3 form, else it is converted from x
int conv_bwd_pre(const float* x, const void* xs, const float* w, float* dx, float* dw, int N, int C, int D, int H, int W, int K, int ks,
                 void* ws, size_t ws_bytes, void* stream, bool dy_guarded, const S3xPrepared* prep) {
  ConvDims d;
  hipStream_t s = (hipStream_t)stream;
  if (!conv_bwd_pre_supported(N, C, D, H, W, K, ks, dx != nullptr, ws_bytes) || !make_dims(d, N, C, D, H, W, K, ks, ks, ks, 1, ks / 2)) {
    set_error("conv_bwd_pre: layer not on the split-operand kernels");
    return NC_ERR_SHAPE;
  }
  if ((!x && !xs) || !w || !dw || !ws) { set_error("conv_bwd_pre: null pointer"); return NC_ERR_ARG; }
  if (dx) {
    ProfScope ps(1, kPathSplit, d, 0, s);
    if (int e = conv_bwd_s3(x, nullptr, w, dx, dw, d, ws, ws_bytes, s, 1, nullptr, dy_guarded, prep)) return e;
  }
  ProfScope ps(2, kPathSplit, d, 0, s);
  return conv_bwd_s3(x, nullptr, w, dx, dw, d, ws, ws_bytes, s, 2, xs, dy_guarded);
}

int conv_bwd_keep(const float* x, const void* xs, const float* dy, const float* w, float* dx, float* dw, int N, int C, int D, int H,
                  int W, int K, int ks, void* ws, size_t ws_bytes, void* stream) {
  ConvDims d;
  if (xs && ws && conv_bwd_pre_supported(N, C, D, H, W, K, ks, dx != nullptr, ws_bytes) && make_dims(d, N, C, D, H, W, K, ks, ks, ks, 1, ks / 2)) {
    if (!x || !dy || !w || !dw) { set_error("conv_bwd: null pointer"); return NC_ERR_ARG; }
    return bwd_s3_fused(x, xs, dy, w, dx, dw, d, ws, ws_bytes, (hipStream_t)stream);
  }
  return nc_conv_bwd(x, dy, w, dx, dw, nullptr, N, C, D, H, W, K, ks, ks, ks, 1, ks / 2, ws, ws_bytes, stream);
}
}  // namespace nc

// Test exports of the 1 x 1 layer that normalises its operand as it reads it (conv_1x1.hip, the NORM forms; tests/test_gpu_unet_lean2.py): the
// calls the U-Net training step issues for one_by_one, refused (NC_ERR_SHAPE) where the step would not take them.
extern "C" {
int nc_conv_fwd_norm_1x1_debug(const float* raw, const float* mean, const float* rstd, float slope, const float* w, const float* bias, float* y, int N,
                               int C, int D, int H, int W, int K, void* ws, size_t ws_bytes, void* stream) {
  if (!norm_1x1_taken(N, C, D, H, W, K)) { set_error("conv_fwd_norm_1x1_debug: the flat 1 x 1 kernels do not take this layer"); return NC_ERR_SHAPE; }
  return conv_fwd_norm_1x1(raw, mean, rstd, slope, w, bias, y, N, C, D, H, W, K, ws, ws_bytes, stream);
}
int nc_conv_wgrad_norm_1x1_debug(const float* raw, const float* mean, const float* rstd, float slope, const float* dy, float* dw, float* dbias, int N,
                                 int C, int D, int H, int W, int K, void* ws, size_t ws_bytes, void* stream) {
  if (!norm_1x1_taken(N, C, D, H, W, K)) { set_error("conv_wgrad_norm_1x1_debug: the flat 1 x 1 kernels do not take this layer"); return NC_ERR_SHAPE; }
  return conv_wgrad_norm_1x1(raw, mean, rstd, slope, dy, dw, dbias, N, C, D, H, W, K, ws, ws_bytes, stream);
}
}  // extern "C"
