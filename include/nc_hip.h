/*
 * nc_hip.h -- C ABI of libnc_hip.so: the MI355X (gfx950) hot path of Neuroclear.
 *
 * The reference (peterhpark/neuroclear) has NO native / FFI interface: its hot path is torch.nn modules executed by
 * cuDNN/ATen.  Each entry point below therefore cites the reference *call site* it replaces
 * (paths relative to the reference checkout), and INTEGRATION.md shows the ctypes stub a maintainer adds.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch tensors on the Python side), dense, fp32 unless
 *    the name says otherwise; activations are NCDHW (2-D data: D = 1, kd = 1);
 *  - `stream` is a hipStream_t passed as void*; nothing here allocates or frees, and nothing synchronises -- with ONE exception:
 *    the image-staged PatchGAN kernels (nc_conv_* on 2-D 4x4 layers at large batches, conv2d_img.hip) time their candidate tile
 *    shapes on the FIRST call of a problem shape: a hipDeviceSynchronize plus a few timed launches, skipped when the stream is
 *    being captured.  nc_sconv_set_tune(0) (or NC_SCONV_TUNE=0) switches that off for the whole process: then the rule holds
 *    without exception (a fixed heuristic picks the shape; results are bit-identical either way);
 *  - process-wide switches (nc_set_conv_split, nc_set_c8x_mode, nc_set_s3_fusion, nc_sconv_set_tune, nc_sconv_set_cfg, nc_set_force_direct) are
 *    atomics read once per call: flip them between calls, not while other host threads are inside the library;
 *  - scratch memory comes from the caller: `ws` / `ws_bytes`; query the size with the matching *_ws_bytes();
 *  - return value: 0 = ok, negative = NC_ERR_*; nc_last_error() gives a thread-local message.
 */
#ifndef NC_HIP_H
#define NC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NC_OK 0
#define NC_ERR_SHAPE (-1)  /* unsupported / inconsistent dimensions                       */
#define NC_ERR_WS (-2)     /* workspace missing or too small                              */
#define NC_ERR_HIP (-3)    /* a HIP runtime call failed (message has hipGetErrorString)   */
#define NC_ERR_ARG (-4)    /* null pointer / bad enum                                     */

const char* nc_last_error(void);
int nc_version(void);
/* Which implementation nc_conv_* would pick for a shape: 0 = direct (VALU), 1 = MFMA brick implicit GEMM (3^3/5^3,
 * stride 1), 2 = MFMA gather implicit GEMM (any kernel / stride), 3 = flat-voxel MFMA kernel of the 1x1 weight
 * gradient (<= 64 channels, planes of >= 16384 voxels), 4 = tap-axis MFMA kernel of the 1 -> 64 channel weight
 * gradient (3^3 / 7^3, W % 4 == 0), ... -- the path field of the profiler's cls; nc_conv_path_name gives the tag of every number.  The query
 * assumes batch 1, a 256^2 plane for pointwise kernels, a 32^2 image / 32^3 volume otherwise, and a sufficient workspace; kernels whose
 * coverage depends on the batch or the image (5, 7, 10, 13, the one-channel 3^3 kernel among the 1s; 8 for the weight gradient) are not
 * reported: the answer is the one behind them. */
int nc_conv_fwd_path(int C, int K, int kd, int kh, int kw, int stride, int pad);
int nc_conv_wgrad_path(int C, int K, int kd, int kh, int kw, int stride, int pad);
/* What nc_conv_fwd (op 0), nc_conv_dgrad (1) or nc_conv_wgrad (2) launch for exactly this layer under the switches as they are, called with a
 * workspace of ws_bytes (0: ws = NULL): path | rung << 8, or -1 for dimensions the entry points refuse.  rung: the kernel family in the order
 * the dispatch tries them (csrc/conv_route.hpp ConvRung; finer than the path).  Host arithmetic, launches nothing. */
int nc_conv_route(int op, int N, int C, int D, int H, int W, int K, int kd, int kh, int kw, int stride, int pad, size_t ws_bytes);
/* The tag of a profiler path (0 'direct', 1 'mfma', ... 12 'lk', 13 'k3img'; 9 and 11 are both 'split') copied to buf (cap bytes with the
 * terminator); returns its length, 0 for a number no kernel reports. */
int nc_conv_path_name(int path, char* buf, int cap);
/* Test query (tests/test_gpu_conv_fp32.py): which variant of the fp32 brick kernels (csrc/conv_mfma_fwd.hip, conv_mfma_wgrad.hip) a k^3, stride 1,
 * padding k / 2 layer takes; launches nothing.  out: 8 ints (host).  what = 0 forward, 1 data gradient: cfg (0 .. 4: waves along M x waves along
 * N x position blocks 8x1x4, 8x1x2, 4x2x2, 2x4x2, 2x4x1), CK, Tz, Ty, 1 for the TAIL kernels (W % 4 != 0), nchunks, units (stream-K: tiles x
 * nchunks over 256 workgroups), tiles.  what = 2 weight gradient: kernel (0 k_wgrad_rows<3>, 1 k_wgrad_dma<KS, AB>, 2 k_wgrad_mfma<KS, AB>), KS,
 * AB (kernel 0: rows per step), column blocks (kernel 1), parts, G, 0, 0.  NC_ERR_SHAPE where the brick kernels do not take the layer (a data
 * gradient with K = 1 among them: the single-channel mode is forward only). */
int nc_conv_mfma_plan_debug(int what, int N, int C, int D, int H, int W, int K, int k, int* out);
/* Live launch profiler (bench.py's `roofline`): between nc_prof_begin and nc_prof_end every convolution entry point of
 * >= min_flop algorithmic FLOP is bracketed by HIP events on the stream it is launched on.  nc_prof_end returns the number
 * of recorded calls and fills the first `max`: cls = op (0 fwd, 1 dgrad, 2 wgrad) | path << 4 | kernel edge << 8 |
 * (16-bit kernel ? 1 << 16 : 0), flop = 2 C K kd kh kw x output voxels, ms = event-to-event duration.  Synchronise first. */
void nc_prof_begin(double min_flop);
int nc_prof_end(int max, int* cls, double* flop, float* ms);
int nc_prof_end2(int max, int* cls, double* flop, float* ms, double* abytes); /* + the launch's algorithmic bytes: operands once (4 B; 2 B on the
                                   * 16-bit path), result, weights */
/* Force the direct path everywhere (tests cross-check MFMA vs direct on the GPU). 0 = auto (default), 1 = force. */
void nc_set_force_direct(int on);
/* The image-staged PatchGAN kernels (conv2d_img.hip) pick their tile shape per problem by timing the candidates on the
 * first call (NC_SCONV_TUNE=0: a fixed heuristic).  Every shape gives the same bits; this pins shape `cfg` (0-based, -1 =
 * back to automatic) so that a test can check exactly that. */
void nc_sconv_set_cfg(int cfg);
/* 1 (default; NC_SCONV_TUNE): time the candidate shapes on the first call of a problem shape (synchronises once per shape, see
 * Conventions); 0: never time, never synchronise -- the heuristic shape; -1: back to the environment's choice. */
void nc_sconv_set_tune(int on);

/* ---- Convolution: nn.Conv3d / nn.Conv2d (models/networks.py:361-369; used at :420-425,:442,:460-469 (U-Net 3^3),
 *      :899-911 (deep_linear 7^3/5^3/3^3/1^3), :507-508 (1x1 tail), :1030-1057 (PatchGAN 4x4 s2/s1)).
 *      x[N,C,D,H,W], w[K,C,kd,kh,kw], bias[K] or NULL, y[N,K,Do,Ho,Wo]; Do = (D+2p-kd)/s+1 (p,s apply to depth only
 *      when kd > 1).  dgrad / wgrad are the autograd backward of the same call (loss.backward(), apollo:283).      */
size_t nc_conv_ws_bytes(int N, int C, int D, int H, int W, int K, int kd, int kh, int kw, int stride, int pad);
int nc_conv_fwd(const float* x, const float* w, const float* bias, float* y, int N, int C, int D, int H, int W,
                int K, int kd, int kh, int kw, int stride, int pad, void* ws, size_t ws_bytes, void* stream);
int nc_conv_dgrad(const float* dy, const float* w, float* dx, int N, int C, int D, int H, int W, int K, int kd,
                  int kh, int kw, int stride, int pad, void* ws, size_t ws_bytes, void* stream);
int nc_conv_wgrad(const float* x, const float* dy, float* dw, float* dbias /* or NULL */, int N, int C, int D, int H,
                  int W, int K, int kd, int kh, int kw, int stride, int pad, void* ws, size_t ws_bytes, void* stream);
/* Backward of one layer in one call: dx (or NULL) and dw (+ dbias or NULL) -- nc_conv_dgrad followed by nc_conv_wgrad with
 * the conversions of dy shared where the kernels have one (nn.Conv3d backward, same call sites). */
int nc_conv_bwd(const float* x, const float* dy, const float* w, float* dx, float* dw, float* dbias, int N, int C, int D, int H, int W,
                int K, int kd, int kh, int kw, int stride, int pad, void* ws, size_t ws_bytes, void* stream);

/* Conv2d(k 3, s 1, p 1) of the 2-D generators (networks.py:413-476 with dimension == 2): nc_conv_fwd / nc_conv_dgrad run such a layer on the
 * image-tiled fp32 matrix-core kernel of csrc/conv2d_k3.hip where it covers the shape -- reduction side (C forward, K backward) even and >= 16,
 * output side a multiple of 64, enough tiles to fill the chip -- and on the gather GEMM otherwise.  nc_set_conv2d_k3(0) puts every such layer
 * back on the gather GEMM (process-wide, default 1, no environment variable; nc_set_force_direct(1) overrides it).  nc_conv2d_k3_active: does
 * the call with these dimensions take the kernel right now (what: 0 forward, 1 data gradient)?  nc_conv2d_k3_set_cfg(i) pins tile configuration
 * i of nc_conv2d_k3_num_cfgs() (tests: every configuration gives the same bits), -1 returns to the launcher's choice.                        */
int nc_set_conv2d_k3(int on);                 /* returns the previous setting */
int nc_get_conv2d_k3(void);
int nc_conv2d_k3_active(int what, int N, int C, int H, int W, int K);
int nc_conv2d_k3_set_cfg(int cfg);            /* returns the previous pin */
int nc_conv2d_k3_num_cfgs(void);

/* ---- The ResNet generators (networks.py:724-837, --netG resnet_6blocks | resnet_9blocks; 2-D only).
 *      ReflectionPad2d(1) + Conv2d(C, K, 3) of a ResnetBlock (networks.py:808-830) as ONE layer: x[N,C,H,W], w[K,C,3,3], bias[K] or NULL, y[N,K,H,W],
 *      H, W >= 2.  Where nc_conv2d_k3_active covers the zero-padded layer of the same dimensions (same rule, same switches nc_set_conv2d_k3 /
 *      nc_conv2d_k3_set_cfg), forward and data gradient run on the image-tiled kernel of csrc/conv2d_k3.hip: the forward with mirrored halo slots, the
 *      data gradient as the zero-padded data gradient on the (H + 2) x (W + 2) domain followed by the fold of nc_reflect_pad2d_bwd.  Elsewhere the same
 *      entry points pad explicitly into the workspace and call nc_conv_* with padding 0; the weight gradient always does.  Run-to-run identical bits. */
size_t nc_conv2d_k3_reflect_ws_bytes(int N, int C, int H, int W, int K);
int nc_conv2d_k3_reflect_active(int what, int N, int C, int H, int W, int K); /* what: 0 forward, 1 data gradient */
int nc_conv2d_k3_reflect_fwd(const float* x, const float* w, const float* bias, float* y, int N, int C, int H, int W, int K,  /* networks.py:809,817 / 823,830 */
                             void* ws, size_t ws_bytes, void* stream);
int nc_conv2d_k3_reflect_dgrad(const float* dy, const float* w, float* dx, int N, int C, int H, int W, int K,  /* backward of networks.py:809,817 / 823,830 */
                               void* ws, size_t ws_bytes, void* stream);
int nc_conv2d_k3_reflect_wgrad(const float* x, const float* dy, float* dw, float* dbias /* or NULL */, int N, int C, int H, int W, int K,  /* backward of networks.py:817,830 */
                               void* ws, size_t ws_bytes, void* stream);
/* nn.ReflectionPad2d(p), p in {1, 3}, H and W > p (networks.py:747,772 p 3; :809,823 p 1): x[NC,H,W] -> y[NC,H+2p,W+2p], a pure copy; the backward
 * gathers the up-to-nine padded positions of a pixel in a fixed order (csrc/resnet2d.hip), no atomics. */
int nc_reflect_pad2d_fwd(const float* x, float* y, int NC, int H, int W, int p, void* stream);   /* networks.py:747,772 */
int nc_reflect_pad2d_bwd(const float* dy, float* dx, int NC, int H, int W, int p, void* stream); /* backward of networks.py:747,772 */
/* The tail of a ResnetBlock with instance norm, `x + conv_block(x)` (networks.py:830,836): y = skip + (x - mean) * rstd in one pass; mean / rstd from
 * nc_instnorm_stats.  Backward: the skip gradient is dy itself, the other branch nc_instnorm_act_bwd with slope 1. */
int nc_instnorm_res_fwd(const float* x, const float* mean, const float* rstd, const float* skip, float* y, int NC, long S, void* stream);
/* y = a + b: the same skip connection behind a BatchNorm (networks.py:836 with --norm batch). */
int nc_residual_add(const float* a, const float* b, float* y, long n, void* stream);
/* nn.Dropout(0.5) of a ResnetBlock in training mode (networks.py:818-819): y = mask ? scale * x : 0 with one mask byte (0 / 1) per element; the
 * backward is the same call on dy. */
int nc_dropout_mul(const float* x, const void* mask, float scale, float* y, long n, void* stream);

/* ---- The same convolution on the 16-bit matrix cores (BASELINE.json configs[3]: "fp16 MFMA path with fp32
 *      InstanceNorm accumulate").  Tensors and master weights stay fp32 at this boundary; inside, operands are rounded
 *      (round-to-nearest-even) to `dtype` (NC_DT_BF16: v_mfma_f32_32x32x16_bf16, NC_DT_F16: ..._f16), products are
 *      accumulated in fp32 and the result is written in fp32.  Covers odd cubic kernels 3^3 / 5^3, stride 1, "same"
 *      padding with C % 16 == 0 and K % 64 == 0 (fwd), K % 16 == 0 and C % 64 == 0 (dgrad) -- every 3^3 layer of
 *      unet_deconv except the first, G_B's feature block; nc_conv_lp_supported tells (what: 0 fwd, 1 dgrad, 2 wgrad);
 *      unsupported shapes return NC_ERR_SHAPE (callers use nc_conv_* for those -- there is no silent fallback).       */
#define NC_DT_F32 0
#define NC_DT_F16 1
#define NC_DT_BF16 2
int nc_conv_lp_supported(int what, int N, int C, int D, int H, int W, int K, int kd, int kh, int kw, int stride, int pad);
size_t nc_conv_lp_ws_bytes(int N, int C, int D, int H, int W, int K, int kd, int kh, int kw, int stride, int pad);
/* Operand layout of the 16-bit kernels, "C8": [N][C/8][S voxels][8 channels] 16-bit (S = D*H*W), C % 8 == 0.  Each
 * operand of the *_lp calls is given EITHER as the fp32 NCDHW tensor (x / dy; converted into the workspace on every
 * call) OR already converted (xh / dyh non-NULL, then the fp32 pointer may be NULL) -- a caller that needs the same
 * tensor twice (x: forward and weight gradient; dy: data and weight gradient) converts it once with nc_to_c8.        */
size_t nc_c8_bytes(int N, int C, long S);
int nc_to_c8(const float* x, void* xh, int N, int C, long S, int dtype, void* stream);
int nc_conv_fwd_lp(const float* x, const void* xh, const float* w, const float* bias, float* y, int N, int C, int D, int H,
                   int W, int K, int kd, int kh, int kw, int stride, int pad, int dtype, void* ws, size_t ws_bytes,
                   void* stream);
int nc_conv_dgrad_lp(const float* dy, const void* dyh, const float* w, float* dx, int N, int C, int D, int H, int W, int K,
                     int kd, int kh, int kw, int stride, int pad, int dtype, void* ws, size_t ws_bytes, void* stream);
/* weight gradient: 3^3 / 5^3, C % 32 == 0, K % 64 == 0; dbias (nullable) is summed in fp32 from the fp32 dy */
int nc_conv_wgrad_lp(const float* x, const void* xh, const float* dy, const void* dyh, float* dw,
                     float* dbias /* or NULL */, int N, int C, int D, int H, int W, int K, int kd, int kh, int kw,
                     int stride, int pad, int dtype, void* ws, size_t ws_bytes, void* stream);

/* ---- ConvTranspose3d(k=2, s=2) (networks.py:500,503): x[N,C,D,H,W], w[C,K,2,2,2], bias[K], y[N,K,2D,2H,2W].   */
size_t nc_convT_ws_bytes(int N, int C, int D, int H, int W, int K);
int nc_convT_k2s2_fwd(const float* x, const float* w, const float* bias, float* y, int N, int C, int D, int H, int W,
                      int K, void* stream);
int nc_convT_k2s2_dgrad(const float* dy, const float* w, float* dx, int N, int C, int D, int H, int W, int K,
                        void* ws, size_t ws_bytes, void* stream);
int nc_convT_k2s2_wgrad(const float* x, const float* dy, float* dw, float* dbias, int N, int C, int D, int H, int W,
                        int K, void* ws, size_t ws_bytes, void* stream);

/* ---- ConvTranspose2d(k=2, s=2): the same layer of a generator built with dimension=2 (networks.py:382-390, 500, 503):
 *      x[N,C,H,W], w[C,K,2,2], bias[K] or NULL, y[N,K,2H,2W]; y[n,k,2u+a,2v+b] = bias[k] + sum_c x[n,c,u,v] w[c,k,a,b].  fp32; the forward runs
 *      on the fp32 matrix cores for K % 32 == 0, C % 16 == 0, C >= 128 (the U-Nets' 512->256, 256->128, 128->64), on the VALU otherwise and under
 *      nc_set_force_direct(1).  dgrad / wgrad take the gather GEMM where it applies and `ws` covers nc_convT2d_ws_bytes, VALU kernels otherwise;
 *      dbias (nullable) needs the workspace.  Results are run-to-run bit-identical.                                              */
size_t nc_convT2d_ws_bytes(int N, int C, int H, int W, int K);
int nc_convT2d_k2s2_fwd(const float* x, const float* w, const float* bias, float* y, int N, int C, int H, int W, int K,  /* networks.py:500,503 */
                        void* stream);
int nc_convT2d_k2s2_dgrad(const float* dy, const float* w, float* dx, int N, int C, int H, int W, int K,  /* backward of networks.py:500,503 */
                          void* ws, size_t ws_bytes, void* stream);
int nc_convT2d_k2s2_wgrad(const float* x, const float* dy, float* dw, float* dbias, int N, int C, int H, int W,  /* backward of networks.py:500,503 */
                          int K, void* ws, size_t ws_bytes, void* stream);

/* ---- InstanceNorm{2,3}d(affine=False, track_running_stats=False) + ReLU / LeakyReLU(slope)
 *      (networks.py:33-34 with :422-423 (slope 0) and :1042-1046 (slope 0.2)).  One instance = one (n, c) plane of S
 *      elements; biased variance, eps inside the sqrt.  `stats` computes mean / rstd (fp64 accumulation), `fwd`
 *      applies y = act((x-mean)*rstd), `bwd` is the backward of the pair given the pre-norm x.                   */
size_t nc_instnorm_ws_bytes(int NC, long S);
int nc_instnorm_stats(const float* x, int NC, long S, float eps, float* mean, float* rstd, void* ws, size_t ws_bytes,
                      void* stream);
/* stats + fwd in one call (mean / rstd are outputs).  Instances of S <= 2048 elements -- the 2-D PatchGAN layers --
 * run as ONE kernel with a group of 16 or 64 lanes per instance; the three entry points agree bit for bit. */
int nc_instnorm_fwd(const float* x, float eps, float slope, float* mean, float* rstd, float* y, int NC, long S, void* ws,
                    size_t ws_bytes, void* stream);
int nc_instnorm_act_fwd(const float* x, const float* mean, const float* rstd, float slope, float* y, int NC, long S,
                        void* stream);
int nc_instnorm_act_bwd(const float* dy, const float* x, const float* mean, const float* rstd, float slope, float* dx,
                        int NC, long S, void* ws, size_t ws_bytes, void* stream);
/* --norm batch: nn.BatchNorm{2,3}d(affine=True, track_running_stats=True) (+ the ReLU / LeakyReLU behind it) of get_norm_layer
 * (models/networks.py:30-31) -- statistics over (N, spatial) per channel; training: running statistics updated in place (momentum, unbiased
 * variance), evaluation (training = 0): the running statistics are used.  mean / rstd: [C]; ws: nc_instnorm_ws_bytes(N * C, S); N * C <= 65535. */
int nc_batchnorm_stats(const float* x, int N, int C, long S, float eps, float momentum, int training, float* mean, float* rstd,
                       float* running_mean, float* running_var, void* ws, size_t ws_bytes, void* stream);
int nc_batchnorm_act_fwd(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float slope, float* y,
                         int N, int C, long S, void* stream);
int nc_batchnorm_act_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         float slope, int training, float* dx, float* dgamma, float* dbeta, float* coef /* 2 C floats of scratch */, int N, int C,
                         long S, void* ws, size_t ws_bytes, void* stream);
/* Same backward, and dbias[C] = the per-channel sum of dx over samples and voxels: dx is the gradient at the output of
 * the convolution in front of the norm (networks.py:420-423), so this IS that convolution's bias gradient -- taken
 * while dx is in registers instead of by a second pass over dx (nc_conv_wgrad with dbias = NULL then). */
size_t nc_instnorm_bwd_dbias_ws_bytes(int NC, long S);
int nc_instnorm_act_bwd_dbias(const float* dy, const float* x, const float* mean, const float* rstd, float slope, float* dx,
                              float* dbias, int N, int C, long S, void* ws, size_t ws_bytes, void* stream);
/* The same backward with dx delivered ONLY as an S3 tensor [N][C/8][3][S][8] bf16 (the three-term operand form of the split-operand
 * convolutions, nc_to_s3): dx is the dY of the convolution in front of the norm, and when that convolution's gradients run on the
 * split-operand kernels nothing else reads it (nc_unet_deconv_bwd writes it straight into the convolution's workspace).  Values are bit
 * for bit those nc_instnorm_act_bwd_dbias stores; C % 8 == 0, S > 2048 (longer than the short-instance path), N * C <= 65535. */
int nc_instnorm_act_bwd_dbias_s3(const float* dy, const float* x, const float* mean, const float* rstd, float slope, void* dxs, float* dbias,
                                 int N, int C, long S, void* ws, size_t ws_bytes, void* stream);
/* The normalise + activate pass and its backward for the 16-bit convolution path: next to the fp32 result they emit it
 * in the C8 operand layout (nc_to_c8) of the convolution that consumes it -- yh for the next layer's forward, dxh (the
 * gradient at the previous convolution's output) for its data / weight gradient -- which saves those conversion passes.
 * C % 8 == 0; dbias nullable (see nc_instnorm_act_bwd_dbias); workspace: nc_instnorm_bwd_dbias_ws_bytes. */
int nc_instnorm_act_fwd_c8(const float* x, const float* mean, const float* rstd, float slope, float* y /* or NULL */, void* yh,
                           int N, int C, long S, int dtype, void* stream);
int nc_instnorm_act_bwd_c8(const float* dy, const float* x, const float* mean, const float* rstd, float slope, float* dx,
                           void* dxh, float* dbias /* or NULL */, int N, int C, long S, int dtype, void* ws, size_t ws_bytes,
                           void* stream);
/* LeakyReLU alone (PatchGAN first block, networks.py:1030) */
int nc_leaky_relu_fwd(const float* x, float slope, float* y, long n, void* stream);
int nc_leaky_relu_bwd(const float* dy, const float* x, float slope, float* dx, long n, void* stream);

/* ---- MaxPool3d(2) (networks.py:491,494): floor mode; first maximum wins on ties (scan order d,h,w).             */
int nc_maxpool2_fwd(const float* x, float* y, int NC, int D, int H, int W, void* stream);
int nc_maxpool2_bwd(const float* dy, const float* x, float* dx, int NC, int D, int H, int W, void* stream);
/* dx = skip + pool-backward(dy): the pooled tensor of Unet_deconv also feeds the skip concat (networks.py:526,531), so its
 * gradient is the sum of both paths (autograd adds them in a separate pass); even D (or D == 1), H, W only.        */
int nc_maxpool2_bwd_add(const float* dy, const float* x, const float* skip, float* dx, int NC, int D, int H, int W,
                        void* stream);

/* ---- Sigmoid (networks.py:510,536) */
int nc_sigmoid_fwd(const float* x, float* y, long n, void* stream);
int nc_sigmoid_bwd(const float* dy, const float* y, float* dx, long n, void* stream);

/* ---- Volume.get_slice / get_projection (apollo_model.py:328-351): vol[N,C,D,H,W], axis in {0,1,2} = (D,H,W).
 *      slice: out = vol[..., index, ...]; mip: out = max over [start, start+depth) along axis (+ int32 argmax).
 *      The *_bwd kernels write the FULL dvol (zeros elsewhere).                                                   */
int nc_slice_fwd(const float* vol, float* out, int NC, int D, int H, int W, int axis, int index, void* stream);
int nc_slice_bwd(const float* dout, float* dvol, int NC, int D, int H, int W, int axis, int index, void* stream);
int nc_mip_fwd(const float* vol, float* out, int32_t* arg, int NC, int D, int H, int W, int axis, int start, int depth,
               void* stream);
int nc_mip_bwd(const float* dout, const int32_t* arg, float* dvol, int NC, int D, int H, int W, int axis,
               void* stream);

/* ---- Athena's iter_f (axial_to_lateral_gan_athena_model.py:286-296): every slice along `axis` as one batch.
 *      to_volume = 0: slices[(n*L+s), c, a, b] = vol[n, c, ...s...]; to_volume = 1: the inverse permutation (backward). */
int nc_volume_slices(const float* src, float* dst, int N, int C, int D, int H, int W, int axis, int to_volume,
                     void* stream);

/* ---- GANLoss('lsgan') = MSELoss against a constant (networks.py:276,299-313) and L1Loss (apollo:128,279).
 *      out[0] = mean; backward scales by the device scalar gscale[0] (autograd's incoming gradient).              */
size_t nc_loss_ws_bytes(long n);
int nc_mse_const_fwd(const float* pred, long n, float target, float* out, void* ws, size_t ws_bytes, void* stream);
int nc_mse_const_bwd(const float* pred, long n, float target, const float* gscale, float* dpred, void* stream);
/* GANLoss('vanilla') = nn.BCEWithLogitsLoss against the constant label (networks.py:278, 308-313): mean(max(p,0) - p t + log(1 + exp(-|p|)));
 * GANLoss('wgangp') = -+mean(p) (networks.py:314-318): nc_mean_fwd gives mean(p), the caller applies the sign (gscale carries it backward). */
int nc_bce_logits_const_fwd(const float* pred, long n, float target, float* out, void* ws, size_t ws_bytes, void* stream);
int nc_bce_logits_const_bwd(const float* pred, long n, float target, const float* gscale, float* dpred, void* stream);
int nc_mean_fwd(const float* pred, long n, float* out, void* ws, size_t ws_bytes, void* stream);
int nc_mean_bwd(long n, const float* gscale, float* dpred, void* stream);
int nc_l1_fwd(const float* a, const float* b, long n, float* out, void* ws, size_t ws_bytes, void* stream);
int nc_l1_bwd(const float* a, const float* b, long n, const float* gscale, float* da, void* stream);

/* ---- torch.optim.Adam step over one flat parameter buffer (apollo:131-136, step at :295,:307).                  */
int nc_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                 int step, void* stream);

/* ---- Dice / assemble (data/diceImage_dataset.py:95-120 + base_dataset.py:134-143; util/assemble_dice.py:130-213).
 *      vol: ORIGINAL (unpadded) uint16 / uint8 volume [L0,L1,L2] resident in HBM.  cut_cube writes cube `index` of
 *      edge E = roi + 2*border, float32 in [0,1]: zero dicing pad (util/util.py:196-215) then reflect border.
 *      scatter_add: acc[P0,P1,P2] += cube[border:-border]^3 / 8 at the cube's origin; finalize: (acc/cnt)*8*scale,
 *      truncating cast, crop to the original size; cnt is computed analytically from the grid.                    */
int nc_dice_cut_cube(const void* vol, int is_u16, int L0, int L1, int L2, int roi, int overlap, int border, int index,
                     float* cube, void* stream);
/* ---- Training augmentation "clean rotation" (data/base_dataset.py:306-460: rotate every z-slice with cv2.warpAffine,
 *      crop to the inscribed rectangle) fused with the random crop (:187-206) and __normalize (:134-143): produces only
 *      the crop.  inv_affine = 2x3 row-major map from rotated-image pixel (x, y) to source pixel; (x0, y0) = crop origin
 *      in the rotated image (inscribed-rectangle offset + random crop offset); z0 = first source slice.           */
int nc_rotate_crop(const void* vol, int is_u16, int D, int H, int W, int z0, int y0, int x0, int cz, int cy, int cx,
                   const double* inv_affine, float* out, void* stream);
int nc_assemble_scatter_add(const float* cube, float* acc, int P0, int P1, int P2, int roi, int overlap, int border,
                            int index, void* stream);
int nc_assemble_finalize(const float* acc, void* out, int out_is_u16, int P0, int P1, int P2, int L0, int L1, int L2,
                         int roi, int overlap, void* stream);
/* The same for planes [z0, z0 + nz) of the volume: acc_slab holds the PADDED planes from za (<= z0) on, out [nz][L1][L2] (sharded
 * inference: every rank finalises the z-slab it owns, neuroclear_amd/test_dice.py assemble='slab').  nc_assemble_scatter_add adds into
 * such a slab when it is given the slab's address minus za * P1 * P2 floats (it only touches the planes of its cube). */
int nc_assemble_finalize_slab(const float* acc_slab, void* out, int out_is_u16, int P0, int P1, int P2, int L0, int L1, int L2, int roi,
                              int overlap, int z0, int nz, int za, void* stream);

/* ---- 2-D dice / assemble for the 2-D generators (--image_dimension 2): the arithmetic above on the two in-plane axes of a stack
 *      [L0,L1,L2] of planes; axis 0 is not diced, padded or reflected.  P1, P2 and the grid n1 x n2 are util/util.py:196-215 and
 *      data/diceImage_dataset.py:91-93 of (L1, L2); tile t lies in plane t / (n1 n2) at yi = (t % (n1 n2)) / n2, xi = t % n2
 *      (data/diceImage_dataset.py:100-106, x fastest).  Each call handles the `count` tiles from `first` on in ONE launch; a batch may
 *      straddle planes.
 *      cut_tiles (data/diceImage_dataset.py:95-96, :108-120 + base_dataset.py:134-143): tiles [count][E][E], E = roi + 2*border, float32
 *      in [0,1], zero dicing pad then reflect border.                                                                              */
int nc_dice2d_cut_tiles(const void* img, int is_u16, int L0, int L1, int L2, int roi, int overlap, int border, long first, int count,
                        float* tiles, void* stream);
/*      scatter_add (util/assemble_dice.py:143-145, :167-173): acc[L0][P1][P2] += tile[border:-border]^2 / 8 at each tile's origin.  One
 *      thread per accumulator pixel adds the tiles of the batch that cover it in ascending tile index (no atomics): the bits do not
 *      depend on how the tile sequence is cut into batches and equal those of adding the tiles one by one.                          */
int nc_assemble2d_scatter_add(const float* tiles, float* acc, int L0, int P1, int P2, int roi, int overlap, int border, long first,
                              int count, void* stream);
/*      finalize (util/assemble_dice.py:176-183, :202-213): out[L0][L1][L2] = (acc / cnt) * 8 * scale, truncating cast, crop of the
 *      dicing pad; cnt = cover(y) * cover(x) from the grid.                                                                         */
int nc_assemble2d_finalize(const float* acc, void* out, int out_is_u16, int L0, int P1, int P2, int L1, int L2, int roi, int overlap,
                           void* stream);

/* ---- --normalize_intensity (util/assemble_dice.py:188-192): merged = (acc / count) * 8 on the padded volume;
 *      nc_radix_hist = one pass of an exact radix select (order-preserving 32-bit key of a float: pass 0 bins key >> 20,
 *      pass 1 bins (key >> 8) & 0xfff among key >> 20 == prefix, pass 2 bins key & 0xff among key >> 8 == prefix;
 *      hist4096 is zeroed by the call) from which the host takes the order statistics np.percentile interpolates;
 *      rescale_finalize = skimage.exposure.rescale_intensity(in_range=(lo, hi)) on a float32 image (clip to [lo, hi],
 *      (v - lo) / range with range = float32(hi64 - lo64), output range (0, 1) or (-1, 1) if lo < 0) + cast + crop.     */
int nc_assemble_merge(const float* acc, float* merged, int L0, int L1, int L2, int roi, int overlap, void* stream);
int nc_radix_hist(const float* x, long n, int pass, unsigned prefix, unsigned* hist4096, void* stream);
int nc_assemble_rescale_finalize(const float* merged, void* out, int out_is_u16, int L0, int L1, int L2, int roi,
                                 int overlap, float lo, float hi, float range, void* stream);

/* ---- --histogram_match (util/assemble_dice.py:149-151): skimage.exposure.match_histograms(fake_cube, real_cube) on
 *      the border-cropped cubes, restated from scikit-image 0.18.3 (_match_cumulative_cdf: np.unique + np.cumsum +
 *      np.interp, float64).  source / tmpl / out: n floats each (out = the float64 result rounded to float32).      */
size_t nc_match_histograms_ws_bytes(long n);
int nc_match_histograms(const float* source, const float* tmpl, float* out, long n, void* ws, size_t ws_bytes,
                        void* stream);

/* ---- torch.nn.utils.spectral_norm on a convolution weight (NLayerDiscriminatorSN, networks.py:1069-1111; --netD
 *      basic_SN / n_layers_SN).  w_orig viewed as [K][M]; power_iteration = 1 (training): v <- normalize(W^T u),
 *      u <- normalize(W v) in place (eps 1e-12), then sigma = u . W v and w_out = W / sigma; 0 (eval): u, v as stored.
 *      scratch_k: K floats.  bwd: dw_orig = (g - <g, w_sn> u v^T) / sigma (u, v are constants of the forward).          */
int nc_spectral_norm_fwd(const float* w_orig, float* u, float* v, float* w_out, float* sigma, float* scratch_k, int K, int M,
                         int power_iteration, float eps, void* stream);
int nc_spectral_norm_bwd(const float* g, const float* w_sn, const float* u, const float* v, const float* sigma, float* dw_orig, int K,
                         int M, void* stream);

/* ---- Whole-network PatchGAN (NLayerDiscriminator with InstanceNorm, networks.py:1009-1067; called from
 *      apollo_model.py:195-283 through netD_*): forward and backward as ONE call each (the op-by-op path is
 *      host-enqueue-bound on these ~25-kernel chains).  params = the 2 * (n_layers + 2) tensors in state-dict order,
 *      packed; saved = activations / raw conv outputs / InstanceNorm statistics for the backward
 *      (nc_patchgan_saved_floats); nd = 2 (x is [B,1,H,W], pass D = 1) or 3.  bwd: dx and dparams may be NULL;
 *      dparams is overwritten (not accumulated).                                                                    */
size_t nc_patchgan_param_floats(int n_layers, int ndf, int nd);
size_t nc_patchgan_saved_floats(int B, int D, int H, int W, int n_layers, int ndf, int nd);
size_t nc_patchgan_ws_bytes(int B, int D, int H, int W, int n_layers, int ndf, int nd);
int nc_patchgan_out_shape(int B, int D, int H, int W, int n_layers, int ndf, int nd, int* oD, int* oH, int* oW);
int nc_patchgan_fwd(const float* params, const float* x, float* y, float* saved, int B, int D, int H, int W,
                    int n_layers, int ndf, int nd, void* ws, size_t ws_bytes, void* stream);
int nc_patchgan_bwd(const float* params, const float* x, const float* saved, const float* dy, float* dx, float* dparams,
                    int B, int D, int H, int W, int n_layers, int ndf, int nd, void* ws, size_t ws_bytes, void* stream);
/* Planes b0 .. b0 + B - 1 of a batch of Btot (x / y / dy / dx hold the B planes; saved and the workspace are the whole
 * batch's).  Athena sends the slices of `fake` through every discriminator twice with the same weights -- in the
 * generator loss (athena_model.py:240-260) and, detached, next to the slices of `real` in the discriminator loss
 * (:190-238, before optimizer_D.step()): the first pass is run as the second half of that batch (fwd_part + bwd_part, input
 * gradient only), the discriminator loss then only runs the `real` half and nc_patchgan_bwd over the whole batch. */
int nc_patchgan_fwd_part(const float* params, const float* x, float* y, float* saved, int Btot, int b0, int B, int D, int H,
                         int W, int n_layers, int ndf, int nd, void* ws, size_t ws_bytes, void* stream);
int nc_patchgan_bwd_part(const float* params, const float* x, const float* saved, const float* dy, float* dx, int Btot, int b0,
                         int B, int D, int H, int W, int n_layers, int ndf, int nd, void* ws, size_t ws_bytes, void* stream);
/* WGAN-GP gradient penalty of the same network (cal_gradient_penalty, networks.py:321-359), 2-D only (nd = 2, D = 1; anything
 * else is NC_ERR_SHAPE).  fwd: D's forward on x, its backward with dy = 1 -> g = d(sum D)/dx (shape of x), and
 * *pen = lambda_gp * mean_b (||g_b + 1e-16||_2 - constant)^2 (fp64 sums of squares); saved (nc_patchgan_gp_saved_floats) keeps
 * what bwd needs.  bwd: *dpen (a device scalar) times the penalty's gradient -- dparams (OVERWRITTEN, packed like params; the head's
 * bias and every bias in front of an InstanceNorm are exact zeros) and dx (the gradient with respect to x); either may be NULL.
 * Bit-identical from run to run (csrc/patchgan_gp.hip; no float atomics).  Both need the workspace (nc_patchgan_gp_ws_bytes). */
size_t nc_patchgan_gp_saved_floats(int B, int D, int H, int W, int n_layers, int ndf, int nd);
size_t nc_patchgan_gp_ws_bytes(int B, int D, int H, int W, int n_layers, int ndf, int nd);
int nc_patchgan_gp_fwd(const float* params, const float* x, float* g, float* pen, float* saved, int B, int D, int H, int W, int n_layers,
                       int ndf, int nd, float constant, float lambda_gp, void* ws, size_t ws_bytes, void* stream);
int nc_patchgan_gp_bwd(const float* params, const float* x, const float* saved, const float* g, const float* dpen, float* dparams, float* dx,
                       int B, int D, int H, int W, int n_layers, int ndf, int nd, float constant, float lambda_gp, void* ws, size_t ws_bytes,
                       void* stream);

/* ---- Whole-network forward of Unet_deconv (networks.py:512-538; called from TestModel.forward test_model.py:60-62):
 *      params = the 28 tensors in state-dict order, packed back to back (see neuroclear_amd.models.networks).       */
size_t nc_unet_deconv_fwd_ws_bytes(int N, int S0, int S1, int S2);
int nc_unet_deconv_fwd(const float* params, const float* x, float* y, int N, int S0, int S1, int S2, void* ws,
                       size_t ws_bytes, void* stream);


/* ---- Whole-network TRAINING entry points of the generators (one C call per direction, like nc_patchgan_*):
 *      Unet_deconv.forward (networks.py:512-538) with everything its backward needs kept in `saved`, and the autograd
 *      backward of it (driven by loss_G.backward(), apollo_model.py:283); DeepLinearGenerator.forward (networks.py:
 *      913-917) and its backward.  params / dparams: the tensors in state-dict order, packed (28 for unet_deconv, 6 for
 *      deep_linear_gen); dparams is OVERWRITTEN.  dx may be NULL (the data gradient of the first layer is then skipped).
 *      Same kernels in the same order as the layer-by-layer path: bit-identical results.  The skip concats cost no copy
 *      (producers write into halves of the concat buffers) and the two gradients of a skip tensor are merged inside the
 *      max-pool backward (nc_maxpool2_bwd_add).  nc_deep_linear_fwd with saved == NULL is the inference form.          */
size_t nc_unet_deconv_param_floats(void);
size_t nc_unet_deconv_saved_floats(int N, int S0, int S1, int S2);
size_t nc_unet_deconv_train_ws_bytes(int N, int S0, int S1, int S2);
/* The `kept` word nc_unet_deconv_train_fwd would return for this shape under the switches of now (the forward's plan, gen_nets.hip u_fwd_forms);
 * launches nothing.  0: an edge is not a positive multiple of 4. */
unsigned nc_unet_deconv_kept_expected(int N, int S0, int S1, int S2);
/* `kept` (HOST word, out, may be NULL): bit i set = the forward left the three-term (S3) copy of layer i's input in `saved`; hand the
 * same word to the backward that reads this `saved` buffer (0 is always valid: the backward then converts the inputs again).  The
 * word travels with the caller's record of the forward (the autograd context), there is no library-side table.
 * Bits 16 + i: that copy is a two-term (H2) tensor.  Bits 10 .. 14 (the lean forward, below): the fp32 activation a1 / a2 / b1 / b2 / e2a
 * (the input of block 1 / 3 / 5 / 6 / 8) was NOT written into `saved` -- the backward reads the kept H2 copy, or writes the tensor again from
 * raw / mean / rstd into its own workspace when it cannot use that copy (the terms switch moved between the two calls) or when the range
 * guard may switch to the three-term kernels inside the call (nc_set_h2_guard(2): those build their x operand from the fp32 tensor). */
int nc_unet_deconv_train_fwd(const float* params, const float* x, float* y, float* saved, int N, int S0, int S1, int S2,
                             void* ws, size_t ws_bytes, void* stream, unsigned* kept);
int nc_unet_deconv_bwd(const float* params, const float* x, const float* y, const float* saved, const float* dy, float* dx,
                       float* dparams, int N, int S0, int S1, int S2, void* ws, size_t ws_bytes, void* stream, unsigned kept);
/* The lean forms of the two-term training step (default on; NC_UNET_LEAN=0 at load time): the forward does not write fp32 activations whose only
 * regular reader is a two-term convolution that has its own H2 copy, and the backward (one sample) never expands the rank-one data gradient
 * behind one_by_one -- block 9's InstanceNorm backward forms w12[c] * s2[v] itself.  Outputs and gradients are bit for bit what the full forms
 * give.  With nc_set_split_terms(3) or the split kernels off: no effect.
 * Three more full-resolution fp32 tensors stay unwritten, each recorded in `kept` (the backward decides from the bits, not from the switch):
 *   bit 27       e1, block 9's output: one_by_one's forward and weight gradient take raw / mean / rstd and normalise the operand as they read it
 *                -- only where the two flat 1 x 1 kernels take the layer (>= 16384 voxels, nc_set_force_direct off); else e1 is written.
 *   bits 28, 29  the fp32 upper half of cat1 / cat2: the transposed convolution writes the H2 half of block 9 / 7's operand alone.
 *   bits 30, 31  TOGETHER WITH bit 26, the fp32 lower half of cat1 / cat2: blocks 1 / 3 write the H2 half, the fp32 POOLED tensor and the pool's
 *                winner bytes in one pass and the max-pool is not launched -- only when the forward writes winner bytes (nc_set_in_bwd_fold on
 *                at that call: bit 26, the one bit that switch moves; bits 30 / 31 say that the block is in the form otherwise).
 * A backward that reads one of them after all (block 9 / 7 without the kept H2 copy or with nc_set_h2_guard(2), a pool backward outside the norm
 * backward, one_by_one off the flat kernels) first writes it again with the bits the full forward stores: the concat halves into their own
 * slots of `saved` (which the backward therefore WRITES in these cases), e1 into its workspace.  The layout of `saved`,
 * nc_unet_deconv_saved_floats and the workspace sizes are unchanged. */
void nc_set_unet_lean(int on);
int nc_get_unet_lean(void);
/* Prepared weights of the two-term training step (default on; NC_UNET_WPREP=0 at load time; process-wide, sampled once per call):
 * nc_unet_deconv_train_fwd computes the weight cells and the two-term packed weights of blocks 1 .. 9 -- forward and data-gradient form, and
 * the output bounds of the two transposed convolutions that the concat blocks' forward packs need -- in ONE batched pass at its start, into a
 * region of `saved` (about 54 MB, independent of the crop; nc_unet_deconv_saved_floats counts it), instead of three small launches in front of
 * every convolution.  `kept` bit 15: the packs are in `saved`.  The backward takes a block's data-gradient pack from there when the bit is set,
 * the block's form is still the forward's (bits 16 + i, as for the kept operand) and the switch is still on; otherwise it launches what it
 * launched before.  CONTRACT: with bit 15 set the data gradients of nc_unet_deconv_bwd use the weights AS THEY WERE AT FORWARD TIME (autograd's
 * semantics); `params` must not change between a forward and its backward (neuroclear_amd.ops refuses such a backward).  Same bits as the
 * per-layer preparation: outputs and gradients do not change.  Not prepared (per-layer launches as before): three-term blocks
 * (nc_set_split_terms(3), a call the range guard flags in mode 2 packs its three-term weights itself), the split kernels off, NC_S3_TRAIN_FUSE=0,
 * and with NC_CONVT_H2=0 the forward packs of blocks 7 and 9 (a measured cell). */
void nc_set_unet_wprep(int on);
int nc_get_unet_wprep(void);
/* The folded InstanceNorm backward of the two-term training step (default on; NC_IN_BWD_FOLD=0 at load time; process-wide, sampled once per
 * call; nc_set_in_bwd_fold returns the previous setting).  Per two-term block of nc_unet_deconv_bwd: the sums pass keeps the loads of four
 * iterations in flight (same element sequence and order of additions per thread), the apply pass takes the tensor's bound itself, the range
 * guard's words are zeroed with the cells, and the bias sums and the guard's decision are one launch -- four launches instead of six.  Blocks 1
 * and 3 (their output feeds a max-pool and a skip connection): nc_unet_deconv_train_fwd's pool kernel also writes one byte per pooled element,
 * the winner's index, into `saved` (nc_unet_deconv_saved_floats counts it; `kept` bit 26), and the norm backward forms skip + pool gradient per
 * element instead of reading the tensor nc_maxpool2_bwd_add would write.  Every stored value and every order of summation is unchanged: outputs
 * and gradients are bit for bit the same.  Launches of before: the switch off at either call, a range guard that may switch kernels inside the
 * call (nc_set_h2_guard(2); mode 1 in the per-layer entry points), three terms, the split kernels off, NC_S3_TRAIN_FUSE=0.
 * nc_in_bwd_launches(which, reset): kernel launches so far of the two-term norm backward (which = 0) or of nc_maxpool2_bwd_add (1), for tests. */
int nc_set_in_bwd_fold(int on);
int nc_get_in_bwd_fold(void);
int nc_in_bwd_launches(int which, int reset);
/* The streaming passes of the training step nearer to the memory system's rate (default on; process-wide, sampled once per call;
 * nc_set_stream_passes returns the previous setting).  On: the folded rank-one form of the two-term norm backward (the last block) issues the
 * nine loads of an apply iteration before it uses the first and keeps eight iterations in flight in its sums pass; the fp32 norm backward on
 * long instances keeps eight iterations in flight in its sums pass (nc_instnorm_act_bwd, _dbias, _c8, _dbias_s3), and its apply pass
 * (nc_instnorm_act_bwd, _dbias) four, the first of them issued before the partial sums are added up; the batched weight preparation takes its
 * cells row by row without a division per element and writes whole 16-byte fragments, both terms from one read of the eight weights.  Off: the
 * kernels as they were.  Every stored value and every order of summation is the same either way: outputs and gradients are bit for bit equal. */
int nc_set_stream_passes(int on);
int nc_get_stream_passes(void);
/* Test exports.  nc_unet_wprep_layout: where block `block`'s (1 .. 9) prepared pack of `form` (0 forward, 1 data gradient) lies in `saved`
 * (byte offsets; cell_off: its weight cell; bound_off: the transposed convolution's bound of blocks 7 / 9, else 0).  nc_s3x_pack_h2_debug: the
 * PER-LAYER preparation of w[K][C][27] (cell_a / cell_b: device words, the two scale groups of a forward input) into wp / wcell.
 * nc_convT_h2_bound_debug: the per-layer bound into a zeroed cell. */
int nc_unet_wprep_layout(int N, int S0, int S1, int S2, int block, int form, size_t* pack_off, size_t* pack_bytes, size_t* cell_off,
                         size_t* bound_off);
int nc_s3x_pack_h2_debug(const float* w, int C, int K, int form, const unsigned* cell_a, const unsigned* cell_b, void* wp, unsigned* wcell,
                         void* stream);
int nc_convT_h2_bound_debug(const float* w, const float* bias, int C, int K, float in_bound, unsigned* cell, void* stream);
size_t nc_deep_linear_param_floats(void);
size_t nc_deep_linear_saved_floats(int N, int S0, int S1, int S2);
size_t nc_deep_linear_ws_bytes(int N, int S0, int S1, int S2);
/* The `kept` word a TRAINING nc_deep_linear_fwd (saved != NULL) would return for this shape under the switches of now (the forward's plan,
 * gen_nets.hip l_fwd_form); launches nothing.  0: N or an extent below 1 -- and the layered form with the split kernels off, which keeps nothing. */
unsigned nc_deep_linear_kept_expected(int N, int S0, int S1, int S2);
int nc_deep_linear_fwd(const float* params, const float* x, float* y, float* saved /* or NULL */, int N, int S0, int S1,
                       int S2, void* ws, size_t ws_bytes, void* stream, unsigned* kept /* as above */);
/* deep_linear_gen's layers 1 .. 5 (5^3, 3^3, then three 1 x 1; reference networks.py:900-911) are bias-free with nothing in between.  Level of
 * nc_set_dl_collapse (NC_DL_COLLAPSE at load time):
 *   0  layer by layer, as the reference's autograd does;
 *   1  (round 5) layers 2 .. 5 in collapsed form -- ONE 64 -> 1 convolution forward, and backward the six parameter gradients and dL/dact1 from
 *      dy, act1 and the weights alone (csrc/dl_tail.hip, "the collapsed tail") -- and the 5^3 layer's two gradients from 27 shifted copies of the
 *      one-channel dy, its forward as a 64 -> 27 convolution plus a shifted sum ("the forward without act1");
 *   2  (default, round 6) layers 1 .. 5 as ONE position-typed 7^3 convolution 64 -> 1 of act0 (csrc/dl_typed.hip): the zero padding of
 *      act1 only matters ON the faces, where it removes the taps of the 3^3 kernel that point outside -- 27 composed kernels, one per position
 *      type; the interior one runs everywhere on the two-term matrix kernels, the voxels on a face are recomputed / corrected with their own.  The
 *      5^3 convolution is not executed at all.  Where the shape does not admit it (an extent below 8, H above 192, W % 4 != 0, W below 16
 *      or above 176 -- the one-channel 7^3 weight gradient kernel's range --, nc_set_split_terms(3)): as 1.
 * Exact algebra in every level (weight-space products in fp64; tests/test_collapse_algebra.py in fp64 against autograd), the same outputs and
 * gradients to fp32 rounding, each level closer to an fp64 evaluation than the one before.  nc_deep_linear_lp_* follows the switch as 0 / non-zero.
 * Both pairs carry the forward's choice in `kept`, so the switch may move between a forward and its backward.
 * nc_deep_linear_fwd's `kept`: bits 0 .. 5 and 16 .. 21 as above (the kept copy of layer i's input and its form); the three top bits say which of
 * the forms ran (csrc/gen_nets.hip: kKeptCollapsed, kKeptNoAct1, kKeptTyped; tests read them to assert the form):
 *   bit 31  a collapsed form: act2 .. act4 were not written, the backward takes layers 2 .. 5 from dy, act1 and the weights (level 1 or 2);
 *   bit 30  ... and act1 was not written either ("the forward without act1", or the typed form);
 *   bit 29  ... because layers 1 .. 5 ran as the ONE position-typed 7^3 kernel of level 2: `saved` holds act0 alone.  Set only by a training
 *           forward (saved != NULL) under level 2 in the two-term arithmetic at a shape every kernel of the form admits; the inference form
 *           (saved == NULL) never takes it: under levels 1 and 2 it runs layers 2 .. 5 as the one 64 -> 1 convolution (bit 31 alone).
 * All three clear: the layered evaluation.  Bit 30 implies bit 31, bit 29 implies both. */
void nc_set_dl_collapse(int on);
int nc_get_dl_collapse(void);
int nc_deep_linear_bwd(const float* params, const float* x, const float* saved, const float* dy, float* dx, float* dparams,
                       int N, int S0, int S1, int S2, void* ws, size_t ws_bytes, void* stream, unsigned kept);

/* ---- The 16-bit END-TO-END path (BASELINE.json configs[3]): operators between which activations and gradients exist in
 *      HBM only as 16-bit "C8" tensors [N][C/8][S][8] (nc_to_c8's layout).  A tensor argument (ptr, ctot, c0) means
 *      channels [c0, c0 + C) of a ctot-channel C8 buffer -- halves of the skip concat buffers (networks.py:526,531) are
 *      read / written in place.  Gradient tensors are bf16.  Statistics: fp32 per-thread partials of x - the instance's first voxel, fp64 reduction.
 *      The nc_c8_* entries and nc_from_c8 refuse N * C / 8 > 65535 (the heads: N > 65535) with NC_ERR_SHAPE before their first launch.
 *      nc_conv_fwd_c8 / nc_conv_dgrad_c8: nc_conv_fwd_lp / nc_conv_dgrad_lp with a C8 result (rounded to dtype);
 *      nc_c8_instnorm_*: InstanceNorm3d(affine=False) + ReLU / LeakyReLU (networks.py:33-34,422-423) and its backward
 *      (g = gradient at the activation output, xh = raw convolution output; dbias nullable = sum of dx per channel);
 *      nc_c8_maxpool2_*: MaxPool3d(2) (networks.py:491,494), backward fused with the add of the skip gradient;
 *      nc_convT_k2s2_*_c8: ConvTranspose3d(k 2, s 2) (networks.py:500,503) on the 16-bit matrix cores (C, K % 32 == 0);
 *      nc_from_c8: C8 -> fp32 NCDHW.                                                                                   */
int nc_conv_fwd_c8(const void* xh, const float* w, const float* bias, void* yh, int out_ctot, int out_c0, int N, int C, int D, int H,
                   int W, int K, int kd, int kh, int kw, int stride, int pad, int dtype, void* ws, size_t ws_bytes, void* stream);
int nc_conv_dgrad_c8(const void* dyh, const float* w, void* dxh, int N, int C, int D, int H, int W, int K, int kd, int kh, int kw,
                     int stride, int pad, int dtype, void* ws, size_t ws_bytes, void* stream);
/* One-channel layers (Conv3d(1, 64, ks, padding ks/2), ks = 3: networks.py:420 first U-Net layer; ks = 7: :899 first
 * deep_linear layer) on the 16-bit cores in "pseudo-channel" form: the ks taps along x become 8 input channels
 * X8[v][j] = x[v + j - ks/2], the layer a ks x ks x 1 convolution of that C8 tensor.  fwd: x fp32 [N,1,D,H,W] -> C8 result
 * in channels [out_c0, out_c0 + 64); dgrad: dyh C8 [N][8][S][8] (bf16) -> dx fp32 [N,1,D,H,W].                        */
size_t nc_conv_c1_c8_ws_bytes(int N, int D, int H, int W, int ks);
int nc_conv_c1_fwd_c8(const float* x, const float* w, const float* bias, void* yh, int out_ctot, int out_c0, int N, int D, int H, int W,
                      int ks, int dtype, void* ws, size_t ws_bytes, void* stream);
int nc_conv_c1_dgrad_c8(const void* dyh, const float* w, float* dx, int N, int D, int H, int W, int ks, void* ws, size_t ws_bytes,
                        void* stream);
/* Weight gradient of the same layers from the C8 (bf16) gradient: dw fp32 [64,1,ks,ks,ks] = sum dyh * shifted x.  The K-dim of
 * the 16-bit MFMA is 16 consecutive voxels of an x row (planar 16-bit copies of dy and of the 8 x-shifted copies of x are built
 * in the workspace); W <= 192. */
size_t nc_conv_c1_wgrad_c8_ws_bytes(int N, int D, int H, int W, int ks);
int nc_conv_c1_wgrad_c8(const float* x, const void* dyh, float* dw, int N, int D, int H, int W, int ks, void* ws, size_t ws_bytes,
                        void* stream);
size_t nc_c8_instnorm_ws_bytes(int N, int C, long S);
int nc_c8_instnorm_stats(const void* xh, int N, int C, long S, float eps, float* mean, float* rstd, int dtype, void* ws,
                         size_t ws_bytes, void* stream);
int nc_c8_instnorm_act_fwd(const void* xh, const float* mean, const float* rstd, float slope, void* yh, int out_ctot, int out_c0,
                           int N, int C, long S, int dtype, void* stream);
int nc_c8_instnorm_act_bwd(const void* gh, int g_ctot, int g_c0, const void* xh, const float* mean, const float* rstd, float slope,
                           void* dxh, float* dbias /* or NULL */, int N, int C, long S, int dtype, void* ws, size_t ws_bytes,
                           void* stream);
int nc_c8_maxpool2_fwd(const void* xh, int x_ctot, int x_c0, void* yh, int N, int C, int D, int H, int W, int dtype, void* stream);
int nc_c8_maxpool2_bwd_add(const void* dph, const void* xh, int x_ctot, int x_c0, const void* skiph, int s_ctot, int s_c0, void* dxh,
                           int N, int C, int D, int H, int W, int dtype, void* stream);
int nc_from_c8(const void* xh, int x_ctot, int x_c0, float* y, int N, int C, long S, int dtype, void* stream);
size_t nc_convT_c8_ws_bytes(int N, int C, int D, int H, int W, int K);
int nc_convT_k2s2_fwd_c8(const void* xh, const float* w, const float* bias, void* yh, int out_ctot, int out_c0, int N, int C, int D,
                         int H, int W, int K, int dtype, void* ws, size_t ws_bytes, void* stream);
int nc_convT_k2s2_dgrad_c8(const void* dyh, int dy_ctot, int dy_c0, const float* w, void* dxh, int N, int C, int D, int H, int W, int K,
                           void* ws, size_t ws_bytes, void* stream);
int nc_convT_k2s2_wgrad_c8(const void* xh, const void* dyh, int dy_ctot, int dy_c0, float* dw, float* dbias /* or NULL */, int N,
                           int C, int D, int H, int W, int K, void* ws, size_t ws_bytes, void* stream);
/* Test exports of the 64 -> 1 pointwise heads of both generators on this path (csrc/c8_ops.hip; tests/test_gpu_c8_ops.py): each validates
 * its arguments and forwards.  nc_c8_dot64_debug: out fp32 [N][S] = bias (nullable) + sum_c w[c] xh[n][c][v], xh a dense 64-channel C8
 * tensor.  nc_c8_outer64_debug: the backward, dxh (nullable; bf16 C8) = w (x) g, dw[64] = sum g x, db (nullable) = sum g; N <= 65535. */
int nc_c8_dot64_debug(const void* xh, const float* w, const float* bias, float* out, int N, long S, int dtype, void* stream);
size_t nc_c8_outer64_ws_bytes_debug(int N, long S);
int nc_c8_outer64_debug(const float* g, const void* xh, const float* w, void* dxh, float* dw, float* db, int N, long S, int dtype, void* ws,
                        size_t ws_bytes, void* stream);

/* ---- Whole-network training passes of the generators on that path (dtype = NC_DT_BF16): same contract as
 *      nc_unet_deconv_train_fwd / _bwd and nc_deep_linear_fwd / _bwd, `saved` in bytes.  The one-channel first layers
 *      (3^3 of the U-Net, 7^3 of deep_linear_gen), statistics, weight gradients and the pointwise heads' sums stay fp32;
 *      deep_linear_gen's bias-free linear tail 64 -> 32 -> 16 -> 1 (networks.py:903-911) is evaluated as the single
 *      64-vector W6 W5 W4 and its weight gradients as the rank-1 products they are.  *_supported: every layer's shape is
 *      covered by the 16-bit kernels (otherwise callers use the layer-by-layer 16-bit path).                         */
int nc_unet_deconv_lp_supported(int N, int S0, int S1, int S2, int dtype);
size_t nc_unet_deconv_lp_saved_bytes(int N, int S0, int S1, int S2);
size_t nc_unet_deconv_lp_ws_bytes(int N, int S0, int S1, int S2);
int nc_unet_deconv_lp_fwd(const float* params, const float* x, float* y, void* saved, int N, int S0, int S1, int S2, int dtype,
                          void* ws, size_t ws_bytes, void* stream);
int nc_unet_deconv_lp_bwd(const float* params, const float* x, const float* y, const void* saved, const float* dy, float* dx,
                          float* dparams, int N, int S0, int S1, int S2, int dtype, void* ws, size_t ws_bytes, void* stream);
int nc_deep_linear_lp_supported(int N, int S0, int S1, int S2, int dtype);
size_t nc_deep_linear_lp_saved_bytes(int N, int S0, int S1, int S2);
size_t nc_deep_linear_lp_ws_bytes(int N, int S0, int S1, int S2);
/* `kept` (round 6, as nc_deep_linear_fwd / _bwd): the form the forward took (layered / collapsed tail / without f2 -- it depends on
 * nc_set_dl_collapse at forward time and decides what `saved` holds); the caller hands it to the backward, which follows it whatever the
 * switches say by then (a value the forward cannot return: NC_ERR_ARG). */
int nc_deep_linear_lp_fwd(const float* params, const float* x, float* y, void* saved, int N, int S0, int S1, int S2, int dtype,
                          void* ws, size_t ws_bytes, void* stream, unsigned* kept);
int nc_deep_linear_lp_bwd(const float* params, const float* x, const void* saved, const float* dy, float* dx, float* dparams,
                          int N, int S0, int S1, int S2, int dtype, void* ws, size_t ws_bytes, void* stream, unsigned kept);

/* ---- fp32 3^3 / 5^3 convolutions on the 16-bit matrix cores (csrc/conv_split.hip): an fp32 value is exactly the sum of three
 *      bf16 terms; the six products a_i b_j with i + j <= 2 are bf16 MFMAs on one fp32 accumulator (what is dropped is below
 *      2^-23 of a product).  Same operands and results as nc_conv_fwd / nc_conv_dgrad (networks.py:420-425, 460-469) to
 *      fp32 rounding.  "S3" tensor: [N][C/8][3 terms][D][H][W][8] bf16 (nc_to_s3); xs / dys: the operand already in that
 *      form, or NULL (then converted into the workspace).  what: 0 forward, 1 data gradient, 2 weight gradient.                             */
void nc_set_conv_split(int on); /* 1 (default; or the value of NC_CONV_SPLIT at load time): nc_conv_fwd / nc_conv_dgrad and the
                                  * whole-network calls built on them take this path for the shapes it covers; 0: the fp32
                                  * MFMA kernels (v_mfma_f32_32x32x2_f32) serve those shapes */
int nc_get_conv_split(void);
/* The TWO-TERM form (round 4; csrc/conv_s3x.hip NT = 2, csrc/h2.hip, s3_common.hpp; the default): each operand as two fp16 terms of the tensor
 * times a power of two (chosen per tensor from its largest finite magnitude, or from a bound known by construction; results scaled back
 * exactly) and THREE fp16 MFMA products per fp32 product -- half the matrix work of the three-term bf16 form at the same error against fp64
 * (tests/test_gpu_h2.py).  The price is fp16's exponent range WITHIN one tensor: elements below 2^-17 of the tensor's largest magnitude keep
 * fewer than 22 bits, below 2^-39 they vanish (fp32: 2^-126) -- immaterial for normalised activations and their gradients, wrong for a tensor
 * that mixes magnitudes 1e12 apart; nc_set_split_terms(3) is for those.  terms = 2 (default; NC_SPLIT_TERMS at load time): two-term wherever
 * it exists -- nc_conv_fwd / _dgrad / _wgrad / _bwd of the covered shapes (channels % 64) and the whole-network training and inference calls
 * built on them; 3: three-term everywhere; 0: two-term in the inference forward nc_unet_deconv_fwd only.  The explicit S3 entry points below
 * (nc_to_s3, nc_conv_*_split) are three-term by definition.  In the whole-network calls InstanceNorm outputs are converted with the power of
 * two their bound sqrt(voxels) allows, the norm's backward with a bound from its own first pass, everything else with a measured one; the
 * ratio between the halves of a concatenation is folded into the consuming layer's weights.  Do not change the setting between a training
 * forward and its backward (the backward then re-converts what the forward kept). */
void nc_set_split_terms(int terms);
int nc_get_split_terms(void);
/* The PatchGAN's 4 x 4 layers at Athena's batches (csrc/conv_p2d.hip; reference networks.py:1030-1057): 1 (default; NC_P2D_TERMS at load time): the
 * stride-1 256 -> 512 layer's forward and data gradient on the two-term form whenever nc_get_split_terms() == 2 (a measured power of two per
 * call: results depend in the last bit on which planes share a call); 3: three-term everywhere (bit-identical however the planes are batched);
 * 2: two-term for the stride-2 layers too (slower: their conversion dominates). */
void nc_set_p2d_terms(int mode);
int nc_get_p2d_terms(void);
/* The RANGE GUARD of the two-term form (round 5; csrc/h2.hip, csrc/common.hpp): wherever a call converts an fp32 operand ITSELF with a measured
 * power of two -- nc_conv_fwd / _dgrad / _wgrad / _bwd and every dY of the whole-network backward calls that arrives as fp32 -- the conversion
 * pass also counts the CHUNKS (64 voxels x 8 channels) whose largest magnitude lies below 2^-17 of the tensor's; when more than 1/64 of the
 * non-zero chunks do (a region of the volume or a block of channels far below the rest: the one case the two-term form degrades, see above),
 * THAT CALL runs on the exact three-term kernels instead.  The decision is taken on the device (no host synchronisation): both kernel
 * families are launched and the one whose turn it is not leaves at its first instruction.  Modes (nc_set_h2_guard; NC_H2_GUARD at load
 * time): 0 off (round-4 behaviour); 1 (default): the in-call fallback in the per-layer entry points (nc_conv_fwd / _dgrad / _wgrad / _bwd);
 * INSIDE the whole-network calls (nc_unet_deconv_*, nc_deep_linear_*) every data-derived power of two is checked the same way -- fp32 dY
 * tensors, the dY tensors the InstanceNorm backward writes in two-term form itself (power of two from the tensor's own per-instance maxima),
 * the activations deep_linear_gen keeps -- but a flagged tensor is only COUNTED (the fallback would cost the training step ~65 near-empty
 * launches, 0.5 ms of 35, for an event InstanceNorm networks do not produce); 2: in-call fallback everywhere it exists (everything but the
 * kept activations of deep_linear_gen).  Operands whose power of two is a bound by construction (InstanceNorm
 * outputs, ConvTranspose outputs) and WEIGHTS (one measured power of two per weight tensor: assumed well-conditioned, as any initialisation
 * and training of this path leaves them) are not guarded.  nc_h2_guard_stats(out, reset): out[0] = tensors measured, out[1] = calls that fell
 * back to three terms, out[2] = flagged tensors that could not switch (the Python models go to nc_set_split_terms(3) when they see one,
 * models/base_model.py), out[3] = the largest share of low chunks seen, in parts per million; host-visible counters, readable at any time
 * without synchronising (they trail the device by whatever is still queued). */
void nc_set_h2_guard(int on);
int nc_get_h2_guard(void);
int nc_h2_guard_stats(unsigned long long* out4, int reset);
/* Epilogue statistics of the inference forward (round 5; csrc/conv_s3x.hip, template parameter ST): in nc_unet_deconv_fwd's two-term mode every
 * 3^3 convolution leaves, per (tile, wave), the sum and the sum of squares of its bias-free outputs, and a small pass adds them up in fp64 in a
 * fixed order -- InstanceNorm (reference networks.py:513-515, nn.InstanceNorm3d after every Conv3d) needs no pass of its own over the raw
 * output.  mean / rstd agree with the separate pass to 4e-8 relative.  1 (default; NC_EPI_STATS at load time); 0: the separate pass; 2: also in
 * nc_unet_deconv_train_fwd's blocks whose input arrives converted (tested; no measurable gain in the training step, hence not the default). */
void nc_set_epi_stats(int on);
int nc_get_epi_stats(void);
/* Which kernel serves the whole 512-position tiles of a two-term 3^3 launch (forward and data gradient of every 3^3 layer of the U-Net,
 * reference networks.py:496-561, whose input channels are a multiple of 64; csrc/conv_s3x.hip): 1 (default; NC_S3X_W64 at load time) = k_conv_s3w,
 * the 64-channel x 64-position wave tile with the weights staged through LDS (round 6; -4 % on the 140^3 / 108^3 layers, profiles/r06_ab_w64.txt);
 * 0 = k_conv_s3x everywhere.  Same tiles, same records of the epilogue statistics; results differ by the order of the fp32 sums only (one running
 * accumulator per tile instead of restarts every four k-steps). */
void nc_set_s3x_w64(int on);
int nc_get_s3x_w64(void);
int nc_unet_deconv_fwd_terms(int S0, int S1, int S2); /* 2: nc_unet_deconv_fwd runs its 3^3 layers on the two-term form at this size under the
                                                       * current switches; 3: on the three-term form (or the fp32 kernels); 0: bad size */
void nc_set_c8x_mode(int mode); /* which kernel serves the 16-bit 3^3 / 5^3 forward / data-gradient calls (nc_conv_fwd_lp, nc_conv_*_c8, the
                                  * *_lp whole-network calls; csrc/conv_c8x.hip): 1 (default; NC_C8X at load time) = for 3^3 layers the tap-stream kernel
                                  * k_conv_c8x where its 512-position tiles fill the launch's rounds of 512 workgroups to >= 60 %, k_conv_h elsewhere (a few planes); 2 = k_conv_c8x
                                  * wherever the shape fits (channels read and written % 64 == 0); 0 = k_conv_h everywhere.  Both kernels multiply
                                  * the same 16-bit operands and accumulate in fp32; only the summation order differs */
int nc_get_c8x_mode(void);
int nc_conv_lp_uses_c8x(int what /* 0 forward, 1 data gradient */, int fp32_out, int N, int C, int D, int H, int W, int K, int ks); /* 1: under
                                  * the current mode this call runs on k_conv_c8x (layer C -> K channels; fp32_out: nc_conv_*_lp, else the C8 forms) */
void nc_set_s3_fusion(int on); /* 1 (default; NC_S3_FUSE): nc_unet_deconv_fwd has InstanceNorm + ReLU write the three-term form of a
                                * layer that only feeds a split-operand convolution; 0: separate conversion passes (bit-identical) */
int nc_conv_split_supported(int what, int N, int C, int D, int H, int W, int K, int kd, int kh, int kw, int stride, int pad);
size_t nc_conv_split_ws_bytes(int N, int C, int D, int H, int W, int K, int ks);
size_t nc_s3_bytes(int N, int C, long S);
int nc_to_s3(const float* x, void* xs, int N, int C, long S, void* stream);
int nc_conv_fwd_split(const float* x, const void* xs, const float* w, const float* bias, float* y, int N, int C, int D, int H, int W,
                      int K, int ks /* 3 or 5: cubic kernel, stride 1, padding ks/2 */, void* ws, size_t ws_bytes, void* stream);
int nc_conv_dgrad_split(const float* dy, const void* dys, const float* w, float* dx, int N, int C, int D, int H, int W, int K, int ks,
                        void* ws, size_t ws_bytes, void* stream);
int nc_conv_wgrad_split(const float* x, const void* xs, const float* dy, const void* dys, float* dw, int N, int C, int D, int H, int W,
                        int K, int ks, void* ws, size_t ws_bytes, void* stream); /* nc_conv_wgrad (weights only) */
/* Test exports of the two kernels that add up FIXED-ORDER partial sums (tests/test_gpu_partial_sums.py); each runs exactly the launch the
 * library's own paths make.
 * nc_wgrad_s3_reduce_debug: k_wgrad_s3_reduce (csrc/conv_split.hip) behind the 3^3 / 5^3 weight-gradient kernels.  T3 = 27 or 125, TW = 27 / 25
 *   taps per workgroup, ndg = T3 / TW dz groups, npairs = (K / 64) * (C / 32) * ndg (<= 256), pair = ((k / 64) * (C / 32) + c / 32) * ndg + dz;
 *   part: fp32 [nwp][npairs][NF][TW][64 k][32 c], 16-byte aligned -- workgroup w of a pair, accumulator flush f -- i.e.
 *   npairs * nwp * NF * TW * 64 * 32 floats.  dw[k][c][dz * TW + tap] = the nslots = nwp * NF slots sl = w * NF + f of (pair, tap, k % 64, c % 32)
 *   added as eight segments of per = ceil(nslots / 8) consecutive slots, each from 0.f in slot order (an empty segment is 0.f), the segments
 *   as ((((((s0 + s1) + s2) + s3) + s4) + s5) + s6) + s7; with xcells / ycell (device words, both or neither; then C % 64 == 0) the sum r becomes
 *   r * f.x * f.y, f the two powers of two that undo the cells xcells[c >= C / 2] and *ycell of the two-term operands.  guard (nullable, 8 device
 *   words): the launch leaves dw alone unless word [2] says it is this form's turn (set: the form without cells; zero: the one with).
 * nc_gemm_split_reduce_debug: k_gemm_split_reduce (csrc/conv_gemm.hip) behind every split gather GEMM: slab fp32 [splits][n],
 *   out[i] = ((bias[(i / inner) % K] + slab[0][i]) + slab[1][i]) + ... (bias nullable: 0.f; inner, K are read only with a bias). */
int nc_wgrad_s3_reduce_debug(const float* part, float* dw, int K, int C, int T3, int nwp, int NF, const unsigned* xcells, const unsigned* ycell,
                             const unsigned* guard, void* stream);
int nc_gemm_split_reduce_debug(const float* slab, float* out, long n, int splits, const float* bias, long inner, int K, void* stream);

/* ConvTranspose3d(kernel 2, stride 2) forward -- nn.ConvTranspose3d at networks.py:471-478 -- on the same arithmetic (csrc/convt_s3.hip):
 * C % 32 == 0 (<= 256), K % 16 == 0.  xs: the input in S3 form, or NULL (x is converted into the workspace); y (nullable): fp32 output
 * [N][K][2D][2H][2W]; ys (nullable): channels [ys_c0, ys_c0 + K) of a ys_ctot-channel S3 tensor of the output volume.  At least one of y / ys. */
/* Conv2d 4 x 4, padding 1, stride 1 or 2 of the PatchGAN (networks.py:1037-1055: the 64 -> 128, 128 -> 256 and 256 -> 512 layers) at batches of
 * >= 8192 output pixels on the same arithmetic (csrc/conv_p2d.hip; forward and data gradient; channels % 64 == 0 on the written side, % 16 /
 * % 64 on the read side) and the stride-1 layer's weight gradient (csrc/wgrad_p2d.hip; C % 32 == 0, K % 64 == 0): 1 when nc_conv_fwd (what 0) /
 * nc_conv_dgrad (what 1) / nc_conv_wgrad (what 2) -- and with them nc_patchgan_fwd / _bwd -- take it for this call under the current switches
 * (nc_set_conv_split; NC_P2D at load time: bit 0 the stride-1 layer forward / data gradient, bit 1 the stride-2 layers, bit 2 the stride-1 weight
 * gradient, 0 = never).  Smaller batches, the one-channel first layer and head, and the stride-2 weight gradients run on the kernels of
 * conv2d_img.hip / patchgan_edge.hip / the gather GEMM. */
int nc_conv2d_split_active(int what, int N, int C, int H, int W, int K, int k, int stride, int pad);

int nc_convT_k2s2_split_supported(int N, int C, int D, int H, int W, int K);
int nc_convT_k2s2_split_active(int N, int C, int D, int H, int W, int K); /* supported AND nc_get_conv_split(): what the whole-network calls do */
size_t nc_convT_k2s2_split_ws_bytes(int N, int C, int D, int H, int W, int K);
int nc_convT_k2s2_fwd_split(const float* x, const void* xs, const float* w, const float* bias, float* y, void* ys, int ys_ctot, int ys_c0,
                            int N, int C, int D, int H, int W, int K, void* ws, size_t ws_bytes, void* stream);

/* Test exports of the WRITERS of the two-term form (csrc/h2_debug.hip; tests/test_gpu_h2_writers.py): each validates its arguments and forwards,
 * unchanged, to the internal function the whole-network calls use.  "H2" tensor: [N][ctot/8][2 terms][S][8] fp16 = the two terms of the element
 * times 2^k, k from a CELL (the float bits of a magnitude that bounds the tensor); the cells -- [0] for the first half of the channels, [1] for
 * the second -- sit nc_h2_cells_offset(N * ctot * S) bytes behind the start, nc_h2_bytes = that offset + 256.  cell / cell2 / out_cell / guard
 * are device words; a part is channels [c0, c0 + C) of a ctot-channel tensor, everything % 8.
 * nc_to_h2_debug: bound > 0: h2_set_cell(cell, bound), else the cell is measured (h2_zero_cells, h2_absmax per sample); guard (nullable, 8
 *   words, zeroed here) receives the range guard's chunk counts; then split2h_into.
 * nc_act_split2h_debug: act_split2h (InstanceNorm normalisation + (Leaky)ReLU; y, cell, cell2 nullable).
 * nc_act_split2h_pool_debug: act_split2h_pool (the same and MaxPool3d(2) of the result into `pooled`, a DENSE C-channel tensor; cell nullable).
 * nc_maxpool2_h2_debug: maxpool2_h2 (channels [0, C) of a ctot-channel tensor -> a dense C-channel tensor).
 * nc_h2_to_s3_if_debug: h2_to_s3_if (the S3 form of an H2 tensor; runs when guard is NULL or its flag word [2] is set).
 * nc_instnorm_act_bwd_dbias_h2_debug: instnorm_act_bwd_dbias_h2, or with w1 != NULL instnorm_act_bwd_dbias_h2_rank1 (N == 1, dy one channel,
 *   the gradient is w1[c] * dy[v]); dxs has the capacity of the S3 tensor (nc_s3_bytes), its cells at nc_h2_cells_offset(N * C * S); workspace
 *   nc_instnorm_bwd_dbias_ws_bytes; guard nullable.
 * nc_convT_k2s2_fwd_split_h2_debug: convT_h2_bound(w, bias, in_bound = sqrt(D H W)) into the zeroed *out_cell, then convT_fwd_split_h2 (x fp32,
 *   |x| <= sqrt(D H W), converted into the workspace; y nullable; ys = channels [ys_c0, ys_c0 + K) of a ys_ctot-channel H2 tensor of the output
 *   volume, converted with *out_cell). */
size_t nc_h2_bytes(int N, int C, long S);
size_t nc_h2_cells_offset(size_t elems);
int nc_to_h2_debug(const float* x, long xstride, void* xs, int N, int C, long S, int ctot, int c0, unsigned* cell, float bound, unsigned* guard,
                   void* stream);
int nc_act_split2h_debug(const float* x, const float* mean, const float* rstd, float slope, float* y, long ystride, void* ys, int N, int C, long S,
                         int ctot, int c0, float bound, unsigned* cell, unsigned* cell2, void* stream);
int nc_act_split2h_pool_debug(const float* x, const float* mean, const float* rstd, float slope, void* ys, void* pooled, int N, int C, int D, int H,
                              int W, int ctot, int c0, float bound, unsigned* cell, void* stream);
int nc_maxpool2_h2_debug(const void* in, void* out, int N, int C, int ctot, int D, int H, int W, void* stream);
int nc_h2_to_s3_if_debug(const void* xh, void* xs, int N, int C, long S, const unsigned* cells, const unsigned* guard, void* stream);
int nc_instnorm_act_bwd_dbias_h2_debug(const float* dy, const float* w1, const float* x, const float* mean, const float* rstd, float slope, void* dxs,
                                       float* dbias, int N, int C, long S, void* ws, size_t ws_bytes, unsigned* guard, void* stream);
/* nc_instnorm_act_bwd_dbias_h2_pool_debug: the same inside a whole-network scope (guard mode 1 only counts); gp / arg != NULL: the POOL form --
 * dy is the skip gradient (sample stride dy_stride floats), gp the dense pooled gradient and arg the winner bytes [N][C][D/2 H/2 W/2] (even
 * sizes).  nc_maxpool2_fwd_arg_debug: MaxPool3d(2) that also writes the winner bytes. */
int nc_instnorm_act_bwd_dbias_h2_pool_debug(const float* dy, long dy_stride, const float* gp, const unsigned char* arg, const float* x, const float* mean,
                                            const float* rstd, float slope, void* dxs, float* dbias, int N, int C, int D, int H, int W, void* ws,
                                            size_t ws_bytes, unsigned* guard, void* stream);
int nc_maxpool2_fwd_arg_debug(const float* x, float* y, unsigned char* arg, int NC, int D, int H, int W, void* stream);
/* Test exports of the lean training forms (tests/test_gpu_unet_lean2.py).  nc_act_split2h_pool_arg_debug: act_split2h_pool_arg -- act_split2h's
 * H2 part and, of the same activations, MaxPool3d(2) as fp32 into `pooled` with the winner bytes into `arg` (both dense [N][C][D/2 H/2 W/2]); no
 * fp32 activation.  nc_conv_fwd_norm_1x1_debug / nc_conv_wgrad_norm_1x1_debug: nc_conv_fwd / nc_conv_wgrad (dbias nullable) of a 1 x 1 layer
 * whose input is InstanceNorm + (Leaky)ReLU of `raw` (mean, rstd: [N][C]), normalised inside the kernel; NC_ERR_SHAPE where the two flat 1 x 1
 * kernels do not take the layer (C % 16, fewer than 16384 voxels, nc_set_force_direct). */
int nc_act_split2h_pool_arg_debug(const float* x, const float* mean, const float* rstd, float slope, void* ys, float* pooled, unsigned char* arg, int N,
                                  int C, int D, int H, int W, int ctot, int c0, float bound, unsigned* cell, void* stream);
int nc_conv_fwd_norm_1x1_debug(const float* raw, const float* mean, const float* rstd, float slope, const float* w, const float* bias, float* y, int N,
                               int C, int D, int H, int W, int K, void* ws, size_t ws_bytes, void* stream);
int nc_conv_wgrad_norm_1x1_debug(const float* raw, const float* mean, const float* rstd, float slope, const float* dy, float* dw, float* dbias, int N,
                                 int C, int D, int H, int W, int K, void* ws, size_t ws_bytes, void* stream);
size_t nc_convT_k2s2_split_h2_ws_bytes(int N, int C, int D, int H, int W, int K);
int nc_convT_k2s2_fwd_split_h2_debug(const float* x, const float* w, const float* bias, float* y, void* ys, int ys_ctot, int ys_c0, int N, int C,
                                     int D, int H, int W, int K, unsigned* out_cell, void* ws, size_t ws_bytes, void* stream);
/* Test export of the THREE-term (S3) output of the fp32 matrix-core kernel (csrc/convt.hip convT_fwd_s3; tests/test_gpu_convt.py): y nullable;
 * ys = channels [ys_c0, ys_c0 + K) of a ys_ctot-channel S3 tensor of the output volume (nc_s3_bytes), everything % 8.  A shape the kernel does
 * not cover (C != 128, K % 32 != 0, nc_set_force_direct(1)) is refused with NC_ERR_SHAPE. */
int nc_convT_k2s2_fwd_s3_debug(const float* x, const float* w, const float* bias, float* y, void* ys, int ys_ctot, int ys_c0, int N, int C, int D,
                               int H, int W, int K, void* stream);
/* Test export of the one-pass inference tail of Unet_deconv (csrc/norm_act.hip k_in_act_tail; tests/test_gpu_norm.py), which otherwise runs only
 * inside nc_unet_deconv_fwd: y[v] = sigmoid(w2 * (b1 + sum_c w1[c] * relu((x[c][v] - mean[c]) * rstd[c])) + b2) for one sample of C <= 256
 * channels and S voxels (more channels: NC_ERR_SHAPE); w2, b1, b2 point at one float each. */
int nc_instnorm_relu_tail_sigmoid_debug(const float* x, const float* mean, const float* rstd, const float* w1, const float* b1, const float* w2,
                                        const float* b2, float* y, int C, long S, void* stream);
/* Test exports of the boundary pieces of deep_linear_gen's position-typed path (csrc/dl_typed.hip and csrc/dl_bnd.hip, whose kernels do the
 * same arithmetic in the same order; tests/test_gpu_dl_bnd.py compares the two bit by bit).  piece: 0 = the forward's boundary voxels (io = y
 * [N][1][D][H][W]: boundary voxels overwritten, the others untouched; dy may be NULL), 1 = dL/dact0's boundary terms (io = g [N][64][D][H][W],
 * added to), 2 = the boundary types' sums (io = Pq [64][32][125], overwritten; the interior's correlation dWsw taken as zero).  variant: 0 =
 * dl_typed.hip's kernels, 1 = dl_bnd.hip's (NC_ERR_SHAPE where it has none for the piece and the shape), -1 = what the whole-network calls take:
 * nc_dl_bnd_variant_debug's answer.  F: the 27 composed 5^3 kernels [27][64][125]; act0: [N][64][D][H][W]; dy: [N][1][D][H][W]; scratch:
 * nc_dl_typed_scratch_bytes_debug bytes (0: the typed form does not take the shape), the layout of dl_typed.hip's dl_typed_plan.  The call runs
 * the composition of the typed kernels, the transposed copies and the one piece on `stream`; a bad piece or variant, a null pointer
 * (NC_ERR_ARG), an uncovered shape (NC_ERR_SHAPE) or a short scratch (NC_ERR_WS) is refused before anything is written. */
size_t nc_dl_typed_scratch_bytes_debug(int N, int D, int H, int W);
int nc_dl_bnd_variant_debug(int piece, int N, int D, int H, int W);
int nc_dl_bnd_piece_debug(int piece, const float* F, const float* act0, const float* dy, float* io, void* scratch, size_t scratch_bytes, int N, int D,
                          int H, int W, int variant, void* stream);

/* ---- Learned-PSF generators (--netG_B linearkernel / linearkernel_double / linearkernel_LK31): LinearKernel and LinearKernel_double at
 *      models/networks.py:840-871, one bias-free Conv3d(1, 1, k, stride 1, padding (k - 1) / 2) -- applied twice with one weight in the
 *      _double form -- and its autograd backward (loss.backward(), apollo:283).  x, y, dy, dx: [N][1][D][H][W]; w, dw: [1][1][k][k][k].
 *      Odd k from 3 to 31, any N, D, H, W >= 1 (extents below k included); anything else is NC_ERR_SHAPE.  Exact fp32 products with fp32
 *      accumulation on v_mfma_f32_16x16x4_f32 (csrc/conv_lk.hip); bit-identical from run to run.  Only nc_lk_wgrad uses the workspace
 *      (fixed-order partial sums, nc_lk_ws_bytes); nc_lk_fwd / nc_lk_dgrad accept ws = NULL. */
size_t nc_lk_ws_bytes(int N, int D, int H, int W, int k);
int nc_lk_fwd(const float* x, const float* w, float* y, int N, int D, int H, int W, int k, void* ws, size_t ws_bytes, void* stream);
int nc_lk_dgrad(const float* dy, const float* w, float* dx, int N, int D, int H, int W, int k, void* ws, size_t ws_bytes, void* stream);
int nc_lk_wgrad(const float* x, const float* dy, float* dw, int N, int D, int H, int W, int k, void* ws, size_t ws_bytes, void* stream);

/* ---- KernelGAN patch discriminator (--netD kernelGAN): KernelPatchDiscriminator at models/networks.py:1113-1145, built by define_D at
 *      :243-244 with n_layers = 5, here with InstanceNorm, input_nc = 1 and ndf = 64 (any other ndf is NC_ERR_SHAPE): a valid 7^nd conv
 *      (1 -> 64), three [1x1 conv 64 -> 64, InstanceNorm, ReLU], a 1x1 conv 64 -> 1, every conv with a bias.  Forward and backward as
 *      one call each, like nc_patchgan_*: params = the 10 tensors in state-dict order, packed (nc_kgan_param_floats); saved is opaque
 *      (nc_kgan_saved_floats); nd = 2 (x is [B,1,H,W], pass D = 1) or 3; y is [B,1,(D-6),H-6,W-6].  bwd: dx and dparams may be NULL;
 *      dparams is overwritten (not accumulated).  A spatial edge below 7, or an output plane of one element (InstanceNorm in training
 *      mode refuses it), is NC_ERR_SHAPE.  The first two convs run collapsed into one; exact fp32 products with fp32
 *      accumulation (csrc/kgan.hip); bit-identical from run to run.  Both directions need the workspace (nc_kgan_ws_bytes). */
size_t nc_kgan_param_floats(int ndf, int nd);
size_t nc_kgan_saved_floats(int B, int D, int H, int W, int ndf, int nd);
size_t nc_kgan_ws_bytes(int B, int D, int H, int W, int ndf, int nd);
int nc_kgan_out_shape(int B, int D, int H, int W, int ndf, int nd, int* oD, int* oH, int* oW);
int nc_kgan_fwd(const float* params, const float* x, float* y, float* saved, int B, int D, int H, int W, int ndf, int nd, void* ws,
                size_t ws_bytes, void* stream);
int nc_kgan_bwd(const float* params, const float* x, const float* saved, const float* dy, float* dx, float* dparams, int B, int D, int H,
                int W, int ndf, int nd, void* ws, size_t ws_bytes, void* stream);

/* ---- Training progress views (--display_freq; csrc/views.hip).  nc_tensor2im is util.tensor2im (util/util.py:26-39) on n dense fp32
 *      values: v = min(max(x, 0), 1) * 255.0f (out_is_u16 = 1: 65535.0f) in fp32, as numpy computes it on a float32 array, clipped to the
 *      range again, truncating cast to uint8 / uint16 (out: n elements of that type).  NaN input is outside the contract.
 *      nc_progress_views is what Visualizer.display_current_results shows of one visual (util/visualizer.py:138-144, 171-173): from sample 0,
 *      channel 0 of vol[N][C][D][H][W], after tensor2im(., uint8), six arrays packed back to back into `views` (nc_progress_views_bytes):
 *      the slices [index,:,:] (H x W), [:,index,:] (D x W), [:,:,index] (D x H), then the maxima over axis 0 (H x W), axis 1 (D x W), axis 2
 *      (D x H); hist256[v] = the number of voxels of that sample with uint8 value v (zeroed by the call first; the sum is D*H*W).  views and
 *      hist256 may each be NULL.  One call per visual, on the given stream, no host synchronisation; integer maxima and integer adds only, so
 *      the bytes are the same from run to run and on every stream.  Refused before anything is written: a NULL vol (NC_ERR_ARG); an extent
 *      below 1, index outside [0, min(D, H, W)), D*H*W >= 2^31 (NC_ERR_SHAPE).  nc_progress_views_bytes is 0 for an extent below 1. */
int nc_tensor2im(const float* x, void* out, int out_is_u16, long n, void* stream);
size_t nc_progress_views_bytes(int D, int H, int W);
int nc_progress_views(const float* vol, int N, int C, int D, int H, int W, int index, uint8_t* views, uint32_t* hist256, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NC_HIP_H */
