// Batched weight preparation of the U-Net training step (gen_nets.hip, nc_unet_deconv_train_fwd): the weight cells and the two-term packed
// weights of EVERY 3^3 block, forward and data-gradient form, in four launches at the start of the call instead of three launches in front of
// each convolution (conv_s3x.hip conv_s3x_h2: zero the cell, k_absmax_w, k_pack_w_s3x<2>).  Nothing here depends on the data: the weights are
// those of the call, the forward packs fold in the ratio of the input's two cells, and those are bounds the host knows (InstanceNorm: sqrt of
// the voxels) or that follow from weights alone (the transposed convolutions' output bound, computed here as well).  The bits come from the
// per-layer kernels' own device functions (w_prep.hpp): same cells, same packs.
//   1. one k_set_cells launch zeroes the contiguous cell block
//   2. k_wprep_bounds: the output bounds of the transposed convolutions (inputs of the concat blocks' forward packs)
//   3. k_wprep_absmax: every segment's weight cell (blockIdx.y = segment), integer atomicMax
//   4. k_wprep_pack: every segment's packed weights; the segment of a concat block also leaves the bound in the H2 tensor's second cell
// With nc_set_stream_passes (default) launches 3 and 4 are k_wprep_absmax_rows (rows of an output channel, no division per element) and
// k_wprep_pack_frag (one thread per 16-byte unit of a fragment, both terms from one read of the eight weights): the same cells, the same packs.
#include "common.hpp"
#include "w_prep.hpp"

namespace nc {
namespace {

struct WPrepDevSeg {
  const float* w;
  unsigned short* wp;
  unsigned* ext_cell;   // nullable
  long total, so, si;   // packed elements; strides of w as k_pack_w_s3x takes them
  long nw;              // weights
  int Cin, NS, flip, split_c;
  int b_cell;           // < 0: cell_b = cell_a
  unsigned a_bits;
};
struct WPrepDevTable {
  WPrepDevSeg seg[kWPrepMaxSegs];
  unsigned blk0[kWPrepMaxSegs + 1];  // first block of each segment in the pack's grid: blocks of 256 elements (k_wprep_pack) or of 256 16-byte units (k_wprep_pack_frag)
  int nseg;
};
struct WPrepDevBounds {
  WPrepBound b[kWPrepMaxBounds];
  int n;
};

__global__ void __launch_bounds__(256) k_wprep_bounds(const WPrepDevBounds t, unsigned* __restrict__ cells) {
  __shared__ float part[4][64];
  __shared__ float red[64];
  const WPrepBound& b = t.b[blockIdx.y];
  if ((int)blockIdx.x * 64 >= b.K * 8) return;  // (the grid is sized for the widest layer)
  convT_bound_block(b.w, b.bias, b.C, b.K, b.in_bound, cells + b.cell, (int)blockIdx.x, part, red);
}

__global__ void __launch_bounds__(256) k_wprep_absmax(const WPrepDevTable t, unsigned* __restrict__ cells) {
  __shared__ unsigned wm[4];
  const WPrepDevSeg& g = t.seg[blockIdx.y];
  if (!g.w) return;
  const unsigned ca = g.a_bits, cb = g.b_cell >= 0 ? cells[g.b_cell] : ca;
  absmax_w_block(g.w, g.nw, 27, g.Cin, g.split_c, ca, cb, cells + blockIdx.y, blockIdx.x, gridDim.x, wm);
}
// nc_set_stream_passes: the same cells, walked by rows (w_prep.hpp)
__global__ void __launch_bounds__(256) k_wprep_absmax_rows(const WPrepDevTable t, unsigned* __restrict__ cells) {
  __shared__ unsigned wm[4];
  const WPrepDevSeg& g = t.seg[blockIdx.y];
  if (!g.w) return;
  const unsigned ca = g.a_bits, cb = g.b_cell >= 0 ? cells[g.b_cell] : ca;
  absmax_w_rows_block(g.w, g.nw, 27, g.Cin, g.split_c, ca, cb, cells + blockIdx.y, (int)blockIdx.x, (int)gridDim.x, wm);
}

__global__ void __launch_bounds__(256) k_wprep_pack(const WPrepDevTable t, const unsigned* __restrict__ cells) {
  int k = 0;
  while (k + 1 < t.nseg && blockIdx.x >= t.blk0[k + 1]) ++k;
  const WPrepDevSeg& g = t.seg[k];
  const unsigned ca = g.a_bits, cb = g.b_cell >= 0 ? cells[g.b_cell] : ca;
  const long i = (long)(blockIdx.x - t.blk0[k]) * 256 + threadIdx.x;
  if (i == 0 && g.ext_cell) *g.ext_cell = cb;
  if (i >= g.total) return;
  g.wp[i] = pack_w_s3x_elem<2>(g.w, i, g.Cin / 8, 3, g.NS, g.so, g.si, g.flip, cells[k], g.split_c, ca, cb);
}
// nc_set_stream_passes: the same packs, one thread per 16-byte unit of a fragment -- the eight weights are read and split once and written for
// both terms (k_wprep_pack: sixteen threads, sixteen scattered reads and splits, sixteen 2-byte stores).  blk0 counts blocks of 256 UNITS here.
__global__ void __launch_bounds__(256) k_wprep_pack_frag(const WPrepDevTable t, const unsigned* __restrict__ cells) {
  int k = 0;
  while (k + 1 < t.nseg && blockIdx.x >= t.blk0[k + 1]) ++k;
  const WPrepDevSeg& g = t.seg[k];
  const unsigned ca = g.a_bits, cb = g.b_cell >= 0 ? cells[g.b_cell] : ca;
  const long u = (long)(blockIdx.x - t.blk0[k]) * 256 + threadIdx.x;
  if (u == 0 && g.ext_cell) *g.ext_cell = cb;
  if (u >= g.total / 16) return;  // (total: a multiple of the 2048 elements of a fragment pair)
  pack_w_s3x_frag2(g.w, u, g.Cin / 8, 3, g.NS, g.so, g.si, g.flip, cells[k], g.split_c, ca, cb, (uint4*)g.wp);
}

}  // namespace

size_t wprep_bytes(const WPrepSeg* segs, int n) {
  size_t b = kWPrepCellBytes;
  for (int i = 0; i < n; ++i) b += s3x_packed_bytes(segs[i].Cin, segs[i].Kout, 3, 2);
  return b;
}

// region: [kWPrepCellBytes of cells: word k = segment k's weight cell, words kWPrepBoundCell0 + j = bound j | the segments' packs in order].
// out[k] (nullable) <- what conv_s3x_h2 takes for segment k.
int wprep_run(const WPrepSeg* segs, int n, const WPrepBound* bounds, int nb, void* region, S3xPrepared* out, hipStream_t s) {
  if (n < 0 || n > kWPrepMaxSegs || nb < 0 || nb > kWPrepMaxBounds || !region) { set_error("wprep_run: bad table"); return NC_ERR_ARG; }
  unsigned* cells = (unsigned*)region;
  char* packs = (char*)region + kWPrepCellBytes;
  WPrepDevTable t{};
  WPrepDevBounds tb{};
  const bool frag = sw::get(sw::STREAM_PASSES) != 0;  // (k_wprep_absmax_rows + k_wprep_pack_frag; off: the kernels as they were)
  if (frag && ((uintptr_t)packs & 15) != 0) { set_error("wprep_run: the region must be 16-byte aligned"); return NC_ERR_ARG; }  // (the convolutions read the packs as uint4)
  t.nseg = n;
  size_t off = 0;
  unsigned blk = 0;
  for (int k = 0; k < n; ++k) {
    const WPrepSeg& h = segs[k];
    t.blk0[k] = blk;
    if (out) out[k] = S3xPrepared{nullptr, nullptr};
    if (!h.w) { off += s3x_packed_bytes(h.Cin, h.Kout, 3, 2); continue; }  // (a segment left out keeps its place: the layout is the caller's plan)
    if (h.Cin % 64 || h.Kout % 64 || (!h.flip && h.b_cell >= 0 && (h.b_cell < kWPrepBoundCell0 || h.b_cell >= kWPrepBoundCell0 + nb)) ||
        (h.flip && h.b_cell >= 0)) {
      set_error("wprep_run: segment %d not covered", k);
      return NC_ERR_SHAPE;
    }
    WPrepDevSeg& g = t.seg[k];
    const size_t bytes = s3x_packed_bytes(h.Cin, h.Kout, 3, 2);
    g.w = h.w; g.wp = (unsigned short*)(packs + off); g.ext_cell = h.ext_cell;
    g.total = (long)(bytes / 2); g.nw = (long)h.Cin * h.Kout * 27;
    g.Cin = h.Cin; g.NS = s3x_ksteps(h.Cin, 3); g.flip = h.flip;
    // forward: w[co][ci][tap], the second half of the input channels is the second scale group (conv_split.hip run_s3 passes Cin / 2 whatever
    // the input is: both cells of a whole tensor are equal, the factor is 1); data gradient: w[co as ci][ci as co][26 - tap], no groups
    g.so = h.flip ? 27 : (long)h.Cin * 27; g.si = h.flip ? (long)h.Kout * 27 : 27;
    g.split_c = h.flip ? h.Cin : h.Cin / 2;
    g.b_cell = h.b_cell; g.a_bits = h.a_bits;
    blk += (unsigned)cdiv(frag ? g.total / 16 : g.total, 256);
    if (out) { out[k].wp = packs + off; out[k].wcell = cells + k; }
    off += bytes;
  }
  t.blk0[n] = blk;
  int kmax = 0;
  for (int j = 0; j < nb; ++j) {
    tb.b[j] = bounds[j];
    tb.b[j].cell = kWPrepBoundCell0 + j;
    if (bounds[j].K > kmax) kmax = bounds[j].K;
  }
  tb.n = nb;
  if (int e = h2_zero_cells(cells, kWPrepBoundCell0 + kWPrepMaxBounds, s)) return e;
  if (nb) hipLaunchKernelGGL(k_wprep_bounds, dim3((unsigned)cdiv((long)kmax * 8, 64), (unsigned)nb), dim3(256), 0, s, tb, cells);
  // (256 blocks per segment, as before: every block ends in one atomicMax and the cells share a cache line -- with 1024 blocks per segment the
  // pass took twice as long)
  if (n && frag) hipLaunchKernelGGL(k_wprep_absmax_rows, dim3(256, (unsigned)n), dim3(256), 0, s, t, cells);
  else if (n) hipLaunchKernelGGL(k_wprep_absmax, dim3(256, (unsigned)n), dim3(256), 0, s, t, cells);
  if (blk && frag) hipLaunchKernelGGL(k_wprep_pack_frag, dim3(blk), dim3(256), 0, s, t, (const unsigned*)cells);
  else if (blk) hipLaunchKernelGGL(k_wprep_pack, dim3(blk), dim3(256), 0, s, t, (const unsigned*)cells);
  return check_launch("wprep_run");
}

}  // namespace nc
