// 2-D dice / assemble on the device: the arithmetic of dice.hip (reference data/diceImage_dataset.py:95-120, data/base_dataset.py:134-143,
// util/util.py:196-215, util/assemble_dice.py:130-213) restricted to the two in-plane axes.  The image is a stack [L0][L1][L2] of planes;
// axis 0 is neither diced, padded nor reflected.  Tile t lies in plane t / (n1 n2), at yi = (t % (n1 n2)) / n2, xi = t % n2 (x fastest).
//   tile  = float32( double(v) / 65535.0 )                  zero dicing pad, reflect border
//   acc  += tile[b:-b, b:-b] / 8   in tile-index order       (the / 8 ... * 8 of the 3-D assembler is kept: a plane then equals a z-layer
//   out   = uintN( ((acc / cnt) * 8) * scale )  truncating    of the 3-D path that one layer of cubes covers)
// Every entry point handles `count` consecutive tiles in ONE launch.  The scatter-add runs one thread per ACCUMULATOR pixel, which adds the
// tiles of the batch that cover it in ascending tile index: no two threads write one address (no atomics), and the sum does not depend
// on how the tile sequence is cut into batches.
#include "dice_geom.hpp"

namespace nc {

template <typename T>
__global__ void k_cut_tiles2d(const T* __restrict__ img, DiceGeom g, long first, int count, double den, float* __restrict__ tiles) {
  const int E = g.roi + 2 * g.border;
  const long per = (long)g.n1 * g.n2, total = (long)count * E * E;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cx = (int)(i % E), cy = (int)((i / E) % E);
    const long t = first + i / ((long)E * E);
    const long z = t / per;
    const int r = (int)(t % per), yi = r / g.n2, xi = r % g.n2;
    const int qy = reflect_idx(yi * g.step + cy - g.border, g.P1);
    const int qx = reflect_idx(xi * g.step + cx - g.border, g.P2);
    float v = 0.f;
    if (qy < g.L1 && qx < g.L2) v = (float)((double)img[(z * g.L1 + qy) * g.L2 + qx] / den);
    tiles[i] = v;
  }
}

// rows [row0, row0 + nrows) of the accumulator seen as (L0 * P1) rows of P2 floats: the rows from the first tile's first to the last tile's last
__global__ void k_scatter_add2d(const float* __restrict__ tiles, float* __restrict__ acc, DiceGeom g, long first, int count, long row0,
                                long nrows) {
  const int E = g.roi + 2 * g.border;
  const long per = (long)g.n1 * g.n2, total = nrows * g.P2, last = first + count;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = row0 + i / g.P2;
    const int x = (int)(i % g.P2), y = (int)(row % g.P1);
    const long z = row / g.P1;
    int ylo, yhi, xlo, xhi;
    cover_range(y, g.n1, g.step, g.roi, ylo, yhi);
    cover_range(x, g.n2, g.step, g.roi, xlo, xhi);
    float* a = acc + row * g.P2 + x;
    float v = 0.f;
    bool hit = false;
    for (int yi = ylo; yi <= yhi; ++yi)
      for (int xi = xlo; xi <= xhi; ++xi) {  // ascending tile index
        const long t = z * per + (long)yi * g.n2 + xi;
        if (t < first || t >= last) continue;
        if (!hit) { v = *a; hit = true; }
        const float c = tiles[((t - first) * E + (y - yi * g.step + g.border)) * E + (x - xi * g.step + g.border)];
        v = __fadd_rn(v, __fdiv_rn(c, 8.f));
      }
    if (hit) *a = v;
  }
}

template <typename T>
__global__ void k_finalize2d(const float* __restrict__ acc, T* __restrict__ out, DiceGeom g, float scale) {
  const long total = (long)g.L0 * g.L1 * g.L2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int x = (int)(i % g.L2), y = (int)((i / g.L2) % g.L1);
    const long z = i / ((long)g.L2 * g.L1);
    const float cnt = (float)(cover_count(y, g.n1, g.step, g.roi) * cover_count(x, g.n2, g.step, g.roi));
    float v = acc[(z * g.P1 + y) * g.P2 + x];
    v = __fmul_rn(__fmul_rn(__fdiv_rn(v, cnt), 8.f), scale);
    out[i] = (T)v;  // truncation toward zero == ndarray.astype for in-range values
  }
}

}  // namespace nc

using namespace nc;

extern "C" {

int nc_dice2d_cut_tiles(const void* img, int is_u16, int L0, int L1, int L2, int roi, int overlap, int border, long first, int count,
                        float* tiles, void* stream) {
  if (!img || !tiles) { set_error("dice2d_cut_tiles: null pointer"); return NC_ERR_ARG; }
  DiceGeom g;
  if (!make_geom(g, kPlanes, kOriginal, L0, L1, L2, roi, overlap, border) || !g.reflect_fits(kPlanes)) {
    set_error("dice2d_cut_tiles: bad geometry (border_cut must be >= 1)");
    return NC_ERR_SHAPE;
  }
  if (first < 0 || count < 1 || first + count > g.pieces()) {
    set_error("dice2d_cut_tiles: tiles [%ld, %ld + %d) out of [0,%ld)", first, first, count, g.pieces());
    return NC_ERR_SHAPE;
  }
  const long E = roi + 2 * border;
  hipStream_t s = (hipStream_t)stream;
  if (is_u16)
    hipLaunchKernelGGL(k_cut_tiles2d<uint16_t>, dim3(flat_grid(count * E * E)), dim3(256), 0, s, (const uint16_t*)img, g, first, count,
                       65535.0, tiles);
  else
    hipLaunchKernelGGL(k_cut_tiles2d<uint8_t>, dim3(flat_grid(count * E * E)), dim3(256), 0, s, (const uint8_t*)img, g, first, count, 255.0,
                       tiles);
  return check_launch("dice2d_cut_tiles");
}

int nc_assemble2d_scatter_add(const float* tiles, float* acc, int L0, int P1, int P2, int roi, int overlap, int border, long first,
                              int count, void* stream) {
  if (!tiles || !acc) { set_error("assemble2d_scatter_add: null pointer"); return NC_ERR_ARG; }
  if (overlap < 1) { set_error("assemble2d_scatter_add: overlap must be >= 1 (the reference assembler adds nothing for overlap 0, util/assemble_dice.py:170)"); return NC_ERR_SHAPE; }
  DiceGeom g;
  if (!make_geom(g, kPlanes, kPadded, L0, P1, P2, roi, overlap, border) || !g.reflect_fits(kPlanes)) {
    set_error("assemble2d_scatter_add: bad geometry (border_cut must be >= 1)");
    return NC_ERR_SHAPE;
  }
  if (first < 0 || count < 1 || first + count > g.pieces()) { set_error("assemble2d_scatter_add: tile index out of range"); return NC_ERR_SHAPE; }
  const long per = (long)g.n1 * g.n2, tl = first + count - 1;
  const long row0 = (first / per) * P1 + ((first % per) / g.n2) * (long)g.step;
  const long row1 = (tl / per) * P1 + ((tl % per) / g.n2) * (long)g.step + roi;  // <= (plane + 1) * P1: (n1 - 1) step + roi <= P1
  hipLaunchKernelGGL(k_scatter_add2d, dim3(flat_grid((row1 - row0) * P2)), dim3(256), 0, (hipStream_t)stream, tiles, acc, g, first, count,
                     row0, row1 - row0);
  return check_launch("assemble2d_scatter_add");
}

int nc_assemble2d_finalize(const float* acc, void* out, int out_is_u16, int L0, int P1, int P2, int L1, int L2, int roi, int overlap,
                           void* stream) {
  if (!acc || !out) { set_error("assemble2d_finalize: null pointer"); return NC_ERR_ARG; }
  if (overlap < 1) { set_error("assemble2d_finalize: overlap must be >= 1 (util/assemble_dice.py:170)"); return NC_ERR_SHAPE; }
  DiceGeom g;
  if (!make_geom(g, kPlanes, kOriginal, L0, L1, L2, roi, overlap, 1) || g.P1 != P1 || g.P2 != P2) {
    set_error("assemble2d_finalize: padded size does not match pad_for_dicing of the original size");
    return NC_ERR_SHAPE;
  }
  const long total = (long)L0 * L1 * L2;
  hipStream_t s = (hipStream_t)stream;
  if (out_is_u16)
    hipLaunchKernelGGL(k_finalize2d<uint16_t>, dim3(flat_grid(total)), dim3(256), 0, s, acc, (uint16_t*)out, g, 65535.f);
  else
    hipLaunchKernelGGL(k_finalize2d<uint8_t>, dim3(flat_grid(total)), dim3(256), 0, s, acc, (uint8_t*)out, g, 255.f);
  return check_launch("assemble2d_finalize");
}

}  // extern "C"
