// Unet_deconv (reference models/networks.py:478-538) described once, for the inference forward (unet_fwd.hip) and the two training paths
// (gen_nets.hip, gen_nets_lp.hip): the ten blocks, the parameter blob's offsets, the edge rule and the three resolution levels.
#pragma once
#include <cstddef>

namespace nc {

struct UBlock { int C, K, lvl; };  // 3^3 conv + InstanceNorm + ReLU; lvl 0 = full resolution, 1 = half, 2 = quarter
constexpr UBlock kUB[10] = {{1, 64, 0},    {64, 64, 0},   {64, 128, 1},  {128, 128, 1}, {128, 256, 2},
                            {256, 256, 2}, {256, 256, 2}, {256, 128, 1}, {128, 128, 1}, {128, 64, 0}};

// MaxPool3d floors and the skip concatenations would not line up otherwise (reference networks.py:526,531)
inline bool u_edges_ok(int S0, int S1, int S2) { return S0 >= 4 && S1 >= 4 && S2 >= 4 && !((S0 | S1 | S2) & 3); }

// spatial size and voxels per level
inline void u_level_dims(int S0, int S1, int S2, int (&d)[3][3], long (&S)[3]) {
  for (int l = 0; l < 3; ++l) {
    d[l][0] = S0 >> l; d[l][1] = S1 >> l; d[l][2] = S2 >> l;
    S[l] = (long)d[l][0] * d[l][1] * d[l][2];
  }
}

// offsets (floats) of the 28 tensors inside the packed parameter blob, state-dict order, fp32, back to back:
// dc1.0 dc1.3 dc2.0 dc2.3 bot.0 bot.3 bot.6 t_conv2 ex2.0 ex2.3 t_conv1 ex1.0 1x1 1x1_2
struct UOff { size_t w[14], b[14], total; };  // ids 0..9 = blocks, 10 = t_conv2, 11 = t_conv1, 12 = one_by_one, 13 = one_by_one_2
inline UOff u_offsets() {
  struct L { int id; size_t wn, bn; };
  const L order[14] = {{0, 64 * 1 * 27, 64},     {1, 64 * 64 * 27, 64},    {2, 128 * 64 * 27, 128},  {3, 128 * 128 * 27, 128},
                       {4, 256 * 128 * 27, 256}, {5, 256 * 256 * 27, 256}, {6, 256 * 256 * 27, 256}, {10, 256 * 128 * 8, 128},
                       {7, 128 * 256 * 27, 128}, {8, 128 * 128 * 27, 128}, {11, 128 * 64 * 8, 64},   {9, 64 * 128 * 27, 64},
                       {12, 64, 1},              {13, 1, 1}};
  UOff o{};
  size_t off = 0;
  for (const L& l : order) {
    o.w[l.id] = off; off += l.wn;
    o.b[l.id] = off; off += l.bn;
  }
  o.total = off;
  return o;
}

}  // namespace nc
