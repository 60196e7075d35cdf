// The dice grid shared by dice.hip (cubes of a volume) and dice2d.hip (tiles of a stack of planes): reference data/diceImage_dataset.py:95-120,
// util/util.py:196-215.  An axis of length L is zero-padded to P = pad_len(L) and cut into n = (P - overlap) / step pieces of `roi` at
// multiples of step = roi - overlap.  A stack of planes is the same grid with axis 0 neither diced nor padded: P0 = n0 = L0, one piece per plane,
// so that piece t lies at (t / (n1 n2), (t % (n1 n2)) / n2, t % n2) in both cases (x fastest).
#pragma once
#include "common.hpp"

namespace nc {

__device__ __forceinline__ int reflect_idx(int q, int P) {  // np.pad(mode='reflect') for |overhang| < P
  if (q < 0) q = -q;
  if (q >= P) q = 2 * (P - 1) - q;
  return q;
}

__host__ __device__ inline int pad_len(int L, int roi, int overlap) {
  const int step = roi - overlap;
  return step * ((L + overlap) / step) + roi;  // L + pad
}

// the piece indices i in [0, n) with i*step <= p < i*step + roi are lo .. hi
__device__ __forceinline__ void cover_range(int p, int n, int step, int roi, int& lo, int& hi) {
  hi = p / step;
  if (hi > n - 1) hi = n - 1;
  lo = p - roi + 1;
  lo = lo <= 0 ? 0 : (lo + step - 1) / step;
}

__device__ __forceinline__ int cover_count(int p, int n, int step, int roi) {
  int lo, hi;
  cover_range(p, n, step, roi, lo, hi);
  return hi - lo + 1;
}

enum DiceAxes { kVolume, kPlanes };    // all three axes diced | axis 0 neither diced nor padded
enum DiceSize { kOriginal, kPadded };  // what the caller knows: the original size (padded here) | the padded size only

struct DiceGeom {
  int L0, L1, L2, P0, P1, P2, n0, n1, n2, roi, overlap, border, step;
  long pieces() const { return (long)n0 * n1 * n2; }
  // np.pad(mode='reflect') with border >= padded length is multi-fold; the reference never gets there
  bool reflect_fits(DiceAxes axes) const { return (axes == kPlanes || border < P0) && border < P1 && border < P2; }
};

// The one checker: false for a grid the reference cannot dice.  From kPadded sizes the original ones stay 0 (but L0 of kPlanes).
inline bool make_geom(DiceGeom& g, DiceAxes axes, DiceSize given, int S0, int S1, int S2, int roi, int overlap, int border) {
  if (S0 < 1 || S1 < 1 || S2 < 1 || roi < 1 || overlap < 0 || overlap >= roi || border < 1) return false;
  const bool padded = given == kPadded, planes = axes == kPlanes;
  g = DiceGeom{};
  g.roi = roi; g.overlap = overlap; g.border = border; g.step = roi - overlap;
  if (!padded) { g.L1 = S1; g.L2 = S2; }
  if (!padded || planes) g.L0 = S0;
  g.P0 = padded || planes ? S0 : pad_len(S0, roi, overlap);
  g.P1 = padded ? S1 : pad_len(S1, roi, overlap);
  g.P2 = padded ? S2 : pad_len(S2, roi, overlap);
  g.n0 = planes ? S0 : (g.P0 - overlap) / g.step; g.n1 = (g.P1 - overlap) / g.step; g.n2 = (g.P2 - overlap) / g.step;
  return g.n0 >= 1 && g.n1 >= 1 && g.n2 >= 1;
}

inline unsigned flat_grid(long n) {
  long b = cdiv(n, 256);
  if (b > 8192) b = 8192;
  return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace nc
