// The convolution layer dispatch: the profiler's path numbers, the rungs nc_conv_fwd / nc_conv_dgrad / nc_conv_wgrad can launch, and the function
// that picks one from api.hip's table kRungs.  A new kernel family is one row there plus one `case` in the entry point.
#pragma once
#include <cstddef>

namespace nc {

struct ConvDims;

// The path field of ProfScope's cls (4 bits): every ProfScope names one of these; nc_conv_path_name gives the tags (DESIGN.md 1 lists them).
enum ConvPath {
  kPathDirect, kPathMfma, kPathGemm, kPathFlat, kPathTaps, kPathK1, kPathTo1, kPathImg, kPathPg1, kPathSplit, kPathSplit2d, kPathC1k7,
  kPathLk, kPathK3Img
};
static_assert(kPathLk == 12 && kPathK3Img == 13, "recorded profiles carry these numbers");

// One value per thing a layer entry point can launch, in the order the route tries them (finer than the path: two rungs may report one path).
enum ConvRung {
  kRungS3, kRungP2d, kRungC1k7, kRungK3Img, kRungC1k3, kRungBrick, kRungFlat, kRungTaps, kRungK1, kRungTo1Mfma, kRungTo1, kRungPg1, kRungImg,
  kRungImgWgrad, kRungGemm, kRungDirect, kRungCount
};

int path_of(ConvRung r);
// The rung op (0 forward, 1 data gradient, 2 weight gradient) of a layer runs on with the workspace the call brings: every switch read once,
// the first row of kRungs that applies.  skip: a bit per rung the caller does not want reported (the batch-free path queries).
ConvRung conv_route(int op, const ConvDims& d, const void* ws = nullptr, size_t ws_bytes = 0, unsigned skip = 0);

}  // namespace nc
