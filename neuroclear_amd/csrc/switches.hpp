// Every switch of libnc_hip.so in ONE table.  Plain C++17, no HIP header: the host compiler builds switches.cpp alone (tests/switches_driver.cpp).
// A switch is process-wide, one relaxed atomic int.  The table is filled once, when the library is loaded: a row's variable is read THEN
// (getenv once, atoi once; text that does not parse is 0), never at first use.  The C ABI moves the first rows at run time (api.hip: one-liners
// over sw::set); the others are A/B flags of the environment alone.  Rows marked frozen are sampled when the outermost scope of a thread opens
// (SwitchScope / NetworkScope) and sw::get returns that sample until it closes: another thread cannot desynchronise the phases of one call.
#pragma once
#include <atomic>

namespace nc {
namespace sw {

// how a value is made legal: kRaw as given; kBool v != 0; kRange02 clamped to [0, 2]; kTerms 0 or 3, else 2; kGuard 2, else v != 0; kP2dTerms 1 or 2, else 3
enum Clamp { kRaw, kBool, kRange02, kTerms, kGuard, kP2dTerms };

// X(identifier, variable or nullptr, default, clamp of the variable's value, clamp of sw::set, frozen per call); S3X onwards: no setter
// (the two clamps differ where the setter was always stricter than the load-time read: NC_SPLIT_TERMS=5 is stored as 5, nc_set_split_terms(5) as 2)
#define NC_SWITCH_TABLE(X)                                                                                                    \
  X(FORCE_DIRECT, nullptr, 0, kRaw, kRaw, false)             /* the VALU kernels everywhere (tests) */                        \
  X(CONV_SPLIT, "NC_CONV_SPLIT", 1, kRaw, kRaw, false)       /* the split-operand kernels (conv_split.hip) */                 \
  X(S3_FUSE, "NC_S3_FUSE", 1, kRaw, kRaw, false)             /* nc_unet_deconv_fwd: the norm pass writes the operand form */  \
  X(SPLIT_TERMS, "NC_SPLIT_TERMS", 2, kRaw, kTerms, true)    /* 2 two-term fp16, 3 three-term bf16, 0 (conv_s3x.hip) */       \
  X(H2_GUARD, "NC_H2_GUARD", 1, kRaw, kGuard, true)          /* the range guard's mode (common.hpp) */                        \
  X(IN_BWD_FOLD, "NC_IN_BWD_FOLD", 1, kBool, kBool, true)    /* pool backward folded into the norm backward */                \
  X(STREAM_PASSES, nullptr, 1, kRaw, kBool, true)            /* the streaming passes at the HBM rate */                       \
  X(EPI_STATS, "NC_EPI_STATS", 1, kRaw, kRange02, false)     /* InstanceNorm sums from the convolution's epilogue */          \
  X(S3X_W64, "NC_S3X_W64", 1, kRaw, kBool, false)            /* k_conv_s3w */                                                 \
  X(P2D_TERMS, "NC_P2D_TERMS", 1, kRaw, kP2dTerms, false)    /* operand form of the PatchGAN 4 x 4 layers (conv_p2d.hip) */   \
  X(C8X, "NC_C8X", 1, kRaw, kRange02, false)                 /* 0 k_conv_h, 1 where the launch fills its rounds, 2 wherever */\
  X(UNET_LEAN, "NC_UNET_LEAN", 1, kBool, kBool, false)       /* U-Net train step without unread fp32 tensors */               \
  X(UNET_WPREP, "NC_UNET_WPREP", 1, kBool, kBool, false)     /* U-Net train step: one weight-preparation pass */              \
  X(DL_COLLAPSE, "NC_DL_COLLAPSE", 2, kRange02, kRange02, false) /* deep_linear_gen's collapsed tail; 2: typed kernel */      \
  X(CONV2D_K3, nullptr, 1, kRaw, kBool, false)               /* the image-tiled Conv2d 3 x 3 kernel */                        \
  X(CONV2D_K3_CFG, nullptr, -1, kRaw, kRaw, false)           /* its pinned tile configuration; -1: the heuristic */           \
  X(SCONV_CFG_PIN, nullptr, -1, kRaw, kRaw, false)           /* nc_sconv_set_cfg; -1: none */                                 \
  X(SCONV_TUNE_MODE, nullptr, -1, kRaw, kRaw, false)         /* nc_sconv_set_tune: 0 / 1; negative: SCONV_TUNE decides */     \
  X(S3X, "NC_S3X", 1, kRaw, kRaw, false)                     /* 0: the round-2 kernels of conv_split.hip, three-term only */  \
  X(S3X_WGRAD, "NC_S3X_WGRAD", 1, kRaw, kRaw, false)                                                                          \
  X(HX_WGRAD, "NC_HX_WGRAD", 1, kRaw, kRaw, false)           /* 0: conv_h.hip's k_wgrad_h */                                  \
  X(S3X_TAIL, "NC_S3X_TAIL", 1, kRaw, kRaw, false)                                                                            \
  X(S3X_NCB7, "NC_S3X_NCB7", 1, kRaw, kRaw, false)           /* 0: even column-block counts only */                           \
  X(S3X_FLUSH, "NC_S3X_FLUSH", 4, kRaw, kRaw, false)         /* k-steps between accumulator restarts */                       \
  X(C1K7_H2, "NC_C1K7_H2", 1, kRaw, kRaw, false)             /* 0: the fp32 matrix kernel */                                  \
  X(C1K3, "NC_C1K3", 1, kRaw, kRaw, false)                   /* 0: the general brick kernel */                                \
  X(C1_WGRAD, "NC_C1_WGRAD", 1, kRaw, kRaw, false)                                                                            \
  X(CONVT_S3X, "NC_CONVT_S3X", 1, kRaw, kRaw, false)         /* 0: the fp32 kernels of convt.hip */                           \
  X(CONVT_H2, "NC_CONVT_H2", 1, kRaw, kRaw, false)           /* 0: three-term input, fp32 output measured and converted */    \
  X(S3_TRAIN_FUSE, "NC_S3_TRAIN_FUSE", 1, kRaw, kRaw, false)                                                                  \
  X(INFER_BATCHED, "NC_INFER_BATCHED", 1, kRaw, kRaw, false)                                                                  \
  X(DL_K32, "NC_DL_K32", 1, kRaw, kRaw, false)                                                                                \
  X(DL_RANK_WGRAD, "NC_DL_RANK_WGRAD", 1, kRaw, kRaw, false)                                                                  \
  X(DL_RANK_DGRAD, "NC_DL_RANK_DGRAD", 1, kRaw, kRaw, false)                                                                  \
  X(PG1, "NC_PG1", 1, kRaw, kRaw, false)                     /* 0: the PatchGAN's first layer on the generic kernels */       \
  X(PG1_FEW, "NC_PG1_FEW", 1, kRaw, kRaw, false)             /* 0: the one-thread-per-pixel-block kernel at every size */     \
  X(P2D, "NC_P2D", 7, kRaw, kRaw, false)                     /* bits: 1 stride-1 layer, 2 stride-2 layers, 4 weight gradient */\
  X(SCONV, "NC_SCONV", 1, kRaw, kRaw, false)                 /* 0: the gather GEMM for the PatchGAN layers */                 \
  X(SCONV_WGRAD, "NC_SCONV_WGRAD", 1, kRaw, kRaw, false)     /* (needs SCONV as well) */                                      \
  X(SCONV_CFG, "NC_SCONV_CFG", -1, kRaw, kRaw, false)        /* i >= 0: only tile configuration i */                          \
  X(SCONV_TUNE, "NC_SCONV_TUNE", 1, kRaw, kRaw, false)       /* 0: never time the configurations */                           \
  X(H_ABLATE, "NC_H_ABLATE", 0, kRaw, kRaw, false)           /* timing experiments: bit mask (conv_h.hip) */                  \
  X(W_DIFFUSE, "NC_W_DIFFUSE", 1, kRaw, kRaw, false)         /* 0: no tap-diffused 16-bit weight rounding */

enum Id {
#define NC_SW_ID(id, env, def, eclamp, sclamp, frozen) id,
  NC_SWITCH_TABLE(NC_SW_ID)
#undef NC_SW_ID
  kCount
};

struct Row { const char* name; const char* env; int def; Clamp env_clamp, set_clamp; bool frozen; };
extern const Row kRows[kCount];
extern std::atomic<int> g_value[kCount];  // filled by switches.cpp's initialiser at load

inline int raw(Id id) { return g_value[id].load(std::memory_order_relaxed); }
int get(Id id);         // frozen rows inside a scope of this thread: the sample; else raw
int set(Id id, int v);  // applies the row's clamp, returns the previous (raw) value

}  // namespace sw

// RAII: the frozen switches as THIS call sees them (NetworkScope opens one; the per-layer entry points with more than one phase open their own)
struct SwitchScope { SwitchScope(); ~SwitchScope(); };
// RAII mark of a whole-network call (gen_nets.hip, unet_fwd.hip): inside one, guard mode 1 COUNTS a flagged measured tensor instead of launching the
// three-term kernels beside the two-term ones (h2_guard_can_flip) -- ~65 near-empty launches per training step otherwise
struct NetworkScope { NetworkScope(); ~NetworkScope(); };
// RAII: this thread sees nc_set_split_terms(2) while it lives (kernels that exist in the two-term form only and convert their fp32 operands
// themselves).  The terms alone: the other frozen rows stay as it found them, sampled or not.
struct ForceTwoTerm { ForceTwoTerm(); ~ForceTwoTerm(); int prev_terms; };
// the explicit S3 entry points (nc_conv_*_split, operands from nc_to_s3) are three-term by definition, whatever nc_set_split_terms says
struct ForceThreeTerm { ForceThreeTerm(); ~ForceThreeTerm(); };
bool force_three_term();   // a ForceThreeTerm lives on this thread
bool h2_guard_can_flip();  // mode 2, or mode 1 outside a whole-network call

}  // namespace nc
