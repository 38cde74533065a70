// Launch arguments and host entry points of the fused-step kernel family
// (csrc/fwd_chain.hip, csrc/bwd_chain.hip, csrc/wgrad_frag.hip). The only
// declaration of these functions: the definitions and the binding
// (csrc/shuffle_ops.cpp) both include it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rsdl {

struct ChainWeights {
  const void* W1;   // bf16 fragment-major [512,112] (K padded)
  const float* b1;  // [512]
  const void* W2;   // bf16 fragment-major [256,512]
  const float* b2;  // [256]
  const void* W3;   // bf16 fragment-major [128,256]
  const float* b3;  // [128]
  const void* w4;   // bf16 [128]
  const float* b4;  // [1]
};

// ``rows`` = rows per workgroup slab, 32 or 64 (validated by the binding).
struct FwdChainArgs {
  const void* x0s;  // bf16 fragment-major x (launch_swizzle_x[_both])
  ChainWeights w;
  void* a1t;        // bf16 wgrad fragment-major a1^T
  uint32_t* mask1;  // [m_tiles, 512] relu-mask words
  void* a2t;
  uint32_t* mask2;  // [m_tiles, 256]
  void* a3;         // bf16 [M,128]
  void* out;        // bf16 [M,1]
  // Loss epilogue, all three or none: inv_m is 1/M with a target, 0 without.
  const float* target;  // fp32 [M]
  void* dyb;            // bf16 [M,1]
  float* loss_part;     // [fwd_chain_grid(M, rows)]
  int64_t M;
  int pi16, rows;
  int loss;  // FC_LOSS_MSE = 0, FC_LOSS_BCE = 1
  // The weighted head (needs a target): ``weight`` fp32 [M] or null (every
  // w = 1), ``pos_weight`` > 0 (BCE only). Both are ignored when unset.
  bool weighted;
  const float* weight;
  float pos_weight;
};

struct EvalChainArgs {
  const void* x0s;
  ChainWeights w;
  float* pred;          // fp32 [M], or null
  const float* target;  // fp32 [M], or null (then so is part)
  float* part;  // [fwd_chain_grid(M, rows), weighted ? 8 : 4]
  int64_t M;
  int rows;
  int task;       // FC_LOSS_MSE (regression) or FC_LOSS_BCE (binary)
  int64_t* hist;  // int64 [2,65536] AUC histogram, or null (binary only)
  // Weighted partials (need a target): ``weight`` fp32 [M] or null.
  bool weighted;
  const float* weight;
};

struct BwdChainArgs {
  const void* dy;     // bf16 [M]
  const void* a3;     // bf16 [M,128]
  const void* mask1;  // [m_tiles, 512] relu-mask words
  const void* mask2;  // [m_tiles, 256]
  const void* w4;     // bf16 [128]
  const void* W3T;    // bf16 fragment-major W3^T [256,128]
  const void* W2T;    // bf16 fragment-major W2^T [512,256]
  void* dz1t;         // bf16 wgrad fragment-major dz^T
  void* dz2t;
  void* dz3t;
  float* db_part;  // [bwd_chain_grid(M, rows), 1156]
  int64_t M;
  int pi16, rows;
};

// csrc/fwd_chain.hip
int64_t fwd_chain_grid(int64_t M, int rows);
void launch_swizzle_x(const void* x, void* out, int64_t M,
                      hipStream_t stream);
void launch_swizzle_xt(const void* x, void* out, int64_t M, int pi16,
                       hipStream_t stream);
void launch_swizzle_x_both(const void* x, void* xs, void* xt, int64_t M,
                           int pi16, hipStream_t stream);
void launch_fwd_chain(const FwdChainArgs& p, hipStream_t stream);
void launch_eval_chain(const EvalChainArgs& p, hipStream_t stream);

// csrc/bwd_chain.hip
int64_t bwd_chain_grid(int64_t M, int rows);
void launch_bwd_chain(const BwdChainArgs& p, hipStream_t stream);

// csrc/wgrad_frag.hip
int64_t wgrad_frag_nslabs(int64_t mchunks, int32_t N, int32_t K,
                          int32_t nt_w, int32_t kt_w);
// variant: 0 = default (RSDL_WGRAD_LDS, then the per-shape default),
// 1 = direct kernel, 2 = LDS-ring kernel (12-fragment tiles only).
bool wgrad_frag_has_lds(int32_t nt_w, int32_t kt_w);
void launch_wgrad_frag(const void* AT, const void* BT, float* dW, int32_t N,
                       int32_t K, int64_t mchunks, int32_t nt_w,
                       int32_t kt_w, int32_t variant, hipStream_t stream);
void launch_slab_reduce(const float* part, float* out, int64_t nk,
                        int64_t nslabs, hipStream_t stream);
// The train step's three wgrads (dW1 [512,128], dW2 [256,512], dW3
// [128,256]; the 12-fragment ring tiles) as one launch. part_i must hold
// wgrad_grouped_nslabs(mchunks).ns[i] slabs of N*K floats; the launcher
// returns the same counts. Needs mchunks > 0.
struct WgradGroupedSlabs {
  int64_t ns[3];
};
WgradGroupedSlabs wgrad_grouped_nslabs(int64_t mchunks);
WgradGroupedSlabs launch_wgrad_grouped(const void* AT1, const void* BT1,
                                       float* part1, const void* AT2,
                                       const void* BT2, float* part2,
                                       const void* AT3, const void* BT3,
                                       float* part3, int64_t mchunks,
                                       hipStream_t stream);
// RSDL_WGRAD_GROUPED and the knobs that rule the grouped launch out,
// latched at the first call.
bool wgrad_grouped_default();

}  // namespace rsdl
