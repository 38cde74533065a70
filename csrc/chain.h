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

#if defined(__HIPCC__)
// The epilogue arithmetic of the chain layers on one MFMA D fragment
// (v_mfma_f32_32x32x16_bf16: regs 2q / 2q+1 are consecutive rows of one
// column), shared by fc_layer (csrc/fwd_chain.hip) and the dW2 wgrad body
// that recomputes a1 (csrc/wgrad_frag.hip): the recomputed fragments are
// the emitted ones bit for bit because both run exactly this code.
typedef __attribute__((__vector_size__(2 * sizeof(float)))) float fc_f32x2;
typedef __attribute__((__vector_size__(4 * sizeof(unsigned int))))
unsigned int fc_u32x4;

__device__ __forceinline__ fc_f32x2 fc_pk_max0(fc_f32x2 v) {
  // no packed f32 max on gfx950; two v_max_f32
  fc_f32x2 r = {fmaxf(v[0], 0.f), fmaxf(v[1], 0.f)};
  return r;
}
__device__ __forceinline__ uint32_t fc_cvt_pk_bf16(fc_f32x2 v) {
  uint32_t p;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(p) : "v"(v[0]), "v"(v[1]));
  return p;
}
// One row pair: packed bias add, (relu), packed bf16 convert.
template <bool RELU>
__device__ __forceinline__ uint32_t fc_epi_pair(float r0, float r1,
                                                fc_f32x2 bv2) {
  fc_f32x2 v2 = {r0, r1};
  v2 += bv2;
  if (RELU) v2 = fc_pk_max0(v2);
  return fc_cvt_pk_bf16(v2);
}
// The half-row exchange of the transposed emission (not PI16): lanes l and
// l + 32 (h = lane >> 5) hold complementary 4-row runs of a column in
// p[0..8); 4 shuffles of packed pairs assemble the 8-row runs. Lane h = 0
// ends with rows {0-7} (run0) and {16-23} (run1), h = 1 with {8-15} and
// {24-31}: run0 / run1 are this lane's 16 bytes of the wgrad fragments of
// the m-tile's two 16-row chunks.
__device__ __forceinline__ void fc_half_row_exchange(const uint32_t (&p)[8],
                                                     int32_t h,
                                                     fc_u32x4& run0,
                                                     fc_u32x4& run1) {
  uint32_t rx[4];
  #pragma unroll
  for (int j = 0; j < 2; j++) {
    rx[j] = __shfl_xor((int)(h == 0 ? p[2 + j] : p[j]), 32);
    rx[2 + j] = __shfl_xor((int)(h == 0 ? p[6 + j] : p[4 + j]), 32);
  }
  run0[0] = h == 0 ? p[0] : rx[0];
  run0[1] = h == 0 ? p[1] : rx[1];
  run0[2] = h == 0 ? rx[0] : p[2];
  run0[3] = h == 0 ? rx[1] : p[3];
  run1[0] = h == 0 ? p[4] : rx[2];
  run1[1] = h == 0 ? p[5] : rx[3];
  run1[2] = h == 0 ? rx[2] : p[6];
  run1[3] = h == 0 ? rx[3] : p[7];
}
#endif  // __HIPCC__

// ``rows`` = rows per workgroup slab, 32 or 64 (validated by the binding).
struct FwdChainArgs {
  const void* x0s;  // bf16 fragment-major x (launch_swizzle_x[_both])
  ChainWeights w;
  void* a1t;        // bf16 wgrad fragment-major a1^T; null (rows = 64,
                    // pi16 = 0 only): layer 1 does not emit it
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
// The forward's layer-1 inputs. With ``rc`` the dW2 workgroups of the
// grouped launch recompute a1 = relu(x W1^T + b1) from them, bit for bit
// what fwd_chain emits as a1^T, and BT2 is not read (may be null). The
// slabs and the partials are the same either way.
struct WgradRecompute {
  const void* xs;   // bf16 fragment-major x (launch_swizzle_x[_both])
  const void* W1s;  // bf16 fragment-major W1 [512,112]
  const float* b1;  // [512]
};
WgradGroupedSlabs wgrad_grouped_nslabs(int64_t mchunks);
WgradGroupedSlabs launch_wgrad_grouped(const void* AT1, const void* BT1,
                                       float* part1, const void* AT2,
                                       const void* BT2, float* part2,
                                       const void* AT3, const void* BT3,
                                       float* part3, int64_t mchunks,
                                       const WgradRecompute* rc,
                                       hipStream_t stream);
// RSDL_WGRAD_GROUPED and the knobs that rule the grouped launch out,
// latched at the first call.
bool wgrad_grouped_default();
// RSDL_WGRAD_RECOMPUTE, latched at the first call.
bool wgrad_recompute_default();
// The recompute body alone: the dW2 partials [ns[1], 256*512] of the
// grouped launch's slabs from dz2^T (AT2) and ``rc``. Returns the slab
// count. Needs mchunks > 0.
int64_t launch_wgrad_recompute(const WgradRecompute& rc, const void* AT2,
                               float* part2, int64_t mchunks,
                               hipStream_t stream);

}  // namespace rsdl
