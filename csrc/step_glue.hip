// Glue kernels of the fused train step for MI355X (gfx950): everything
// that stages data for the chain / wgrad kernels or folds their partials,
// in two launches per step instead of ~20 helper kernels.
//
//   step_prep      fp32 master weights -> the five bf16 fragment-major
//                  buffers the chain kernels read (W1s with K padded
//                  100 -> 112, W2s, W3s, W2^T s, W3^T s) + bf16 w4 + the
//                  fp32 target (from fp64), straight from the parameters:
//                  no bf16 staging copy, no view/permute/contiguous pass.
//   step_finalize  per-slab wgrad partials + the backward chain's db/dW4
//                  partials + the loss partials -> final fp32 gradients
//                  and the scalar loss. Writes every output element
//                  exactly once (no zero-fill, no atomics) and sums in a
//                  fixed order, so equal partials give bit-equal results.
//   step_finalize_update  step_finalize plus the SGD / AdamW update of
//                  every parameter from the gradient just stored: fp32
//                  masters and state in place, and the bf16 images of the
//                  new weights where step_prep would put them, so the next
//                  step needs no step_prep.
//   step_update    the same update from gradients that were folded before.
//   eval_accumulate  the evaluation chain's per-workgroup metric partials
//                  -> a persistent fp64 accumulator (models/fused_eval.py).
//
// Fragment-major layout (see csrc/fwd_chain.hip): a [N,K] matrix becomes
// [N/32][K/16][2][32][8]; element (a,c,h,r,e) is W[a*32+r][c*16+h*8+e].
// One thread of step_prep produces one 16-byte (r, 8 x e) run.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "step_glue.h"

namespace rsdl {

typedef __attribute__((__vector_size__(4 * sizeof(float)))) float sg_f32x4;
typedef __attribute__((__vector_size__(4 * sizeof(uint32_t)))) uint32_t
    sg_u32x4;

// fp32 -> bf16 bits, round-to-nearest-even; the same integer formula as
// c10::detail::round_to_nearest_even (NaN -> 0x7FC0), so the result is
// bit-identical to Tensor.bfloat16().
__device__ __forceinline__ uint32_t sg_f2b(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ sg_u32x4 sg_pack8(const float (&v)[8]) {
  sg_u32x4 o;
  o[0] = sg_f2b(v[0]) | (sg_f2b(v[1]) << 16);
  o[1] = sg_f2b(v[2]) | (sg_f2b(v[3]) << 16);
  o[2] = sg_f2b(v[4]) | (sg_f2b(v[5]) << 16);
  o[3] = sg_f2b(v[6]) | (sg_f2b(v[7]) << 16);
  return o;
}

// out[(a,c,h,r)] <- W[a*32+r][c*16+h*8 .. +8], W fp32 [N, Ksrc] row-major,
// output K padded to Kpad (a 16-multiple); the pad is written as zeros.
// Ksrc must be a 4-multiple so both float4 halves are all-in or all-out.
__device__ __forceinline__ void sg_swizzle(const float* __restrict__ W,
                                           uint16_t* __restrict__ out,
                                           int32_t Ksrc, int32_t Kpad,
                                           int32_t t) {
  const int32_t r = t & 31;
  const int32_t h = (t >> 5) & 1;
  const int32_t kc = Kpad >> 4;
  const int32_t c = (t >> 6) % kc;
  const int32_t a = (t >> 6) / kc;
  const int32_t n = a * 32 + r;
  const int32_t k0 = c * 16 + h * 8;
  const float* src = W + (int64_t)n * Ksrc + k0;
  float v[8];
  #pragma unroll
  for (int q = 0; q < 2; q++) {
    sg_f32x4 l = {0.f, 0.f, 0.f, 0.f};
    if (k0 + q * 4 + 4 <= Ksrc) {
      l = *reinterpret_cast<const sg_f32x4*>(src + q * 4);
    }
    #pragma unroll
    for (int e = 0; e < 4; e++) v[q * 4 + e] = l[e];
  }
  *reinterpret_cast<sg_u32x4*>(out + (int64_t)t * 8) = sg_pack8(v);
}

// Swizzle of W^T from model-layout W [K, N] (the dgrad B operand):
// out[(a,c,h,r)][e] <- W[c*16+h*8+e][a*32+r]. Lanes walk r, so each of
// the 8 gathered loads is a coalesced 128-byte row segment.
__device__ __forceinline__ void sg_swizzle_t(const float* __restrict__ W,
                                             uint16_t* __restrict__ out,
                                             int32_t K, int32_t N,
                                             int32_t t) {
  const int32_t r = t & 31;
  const int32_t h = (t >> 5) & 1;
  const int32_t kc = K >> 4;
  const int32_t c = (t >> 6) % kc;
  const int32_t a = (t >> 6) / kc;
  const float* src = W + (int64_t)(c * 16 + h * 8) * N + a * 32 + r;
  float v[8];
  #pragma unroll
  for (int e = 0; e < 8; e++) v[e] = src[(int64_t)e * N];
  *reinterpret_cast<sg_u32x4*>(out + (int64_t)t * 8) = sg_pack8(v);
}

// Block ranges of step_prep (256 threads, one 16-byte output run each).
constexpr int32_t SG_B_W1 = 512 * 112 / 8 / 256;   // 28
constexpr int32_t SG_B_W2 = 256 * 512 / 8 / 256;   // 64
constexpr int32_t SG_B_W3 = 128 * 256 / 8 / 256;   // 16
constexpr int32_t SG_B_W = SG_B_W1 + 2 * SG_B_W2 + 2 * SG_B_W3 + 1;

__global__ void __launch_bounds__(256) step_prep_kernel(StepPrepArgs p) {
  int32_t b = blockIdx.x + p.b0;
  const int32_t tid = threadIdx.x;
  if (b < SG_B_W1) {
    sg_swizzle(p.W1, p.W1s, 100, 112, b * 256 + tid);
    return;
  }
  b -= SG_B_W1;
  if (b < SG_B_W2) {
    sg_swizzle(p.W2, p.W2s, 512, 512, b * 256 + tid);
    return;
  }
  b -= SG_B_W2;
  if (b < SG_B_W3) {
    sg_swizzle(p.W3, p.W3s, 256, 256, b * 256 + tid);
    return;
  }
  b -= SG_B_W3;
  if (b < SG_B_W2) {  // W2 [256,512] -> swizzle of W2^T [512,256]
    sg_swizzle_t(p.W2, p.W2Ts, 256, 512, b * 256 + tid);
    return;
  }
  b -= SG_B_W2;
  if (b < SG_B_W3) {  // W3 [128,256] -> swizzle of W3^T [256,128]
    sg_swizzle_t(p.W3, p.W3Ts, 128, 256, b * 256 + tid);
    return;
  }
  b -= SG_B_W3;
  if (b == 0) {
    if (tid < 16) {
      float v[8];
      #pragma unroll
      for (int e = 0; e < 8; e++) v[e] = p.w4[tid * 8 + e];
      *reinterpret_cast<sg_u32x4*>(p.w4b + tid * 8) = sg_pack8(v);
    }
    return;
  }
  b -= 1;
  // fp64 target -> fp32, 4 per thread (only launched for an fp64 target).
  const int64_t i0 = ((int64_t)b * 256 + tid) * 4;
  if (i0 + 4 <= p.M) {
    sg_f32x4 o;
    #pragma unroll
    for (int e = 0; e < 4; e++) o[e] = (float)p.tgt64[i0 + e];
    *reinterpret_cast<sg_f32x4*>(p.tgt32 + i0) = o;
  } else {
    for (int64_t i = i0; i < p.M; i++) p.tgt32[i] = (float)p.tgt64[i];
  }
}

void launch_step_prep(const StepPrepArgs& p, hipStream_t stream) {
  const int64_t tb = p.tgt64 != nullptr ? (p.M + 1023) / 1024 : 0;
  const int64_t nb = SG_B_W - p.b0 + tb;
  if (nb <= 0) return;  // weights skipped and no fp64 target: nothing to do
  hipLaunchKernelGGL(step_prep_kernel, dim3((uint32_t)nb), dim3(256), 0,
                     stream, p);
}

int32_t step_prep_target_only() { return SG_B_W; }

// ---------------------------------------------------------------------
// Optimizer update, specified once: (g, p, state..., h) -> (p', state'...)
// in fp32, one rounding per operation, nothing fused. The file is built
// with floating-point contraction on, and in the HIP headers __fmul_rn and
// friends are the plain operators (contractible once inlined) while
// __fsqrt_rn is the native, not correctly rounded, square root. So the
// bodies below switch contraction off for themselves and use the plain
// operators and __builtin_sqrtf, which hipcc rounds correctly for fp32
// (denormals kept). Every statement is one IEEE operation; the numpy
// oracle of tests/_optim_cases.py is the same list.
// ---------------------------------------------------------------------
__device__ __forceinline__ void sg_sgd(float g, float& p, float& b,
                                       const float (&h)[8]) {
  #pragma clang fp contract(off)
  const float lr = h[1], mu = h[2], wd = h[3];
  g = g * h[0];
  if (wd != 0.f) {
    const float wp = wd * p;
    g = g + wp;
  }
  float d = g;
  if (mu != 0.f) {
    const float mb = mu * b;
    b = mb + g;
    if (h[4] != 0.f) {
      const float nb = mu * b;
      d = g + nb;
    } else {
      d = b;
    }
  }
  const float u = lr * d;
  p = p - u;
}

__device__ __forceinline__ void sg_adamw(float g, float& p, float& m,
                                         float& v, const float (&h)[8]) {
  #pragma clang fp contract(off)
  g = g * h[0];
  p = p * h[1];
  const float gm = g - m;
  const float am = h[2] * gm;
  m = m + am;
  const float bv = h[3] * v;
  const float gg = g * g;
  const float ag = h[4] * gg;
  v = bv + ag;
  const float sv = __builtin_sqrtf(v);
  const float dq = sv / h[6];
  const float den = dq + h[7];
  const float r = m / den;
  const float u = h[5] * r;
  p = p - u;
}

// Update element ``i`` of parameter ``w`` (order of StepOptArgs) from its
// gradient; master and state are read and written in place. Returns p'.
template <int KIND>
__device__ __forceinline__ float sg_opt1(const StepOptArgs& o, int w, float g,
                                         int32_t i) {
  float p = o.prm[w][i];
  if (KIND == kOptSgd) {
    const bool mom = o.h[2] != 0.f;
    float b = mom ? o.s1[w][i] : 0.f;
    sg_sgd(g, p, b, o.h);
    if (mom) o.s1[w][i] = b;
  } else {
    float m = o.s1[w][i], v = o.s2[w][i];
    sg_adamw(g, p, m, v, o.h);
    o.s1[w][i] = m;
    o.s2[w][i] = v;
  }
  o.prm[w][i] = p;
  return p;
}

// The same for float4 ``j`` of a 16-byte aligned parameter.
template <int KIND>
__device__ __forceinline__ sg_f32x4 sg_opt4(const StepOptArgs& o, int w,
                                            sg_f32x4 g, int32_t j) {
  sg_f32x4 p = reinterpret_cast<const sg_f32x4*>(o.prm[w])[j];
  if (KIND == kOptSgd) {
    const bool mom = o.h[2] != 0.f;
    sg_f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (mom) b = reinterpret_cast<const sg_f32x4*>(o.s1[w])[j];
    #pragma unroll
    for (int e = 0; e < 4; e++) {
      float pe = p[e], be = b[e];
      sg_sgd(g[e], pe, be, o.h);
      p[e] = pe;
      b[e] = be;
    }
    if (mom) reinterpret_cast<sg_f32x4*>(o.s1[w])[j] = b;
  } else {
    sg_f32x4 m = reinterpret_cast<const sg_f32x4*>(o.s1[w])[j];
    sg_f32x4 v = reinterpret_cast<const sg_f32x4*>(o.s2[w])[j];
    #pragma unroll
    for (int e = 0; e < 4; e++) {
      float pe = p[e], me = m[e], ve = v[e];
      sg_adamw(g[e], pe, me, ve, o.h);
      p[e] = pe;
      m[e] = me;
      v[e] = ve;
    }
    reinterpret_cast<sg_f32x4*>(o.s1[w])[j] = m;
    reinterpret_cast<sg_f32x4*>(o.s2[w])[j] = v;
  }
  reinterpret_cast<sg_f32x4*>(o.prm[w])[j] = p;
  return p;
}

// Update float4 ``j`` = W[n][k..k+3] of weight matrix MAT (0: W1 [512,100],
// 1: W2 [256,512], 2: W3 [128,256]) and store the bf16 image of the new
// values where step_prep would put it: the inverse of sg_swizzle (one
// 8-byte store; k..k+3 stay inside one 8-element run) and, for W2 / W3,
// of sg_swizzle_t (four 2-byte stores 16 bytes apart: the columns k..k+3
// are consecutive r of one 32-column block). W1s columns 100..111 are
// never touched.
template <int KIND, int MAT>
__device__ __forceinline__ void sg_update_w(const StepOptArgs& o, sg_f32x4 g,
                                            int32_t j) {
  constexpr int32_t K = MAT == 0 ? 100 : MAT == 1 ? 512 : 256;
  constexpr int32_t KC = MAT == 0 ? 7 : K / 16;  // 16-wide chunks of Kpad
  constexpr int32_t NC = (MAT == 0 ? 512 : MAT == 1 ? 256 : 128) / 16;
  const sg_f32x4 p = sg_opt4<KIND>(o, MAT, g, j);
  const int32_t n = j / (K / 4);
  const int32_t k = (j % (K / 4)) * 4;
  const uint32_t lo = sg_f2b(p[0]) | (sg_f2b(p[1]) << 16);
  const uint32_t hi = sg_f2b(p[2]) | (sg_f2b(p[3]) << 16);
  const int32_t f =
      ((((n >> 5) * KC + (k >> 4)) * 2 + ((k >> 3) & 1)) * 32 + (n & 31)) * 8 +
      (k & 7);
  *reinterpret_cast<uint2*>(o.stg[MAT] + f) = make_uint2(lo, hi);
  if (MAT != 0) {
    uint16_t* t = o.stg[2 + MAT] +
                  ((((k >> 5) * NC + (n >> 4)) * 2 + ((n >> 3) & 1)) * 32 +
                   (k & 31)) * 8 + (n & 7);
    t[0] = (uint16_t)(lo & 0xffffu);
    t[8] = (uint16_t)(lo >> 16);
    t[16] = (uint16_t)(hi & 0xffffu);
    t[24] = (uint16_t)(hi >> 16);
  }
}

// w4[k] and its bf16 image.
template <int KIND>
__device__ __forceinline__ void sg_update_w4(const StepOptArgs& o, float g,
                                             int32_t k) {
  o.stg[5][k] = (uint16_t)sg_f2b(sg_opt1<KIND>(o, 3, g, k));
}


// ---------------------------------------------------------------------
// step_finalize
//
// Column sums of row-major fp32 partial slabs. A workgroup owns C = 2^LOG_C
// float4 columns and splits the rows S = 256/C ways (thread (s, c) sums
// rows s, s+S, s+2S, ... in groups of SG_U independent loads); the S
// partial sums meet in LDS and thread (0, c) adds them in split order.
// Every step of that order is fixed by (nrows, S) alone. The kernel is
// bound by how many dependent load round trips the longest thread makes
// (db_part has 7813 rows at the flagship batch), hence the wide groups.
// ---------------------------------------------------------------------
constexpr int SG_U = 16;

template <int LOG_C>
__device__ __forceinline__ sg_f32x4 sg_colsum(const float* __restrict__ part,
                                              int64_t stride4, int64_t col4,
                                              int64_t nrows, bool valid,
                                              sg_f32x4* lds, int32_t tid) {
  constexpr int C = 1 << LOG_C;
  constexpr int S = 256 / C;
  const int32_t s = tid >> LOG_C;
  const int32_t c = tid & (C - 1);
  sg_f32x4 acc[4];
  #pragma unroll
  for (int j = 0; j < 4; j++) acc[j] = sg_f32x4{0.f, 0.f, 0.f, 0.f};
  if (valid && s < nrows) {
    const sg_f32x4* base = reinterpret_cast<const sg_f32x4*>(part) + col4;
    int64_t r = s;
    for (; r + (SG_U - 1) * S < nrows; r += SG_U * S) {
      sg_f32x4 l[SG_U];
      #pragma unroll
      for (int j = 0; j < SG_U; j++) l[j] = base[(r + j * S) * stride4];
      #pragma unroll
      for (int j = 0; j < SG_U; j++) acc[j & 3] += l[j];
    }
    if (r < nrows) {
      // Tail as ONE more group, not a chain of dependent single loads:
      // rows past the end re-read the last row and count as zero.
      sg_f32x4 l[SG_U];
      #pragma unroll
      for (int j = 0; j < SG_U; j++) {
        const int64_t rr = r + j * S;
        l[j] = base[(rr < nrows ? rr : nrows - 1) * stride4];
      }
      #pragma unroll
      for (int j = 0; j < SG_U; j++) {
        if (r + j * S < nrows) acc[j & 3] += l[j];
      }
    }
  }
  lds[s * C + c] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  __syncthreads();
  sg_f32x4 tot = {0.f, 0.f, 0.f, 0.f};
  if (s == 0) {
    #pragma unroll 4
    for (int q = 0; q < S; q++) tot += lds[q * C + c];
  }
  return tot;
}

constexpr int32_t SG_DB_LOG_C = 1;      // db_part: 2 float4 cols x 128 splits
constexpr int32_t SG_DW_LOG_C = 6;      // dW slabs: 64 float4 cols x 4 splits
constexpr int32_t SG_DB_COLS4 = 225;    // float4 cols holding db1..db4
constexpr int32_t SG_DB_GROUPS = (SG_DB_COLS4 + 1) / 2;       // 113
constexpr int32_t SG_DW4_PAIRS = 33;    // float4 column pairs holding dW4
// db + dW4 groups, padded to 8 x SG_DBX_PER_XCD block indices
constexpr int32_t SG_DBX_PER_XCD = (SG_DB_GROUPS + SG_DW4_PAIRS + 7) / 8;
constexpr int32_t SG_DBX_BLOCKS = 8 * SG_DBX_PER_XCD;         // 152
constexpr int32_t SG_DW2_BLOCKS = 256 * 512 / 4 / 64;         // 512
constexpr int32_t SG_DW1_BLOCKS = 512 * 25 / 64;              // 200
constexpr int32_t SG_DW3_BLOCKS = 128 * 256 / 4 / 64;         // 128
constexpr int32_t SG_FIN_BLOCKS = SG_DBX_BLOCKS + 1 + SG_DW2_BLOCKS +
                                  SG_DW1_BLOCKS + SG_DW3_BLOCKS;
constexpr int32_t SG_PART_W = 1156;     // db_part row stride (floats)

// The db_part workgroups have the longest chains of dependent loads
// (7813 rows over 128 splits), so they take the lowest block indices and
// start first. Each reads a 32-byte piece of every db_part row; block
// indices round-robin over the 8 XCDs, so the groups are dealt out as
// (xcd, seq): neighbouring column groups, which share cache lines, run
// on one XCD and those lines cross into its L2 once.
__global__ void __launch_bounds__(256) step_finalize_kernel(StepFinArgs p) {
  __shared__ sg_f32x4 lds[256];
  int32_t b = blockIdx.x;
  const int32_t tid = threadIdx.x;

  if (b < SG_DBX_BLOCKS) {
    const int32_t g = (b & 7) * SG_DBX_PER_XCD + (b >> 3);
    if (g < SG_DB_GROUPS) {
      // db1 | db2 | db3 | db4 = db_part columns 0..896. Columns 897.. of
      // the last float4 belong to dW4 and are dropped here.
      const int32_t col4 = g * 2 + (tid & 1);
      const sg_f32x4 t = sg_colsum<SG_DB_LOG_C>(
          p.db_part, SG_PART_W / 4, col4, p.db_rows, col4 < SG_DB_COLS4,
          lds, tid);
      if (tid < 2 && col4 < SG_DB_COLS4) {
        #pragma unroll
        for (int e = 0; e < 4; e++) {
          const int32_t q = col4 * 4 + e;
          if (q < 512) p.db1[q] = t[e];
          else if (q < 768) p.db2[q - 512] = t[e];
          else if (q < 896) p.db3[q - 768] = t[e];
          else if (q == 896) p.db4[0] = t[e];
        }
      }
    } else if (g < SG_DB_GROUPS + SG_DW4_PAIRS) {
      // dW4[k] = colsum(897 + k) + colsum(1025 + k): the two halves are
      // summed apart and added last. Columns 897 and 1025 both sit at
      // element 1 of a float4 (224 and 256), so half 0 lives in float4
      // columns 224 + i and half 1, lane for lane, in 256 + i
      // (i = 0..32). One workgroup per pair: thread = (split, half).
      const int32_t i = g - SG_DB_GROUPS;
      const sg_f32x4 t = sg_colsum<SG_DB_LOG_C>(
          p.db_part, SG_PART_W / 4, 224 + i + 32 * (tid & 1), p.db_rows,
          true, lds, tid);
      // threads 0 and 1 hold the two halves' sums; 0 fetches 1's
      sg_f32x4 u;
      #pragma unroll
      for (int e = 0; e < 4; e++) u[e] = __shfl_down(t[e], 1);
      if (tid == 0) {
        #pragma unroll
        for (int e = 0; e < 4; e++) {
          const int32_t k = (224 + i) * 4 + e - 897;
          if (k >= 0 && k < 128) p.dw4[k] = t[e] + u[e];
        }
      }
    }
    return;
  }
  b -= SG_DBX_BLOCKS;

  if (b == 0) {
    // loss = sum(loss_part) / M; each thread's strided share in groups
    // of independent loads, then a fixed tree over the 256 shares.
    float* l0 = reinterpret_cast<float*>(lds);
    float a = 0.f;
    for (int64_t i0 = tid; i0 < p.loss_n; i0 += SG_U * 256) {
      float l[SG_U];
      #pragma unroll
      for (int j = 0; j < SG_U; j++) {
        const int64_t i = i0 + j * 256;
        l[j] = p.loss_part[i < p.loss_n ? i : p.loss_n - 1];
      }
      #pragma unroll
      for (int j = 0; j < SG_U; j++) {
        if (i0 + j * 256 < p.loss_n) a += l[j];
      }
    }
    l0[tid] = a;
    __syncthreads();
    for (int32_t d = 128; d > 0; d >>= 1) {
      if (tid < d) l0[tid] += l0[tid + d];
      __syncthreads();
    }
    if (tid == 0) p.loss[0] = l0[0] / (float)p.M;
    return;
  }
  b -= 1;

  const int32_t c = tid & 63;
  if (b < SG_DW2_BLOCKS) {
    const int32_t col4 = b * 64 + c;
    const sg_f32x4 t = sg_colsum<SG_DW_LOG_C>(p.part2, 256 * 512 / 4, col4,
                                              p.ns2, true, lds, tid);
    if (tid < 64) reinterpret_cast<sg_f32x4*>(p.dw2)[col4] = t;
    return;
  }
  b -= SG_DW2_BLOCKS;
  if (b < SG_DW1_BLOCKS) {
    // dW1 [512,100] out of [512,128]-wide partial rows: output float4 j
    // is (n, k4) = (j / 25, j % 25); pad columns 100..127 (k4 25..31)
    // are never loaded.
    const int32_t j = b * 64 + c;
    const int32_t col4 = (j / 25) * 32 + (j % 25);
    const sg_f32x4 t = sg_colsum<SG_DW_LOG_C>(p.part1, 512 * 128 / 4, col4,
                                              p.ns1, true, lds, tid);
    if (tid < 64) reinterpret_cast<sg_f32x4*>(p.dw1)[j] = t;
    return;
  }
  b -= SG_DW1_BLOCKS;
  {
    const int32_t col4 = b * 64 + c;
    const sg_f32x4 t = sg_colsum<SG_DW_LOG_C>(p.part3, 128 * 256 / 4, col4,
                                              p.ns3, true, lds, tid);
    if (tid < 64) reinterpret_cast<sg_f32x4*>(p.dw3)[col4] = t;
  }
}

// step_finalize_kernel with the update epilogue, for OPT = kOptSgd /
// kOptAdamW: wherever step_finalize_kernel stores a gradient, this stores
// the same gradient and the storing thread then updates the parameter
// element(s) it belongs to (sg_update_w, sg_update_w4, sg_opt1). The
// column sums, the block map and the summation order are those of
// step_finalize_kernel line for line and must stay so: the gradients of
// the two are bit-equal (tests/test_fused_optim_gpu.py). It is a kernel
// of its own, not a third instantiation, so that the code generated for
// step_finalize_kernel does not move.
template <int OPT>
__global__ void __launch_bounds__(256) step_finalize_update_kernel(
    StepFinArgs p, StepOptArgs o) {
  __shared__ sg_f32x4 lds[256];
  int32_t b = blockIdx.x;
  const int32_t tid = threadIdx.x;

  if (b < SG_DBX_BLOCKS) {
    const int32_t g = (b & 7) * SG_DBX_PER_XCD + (b >> 3);
    if (g < SG_DB_GROUPS) {
      // db1 | db2 | db3 | db4 = db_part columns 0..896. Columns 897.. of
      // the last float4 belong to dW4 and are dropped here.
      const int32_t col4 = g * 2 + (tid & 1);
      const sg_f32x4 t = sg_colsum<SG_DB_LOG_C>(
          p.db_part, SG_PART_W / 4, col4, p.db_rows, col4 < SG_DB_COLS4,
          lds, tid);
      if (tid < 2 && col4 < SG_DB_COLS4) {
        #pragma unroll
        for (int e = 0; e < 4; e++) {
          const int32_t q = col4 * 4 + e;
          if (q < 512) {
            p.db1[q] = t[e];
            sg_opt1<OPT>(o, 4, t[e], q);
          } else if (q < 768) {
            p.db2[q - 512] = t[e];
            sg_opt1<OPT>(o, 5, t[e], q - 512);
          } else if (q < 896) {
            p.db3[q - 768] = t[e];
            sg_opt1<OPT>(o, 6, t[e], q - 768);
          } else if (q == 896) {
            p.db4[0] = t[e];
            sg_opt1<OPT>(o, 7, t[e], 0);
          }
        }
      }
    } else if (g < SG_DB_GROUPS + SG_DW4_PAIRS) {
      // dW4[k] = colsum(897 + k) + colsum(1025 + k): the two halves are
      // summed apart and added last. Columns 897 and 1025 both sit at
      // element 1 of a float4 (224 and 256), so half 0 lives in float4
      // columns 224 + i and half 1, lane for lane, in 256 + i
      // (i = 0..32). One workgroup per pair: thread = (split, half).
      const int32_t i = g - SG_DB_GROUPS;
      const sg_f32x4 t = sg_colsum<SG_DB_LOG_C>(
          p.db_part, SG_PART_W / 4, 224 + i + 32 * (tid & 1), p.db_rows,
          true, lds, tid);
      // threads 0 and 1 hold the two halves' sums; 0 fetches 1's
      sg_f32x4 u;
      #pragma unroll
      for (int e = 0; e < 4; e++) u[e] = __shfl_down(t[e], 1);
      if (tid == 0) {
        #pragma unroll
        for (int e = 0; e < 4; e++) {
          const int32_t k = (224 + i) * 4 + e - 897;
          if (k >= 0 && k < 128) {
            const float g = t[e] + u[e];
            p.dw4[k] = g;
            sg_update_w4<OPT>(o, g, k);
          }
        }
      }
    }
    return;
  }
  b -= SG_DBX_BLOCKS;

  if (b == 0) {
    // loss = sum(loss_part) / M; each thread's strided share in groups
    // of independent loads, then a fixed tree over the 256 shares.
    float* l0 = reinterpret_cast<float*>(lds);
    float a = 0.f;
    for (int64_t i0 = tid; i0 < p.loss_n; i0 += SG_U * 256) {
      float l[SG_U];
      #pragma unroll
      for (int j = 0; j < SG_U; j++) {
        const int64_t i = i0 + j * 256;
        l[j] = p.loss_part[i < p.loss_n ? i : p.loss_n - 1];
      }
      #pragma unroll
      for (int j = 0; j < SG_U; j++) {
        if (i0 + j * 256 < p.loss_n) a += l[j];
      }
    }
    l0[tid] = a;
    __syncthreads();
    for (int32_t d = 128; d > 0; d >>= 1) {
      if (tid < d) l0[tid] += l0[tid + d];
      __syncthreads();
    }
    if (tid == 0) p.loss[0] = l0[0] / (float)p.M;
    return;
  }
  b -= 1;

  const int32_t c = tid & 63;
  if (b < SG_DW2_BLOCKS) {
    const int32_t col4 = b * 64 + c;
    const sg_f32x4 t = sg_colsum<SG_DW_LOG_C>(p.part2, 256 * 512 / 4, col4,
                                              p.ns2, true, lds, tid);
    if (tid < 64) {
      reinterpret_cast<sg_f32x4*>(p.dw2)[col4] = t;
      sg_update_w<OPT, 1>(o, t, col4);
    }
    return;
  }
  b -= SG_DW2_BLOCKS;
  if (b < SG_DW1_BLOCKS) {
    // dW1 [512,100] out of [512,128]-wide partial rows: output float4 j
    // is (n, k4) = (j / 25, j % 25); pad columns 100..127 (k4 25..31)
    // are never loaded.
    const int32_t j = b * 64 + c;
    const int32_t col4 = (j / 25) * 32 + (j % 25);
    const sg_f32x4 t = sg_colsum<SG_DW_LOG_C>(p.part1, 512 * 128 / 4, col4,
                                              p.ns1, true, lds, tid);
    if (tid < 64) {
      reinterpret_cast<sg_f32x4*>(p.dw1)[j] = t;
      sg_update_w<OPT, 0>(o, t, j);
    }
    return;
  }
  b -= SG_DW1_BLOCKS;
  {
    const int32_t col4 = b * 64 + c;
    const sg_f32x4 t = sg_colsum<SG_DW_LOG_C>(p.part3, 128 * 256 / 4, col4,
                                              p.ns3, true, lds, tid);
    if (tid < 64) {
      reinterpret_cast<sg_f32x4*>(p.dw3)[col4] = t;
      sg_update_w<OPT, 2>(o, t, col4);
    }
  }
}

void launch_step_finalize(const StepFinArgs& p, hipStream_t stream) {
  hipLaunchKernelGGL(step_finalize_kernel, dim3(SG_FIN_BLOCKS), dim3(256), 0,
                     stream, p);
}

void launch_step_finalize_update(const StepFinArgs& p, const StepOptArgs& o,
                                 int kind, hipStream_t stream) {
  auto kern = kind == kOptAdamW ? step_finalize_update_kernel<kOptAdamW>
                                : step_finalize_update_kernel<kOptSgd>;
  hipLaunchKernelGGL(kern, dim3(SG_FIN_BLOCKS), dim3(256), 0, stream, p, o);
}

// ---------------------------------------------------------------------
// step_update
//
// The update of sg_sgd / sg_adamw element-wise from the eight folded
// gradients in ``o.grad``, with the same outputs as the epilogue of
// step_finalize_update (masters, state, the six staged bf16 buffers): for
// steps whose gradients pass through something else first (an all-reduce,
// a grad_hook) or come from elsewhere. 256 threads, one float4 of a
// weight matrix each; the last blocks walk w4 and the biases one element
// per thread (their gradients need not be 16-byte aligned).
// ---------------------------------------------------------------------
constexpr int32_t SG_U_W1 = 512 * 100 / 4 / 256;   // 50
constexpr int32_t SG_U_W2 = 256 * 512 / 4 / 256;   // 128
constexpr int32_t SG_U_W3 = 128 * 256 / 4 / 256;   // 32
constexpr int32_t SG_U_SMALL = 128 + 512 + 256 + 128 + 1;     // w4, b1..b4
constexpr int32_t SG_U_BLOCKS =
    SG_U_W1 + SG_U_W2 + SG_U_W3 + (SG_U_SMALL + 255) / 256;

template <int KIND>
__global__ void __launch_bounds__(256) step_update_kernel(StepOptArgs o) {
  int32_t b = blockIdx.x;
  const int32_t j = b * 256 + threadIdx.x;
  if (b < SG_U_W1) {
    sg_update_w<KIND, 0>(
        o, reinterpret_cast<const sg_f32x4*>(o.grad[0])[j], j);
    return;
  }
  b -= SG_U_W1;
  if (b < SG_U_W2) {
    const int32_t j2 = j - SG_U_W1 * 256;
    sg_update_w<KIND, 1>(
        o, reinterpret_cast<const sg_f32x4*>(o.grad[1])[j2], j2);
    return;
  }
  b -= SG_U_W2;
  if (b < SG_U_W3) {
    const int32_t j3 = j - (SG_U_W1 + SG_U_W2) * 256;
    sg_update_w<KIND, 2>(
        o, reinterpret_cast<const sg_f32x4*>(o.grad[2])[j3], j3);
    return;
  }
  const int32_t q = j - (SG_U_W1 + SG_U_W2 + SG_U_W3) * 256;
  if (q < 128) sg_update_w4<KIND>(o, o.grad[3][q], q);
  else if (q < 640) sg_opt1<KIND>(o, 4, o.grad[4][q - 128], q - 128);
  else if (q < 896) sg_opt1<KIND>(o, 5, o.grad[5][q - 640], q - 640);
  else if (q < 1024) sg_opt1<KIND>(o, 6, o.grad[6][q - 896], q - 896);
  else if (q == 1024) sg_opt1<KIND>(o, 7, o.grad[7][0], 0);
}

void launch_step_update(const StepOptArgs& o, int kind, hipStream_t stream) {
  auto kern = kind == kOptAdamW ? step_update_kernel<kOptAdamW>
                                : step_update_kernel<kOptSgd>;
  hipLaunchKernelGGL(kern, dim3(SG_U_BLOCKS), dim3(256), 0, stream, o);
}

// ---------------------------------------------------------------------
// eval_accumulate
//
// Folds the evaluation chain's per-workgroup partials part[nrows][4] =
// {sum (o-t)^2, sum |o-t|, sum t, sum t^2} (fp32, csrc/fwd_chain.hip) into
// the persistent fp64 accumulator acc[5] = {rows, sse, sae, sum_t, sum_tt},
// in place. One workgroup: thread i sums partial rows i, i + 256, ... in
// fp64, the 256 shares meet in a fixed LDS tree, and thread 0 adds the
// totals and M into acc. No atomics, no zero fill, no host read: the same
// partials in the same order give the same bits, and the launch can be
// captured in a graph.
//
// NC = 5: the weighted chain's partials, rows of eight floats {c0..c3,
// sum w, 0, 0, 0}, fold into acc[6] = {rows, c0..c3, sum w} the same way
// (the second float4 of a row carries column 4). NC = 4 is the layout and
// the summation order above, unchanged.
// ---------------------------------------------------------------------
template <int NC>
__global__ void __launch_bounds__(256) eval_accumulate_kernel(
    const float* __restrict__ part, int64_t nrows, int64_t M,
    double* __restrict__ acc) {
  static_assert(NC == 4 || NC == 5, "4 or 5 partial columns");
  constexpr int V = NC == 4 ? 1 : 2;  // float4 per partial row
  __shared__ double lds[NC][256];
  const int32_t tid = threadIdx.x;
  double a[NC];
  #pragma unroll
  for (int e = 0; e < NC; e++) a[e] = 0.0;
  // unrolled so several loads are in flight; the add order is unchanged
  #pragma unroll 4
  for (int64_t r = tid; r < nrows; r += 256) {
    const sg_f32x4 v = reinterpret_cast<const sg_f32x4*>(part)[r * V];
    #pragma unroll
    for (int e = 0; e < 4; e++) a[e] += (double)v[e];
    if (NC == 5) a[NC - 1] += (double)part[r * 8 + 4];
  }
  #pragma unroll
  for (int e = 0; e < NC; e++) lds[e][tid] = a[e];
  __syncthreads();
  for (int32_t d = 128; d > 0; d >>= 1) {
    if (tid < d) {
      #pragma unroll
      for (int e = 0; e < NC; e++) lds[e][tid] += lds[e][tid + d];
    }
    __syncthreads();
  }
  if (tid == 0) {
    acc[0] += (double)M;
    #pragma unroll
    for (int e = 0; e < NC; e++) acc[1 + e] += lds[e][0];
  }
}

// ``ncol`` = 4 (part [nrows, 4], acc [5]) or 5 (part [nrows, 8], acc [6]).
void launch_eval_accumulate(const float* part, int64_t nrows, int64_t M,
                            double* acc, int ncol, hipStream_t stream) {
  auto kern = ncol == 5 ? eval_accumulate_kernel<5>
                        : eval_accumulate_kernel<4>;
  hipLaunchKernelGGL(kern, dim3(1), dim3(256), 0, stream, part, nrows, M,
                     acc);
}

}  // namespace rsdl
