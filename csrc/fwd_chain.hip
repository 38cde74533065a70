// Fused forward chain for the flagship TabularMLP on MI355X (gfx950) —
// the DEFAULT bench train-step forward (models/fused_step.py;
// RSDL_FUSED_STEP=0 reverts to eager).
//
//   a1 = relu(x0 @ W1^T + b1)   [M,100] -> [M,512]
//   a2 = relu(a1 @ W2^T + b2)   -> [M,256]
//   a3 = relu(a2 @ W3^T + b3)   -> [M,128]
//   out = a3 @ w4^T + b4        -> [M,1]
//
// One workgroup carries a slab of rows through the whole chain: the
// slab's activations live in LDS between layers, weights are read from
// global (L2-resident, ~0.44 MB total) per MFMA step, and only x0 (read)
// and the a1/a2/a3/out tiles (written once for backward) touch HBM.
// Eliminates the inter-layer activation re-reads of the eager path
// (~448 MB/step at the bench shape; measured eager fwd 0.25 ms vs a
// ~0.1 ms fused roofline).
//
// Slab size (template MT = 32-row m-tiles per workgroup, `rows` = 32 or
// 64 per call, default 64; profiles/PERF.md "Round 4"). Every workgroup
// pulls the whole weight set through the vector-memory path: 442 KB (W1
// with K padded to 112, W2, W3), once per slab. At M = 250k with 32-row
// slabs that is 7813 x 442 KB = 3.45 GB per launch (measured: 3.50 GB
// of L1->L2 read requests, x included) — ~100 us at the chip's ~34.5
// TB/s aggregate L2 rate, on the path the activation streams use too,
// and the reason the 32-row kernel sat at 232 us with HBM (~115 us) and
// MFMA/VALU issue (45-90 us) both far from their limits. A 64-row
// workgroup (8 waves) gives every wave N/8 columns of BOTH m-tiles in
// layers 1 and 2, so each B fragment, once in registers, feeds two
// MFMAs: 1.85 GB measured, 191 us. Layer 3 has only four n-tiles and
// stays unshared (wave w: m-tile w >> 2, n-tile w & 3; 15 % of the
// weight bytes). Results are bit-identical between the slab sizes except
// for the grouping of loss_part (one entry per workgroup).
// Occupancy decides whether this pays: 64 rows with t1 + t2 side by side
// (100 KB, or round 2's 133 KB with an x tile) means one workgroup per
// CU, every barrier spanning the CU — round 2 measured that at 512 us.
// Here t2 and t3 alias t1 (66.8 KB) and the kernel is held to 128
// registers, so two 8-wave workgroups share a CU (4 waves/SIMD, against
// 3 for the 32-row kernel at 50 KB and 140 registers).
//
// MFMA orientation (v_mfma_f32_32x32x16_bf16, probe-verified maps in
// tools/mfma_probe.hip / csrc/wgrad_kernel.hip):
//   D[mrow][ncol] = A[mrow][k] x B[k][ncol], per lane:
//     A[m = lane&31][k = (lane>>5)*8 + j]   j = 0..7 of a bf16x8
//     B[k = (lane>>5)*8 + j][n = lane&31]
//     D col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
// For y[m,n] = sum_k x[m,k] W[n,k] the A fragment is a contiguous row
// segment of the LDS tile. The B (weight) fragment is served from a
// FRAGMENT-MAJOR swizzled weight layout
//   SW[n_tile][k_chunk][h][ml][8]  (n_tile = n/32, k_chunk = k/16,
//   h = lane>>5, ml = lane&31)
// so one wave's 64 16-B fragment loads are a single contiguous 1 KB
// block. In the natural [N][K] layout each B load touched 32 cache
// lines 1 KB apart (rows), which bound the kernel on L1/TCP line
// processing (~16 GB of line traffic per launch) — the swizzle makes
// weight traffic coalesced and line-minimal. The host binding performs
// the swizzle per call (weights are 0.44 MB total; a few us).
//
// Validated by tests/test_gpu_kernels.py (chain numerics, layout
// oracles, whole-step parity), tests/test_chain_rows64_gpu.py (64-row
// slabs bit-equal to 32-row ones, odd tile counts, regrouped partials)
// and tests/test_chain_sim.py (lane-level index simulation); the
// forward-only eval_chain_kernel by tests/test_fused_eval_gpu.py; the BCE
// head, the binary task and the AUC histogram by
// tests/test_fused_bce_gpu.py; the weighted heads (sample weights,
// pos_weight, fixed-point histogram) by tests/test_fused_weights_gpu.py.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdint>

#include "chain.h"

namespace rsdl {

// A/B'd: nontemporal streaming accesses measure ~4% faster than
// cacheable (0.885 vs 0.919 ms fused step) — the activation streams
// evicting L2 hurts more than write-combining helps, even with the
// weight set fragment-swizzled. Keep nontemporal.
#ifndef RSDL_PLAIN_STREAMS
#define RSDL_PLAIN_STREAMS 0
#endif
template <typename T>
__device__ __forceinline__ void _rsdl_store(T v, T* p) {
#if RSDL_PLAIN_STREAMS
  *p = v;
#else
  __builtin_nontemporal_store(v, p);
#endif
}
template <typename T>
__device__ __forceinline__ T _rsdl_load(const T* p) {
#if RSDL_PLAIN_STREAMS
  return *p;
#else
  return __builtin_nontemporal_load(p);
#endif
}


typedef __attribute__((__vector_size__(8 * sizeof(short)))) short fc_bf16x8;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float fc_f32x16;
typedef __attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int fc_u32x4;
typedef __attribute__((__vector_size__(2 * sizeof(unsigned int)))) unsigned int fc_u32x2;
typedef __attribute__((__vector_size__(2 * sizeof(float)))) float fc_f32x2;

// Packed pair helpers (one VALU op per TWO elements on gfx950).
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

#define FC_MT 32            // rows per MFMA m-tile (and per x/mask block)
#define FC_K0 100           // input feature count
#define FC_K0P 112          // padded to a 16-multiple for the k-loop
#define FC_N1 512
#define FC_N2 256
#define FC_N3 128
// LDS halfword strides (16-B aligned: multiples of 8; +8 pad de-banks the
// column writes of the D->tile stores).
#define FC_S0 (FC_K0P + 8)
#define FC_S1 (FC_N1 + 8)
#define FC_S2 (FC_N2 + 8)
#define FC_S3 (FC_N3 + 8)

__device__ __forceinline__ float fc_b2f(short s) {
  __hip_bfloat16 h;
  *reinterpret_cast<short*>(&h) = s;
  return __bfloat162float(h);
}

__device__ __forceinline__ short fc_f2b(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  return *reinterpret_cast<short*>(&h);
}

// One GEMM layer of the chain for one wave: src tile [MT*32][K] (LDS,
// stride SRC_S halfwords) x W[N][K] global -> relu(.+bias) -> dst LDS
// tile (stride DST_S). The wave owns MPW consecutive m-tiles starting at
// mt0 and NT consecutive n-tiles starting at ntile0; each B (weight)
// fragment is loaded ONCE and issued against all MPW m-tiles' A
// fragments, so a 64-row workgroup (MPW = 2) pulls every weight byte
// through the vector-memory path once per 64 rows instead of once per
// 32. Each (m-tile, n-tile) accumulator sees the same MFMAs in the same
// k order whatever MPW is, so the results are bit-identical between the
// slab sizes.
// A_FRAGMAJOR: src is a GLOBAL fragment-major m-tile block (layout as
// the swizzled weights: [kc][h][ml][8], 512 halfwords per k-chunk) —
// used for layer 1, whose input x is pre-swizzled host-side; SRC_S is
// ignored. Otherwise src is the LDS tile of the previous layer.
// EMIT_T: besides the LDS tile, the epilogue emits each m-tile's
// activations TRANSPOSED in wgrad fragment-major layout
// ([N/32][mchunks][2][32][8]; see csrc/wgrad_frag.hip) plus one 32-bit
// relu-mask word per column (maskT[m_tile][n], bit i = row i alive) —
// the backward chain then never reads the activations at all (masks
// only) and the wgrad kernel gets coalesced B fragments for free.
// Lanes l/l+32 hold complementary 4-row runs of a column; one shfl_xor
// per 4 values assembles the 8-row fragment runs in registers.
// has2 (workgroup-uniform, MPW = 2 only): the slab's second m-tile
// exists. When it does not (odd tile count, last workgroup) its x block,
// mask rows and fragment chunks lie past the allocations: the A loads
// then re-read tile 0 and the global emissions are skipped, under this
// one uniform flag — no per-element guards in the loops.
// SYNC_EPI: a workgroup barrier between the k-loop and the epilogue, for
// a dst tile that aliases the src tile.
// __forceinline__: the chain kernels are instantiated once per loss /
// task, so each emitting layer has more than one caller; left to its cost
// model the compiler then keeps the layers out-of-line, and the 64-row
// training kernel spills (200 B of scratch) at its 128-register cap.
// Inlined, every instantiation has the single-caller figures.
template <int K, int N, int MPW, int NT, int SRC_S, int DST_S, bool RELU,
          bool A_FRAGMAJOR = false, bool EMIT_T = false, bool PI16 = false,
          bool SYNC_EPI = false>
__device__ __forceinline__ void fc_layer(
    const short* __restrict__ src_lds, const short* __restrict__ W,
    const float* __restrict__ bias, short* __restrict__ dst_lds,
    int32_t mt0, int32_t ntile0, int32_t lane, bool has2,
    short* __restrict__ at_out = nullptr,
    uint32_t* __restrict__ mask_row = nullptr, int64_t mchunks = 0,
    int64_t mc0 = 0) {
  constexpr int ITERS = K / 16;
  const int32_t n_base = ntile0 * 32;
  const int32_t frag_k0 = (lane >> 5) * 8;
  const int32_t ml = lane & 31;  // A row within m-tile / D col (n)

  // Software-pipelined k-loop: LDS occupancy holds this kernel to 3-4
  // waves/SIMD, so cross-wave latency hiding is thin — the next
  // iteration's A (LDS) and B (global/L2) fragments must be IN FLIGHT
  // while the current MFMAs run. Fully unrolled (compile-time ITERS)
  // double-buffered prefetch: buf indices become constants after unroll,
  // so the fragment arrays stay in registers.
  const short* srcA[MPW];
  #pragma unroll
  for (int mt = 0; mt < MPW; mt++) {
    const int32_t tile = mt0 + ((mt == 0 || has2) ? mt : 0);
    srcA[mt] = A_FRAGMAJOR
                   ? &src_lds[(int64_t)tile * ITERS * 512 + lane * 8]
                   : &src_lds[((mt0 + mt) * 32 + ml) * SRC_S + frag_k0];
  }
  // Swizzled weight base for this wave's n-tiles: block (ntile, kc) is
  // 512 contiguous halfwords; lane's 16-B slice at lane*8.
  const short* srcB[NT];
  #pragma unroll
  for (int nt = 0; nt < NT; nt++) {
    srcB[nt] = &W[((int64_t)(ntile0 + nt) * ITERS) * 512 + lane * 8];
  }

  fc_f32x16 acc[MPW][NT] = {};
  fc_bf16x8 a[2][MPW], b[2][NT];

  #pragma unroll
  for (int mt = 0; mt < MPW; mt++) {
    *reinterpret_cast<uint4*>(&a[0][mt]) =
        *reinterpret_cast<const uint4*>(srcA[mt]);
  }
  #pragma unroll
  for (int nt = 0; nt < NT; nt++) {
    *reinterpret_cast<uint4*>(&b[0][nt]) =
        *reinterpret_cast<const uint4*>(srcB[nt]);
  }
  #pragma unroll
  for (int i = 0; i < ITERS; i++) {
    const int cur = i & 1;
    const int nxt = cur ^ 1;
    if (i + 1 < ITERS) {
      const int32_t k = (i + 1) * 16;
      #pragma unroll
      for (int mt = 0; mt < MPW; mt++) {
        *reinterpret_cast<uint4*>(&a[nxt][mt]) =
            *reinterpret_cast<const uint4*>(
                &srcA[mt][A_FRAGMAJOR ? (i + 1) * 512 : k]);
      }
      #pragma unroll
      for (int nt = 0; nt < NT; nt++) {
        *reinterpret_cast<uint4*>(&b[nxt][nt]) =
            *reinterpret_cast<const uint4*>(&srcB[nt][(i + 1) * 512]);
      }
    }
    #pragma unroll
    for (int mt = 0; mt < MPW; mt++) {
      #pragma unroll
      for (int nt = 0; nt < NT; nt++) {
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            a[cur][mt], b[cur][nt], acc[mt][nt], 0, 0, 0);
      }
    }
  }
  // Epilogue: bias + (relu) + cast + store the D fragments into the dst
  // tile at [mrow][n] (b16 column writes; DST_S padding spreads banks);
  // with EMIT_T also emit the transposed fragment runs + mask word.
  // All arithmetic runs on packed row pairs (v_pk_add/max_f32 +
  // v_cvt_pk_bf16_f32): regs 2q/2q+1 are consecutive rows, and the
  // packed bf16 word IS the emission payload.
  if (SYNC_EPI) __syncthreads();
  const int32_t h = lane >> 5;
  #pragma unroll
  for (int mt = 0; mt < MPW; mt++) {
    #pragma unroll
    for (int nt = 0; nt < NT; nt++) {
      const int32_t n = n_base + nt * 32 + ml;
      const fc_f32x2 bv2 = {bias[n], bias[n]};
      // One base address per column; row offsets are compile-time, so
      // the b16 stores use ds_write immediate offsets instead of ~1.5
      // VALU address ops each.
      short* colbase = dst_lds + ((mt0 + mt) * 32 + 4 * h) * DST_S + n;
      uint32_t p[8];
      #pragma unroll
      for (int q = 0; q < 8; q++) {
        const int32_t roff = (((2 * q) & 3) + 8 * (q >> 1)) * DST_S;
        fc_f32x2 v2 = {acc[mt][nt][2 * q], acc[mt][nt][2 * q + 1]};
        v2 += bv2;
        if (RELU) v2 = fc_pk_max0(v2);
        const uint32_t pk = fc_cvt_pk_bf16(v2);
        p[q] = pk;
        colbase[roff] = (short)(pk & 0xFFFFu);
        colbase[roff + DST_S] = (short)(pk >> 16);
      }
      if (EMIT_T && (mt == 0 || has2)) {
        // Mask word for column n (bit i = bf16 value of row i > 0): a
        // positive nonzero bf16 is 0 < bits < 0x8000.
        uint32_t w = 0;
        #pragma unroll
        for (int q = 0; q < 8; q++) {
          const int32_t mrow = ((2 * q) & 3) + 8 * (q >> 1) + 4 * h;
          const uint32_t lo = p[q] & 0xFFFFu;
          const uint32_t hi = p[q] >> 16;
          w |= (uint32_t)(lo - 1u < 0x7FFFu) << mrow;
          w |= (uint32_t)(hi - 1u < 0x7FFFu) << (mrow + 1);
        }
        // PI16: every producer/consumer of the transposed layout agrees
        // on the pi16 intra-chunk M-permutation (swap bits 2<->3 of the
        // 16-row position), under which each half-wave's own packed
        // pairs ARE the 8-element runs — the 4-shfl half-row exchange
        // and its slot selects disappear. M is the contraction dim of
        // every consumer (wgrad_frag), so dW is invariant.
        // Default (!PI16): exchange the half-rows as packed ints (4
        // shfls); lane h=0 assembles rows {0-7},{16-23}, h=1
        // {8-15},{24-31}.
        fc_u32x4 run0, run1;
        if (PI16) {
          #pragma unroll
          for (int j = 0; j < 4; j++) {
            run0[j] = p[j];
            run1[j] = p[4 + j];
          }
        } else {
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
        const int64_t nt_g = (int64_t)(n_base + nt * 32) >> 5;
        const int64_t mc = mc0 + 2 * (mt0 + mt);
        short* blk0 = at_out + ((nt_g * mchunks + mc) * 512) + h * 256 +
                      ml * 8;
        short* blk1 = at_out + ((nt_g * mchunks + mc + 1) * 512) +
                      h * 256 + ml * 8;
        _rsdl_store(run0,
                                    reinterpret_cast<fc_u32x4*>(blk0));
        _rsdl_store(run1,
                                    reinterpret_cast<fc_u32x4*>(blk1));
        w |= __shfl_xor(w, 32);
        if (h == 0) mask_row[(mt0 + mt) * N + n] = w;
      }
    }
  }
}

// Copy an LDS activation tile [MT*32][N] (stride S halfwords) to the
// global row-major [M, N] tensor, vectorized 16 B.
template <int MT, int N, int S>
__device__ void fc_store_tile(const short* __restrict__ lds, short* out,
                              int64_t m0, int64_t M, int32_t tid) {
  constexpr int VPR = N / 8;  // uint4 vectors per row
  for (int32_t u = tid; u < MT * FC_MT * VPR; u += 256 * MT) {
    const int32_t m = u / VPR;
    const int32_t c = (u % VPR) * 8;
    if (m0 + m < M) {
      // Non-temporal: activations are written once and re-read only by the
      // backward kernel much later — keeping them OUT of L2 preserves the
      // weight working set (which every workgroup re-reads).
      _rsdl_store(
          *reinterpret_cast<const fc_u32x4*>(&lds[m * S + c]),
          reinterpret_cast<fc_u32x4*>(&out[(m0 + m) * N + c]));
    }
  }
}

// Logistic head shared by the BCE instantiations of both chain kernels:
// for the fp32 logit o, e = exp(-|o|) never overflows, the sigmoid is
// 1/(1+e) or e/(1+e) by the sign of o, and the per-row loss is the
// softplus form max(o,0) - o*t + log1p(e), finite at any finite o (the
// naive log(1+exp(o)) is inf from o ~ 89). expf/log1pf, not the fast
// intrinsics: the test tolerances are derived from them.
__device__ __forceinline__ void fc_bce_terms(float o, float t, float& sg,
                                             float& l) {
  const float e = expf(-fabsf(o));
  sg = o >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
  l = fmaxf(o, 0.f) - o * t + log1pf(e);
}

// The pos_weight form of the logistic head (p != 1), torch's definition:
// l = p t softplus(-o) + (1-t) softplus(o), softplus(+-o) = max(+-o, 0) +
// log1p(e) with the same overflow-free e, and g = dl/do = (1-t) sg -
// p t (1-sg). 1-sg is formed as sigmoid(-o) from the same e (the other of
// the two quotients), not by subtraction: sg rounds to 1 from o ~ 17, and
// the positive rows' gradient must not vanish with it.
__device__ __forceinline__ void fc_bce_pw_terms(float o, float t, float p,
                                                float& sg, float& l,
                                                float& g) {
  const float e = expf(-fabsf(o));
  const float big = 1.f / (1.f + e), small = e / (1.f + e);
  sg = o >= 0.f ? big : small;
  const float cs = o >= 0.f ? small : big;  // 1 - sg
  const float lp = log1pf(e);
  const float pt = p * t;
  l = pt * (fmaxf(-o, 0.f) + lp) + (1.f - t) * (fmaxf(o, 0.f) + lp);
  g = (1.f - t) * sg - pt * cs;
}

// Loss selector of fwd_chain_kernel / task selector of eval_chain_kernel
// (exported by the binding as LOSS_MSE / LOSS_BCE).
#define FC_LOSS_MSE 0
#define FC_LOSS_BCE 1

// The 64-row kernels run at exactly 128 registers. Handing each layer an
// opaque copy of the lane index keeps the compiler from carrying lane-
// derived address terms across a whole layer (it spilled one to scratch
// rather than recompute a shift); no-op at MT = 1.
template <int MT>
__device__ __forceinline__ int32_t fc_fresh_lane(int32_t lane) {
  if (MT == 2) asm volatile("" : "+v"(lane));
  return lane;
}

// MT = 32-row m-tiles per workgroup slab (1 or 2); 256 * MT threads. See
// the header for the slab-size reasoning. The second __launch_bounds__
// figure is waves per SIMD: the 64-row kernel must fit 128 registers so
// that two 8-wave workgroups share a CU.
// LOSS picks the head epilogue only (FC_LOSS_MSE: dyb = 2/M (o-t), terms
// (o-t)^2; FC_LOSS_BCE: dyb = 1/M (sigmoid(o)-t), terms from
// fc_bce_terms); the layers, the LDS plan and the barriers do not see it.
// WEIGHTED (fwd_chain_kernel<.., true>; the false instantiations read
// neither argument and compile to what they did before the flag existed): the
// head also takes ``weight`` (fp32 [M], read under the m0 + m < M guard
// only; null = every w is 1) and ``pos_weight`` p, normalisation still by
// M. MSE: dyb = bf16((2/M w)(o-t)), terms w (o-t)^2. BCE, p == 1: dyb =
// bf16((w/M)(sg-t)), terms w l. BCE, p != 1 (a workgroup-uniform branch;
// torch's definition): l = p t softplus(-o) + (1-t) softplus(o) with
// softplus(+-o) = max(+-o, 0) + log1p(exp(-|o|)), dl/do = (1-t) sg -
// p t (1-sg), 1-sg taken as sigmoid(-o). The grouping makes w = 1, p = 1
// reproduce the unweighted bits; a row with w = 0 gives dyb = +-0 and a
// zero term.
template <int MT, bool PI16, int LOSS, bool WEIGHTED>
__device__ __forceinline__ void fc_fwd_chain_body(
    const short* __restrict__ x0s,  // fragment-major swizzled x (see note)
    const short* __restrict__ W1, const float* __restrict__ b1,
    const short* __restrict__ W2, const float* __restrict__ b2,
    const short* __restrict__ W3, const float* __restrict__ b3,
    const short* __restrict__ w4, const float* __restrict__ b4,
    short* __restrict__ a1t,        // wgrad fragment-major a1^T
    uint32_t* __restrict__ mask1,   // [m_tiles][512] relu-mask words
    short* __restrict__ a2t,        // wgrad fragment-major a2^T
    uint32_t* __restrict__ mask2,   // [m_tiles][256]
    short* __restrict__ a3, short* __restrict__ out,
    // Optional fused loss epilogue (target != nullptr), MSE: dyb[m] =
    // (2/M)*(out[m]-target[m]) in bf16 and loss_part[blockIdx] =
    // sum_m (out[m]-target[m])^2 — removes the eager loss/grad kernel
    // chain from the fused train step. BCE: see LOSS above.
    const float* __restrict__ target, short* __restrict__ dyb,
    float* __restrict__ loss_part, float inv_m, int64_t M,
    int64_t mchunks, const float* __restrict__ weight, float pos_weight) {
  // LDS budget is the occupancy lever. x needs no tile (pre-swizzled
  // fragment-major in global, coalesced A loads), and a1 itself leaves
  // through the EMIT_T epilogue, transposed, plus mask words — no
  // row-major a1/a2 tensors exist at all.
  //   MT = 1: t1 + t2 + lsum = ~50 KB -> 3 workgroups/CU; t3 ALIASES t1
  //           (layer 3 runs after layer 2 consumed t1).
  //   MT = 2: t1 + t2 would be 100 KB = one workgroup/CU. t2 ALIASES t1
  //           too (layer 2 puts a barrier between its k-loop, the last
  //           reader of t1, and its epilogue) and t3 sits behind t2
  //           inside t1's storage: 66.8 KB -> 2 workgroups/CU.
  constexpr int ROWS = MT * FC_MT;
  constexpr int T1B = ROWS * FC_S1 * 2;
  constexpr int T2B = ROWS * FC_S2 * 2;
  constexpr int TILEB = MT == 1 ? T1B + T2B : T1B;
  static_assert(MT == 1 || T2B + ROWS * FC_S3 * 2 <= T1B, "t2+t3 in t1");
  __shared__ __align__(16) char smem[TILEB + ROWS * 4];
  short* t1 = reinterpret_cast<short*>(smem);
  short* t2 = reinterpret_cast<short*>(MT == 1 ? smem + T1B : smem);
  // aliased: live ranges are disjoint (barrier-ordered)
  short* t3 = reinterpret_cast<short*>(MT == 1 ? smem : smem + T2B);
  float* lsum = reinterpret_cast<float*>(smem + TILEB);

  const int64_t m0 = (int64_t)blockIdx.x * ROWS;
  const int32_t tid = threadIdx.x;
  const int32_t wave = tid >> 6;
  const int32_t lane = tid & 63;
  const int64_t mt_g0 = (int64_t)blockIdx.x * MT;  // first global m-tile
  const int64_t mc0 = mt_g0 * 2;
  // Workgroup-uniform: the slab's second m-tile exists (see fc_layer).
  const bool has2 = MT == 1 || 2 * (mt_g0 + 1) < mchunks;

  // Layers 1 and 2: every wave takes N/(4*MT) columns of all MT m-tiles,
  // so each weight fragment it loads feeds MT MFMAs.
  // Layer 1: A fragments straight from the swizzled global x block.
  const short* xblk = &x0s[mt_g0 * (FC_K0P / 16) * 512];
  constexpr int NT1 = FC_N1 / (128 * MT), NT2 = FC_N2 / (128 * MT);
  fc_layer<FC_K0P, FC_N1, MT, NT1, 0, FC_S1, true, true, true, PI16>(
      xblk, W1, b1, t1, 0, wave * NT1, fc_fresh_lane<MT>(lane), has2, a1t,
      &mask1[mt_g0 * FC_N1], mchunks, mc0);
  __syncthreads();
  fc_layer<FC_N1, FC_N2, MT, NT2, FC_S1, FC_S2, true, false, true, PI16,
           MT == 2>(
      t1, W2, b2, t2, 0, wave * NT2, fc_fresh_lane<MT>(lane), has2, a2t,
      &mask2[mt_g0 * FC_N2], mchunks, mc0);
  __syncthreads();
  // Layer 3 has only four n-tiles: wave w takes (m-tile w >> 2, n-tile
  // w & 3), unshared (15 % of the weight bytes).
  fc_layer<FC_N2, FC_N3, 1, 1, FC_S2, FC_S3, true>(
      t2, W3, b3, t3, wave >> 2, wave & 3, fc_fresh_lane<MT>(lane), true);
  __syncthreads();

  // Head: out[m] = sum_k a3[m,k] * w4[k] + b4. 8 threads per row,
  // pair-wise LDS-free reduce via wave shuffles (partners are adjacent
  // lanes).
  {
    constexpr int TPR = 256 / FC_MT;       // threads per row
    constexpr int KPT = FC_N3 / TPR;       // k per thread
    const int32_t m = tid / TPR;
    const int32_t part = tid % TPR;
    float s = 0.f;
    #pragma unroll
    for (int32_t kk = 0; kk < KPT; kk++) {
      const int32_t k = part * KPT + kk;
      s += fc_b2f(t3[m * FC_S3 + k]) * fc_b2f(w4[k]);
    }
    #pragma unroll
    for (int32_t d = 1; d < TPR; d <<= 1) {
      s += __shfl_down(s, d);
    }
    if (part == 0) {
      const float o = s + b4[0];
      float d2 = 0.f;
      if (m0 + m < M) {
        out[m0 + m] = fc_f2b(o);
        if (target != nullptr) {
          if (!WEIGHTED) {
            if (LOSS == FC_LOSS_MSE) {
              const float diff = o - target[m0 + m];
              dyb[m0 + m] = fc_f2b(2.f * inv_m * diff);
              d2 = diff * diff;
            } else {
              float sg;
              const float t = target[m0 + m];
              fc_bce_terms(o, t, sg, d2);
              dyb[m0 + m] = fc_f2b(inv_m * (sg - t));
            }
          } else {
            const float w = weight != nullptr ? weight[m0 + m] : 1.f;
            const float t = target[m0 + m];
            if (LOSS == FC_LOSS_MSE) {
              const float diff = o - t;
              dyb[m0 + m] = fc_f2b((2.f * inv_m * w) * diff);
              d2 = w * (diff * diff);
            } else if (pos_weight == 1.f) {
              float sg, l;
              fc_bce_terms(o, t, sg, l);
              dyb[m0 + m] = fc_f2b((inv_m * w) * (sg - t));
              d2 = w * l;
            } else {
              float sg, l, g;
              fc_bce_pw_terms(o, t, pos_weight, sg, l, g);
              dyb[m0 + m] = fc_f2b((inv_m * w) * g);
              d2 = w * l;
            }
          }
        }
      }
      if (target != nullptr) lsum[m] = d2;
    }
  }
  if (target != nullptr) {
    __syncthreads();
    if (tid == 0) {
      float s = 0.f;
      #pragma unroll
      for (int32_t m = 0; m < ROWS; m++) s += lsum[m];
      loss_part[blockIdx.x] = s;
    }
  }

  fc_store_tile<MT, FC_N3, FC_S3>(t3, a3, m0, M, tid);
}

// The one entry point per instantiation. ``weight`` and ``pos_weight`` are
// always in the argument list; the WEIGHTED = false body never reads them.
template <int MT, bool PI16, int LOSS, bool WEIGHTED>
__global__ void __launch_bounds__(256 * MT, MT == 2 ? 4 : 1)
fwd_chain_kernel(
    const short* __restrict__ x0s, const short* __restrict__ W1,
    const float* __restrict__ b1, const short* __restrict__ W2,
    const float* __restrict__ b2, const short* __restrict__ W3,
    const float* __restrict__ b3, const short* __restrict__ w4,
    const float* __restrict__ b4, short* __restrict__ a1t,
    uint32_t* __restrict__ mask1, short* __restrict__ a2t,
    uint32_t* __restrict__ mask2, short* __restrict__ a3,
    short* __restrict__ out, const float* __restrict__ target,
    short* __restrict__ dyb, float* __restrict__ loss_part, float inv_m,
    int64_t M, int64_t mchunks, const float* __restrict__ weight,
    float pos_weight) {
  fc_fwd_chain_body<MT, PI16, LOSS, WEIGHTED>(
      x0s, W1, b1, W2, b2, W3, b3, w4, b4, a1t, mask1, a2t, mask2, a3, out,
      target, dyb, loss_part, inv_m, M, mchunks, weight, pos_weight);
}

// Forward-only sibling of fwd_chain_kernel for evaluation
// (models/fused_eval.py): the same slab scheme, LDS aliasing, barriers and
// three fc_layer calls, with EMIT_T off in layers 1 and 2 — no transposed
// fragments, no mask words, no a3 tile and no dyb leave the workgroup.
// Every accumulator sees the MFMAs of the training kernel in the same
// order, so the head value o is the training kernel's, bit for bit.
//   pred (optional)    pred[m] = o, fp32, unrounded
//   target (optional)  part[blockIdx][0..3] = sum (o-t)^2, sum |o-t|,
//                      sum t, sum t^2 over the slab's rows m < M.
// Column 0 is loss_part of the training kernel: the same diff and d2
// expressions and the same serial sum over lsum[0..ROWS) by one thread.
// Columns 1-3 are summed the same way by threads 1-3. A separate kernel,
// not a template flag of fwd_chain_kernel: the 64-row training
// instantiation sits at exactly 128 registers and must not move.
// TASK = FC_LOSS_BCE (binary classification, o is a logit): the partials
// are {sum l, sum (sg-t)^2, sum t, sum correct} with l and sg from
// fc_bce_terms as in the training kernel and correct = ((o >= 0) ==
// (t >= 0.5)) — at most ROWS per slab, exact in fp32. With ``hist``
// (int64 [2][65536], persistent, optional) every row m < M also adds 1
// to hist[t >= 0.5][key], key = the top 16 bits of the order-preserving
// transform of o's bit pattern (o truncated to bf16 precision, order
// kept): the streaming-AUC histogram. Integer atomics commute, so the
// histogram does not depend on launch or arrival order. A NaN logit lands
// wherever its bits put it. ``hist`` is ignored by the regression task.
// WEIGHTED (eval_chain_kernel<.., true>; the false instantiations never
// read ``weight`` and compile to what they did): ``weight`` (fp32 [M],
// read under the m0 + m < M guard only; null = every w is 1) scales every
// term and a fifth partial carries the weight sum, in rows of EIGHT floats
// (two aligned float4 for eval_accumulate; columns 5-7 are written as 0):
//   regression  {sum w d^2, sum w |d|, sum w t, sum w t^2, sum w, 0, 0, 0}
//   binary      {sum w l, sum w (sg-t)^2, sum w t, sum w correct, sum w, ..}
// Column 0 is loss_part of the weighted training kernel at pos_weight = 1
// (the same w * term expressions, the same serial sum). The histogram add
// becomes llrintf(w * 2^20), a fixed-point weight with quantum 2^-20 —
// still integer atomics, still independent of arrival order. Negative or
// non-finite weights are undefined.
template <int MT, int TASK, bool WEIGHTED>
__device__ __forceinline__ void fc_eval_chain_body(
    const short* __restrict__ x0s,  // fragment-major swizzled x
    const short* __restrict__ W1, const float* __restrict__ b1,
    const short* __restrict__ W2, const float* __restrict__ b2,
    const short* __restrict__ W3, const float* __restrict__ b3,
    const short* __restrict__ w4, const float* __restrict__ b4,
    float* __restrict__ pred, const float* __restrict__ target,
    float* __restrict__ part, int64_t M, int64_t mchunks,
    unsigned long long* __restrict__ hist,
    const float* __restrict__ weight) {
  // LDS plan of fwd_chain_kernel, with four lsum columns instead of one
  // (MT = 1: 50.7 KB, 3 workgroups/CU; MT = 2: 67.6 KB, 2 workgroups/CU);
  // five when WEIGHTED (MT = 1: 50,816 B; MT = 2: 67,840 B = 66.25 KB,
  // under half of the CU's 160 KB, so still 2 workgroups/CU).
  constexpr int NCOL = WEIGHTED ? 5 : 4;
  constexpr int ROWS = MT * FC_MT;
  constexpr int T1B = ROWS * FC_S1 * 2;
  constexpr int T2B = ROWS * FC_S2 * 2;
  constexpr int TILEB = MT == 1 ? T1B + T2B : T1B;
  static_assert(MT == 1 || T2B + ROWS * FC_S3 * 2 <= T1B, "t2+t3 in t1");
  __shared__ __align__(16) char smem[TILEB + NCOL * ROWS * 4];
  short* t1 = reinterpret_cast<short*>(smem);
  short* t2 = reinterpret_cast<short*>(MT == 1 ? smem + T1B : smem);
  // aliased: live ranges are disjoint (barrier-ordered)
  short* t3 = reinterpret_cast<short*>(MT == 1 ? smem : smem + T2B);
  float* lsum = reinterpret_cast<float*>(smem + TILEB);  // [NCOL][ROWS]

  const int64_t m0 = (int64_t)blockIdx.x * ROWS;
  const int32_t tid = threadIdx.x;
  const int32_t wave = tid >> 6;
  const int32_t lane = tid & 63;
  const int64_t mt_g0 = (int64_t)blockIdx.x * MT;  // first global m-tile
  // Workgroup-uniform: the slab's second m-tile exists (see fc_layer).
  const bool has2 = MT == 1 || 2 * (mt_g0 + 1) < mchunks;

  const short* xblk = &x0s[mt_g0 * (FC_K0P / 16) * 512];
  constexpr int NT1 = FC_N1 / (128 * MT), NT2 = FC_N2 / (128 * MT);
  fc_layer<FC_K0P, FC_N1, MT, NT1, 0, FC_S1, true, true>(
      xblk, W1, b1, t1, 0, wave * NT1, fc_fresh_lane<MT>(lane), has2);
  __syncthreads();
  fc_layer<FC_N1, FC_N2, MT, NT2, FC_S1, FC_S2, true, false, false, false,
           MT == 2>(
      t1, W2, b2, t2, 0, wave * NT2, fc_fresh_lane<MT>(lane), has2);
  __syncthreads();
  fc_layer<FC_N2, FC_N3, 1, 1, FC_S2, FC_S3, true>(
      t2, W3, b3, t3, wave >> 2, wave & 3, fc_fresh_lane<MT>(lane), true);
  __syncthreads();

  // Head as in fwd_chain_kernel: 8 threads per row, shuffle reduce.
  {
    constexpr int TPR = 256 / FC_MT;       // threads per row
    constexpr int KPT = FC_N3 / TPR;       // k per thread
    const int32_t m = tid / TPR;
    const int32_t prt = tid % TPR;
    float s = 0.f;
    #pragma unroll
    for (int32_t kk = 0; kk < KPT; kk++) {
      const int32_t k = prt * KPT + kk;
      s += fc_b2f(t3[m * FC_S3 + k]) * fc_b2f(w4[k]);
    }
    #pragma unroll
    for (int32_t d = 1; d < TPR; d <<= 1) {
      s += __shfl_down(s, d);
    }
    if (prt == 0) {
      const float o = s + b4[0];
      float d2 = 0.f, ad = 0.f, t = 0.f, c3 = 0.f, w = 0.f;
      if (m0 + m < M) {
        if (pred != nullptr) pred[m0 + m] = o;
        if (target != nullptr) {
          t = target[m0 + m];
          if (WEIGHTED) w = weight != nullptr ? weight[m0 + m] : 1.f;
          if (TASK == FC_LOSS_MSE) {
            const float diff = o - t;
            d2 = diff * diff;
            ad = fabsf(diff);
          } else {
            float sg;
            fc_bce_terms(o, t, sg, d2);
            const float diff = sg - t;
            ad = diff * diff;
            const bool cls = t >= 0.5f;
            c3 = ((o >= 0.f) == cls) ? 1.f : 0.f;
            if (hist != nullptr) {
              const uint32_t bits = __float_as_uint(o);
              const uint32_t u =
                  bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
              atomicAdd(&hist[(cls ? 65536u : 0u) + (u >> 16)],
                        WEIGHTED ? (unsigned long long)llrintf(
                                       w * 1048576.f)
                                 : 1ULL);
            }
          }
        }
      }
      if (target != nullptr) {
        if (!WEIGHTED) {
          lsum[m] = d2;
          lsum[ROWS + m] = ad;
          lsum[2 * ROWS + m] = t;
          lsum[3 * ROWS + m] = TASK == FC_LOSS_MSE ? t * t : c3;
        } else {
          // rows past M have w = 0 and zero terms: every product is +0
          lsum[m] = w * d2;
          lsum[ROWS + m] = w * ad;
          lsum[2 * ROWS + m] = w * t;
          lsum[3 * ROWS + m] = w * (TASK == FC_LOSS_MSE ? t * t : c3);
          lsum[4 * ROWS + m] = w;
        }
      }
    }
  }
  if (target != nullptr) {
    __syncthreads();
    if (!WEIGHTED) {
      if (tid < 4) {
        const float* col = lsum + tid * ROWS;
        float s = 0.f;
        #pragma unroll
        for (int32_t m = 0; m < ROWS; m++) s += col[m];
        part[(int64_t)blockIdx.x * 4 + tid] = s;
      }
    } else if (tid < 8) {
      float s = 0.f;
      if (tid < NCOL) {
        const float* col = lsum + tid * ROWS;
        #pragma unroll
        for (int32_t m = 0; m < ROWS; m++) s += col[m];
      }
      part[(int64_t)blockIdx.x * 8 + tid] = s;
    }
  }
}

template <int MT, int TASK, bool WEIGHTED>
__global__ void __launch_bounds__(256 * MT, MT == 2 ? 4 : 1)
eval_chain_kernel(
    const short* __restrict__ x0s, const short* __restrict__ W1,
    const float* __restrict__ b1, const short* __restrict__ W2,
    const float* __restrict__ b2, const short* __restrict__ W3,
    const float* __restrict__ b3, const short* __restrict__ w4,
    const float* __restrict__ b4, float* __restrict__ pred,
    const float* __restrict__ target, float* __restrict__ part, int64_t M,
    int64_t mchunks, unsigned long long* __restrict__ hist,
    const float* __restrict__ weight) {
  fc_eval_chain_body<MT, TASK, WEIGHTED>(x0s, W1, b1, W2, b2, W3, b3, w4, b4,
                                         pred, target, part, M, mchunks,
                                         hist, weight);
}

// x [M,100] bf16 -> fragment-major [ceil(M/32)][7][2][32][8] with zero
// padding (cols 100..111 and rows past M). One thread per 8-halfword
// fragment slice; replaces a 3-kernel pad+permute+contiguous chain.
__global__ void __launch_bounds__(256) swizzle_x_kernel(
    const short* __restrict__ x, short* __restrict__ out, int64_t M,
    int64_t total_blocks) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= total_blocks) return;
  // b = ((mt*7 + kc)*2 + h)*32 + ml
  const int32_t ml = (int32_t)(b & 31);
  int64_t r = b >> 5;
  const int32_t h = (int32_t)(r & 1);
  r >>= 1;
  const int32_t kc = (int32_t)(r % 7);
  const int64_t mt = r / 7;
  const int64_t m = mt * 32 + ml;
  const int32_t k0 = kc * 16 + h * 8;
  short v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (m < M) {
    const short* row = &x[m * FC_K0];
    if (k0 + 8 <= FC_K0) {
      // rows are 8-B aligned (100 * 2 B stride), not 16-B: two 8-B loads
      *reinterpret_cast<fc_u32x2*>(&v[0]) = _rsdl_load(
          reinterpret_cast<const fc_u32x2*>(&row[k0]));
      *reinterpret_cast<fc_u32x2*>(&v[4]) = _rsdl_load(
          reinterpret_cast<const fc_u32x2*>(&row[k0 + 4]));
    } else {
      #pragma unroll
      for (int j = 0; j < 8; j++) {
        if (k0 + j < FC_K0) v[j] = row[k0 + j];
      }
    }
  }
  _rsdl_store(*reinterpret_cast<fc_u32x4*>(v),
                              reinterpret_cast<fc_u32x4*>(&out[b * 8]));
}

void launch_swizzle_x(const void* x, void* out, int64_t M,
                      hipStream_t stream) {
  const int64_t mtiles = (M + FC_MT - 1) / FC_MT;
  // fragment blocks per 32-row m-tile: 7 kc * 2 h * 32 ml
  const int64_t total = mtiles * (FC_K0P / 16) * 2 * 32;
  const int64_t grid = (total + 255) / 256;
  hipLaunchKernelGGL(swizzle_x_kernel, dim3((uint32_t)grid), dim3(256), 0,
                     stream, reinterpret_cast<const short*>(x),
                     reinterpret_cast<short*>(out), M, total);
}

// Combined swizzle: one pass over x emits BOTH the forward fragment
// layout (xs: [mt][7][2][32][8] over k-contraction) and the wgrad
// fragment layout (xt: [4][mchunks][2][32][8] over m-contraction).
// One thread per 16-B fwd block (8 k for one row m); the wgrad-side
// elements it holds are scattered, so the wgrad half works via LDS: the
// workgroup stages a [32 m x 128 k] tile and re-emits it transposed.
template <bool PI16 = false>
__global__ void __launch_bounds__(256) swizzle_x_both_kernel(
    const short* __restrict__ x, short* __restrict__ xs,
    short* __restrict__ xt, int64_t M, int64_t mtiles) {
  __shared__ short tile[32 * 136];  // [m][k] stride 136 (16-B rows)
  const int64_t mt = blockIdx.x;
  if (mt >= mtiles) return;
  const int32_t tid = threadIdx.x;
  const int64_t m0 = mt * 32;
  // stage: 32 rows x 100 cols, 8-B vectors (25 uint2 slots per row)
  for (int32_t u = tid; u < 32 * 25; u += 256) {
    const int32_t m = u / 25;
    const int32_t c = (u % 25) * 4;
    fc_u32x2 v = {0, 0};
    if (m0 + m < M) {
      v = _rsdl_load(
          reinterpret_cast<const fc_u32x2*>(&x[(m0 + m) * FC_K0 + c]));
    }
    *reinterpret_cast<fc_u32x2*>(&tile[m * 136 + c]) = v;
  }
  // zero-pad cols 100..127 (fwd uses 100..111; wgrad k-tiles reach 127)
  for (int32_t u = tid; u < 32 * 7; u += 256) {
    const int32_t m = u / 7;
    const int32_t c = 100 + (u % 7) * 4;
    fc_u32x2 z = {0, 0};
    *reinterpret_cast<fc_u32x2*>(&tile[m * 136 + c]) = z;
  }
  __syncthreads();
  // fwd layout: block (kc, h, ml) -> 8 k of row ml
  for (int32_t u = tid; u < 7 * 2 * 32; u += 256) {
    const int32_t ml = u & 31;
    const int32_t h = (u >> 5) & 1;
    const int32_t kc = u >> 6;
    const int32_t k0 = kc * 16 + h * 8;
    fc_u32x4 v = *reinterpret_cast<const fc_u32x4*>(&tile[ml * 136 + k0]);
    _rsdl_store(
        v, reinterpret_cast<fc_u32x4*>(
               &xs[(mt * 14 + (int64_t)u / 32) * 256 + ml * 8]));
  }
  // wgrad layout: block (kt, mc_local, h, ml) -> 8 m of column kt*32+ml
  const int64_t mchunks = mtiles * 2;
  for (int32_t u = tid; u < 4 * 2 * 2 * 32; u += 256) {
    const int32_t ml = u & 31;
    const int32_t h = (u >> 5) & 1;
    const int32_t mcl = (u >> 6) & 1;
    const int32_t kt = u >> 7;
    const int32_t k = kt * 32 + ml;
    const int32_t mb = mcl * 16 + h * 8;
    fc_u32x4 pack;
    short* vp = reinterpret_cast<short*>(&pack);
    #pragma unroll
    for (int j = 0; j < 8; j++) {
      // PI16 intra-chunk M-permutation (pos -> row = swap bits 2<->3):
      // slice h's positions hold rows {0-3,8-11} (h=0) / {4-7,12-15}.
      const int32_t mr = PI16
          ? (mcl * 16 + (j & 3) + ((j & 4) << 1) + 4 * h)
          : (mb + j);
      vp[j] = tile[mr * 136 + k];
    }
    _rsdl_store(
        pack, reinterpret_cast<fc_u32x4*>(
                  &xt[(((int64_t)kt * mchunks + mt * 2 + mcl) * 2 + h) *
                          256 +
                      ml * 8]));
  }
}

void launch_swizzle_x_both(const void* x, void* xs, void* xt, int64_t M,
                           int pi16, hipStream_t stream) {
  const int64_t mtiles = (M + FC_MT - 1) / FC_MT;
  auto kern =
      pi16 ? swizzle_x_both_kernel<true> : swizzle_x_both_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)mtiles),
                     dim3(256), 0, stream,
                     reinterpret_cast<const short*>(x),
                     reinterpret_cast<short*>(xs),
                     reinterpret_cast<short*>(xt), M, mtiles);
}

// x [M,100] bf16 -> wgrad fragment-major x^T:
// [128/32][mchunks][2][32][8] with zero pads (cols 100..127, rows >= M).
// One thread per 16-B out block = 8 consecutive m's of one column k;
// writes fully coalesced, reads gather 8 row-strided elements (L1-local:
// neighboring threads read the same 8 rows).
template <bool PI16 = false>
__global__ void __launch_bounds__(256) swizzle_xt_kernel(
    const short* __restrict__ x, short* __restrict__ out, int64_t M,
    int64_t total_blocks) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= total_blocks) return;
  // b = ((kt*mchunks + mc)*2 + h)*32 + ml
  const int32_t ml = (int32_t)(b & 31);
  int64_t r = b >> 5;
  const int32_t h = (int32_t)(r & 1);
  r >>= 1;
  // total = 4 (kt) * mchunks * 2 (h) * 32 (ml) = 256 * mchunks
  const int64_t mchunks = total_blocks >> 8;
  const int64_t mc = r % mchunks;
  const int32_t kt = (int32_t)(r / mchunks);
  const int32_t k = kt * 32 + ml;
  const int64_t m0 = mc * 16 + h * 8;
  short v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (k < FC_K0) {
    #pragma unroll
    for (int j = 0; j < 8; j++) {
      const int64_t m = PI16
          ? (mc * 16 + (j & 3) + ((j & 4) << 1) + 4 * h)
          : (m0 + j);
      if (m < M) v[j] = x[m * FC_K0 + k];
    }
  }
  _rsdl_store(*reinterpret_cast<fc_u32x4*>(v),
                              reinterpret_cast<fc_u32x4*>(&out[b * 8]));
}

void launch_swizzle_xt(const void* x, void* out, int64_t M, int pi16,
                       hipStream_t stream) {
  const int64_t mtiles = (M + FC_MT - 1) / FC_MT;
  const int64_t mchunks = mtiles * 2;
  const int64_t total = 4 * mchunks * 2 * 32;  // kt * mc * h * ml
  const int64_t grid = (total + 255) / 256;
  auto kern = pi16 ? swizzle_xt_kernel<true> : swizzle_xt_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(256), 0,
                     stream, reinterpret_cast<const short*>(x),
                     reinterpret_cast<short*>(out), M, total);
}

// rows = rows per workgroup slab, 32 or 64 (validated by the binding).
int64_t fwd_chain_grid(int64_t M, int rows) {
  return (M + rows - 1) / rows;
}

// The instantiation of a (rows, pi16, loss, weighted) call, picked in one
// place per family. The weighted instantiations run only when the binding
// asks for them (a weight tensor or a pos_weight != 1, with a target), so
// the default step and the default evaluator launch the unweighted ones.
template <int MT, bool PI16, int LOSS>
static auto fwd_chain_pick(bool weighted) {
  return weighted ? fwd_chain_kernel<MT, PI16, LOSS, true>
                  : fwd_chain_kernel<MT, PI16, LOSS, false>;
}
template <int MT, bool PI16>
static auto fwd_chain_pick(int loss, bool weighted) {
  return loss == FC_LOSS_BCE ? fwd_chain_pick<MT, PI16, FC_LOSS_BCE>(weighted)
                             : fwd_chain_pick<MT, PI16, FC_LOSS_MSE>(weighted);
}
template <int MT>
static auto fwd_chain_pick(int pi16, int loss, bool weighted) {
  return pi16 ? fwd_chain_pick<MT, true>(loss, weighted)
              : fwd_chain_pick<MT, false>(loss, weighted);
}

void launch_fwd_chain(const FwdChainArgs& p, hipStream_t stream) {
  const int32_t grid = (int32_t)fwd_chain_grid(p.M, p.rows);
  // The global layouts are per 32-row m-tile whatever the slab size.
  const int64_t mchunks = (p.M + FC_MT - 1) / FC_MT * 2;
  auto kern = p.rows == 64 ? fwd_chain_pick<2>(p.pi16, p.loss, p.weighted)
                           : fwd_chain_pick<1>(p.pi16, p.loss, p.weighted);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(p.rows == 64 ? 512 : 256), 0,
                     stream,
                     reinterpret_cast<const short*>(p.x0s),
                     reinterpret_cast<const short*>(p.w.W1), p.w.b1,
                     reinterpret_cast<const short*>(p.w.W2), p.w.b2,
                     reinterpret_cast<const short*>(p.w.W3), p.w.b3,
                     reinterpret_cast<const short*>(p.w.w4), p.w.b4,
                     reinterpret_cast<short*>(p.a1t), p.mask1,
                     reinterpret_cast<short*>(p.a2t), p.mask2,
                     reinterpret_cast<short*>(p.a3),
                     reinterpret_cast<short*>(p.out), p.target,
                     reinterpret_cast<short*>(p.dyb), p.loss_part,
                     p.target ? 1.f / (float)p.M : 0.f, p.M, mchunks,
                     p.weight, p.pos_weight);
}

template <int MT, int TASK>
static auto eval_chain_pick(bool weighted) {
  return weighted ? eval_chain_kernel<MT, TASK, true>
                  : eval_chain_kernel<MT, TASK, false>;
}
template <int MT>
static auto eval_chain_pick(int task, bool weighted) {
  return task == FC_LOSS_BCE ? eval_chain_pick<MT, FC_LOSS_BCE>(weighted)
                             : eval_chain_pick<MT, FC_LOSS_MSE>(weighted);
}

// Forward-only evaluation chain (EvalChainArgs in chain.h).
void launch_eval_chain(const EvalChainArgs& p, hipStream_t stream) {
  const int32_t grid = (int32_t)fwd_chain_grid(p.M, p.rows);
  const int64_t mchunks = (p.M + FC_MT - 1) / FC_MT * 2;
  auto kern = p.rows == 64 ? eval_chain_pick<2>(p.task, p.weighted)
                           : eval_chain_pick<1>(p.task, p.weighted);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(p.rows == 64 ? 512 : 256), 0,
                     stream,
                     reinterpret_cast<const short*>(p.x0s),
                     reinterpret_cast<const short*>(p.w.W1), p.w.b1,
                     reinterpret_cast<const short*>(p.w.W2), p.w.b2,
                     reinterpret_cast<const short*>(p.w.W3), p.w.b3,
                     reinterpret_cast<const short*>(p.w.w4), p.w.b4, p.pred,
                     p.target, p.part, p.M, mchunks,
                     reinterpret_cast<unsigned long long*>(p.hist),
                     p.weight);
}

}  // namespace rsdl
