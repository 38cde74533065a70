// Fragment-major weight-gradient kernel for MI355X (gfx950).
//
//   dW[n][k] = sum_m dz[m][n] * src[m][k]
//
// Both inputs arrive TRANSPOSED in the fragment-major layout the MFMA
// wants (same block structure as the chain kernels' swizzled weights,
// csrc/fwd_chain.hip, but over the M contraction):
//
//   AT = dz^T  fragments: [N/32][Mp/16][2][32][8]   (Mp = M padded to 16)
//   BT = src^T fragments: [K/32][Mp/16][2][32][8]
//
// so every wave's fragment load is a contiguous 1 KB block — the round-1
// wgrad kernel (csrc/wgrad_kernel.hip) read m-strided fragments and was
// bound on L1/TCC line processing at ~1.3-1.6 TB/s; the library split-K
// bmm ran ~3x off the stream roofline. The producers emit these layouts
// for free: bwd_chain writes dz^T straight from its epilogue registers
// and fwd_chain/swizzle_x emit src^T (round-2 stage 2/3).
//
// Two kernels compute the same per-slab partials, bit for bit:
// wgrad_frag_kernel (direct, below; the reference, the default for dW1
// and the only one for the small tiles) and wgrad_lds_kernel (further
// down; stages each chunk's unique fragments once per workgroup through
// an LDS ring; the default for dW2 and dW3). launch_wgrad_frag picks:
// explicit variant, then RSDL_WGRAD_LDS, then the per-shape default.
// The train step runs its three wgrads as ONE launch of the ring body,
// wgrad_grouped_kernel (launch_wgrad_grouped, at the end of the file).
//
// Direct kernel: NO LDS, no barriers — per m-chunk (16 rows) each wave loads
// its (NT_W + KT_W) fragments directly from global (coalesced; waves of
// one workgroup share B blocks -> L1 hits) and issues NT_W*KT_W MFMAs,
// 3-deep prefetched, consumed in reverse load order so the final wait
// leaves newer prefetches outstanding. The workgroup owns an output
// block of [128*NT_W n x 32*KT_W k] and one m-slab; fp32 partials land
// in per-slab buffers reduced by slab_reduce_kernel (global atomics at
// ~16M adds/launch measured 35-65 us of contention).
//
// XCD-aware decode: consecutive blockIdx round-robin across the 8 XCDs,
// so the grid is decoded as (xcd, seq) with all output-blocks of one
// m-slab given to ONE xcd — their shared input slab stays in that XCD's
// L2 instead of being refetched from HBM per block.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "chain.h"

namespace rsdl {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short wf_bf16x8;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float wf_f32x16;

template <int NT_W, int KT_W, int MIN_WAVES = 2, int SCHED = 0>
__global__ void __launch_bounds__(256, MIN_WAVES) wgrad_frag_kernel(
    const short* __restrict__ AT, const short* __restrict__ BT,
    float* __restrict__ dW,  // [N,K] fp32, pre-zeroed
    int32_t N, int32_t K, int64_t mchunks, int32_t nblk_n, int32_t nblk_k,
    int64_t nslabs, int64_t chunks_per_slab) {
  const int32_t NBLK = (nblk_n < 0 ? -nblk_n : nblk_n) * nblk_k;
  int64_t slab;
  int32_t blk;
  if (nblk_n < 0) {  // linear decode (A/B: RSDL_WGRAD_LINEAR)
    nblk_n = -nblk_n;
    blk = (int32_t)(blockIdx.x % (uint32_t)NBLK);
    slab = blockIdx.x / (uint32_t)NBLK;
  } else {
    const int32_t xcd = blockIdx.x & 7;
    const int32_t g = blockIdx.x >> 3;
    blk = g % NBLK;
    slab = (int64_t)(g / NBLK) * 8 + xcd;
  }
  if (slab >= nslabs) return;
  const int32_t bn = blk / nblk_k;
  const int32_t bk = blk % nblk_k;
  const int64_t c0 = slab * chunks_per_slab;
  const int64_t cend = min(c0 + chunks_per_slab, mchunks);
  if (c0 >= cend) return;
  const int64_t iters = cend - c0;

  const int32_t wave = threadIdx.x >> 6;
  const int32_t lane = threadIdx.x & 63;
  const int32_t nt0 = bn * (4 * NT_W) + wave * NT_W;
  const int32_t kt0 = bk * KT_W;

  const short* aptr[NT_W];
  const short* bptr[KT_W];
  #pragma unroll
  for (int nt = 0; nt < NT_W; nt++) {
    aptr[nt] = AT + ((int64_t)(nt0 + nt) * mchunks + c0) * 512 + lane * 8;
  }
  #pragma unroll
  for (int kt = 0; kt < KT_W; kt++) {
    bptr[kt] = BT + ((int64_t)(kt0 + kt) * mchunks + c0) * 512 + lane * 8;
  }

  wf_f32x16 acc[NT_W][KT_W] = {};
  wf_bf16x8 a0[NT_W], b0[KT_W], a1[NT_W], b1[KT_W];
  wf_bf16x8 a2[NT_W], b2[KT_W];

#define WF_LOAD(abuf, bbuf, i)                                             \
  {                                                                        \
    _Pragma("unroll") for (int nt = 0; nt < NT_W; nt++) {                  \
      *reinterpret_cast<uint4*>(&abuf[nt]) =                               \
          *reinterpret_cast<const uint4*>(&aptr[nt][(i)*512]);             \
    }                                                                      \
    _Pragma("unroll") for (int kt = 0; kt < KT_W; kt++) {                  \
      *reinterpret_cast<uint4*>(&bbuf[kt]) =                               \
          *reinterpret_cast<const uint4*>(&bptr[kt][(i)*512]);             \
    }                                                                      \
  }
// Consume fragments in REVERSE load order: the final MFMA of a batch
// then depends on the FIRST-issued load, so the backend's waitcnt for
// it leaves the newer prefetch loads outstanding (forward order ended
// each batch with s_waitcnt vmcnt(0), draining the pipeline).
#define WF_MFMA(abuf, bbuf)                                                \
  {                                                                        \
    _Pragma("unroll") for (int nt = NT_W - 1; nt >= 0; nt--) {             \
      _Pragma("unroll") for (int kt = KT_W - 1; kt >= 0; kt--) {           \
        acc[nt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(             \
            abuf[nt], bbuf[kt], acc[nt][kt], 0, 0, 0);                     \
      }                                                                    \
    }                                                                      \
  }

// SCHED=1: pin the load/MFMA group order with sched_barrier(0).
// Without it the backend SINKS one batch's loads to just before their
// consuming MFMAs (seen in the gfx950 asm: a global_load_dwordx4 group
// at offset:2048 immediately followed by s_waitcnt vmcnt(4)/(2)/(0)
// into MFMAs on those registers), collapsing the 3-deep pipeline once
// per 3 chunks and exposing a full HBM latency. With the fences every
// batch's consume sits >= 2 load-groups (12 loads) behind its issue.
// Static property verified by disassembly (profiles/r02/
// wgrad_sched_asm.md); default OFF until measured on hardware.
#define WF_FENCE()                                                         \
  if (SCHED) __builtin_amdgcn_sched_barrier(0)
  // 3-deep prefetch: at depth 1 only ~6 KB/wave was in flight and the
  // kernel ran latency-bound at ~half the stream roofline (depth 4
  // spills the <1,8> config's registers).
  int64_t i = 0;
  // Fenced variants: depth 3 fits <2,4>'s registers; <1,8> (9-quad load
  // groups) spills 36 VGPRs at depth 3 once the fences extend the
  // buffer live ranges, so it runs the 2-buffer depth-2 loop instead.
  // Both hoist an UNCONDITIONAL 2-chunk preheader under an iters>=2
  // guard: with the shared `if (1 < iters)` preheader below, the loop
  // header has a predecessor path with a different outstanding-load
  // count and the waitcnt pass merges to vmcnt(0).
  constexpr bool SCHED3 = SCHED && (NT_W + KT_W <= 6);
  constexpr bool SCHED2 = SCHED && (NT_W + KT_W > 6);
  if (!SCHED) {
    WF_LOAD(a0, b0, 0);
    if (1 < iters) WF_LOAD(a1, b1, 1);
  } else if (iters < 2) {
    WF_LOAD(a0, b0, 0);
    WF_MFMA(a0, b0);
  }
  if (SCHED && iters < 2) {
    // handled above
  } else if (SCHED3) {
    WF_LOAD(a0, b0, 0);
    WF_LOAD(a1, b1, 1);
    // Straight-line steady loop: every prefetch is UNCONDITIONAL (the
    // loop bound guarantees i+4 < iters), so the outstanding-load count
    // is path-independent and the backend can emit precise partial
    // vmcnt waits instead of the vmcnt(0) it is forced to at the
    // control-flow joins of the conditional-load loop below. Fences pin
    // the load/MFMA group order so no load sinks to its consumer.
    while (i + 5 <= iters) {
      WF_LOAD(a2, b2, i + 2);
      WF_FENCE();
      WF_MFMA(a0, b0);
      WF_FENCE();
      WF_LOAD(a0, b0, i + 3);
      WF_FENCE();
      WF_MFMA(a1, b1);
      WF_FENCE();
      WF_LOAD(a1, b1, i + 4);
      WF_FENCE();
      WF_MFMA(a2, b2);
      WF_FENCE();
      i += 3;
    }
    // Drain: rem = iters - i in [1,4]; a0/a1 hold chunks i, i+1.
    if (i + 2 < iters) WF_LOAD(a2, b2, i + 2);
    if (i < iters) WF_MFMA(a0, b0);
    if (i + 3 < iters) WF_LOAD(a0, b0, i + 3);
    if (i + 1 < iters) WF_MFMA(a1, b1);
    if (i + 2 < iters) WF_MFMA(a2, b2);
    if (i + 3 < iters) WF_MFMA(a0, b0);
  } else if (SCHED2) {
    // Same idea at prefetch depth 2 (two buffers): each load group sits
    // one consume-group (NT_W*KT_W MFMAs) ahead of its use, waits stay
    // at vmcnt(NT_W+KT_W) in a single-block loop.
    WF_LOAD(a0, b0, 0);
    WF_LOAD(a1, b1, 1);
    while (i + 4 <= iters) {
      WF_FENCE();
      WF_MFMA(a0, b0);
      WF_FENCE();
      WF_LOAD(a0, b0, i + 2);
      WF_FENCE();
      WF_MFMA(a1, b1);
      WF_FENCE();
      WF_LOAD(a1, b1, i + 3);
      WF_FENCE();
      i += 2;
    }
    // Drain: rem = iters - i in [1,3]; a0/a1 hold chunks i, i+1.
    if (i + 2 < iters) WF_LOAD(a2, b2, i + 2);
    if (i < iters) WF_MFMA(a0, b0);
    if (i + 1 < iters) WF_MFMA(a1, b1);
    if (i + 2 < iters) WF_MFMA(a2, b2);
  } else {
    while (i + 3 <= iters) {
      WF_LOAD(a2, b2, i + 2);
      WF_MFMA(a0, b0);
      if (i + 3 < iters) WF_LOAD(a0, b0, i + 3);
      WF_MFMA(a1, b1);
      if (i + 4 < iters) WF_LOAD(a1, b1, i + 4);
      WF_MFMA(a2, b2);
      i += 3;
    }
    if (i < iters) WF_MFMA(a0, b0);
    if (i + 1 < iters) WF_MFMA(a1, b1);
  }
#undef WF_LOAD
#undef WF_MFMA
#undef WF_FENCE

  // Epilogue: D[row = n-in-tile][col = k-in-tile]; 32 lanes write 32
  // consecutive k's. Plain per-slab partial stores (a second-stage
  // reduce sums the slabs) — global fp32 atomics at ~16M adds per
  // launch cost 35-65 us of contention.
  float* part = dW + slab * (int64_t)N * K;
  #pragma unroll
  for (int nt = 0; nt < NT_W; nt++) {
    #pragma unroll
    for (int kt = 0; kt < KT_W; kt++) {
      const int32_t k = (kt0 + kt) * 32 + (lane & 31);
      #pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int32_t n = (nt0 + nt) * 32 + (reg & 3) + 8 * (reg >> 2) +
                          4 * (lane >> 5);
        part[(int64_t)n * K + k] = acc[nt][kt][reg];
      }
    }
  }
}

// LDS-ring variant of wgrad_frag_kernel: same tile, grid, slab partition,
// XCD decode, MFMAs and epilogue, but the workgroup stages each chunk's
// 12 UNIQUE fragments (4*NT_W of A + KT_W of B, 12 KB) once into a ring
// of kLdsStages LDS stages instead of every wave loading all B fragments
// itself. The fragment layout [2][32][8] is lane-linear at 16 B per lane,
// i.e. exactly the image global_load_lds_dwordx4 writes, so each wave
// issues 3 LDS-DMA loads per chunk (9 register loads in the direct
// kernel) and no prefetch state lives in registers.
//
// Pipeline, per chunk i (stage i % S):
//   s_waitcnt vmcnt(3 * chunks left in flight) lgkmcnt(0)
//       this wave's three DMAs of chunk i have landed, and its ds_reads
//       of chunk i-1 are complete;
//   s_barrier
//       every wave's share of chunk i is in LDS, and nobody still reads
//       stage (i-1) % S;
//   issue the DMAs of chunk i+S-1 into stage (i-1) % S;
//   ds_read_b128 this wave's NT_W + KT_W fragments of chunk i; MFMAs.
// S-2 stages stay in flight ACROSS the barrier (S-1 after the issue),
// hence the raw s_barrier with a counted vmcnt: __syncthreads() would
// drain the DMAs with vmcnt(0). All loads of the loop are LDS-DMA and the
// ring is the kernel's only __shared__ object, so the compiler adds no
// vmcnt(0) of its own. Every acc[nt][kt] sees the same MFMA on the same
// operands in the same chunk order as in wgrad_frag_kernel: the partials
// are bit-identical.
constexpr int kLdsStages = 6;          // 6 x 12 KB = 72 KB: 2 workgroups/CU
constexpr int kLdsStageElems = 12 * 512;

#define WL_WAIT(n) \
  asm volatile("s_waitcnt vmcnt(" #n ") lgkmcnt(0)" ::: "memory")

// One wgrad problem of the ring kernels: everything wgrad_lds_body needs
// besides the ring and the workgroup's index within the problem.
struct WgradProblem {
  const short* AT;
  const short* BT;
  float* part;  // [nslabs][N,K] fp32 partials
  int32_t N, K;
  int64_t mchunks;
  int32_t nblk_n, nblk_k;  // nblk_n < 0: linear decode
  int64_t nslabs, chunks_per_slab;
};

// The ring kernel's whole body. ``ring`` is the calling kernel's one
// __shared__ object; ``wg`` is the workgroup's index within problem ``p``
// (blockIdx.x less a multiple of 8, so wg & 7 is still the XCD).
template <int NT_W, int KT_W>
__device__ __forceinline__ void wgrad_lds_body(short* ring,
                                               const WgradProblem& p,
                                               uint32_t wg) {
  constexpr int S = kLdsStages;
  constexpr int P = S - 1;      // chunks issued ahead of the consumer
  constexpr int NA = 4 * NT_W;  // A fragments per chunk
  static_assert(NA + KT_W == 12, "a stage is 12 fragments, 3 per wave");
  static_assert(P - 1 == 4, "WL_WAIT counts below assume S == 6");
  const short* __restrict__ AT = p.AT;
  const short* __restrict__ BT = p.BT;
  const int32_t N = p.N, K = p.K, nblk_k = p.nblk_k;
  const int64_t mchunks = p.mchunks, nslabs = p.nslabs;
  const int64_t chunks_per_slab = p.chunks_per_slab;
  int32_t nblk_n = p.nblk_n;

  const int32_t NBLK = (nblk_n < 0 ? -nblk_n : nblk_n) * nblk_k;
  int64_t slab;
  int32_t blk;
  if (nblk_n < 0) {  // linear decode (A/B: RSDL_WGRAD_LINEAR)
    nblk_n = -nblk_n;
    blk = (int32_t)(wg % (uint32_t)NBLK);
    slab = wg / (uint32_t)NBLK;
  } else {
    const int32_t xcd = wg & 7;
    const int32_t g = wg >> 3;
    blk = g % NBLK;
    slab = (int64_t)(g / NBLK) * 8 + xcd;
  }
  // Both returns are workgroup-uniform and ahead of the first barrier.
  if (slab >= nslabs) return;
  const int32_t bn = blk / nblk_k;
  const int32_t bk = blk % nblk_k;
  const int64_t c0 = slab * chunks_per_slab;
  const int64_t cend = min(c0 + chunks_per_slab, mchunks);
  if (c0 >= cend) return;
  const int64_t iters = cend - c0;

  const int32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int32_t lane = threadIdx.x & 63;
  const int32_t nt0 = bn * NA + wave * NT_W;
  const int32_t kt0 = bk * KT_W;

  // Loader role: fragments 3*wave .. 3*wave+2 of the stage (A first).
  const short* gp[3];
  #pragma unroll
  for (int j = 0; j < 3; j++) {
    const int32_t f = wave * 3 + j;
    const short* base =
        f < NA ? AT + ((int64_t)(bn * NA + f) * mchunks + c0) * 512
               : BT + ((int64_t)(kt0 + f - NA) * mchunks + c0) * 512;
    gp[j] = base + lane * 8;
  }

  wf_f32x16 acc[NT_W][KT_W] = {};

// One chunk's three DMAs of this wave into stage `st`; the LDS address
// is the wave-uniform fragment base (the hardware adds lane * 16).
#define WL_ISSUE(st)                                                       \
  {                                                                        \
    _Pragma("unroll") for (int j = 0; j < 3; j++) {                        \
      __builtin_amdgcn_global_load_lds(                                    \
          (const __attribute__((address_space(1))) void*)gp[j],            \
          (__attribute__((address_space(3))) void*)(                       \
              ring + (st) * kLdsStageElems + (wave * 3 + j) * 512),        \
          16, 0, 0);                                                       \
      gp[j] += 512;                                                        \
    }                                                                      \
  }
#define WL_CONSUME(st)                                                     \
  {                                                                        \
    const short* sp = ring + (st) * kLdsStageElems + lane * 8;             \
    wf_bf16x8 a[NT_W], b[KT_W];                                            \
    _Pragma("unroll") for (int nt = 0; nt < NT_W; nt++) {                  \
      a[nt] = *reinterpret_cast<const wf_bf16x8*>(                         \
          sp + (wave * NT_W + nt) * 512);                                  \
    }                                                                      \
    _Pragma("unroll") for (int kt = 0; kt < KT_W; kt++) {                  \
      b[kt] = *reinterpret_cast<const wf_bf16x8*>(sp + (NA + kt) * 512);   \
    }                                                                      \
    _Pragma("unroll") for (int nt = 0; nt < NT_W; nt++) {                  \
      _Pragma("unroll") for (int kt = 0; kt < KT_W; kt++) {                \
        acc[nt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(             \
            a[nt], b[kt], acc[nt][kt], 0, 0, 0);                           \
      }                                                                    \
    }                                                                      \
  }

  int32_t ws = 0, rs = 0;  // next stage to fill / to consume
  const int64_t pre = iters < P ? iters : P;
  for (int64_t j = 0; j < pre; j++) {
    WL_ISSUE(ws);
    ws = ws + 1 == S ? 0 : ws + 1;
  }
  int64_t i = 0;
  // Steady state: chunks i .. i+P-1 are in flight; retire chunk i and
  // leave the P-1 newer ones (3 DMAs each) outstanding.
  for (; i + P < iters; i++) {
    WL_WAIT(12);
    __builtin_amdgcn_s_barrier();
    WL_ISSUE(ws);
    ws = ws + 1 == S ? 0 : ws + 1;
    WL_CONSUME(rs);
    rs = rs + 1 == S ? 0 : rs + 1;
  }
  // Drain: every chunk is issued; iters-1-i (<= P-1) are newer than i.
  for (; i < iters; i++) {
    switch (iters - 1 - i) {
      case 0: WL_WAIT(0); break;
      case 1: WL_WAIT(3); break;
      case 2: WL_WAIT(6); break;
      case 3: WL_WAIT(9); break;
      default: WL_WAIT(12); break;
    }
    __builtin_amdgcn_s_barrier();
    WL_CONSUME(rs);
    rs = rs + 1 == S ? 0 : rs + 1;
  }
#undef WL_ISSUE
#undef WL_CONSUME

  // Epilogue: as in wgrad_frag_kernel.
  float* part = p.part + slab * (int64_t)N * K;
  #pragma unroll
  for (int nt = 0; nt < NT_W; nt++) {
    #pragma unroll
    for (int kt = 0; kt < KT_W; kt++) {
      const int32_t k = (kt0 + kt) * 32 + (lane & 31);
      #pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int32_t n = (nt0 + nt) * 32 + (reg & 3) + 8 * (reg >> 2) +
                          4 * (lane >> 5);
        part[(int64_t)n * K + k] = acc[nt][kt][reg];
      }
    }
  }
}
#undef WL_WAIT

template <int NT_W, int KT_W>
__global__ void __launch_bounds__(256, 2) wgrad_lds_kernel(
    const short* __restrict__ AT, const short* __restrict__ BT,
    float* __restrict__ dW,  // [nslabs][N,K] fp32 partials
    int32_t N, int32_t K, int64_t mchunks, int32_t nblk_n, int32_t nblk_k,
    int64_t nslabs, int64_t chunks_per_slab) {
  __shared__ __attribute__((aligned(16))) short
      ring[kLdsStages * kLdsStageElems];
  const WgradProblem p{AT,     BT,     dW,     N,
                       K,      mchunks, nblk_n, nblk_k,
                       nslabs, chunks_per_slab};
  wgrad_lds_body<NT_W, KT_W>(ring, p, blockIdx.x);
}

// The three wgrads of the train step in ONE launch: workgroups
// [0, start[1]) run dW1 with the <2,4> body, [start[1], start[2]) dW2 and
// [start[2], grid) dW3 with the <1,8> body. Every start is a multiple of
// 8, so each problem keeps the XCD decode of its own launch; the partials
// of a problem are those wgrad_lds_kernel writes for the same slab
// partition. With all three resident at once the slab counts no longer
// have to fill the chip per problem: 512 workgroups in all keep every
// slot busy and the partials at 512 x 128 KB.
struct WgradGroupedArgs {
  WgradProblem p[3];
  uint32_t start[3];  // first workgroup of each problem; start[0] == 0
};

__global__ void __launch_bounds__(256, 2) wgrad_grouped_kernel(
    const WgradGroupedArgs g) {
  __shared__ __attribute__((aligned(16))) short
      ring[kLdsStages * kLdsStageElems];
  // Workgroup-uniform problem select, ahead of every barrier and every
  // vector-memory operation.
  const uint32_t b = blockIdx.x;
  if (b < g.start[1]) {
    wgrad_lds_body<2, 4>(ring, g.p[0], b);
  } else {
    const bool dw2 = b < g.start[2];
    wgrad_lds_body<1, 8>(ring, dw2 ? g.p[1] : g.p[2],
                         b - (dw2 ? g.start[1] : g.start[2]));
  }
}

// out[i] = sum_s part[s][i] — the slab-partial reduction (fp32, float4).
// 2-D grid: y splits the slab range so small outputs still fill the
// chip; the few split partials combine with fp32 atomics (<= NSPLIT
// writers per line — negligible contention). out must be zeroed.
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float wf_f32x4;
template <int SCHED = 0>
__global__ void __launch_bounds__(256) slab_reduce_kernel(
    const float* __restrict__ part, float* __restrict__ out, int64_t nk4,
    int64_t nslabs, int64_t s1) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nk4) return;
  const int64_t lo = (int64_t)blockIdx.y * s1;
  const int64_t hi = min(lo + s1, nslabs);
  // 4 independent accumulators with grouped loads: a single add-chain
  // loop serializes on one outstanding load per iteration (the backend
  // waits vmcnt(0) before each accumulate).
  // Plain (cacheable) loads: the partials were JUST written by the
  // producer kernel and are partially L2-resident; nontemporal loads
  // bypassed that and measured ~1.6-2.9 TB/s.
  wf_f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1v = s0, s2 = s0, s3 = s0;
  int64_t sl = lo;
  if (SCHED) {
    // Double-buffered 4-load groups, 2x-unrolled so the buffer roles
    // swap instead of copying (a la[j]=lb[j] rotation materializes as
    // 12 v_movs + a vmcnt(0)): the next group is UNCONDITIONALLY in
    // flight while the current one accumulates, waits sit at vmcnt(4)
    // in a single-block loop.
    wf_f32x4 la[4], lb[4];
#define SR_LOAD(buf, base)                                                 \
  {                                                                        \
    _Pragma("unroll") for (int j = 0; j < 4; j++) {                        \
      buf[j] = *reinterpret_cast<const wf_f32x4*>(                         \
          part + (((base) + j) * nk4 + i) * 4);                            \
    }                                                                      \
  }
#define SR_ACC(buf)                                                        \
  {                                                                        \
    s0 += buf[0];                                                          \
    s1v += buf[1];                                                         \
    s2 += buf[2];                                                          \
    s3 += buf[3];                                                          \
  }
    if (sl + 4 <= hi) {
      SR_LOAD(la, sl);
      while (sl + 12 <= hi) {
        SR_LOAD(lb, sl + 4);
        __builtin_amdgcn_sched_barrier(0);
        SR_ACC(la);
        __builtin_amdgcn_sched_barrier(0);
        SR_LOAD(la, sl + 8);
        __builtin_amdgcn_sched_barrier(0);
        SR_ACC(lb);
        __builtin_amdgcn_sched_barrier(0);
        sl += 8;
      }
      // rem groups: la holds sl; possibly one more unloaded group.
      if (sl + 8 <= hi) {
        SR_LOAD(lb, sl + 4);
        SR_ACC(la);
        SR_ACC(lb);
        sl += 8;
      } else {
        SR_ACC(la);
        sl += 4;
      }
    }
#undef SR_LOAD
#undef SR_ACC
  } else {
    for (; sl + 4 <= hi; sl += 4) {
      const wf_f32x4 l0 = *reinterpret_cast<const wf_f32x4*>(
          part + ((sl + 0) * nk4 + i) * 4);
      const wf_f32x4 l1 = *reinterpret_cast<const wf_f32x4*>(
          part + ((sl + 1) * nk4 + i) * 4);
      const wf_f32x4 l2 = *reinterpret_cast<const wf_f32x4*>(
          part + ((sl + 2) * nk4 + i) * 4);
      const wf_f32x4 l3 = *reinterpret_cast<const wf_f32x4*>(
          part + ((sl + 3) * nk4 + i) * 4);
      s0 += l0;
      s1v += l1;
      s2 += l2;
      s3 += l3;
    }
  }
  for (; sl < hi; sl++) {
    s0 += *reinterpret_cast<const wf_f32x4*>(part + (sl * nk4 + i) * 4);
  }
  const wf_f32x4 s = (s0 + s1v) + (s2 + s3);
  float* o = out + i * 4;
  unsafeAtomicAdd(&o[0], s[0]);
  unsafeAtomicAdd(&o[1], s[1]);
  unsafeAtomicAdd(&o[2], s[2]);
  unsafeAtomicAdd(&o[3], s[3]);
}

// layer configs: 1 -> NT_W=2,KT_W=4 (dW1 [512,128pad]); 2 -> 1,8
// (dW2 [256,512]); 3 -> 1,8 (dW3 [128,256]).
void launch_slab_reduce(const float* part, float* out, int64_t nk,
                        int64_t nslabs, hipStream_t stream) {
  const int64_t nk4 = nk / 4;
  const int64_t gx = (nk4 + 255) / 256;
  // aim for >= 512 workgroups total
  int64_t nsplit = (512 + gx - 1) / gx;
  if (nsplit > nslabs) nsplit = nslabs;
  const int64_t s1 = (nslabs + nsplit - 1) / nsplit;
  nsplit = (nslabs + s1 - 1) / s1;
  static bool sched = [] {
    const char* e = std::getenv("RSDL_WGRAD_SCHED");
    return e && e[0] == '1';
  }();
  auto kern = sched ? slab_reduce_kernel<1> : slab_reduce_kernel<0>;
  hipLaunchKernelGGL(kern,
                     dim3((uint32_t)gx, (uint32_t)nsplit), dim3(256), 0,
                     stream, part, out, nk4, nslabs, s1);
}

static int64_t frag_target(int32_t K, int32_t nt_w) {
  static int64_t env_target = [] {
    const char* e = std::getenv("RSDL_WGRAD_WGS");
    return e ? atoll(e) : 0;
  }();
  if (env_target > 0) return env_target;
  return (nt_w == 2) ? 256 : (K >= 512 ? 512 : 256);
}

int64_t wgrad_frag_nslabs(int64_t mchunks, int32_t N, int32_t K,
                          int32_t nt_w, int32_t kt_w) {
  const int32_t nblk = (N / (nt_w * 128)) * (K / (kt_w * 32));
  int64_t nslabs = (frag_target(K, nt_w) + nblk - 1) / nblk;
  if (nslabs > mchunks) nslabs = mchunks;
  const int64_t cps = (mchunks + nslabs - 1) / nslabs;
  return (mchunks + cps - 1) / cps;
}

// Kernel variant of launch_wgrad_frag: 1 = direct (wgrad_frag_kernel),
// 2 = LDS ring (wgrad_lds_kernel), 0 = the default: RSDL_WGRAD_LDS (0 or
// 1, read once) if set, else the per-shape default below, as measured at
// the flagship shapes (profiles/PERF.md, round 9). The ring kernel exists
// for the 12-fragment tiles only; the default never picks it elsewhere,
// and RSDL_WGRAD_SCHED=1 (the fenced direct kernels) keeps its meaning:
// with it the per-shape default is the direct kernel.
#ifndef RSDL_WGRAD_LDS_DEFAULT_DW1
#define RSDL_WGRAD_LDS_DEFAULT_DW1 0  // [512,128], <2,4>
#endif
#ifndef RSDL_WGRAD_LDS_DEFAULT_DW2
#define RSDL_WGRAD_LDS_DEFAULT_DW2 1  // [256,512], <1,8>
#endif
#ifndef RSDL_WGRAD_LDS_DEFAULT_DW3
#define RSDL_WGRAD_LDS_DEFAULT_DW3 1  // [128,256] and other <1,8> shapes
#endif

bool wgrad_frag_has_lds(int32_t nt_w, int32_t kt_w) {
  return (nt_w == 2 && kt_w == 4) || (nt_w == 1 && kt_w == 8);
}

static bool wgrad_use_lds(int32_t variant, int32_t K, int32_t nt_w,
                          int32_t kt_w, bool sched) {
  if (!wgrad_frag_has_lds(nt_w, kt_w)) return false;
  if (variant != 0) return variant == 2;
  static const int env = [] {
    const char* e = std::getenv("RSDL_WGRAD_LDS");
    return (e != nullptr && (e[0] == '0' || e[0] == '1') && e[1] == '\0')
               ? e[0] - '0'
               : -1;
  }();
  if (env >= 0) return env == 1;
  if (sched) return false;
  if (nt_w == 2) return RSDL_WGRAD_LDS_DEFAULT_DW1 != 0;
  return (K >= 512 ? RSDL_WGRAD_LDS_DEFAULT_DW2
                   : RSDL_WGRAD_LDS_DEFAULT_DW3) != 0;
}

void launch_wgrad_frag(const void* AT, const void* BT, float* dW, int32_t N,
                       int32_t K, int64_t mchunks, int32_t nt_w,
                       int32_t kt_w, int32_t variant, hipStream_t stream) {
  const int32_t nblk_n = N / (nt_w * 128);
  const int32_t nblk_k = K / (kt_w * 32);
  const int32_t nblk = nblk_n * nblk_k;
  // Workgroup-count target: more slabs = more stream parallelism but a
  // bigger partial buffer to reduce. Measured optima at the flagship
  // shapes (profiles/PERF.md). RSDL_WGRAD_WGS overrides for tuning.
  int64_t target = frag_target(K, nt_w);
  int64_t nslabs = (target + nblk - 1) / nblk;
  if (nslabs > mchunks) nslabs = mchunks;
  const int64_t chunks_per_slab = (mchunks + nslabs - 1) / nslabs;
  // re-derive so every slab is non-empty (partial rows must all be
  // written; there is no zero-init)
  nslabs = (mchunks + chunks_per_slab - 1) / chunks_per_slab;
  static bool linear = std::getenv("RSDL_WGRAD_LINEAR") != nullptr;
  // Pinned-schedule variant (see WF_FENCE above); flip on for A/B runs.
  static bool sched = [] {
    const char* e = std::getenv("RSDL_WGRAD_SCHED");
    return e && e[0] == '1';
  }();
  const int64_t grid =
      linear ? nslabs * nblk : ((nslabs + 7) / 8) * 8 * nblk;
  const int32_t nb_n = linear ? -nblk_n : nblk_n;
  if (wgrad_use_lds(variant, K, nt_w, kt_w, sched)) {
    auto kern = nt_w == 2 ? wgrad_lds_kernel<2, 4> : wgrad_lds_kernel<1, 8>;
    hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(256), 0, stream,
                       reinterpret_cast<const short*>(AT),
                       reinterpret_cast<const short*>(BT), dW, N, K, mchunks,
                       nb_n, nblk_k, nslabs, chunks_per_slab);
  } else if (nt_w == 2 && kt_w == 4) {
    auto kern = sched ? wgrad_frag_kernel<2, 4, 2, 1>
                      : wgrad_frag_kernel<2, 4>;
    hipLaunchKernelGGL(kern, dim3((uint32_t)grid),
                       dim3(256), 0, stream,
                       reinterpret_cast<const short*>(AT),
                       reinterpret_cast<const short*>(BT), dW, N, K, mchunks,
                       nb_n, nblk_k, nslabs, chunks_per_slab);
  } else if (nt_w == 1 && kt_w == 8) {
    auto kern = sched ? wgrad_frag_kernel<1, 8, 2, 1>
                      : wgrad_frag_kernel<1, 8>;
    hipLaunchKernelGGL(kern, dim3((uint32_t)grid),
                       dim3(256), 0, stream,
                       reinterpret_cast<const short*>(AT),
                       reinterpret_cast<const short*>(BT), dW, N, K, mchunks,
                       nb_n, nblk_k, nslabs, chunks_per_slab);
  } else if (nt_w == 1 && kt_w == 4) {
    // Small-tile config (RSDL_WGRAD_SMALL_TILES): 64 acc regs -> 3
    // waves/SIMD, and NT_W+KT_W<=6 takes the depth-3 fenced loop when
    // RSDL_WGRAD_SCHED is also set.
    auto kern = sched ? wgrad_frag_kernel<1, 4, 3, 1>
                      : wgrad_frag_kernel<1, 4, 3>;
    hipLaunchKernelGGL(kern, dim3((uint32_t)grid),
                       dim3(256), 0, stream,
                       reinterpret_cast<const short*>(AT),
                       reinterpret_cast<const short*>(BT), dW, N, K, mchunks,
                       nb_n, nblk_k, nslabs, chunks_per_slab);
  }
}

// ---------------------------------------------------------------------
// Grouped launch of the step's three wgrads (wgrad_grouped_kernel).
// ---------------------------------------------------------------------

// Slab targets of dW1, dW2, dW3. Their workgroups (x2, x4, x1 output
// blocks per slab: 144 + 288 + 80) sum to the 512 the chip holds at once,
// and every workgroup gets about the same number of chunks. The default
// is the split measured shortest at the flagship shape (profiles/PERF.md,
// round 11); RSDL_WGRAD_GROUP_SLABS=ns1,ns2,ns3 (read once) overrides it
// for tuning. The partition depends on mchunks and this knob only.
#ifndef RSDL_WGRAD_GROUP_SLABS_DEFAULT
#define RSDL_WGRAD_GROUP_SLABS_DEFAULT {72, 72, 80}
#endif
constexpr int64_t kGroupSlabsMax = 4096;

// Whether fused_step_bf16 takes the grouped launch at wgrad_variant 0:
// RSDL_WGRAD_GROUPED (0 or 1, read once) if set, else this default. Any of
// the tuning knobs of the separate launches keeps the step on them.
#ifndef RSDL_WGRAD_GROUPED_DEFAULT
#define RSDL_WGRAD_GROUPED_DEFAULT 1
#endif

static const int64_t* grouped_targets() {
  static const struct T {
    int64_t v[3] = RSDL_WGRAD_GROUP_SLABS_DEFAULT;
    T() {
      const char* e = std::getenv("RSDL_WGRAD_GROUP_SLABS");
      if (e == nullptr) return;
      long long a = 0, b = 0, c = 0;
      char tail = 0;
      if (std::sscanf(e, "%lld,%lld,%lld%c", &a, &b, &c, &tail) != 3) return;
      if (a < 1 || b < 1 || c < 1 || a > kGroupSlabsMax ||
          b > kGroupSlabsMax || c > kGroupSlabsMax) {
        return;
      }
      v[0] = a, v[1] = b, v[2] = c;
    }
  } t;
  return t.v;
}

// The slab rule of launch_wgrad_frag: no slab is empty.
static void grouped_slabs(int64_t target, int64_t mchunks, int64_t* nslabs,
                          int64_t* cps) {
  int64_t ns = target < mchunks ? target : mchunks;
  *cps = (mchunks + ns - 1) / ns;
  *nslabs = (mchunks + *cps - 1) / *cps;
}

WgradGroupedSlabs wgrad_grouped_nslabs(int64_t mchunks) {
  WgradGroupedSlabs r{};
  int64_t cps;
  for (int i = 0; i < 3; i++) {
    grouped_slabs(grouped_targets()[i], mchunks, &r.ns[i], &cps);
  }
  return r;
}

bool wgrad_grouped_default() {
  static const bool on = [] {
    for (const char* k : {"RSDL_WGRAD_SMALL_TILES", "RSDL_WGRAD_SCHED",
                          "RSDL_WGRAD_LINEAR", "RSDL_WGRAD_WGS",
                          "RSDL_WGRAD_LDS"}) {
      if (std::getenv(k) != nullptr) return false;
    }
    const char* e = std::getenv("RSDL_WGRAD_GROUPED");
    if (e != nullptr && (e[0] == '0' || e[0] == '1') && e[1] == '\0') {
      return e[0] == '1';
    }
    return RSDL_WGRAD_GROUPED_DEFAULT != 0;
  }();
  return on;
}

WgradGroupedSlabs launch_wgrad_grouped(const void* AT1, const void* BT1,
                                       float* part1, const void* AT2,
                                       const void* BT2, float* part2,
                                       const void* AT3, const void* BT3,
                                       float* part3, int64_t mchunks,
                                       hipStream_t stream) {
  // dW1 [512,128] <2,4>; dW2 [256,512] <1,8>; dW3 [128,256] <1,8>
  static const int32_t shp[3][4] = {
      {512, 128, 2, 4}, {256, 512, 1, 8}, {128, 256, 1, 8}};
  const void* at[3] = {AT1, AT2, AT3};
  const void* bt[3] = {BT1, BT2, BT3};
  float* part[3] = {part1, part2, part3};
  WgradGroupedArgs g{};
  WgradGroupedSlabs r{};
  uint32_t grid = 0;
  for (int i = 0; i < 3; i++) {
    WgradProblem& p = g.p[i];
    p.AT = reinterpret_cast<const short*>(at[i]);
    p.BT = reinterpret_cast<const short*>(bt[i]);
    p.part = part[i];
    p.N = shp[i][0];
    p.K = shp[i][1];
    p.mchunks = mchunks;
    p.nblk_n = p.N / (shp[i][2] * 128);
    p.nblk_k = p.K / (shp[i][3] * 32);
    grouped_slabs(grouped_targets()[i], mchunks, &p.nslabs,
                  &p.chunks_per_slab);
    r.ns[i] = p.nslabs;
    g.start[i] = grid;
    // slab count rounded up to the 8 XCDs: the surplus workgroups return
    grid += (uint32_t)(((p.nslabs + 7) / 8) * 8 * p.nblk_n * p.nblk_k);
  }
  hipLaunchKernelGGL(wgrad_grouped_kernel, dim3(grid), dim3(256), 0, stream,
                     g);
  return r;
}

}  // namespace rsdl
