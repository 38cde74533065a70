// Fused multi-table embedding lookup for MI355X (gfx950): the categorical
// half of the reference DATA_SPEC (19 int64 columns -> EmbeddingMLP).
//
//   forward   out[b, t*D:(t+1)*D] = bf16(W_t[max(idx_t[b], 0) % card_t])
//   backward  dW_t[r] = sum over {b : i_t[b] = r} of dOut[b, t*D:(t+1)*D]
//
// embed_concat_fwd: one launch for every table. The output row is T*D*2
// bytes; it is cut into 16-byte pieces and consecutive lanes take
// consecutive pieces of consecutive rows, so a wave's store is one
// contiguous 1 KB block. Piece p of a row belongs to table p / (D/8): the
// lane reads that table's index through (base, stride) - the loader hands
// out strided column views of its packed row block - wraps it, loads 32 B
// of fp32, rounds to nearest-even and stores 8 bf16. The D/8 lanes of one
// (row, table) read the same index. The wrapped index is kept as int32
// [B, T] for the backward.
//
// The backward has no float atomics and a fixed summation order, in two
// regimes picked per table by the caller.
//
// embed_bwd_onehot (small tables): dW_t = onehot(i_t)^T . dOut_t is a
// [card x B] . [B x D] product and runs on the matrix cores. Grid (table,
// batch slab). A workgroup stages its slab once: the wrapped indices as
// int32 [S] and the dOut slice TRANSPOSED as bf16 [D][S + 8], so the batch
// axis - the MFMA's K - is contiguous and a B fragment is one ds_read_b128.
// A wave then owns groups of four 32-row tiles of the table: per 16 batch
// rows it reads 8 indices and one B fragment, builds the four one-hot A
// fragments in registers (index == row ? 1.0 : 0 in bf16) and issues four
// v_mfma_f32_32x32x16_bf16 into fp32 accumulators. 1.0 * g is exact, so
// the MFMA contributes only the fp32 accumulation. Every slab writes one
// fp32 partial [card_pad, D]; embed_bwd_fold sums the slabs in ascending
// order. A 3-row table costs what a 128-row one does: there is no
// same-address traffic at all.
//   Fragment maps (csrc/wgrad_kernel.hip): A[m = lane&31][k = (lane>>5)*8+j],
//   B[k = (lane>>5)*8+j][n = lane&31], D col = lane&31,
//   row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
//   LDS: rows of the transposed slice are (S+8)*2 bytes apart = S/2 + 4
//   dwords, so at S = 1024 the 16 lanes of a B-fragment read start 4 banks
//   apart and cover the 64 banks once.
//   D = 64 and 128: the product is cut into 32-column slices on a third
//   grid axis, grid (table, batch slab, D/32). Workgroup z stages the slab's
//   indices and only its slice, bf16 [32][S + 8], read in 64-byte row
//   segments at column t*D + z*32, runs the same wave loop and writes the
//   columns z*32 .. z*32 + 31 of the slab's [card_pad, D] partial. LDS
//   footprint, bank pattern and the slab cap of 512 rows are those of
//   D = 32, and the partials grow with D, not with D^2 as they would with a
//   slab of 16384 / D rows. Every slice builds the one-hot fragments again.
//
// embed_bwd_runs (large tables): the caller sorts the keys (flat gradient
// row of every (table, batch row)) with a stable sort; D/4 lanes take each
// position, the ones at the head of a run of equal keys walk it in order -
// ascending batch row - gather the 2*D-byte dOut segments and store the
// fp32 row once.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "embed.h"

namespace rsdl {

// The packed fp32 forms are kept out of these kernels (a device-side target
// feature; the host pass does not know it).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(EMBED_ALLOW_PACKED_FP32)
#define EMBED_KERNEL \
  __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define EMBED_KERNEL __global__
#endif

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short em_bf16x8;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float em_f32x16;

#define EM_THREADS 256

__device__ __forceinline__ uint32_t em_bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ float em_bf16_f32(uint32_t h) {
  return __uint_as_float(h << 16);
}

template <int D>
EMBED_KERNEL void __launch_bounds__(EM_THREADS)
    embed_concat_fwd_kernel(const EmbedFwdArgs a, uint4* __restrict__ out,
                            int32_t* __restrict__ widx, int64_t B,
                            int32_t T) {
  constexpr uint32_t PPT = D / 8;  // pieces per table
  const uint32_t P = (uint32_t)T * PPT;
  // One 64-bit division per workgroup, 32-bit ones per lane.
  const int64_t start = (int64_t)blockIdx.x * EM_THREADS;
  const int64_t row0 = start / P;
  const uint32_t q = (uint32_t)(start - row0 * P) + threadIdx.x;
  const int64_t row = row0 + q / P;
  if (row >= B) return;
  const uint32_t piece = q % P;
  const uint32_t t = piece / PPT;
  const uint32_t part = piece % PPT;

  int64_t v = a.idx[t][row * a.stride[t]];
  v = v < 0 ? 0 : v;
  const uint32_t card = (uint32_t)a.card[t];
  const uint32_t i = ((uint64_t)v >> 32)
                         ? (uint32_t)((uint64_t)v % (uint64_t)card)
                         : (uint32_t)v % card;
  const float4* w =
      reinterpret_cast<const float4*>(a.W[t] + (int64_t)i * D + part * 8);
  const float4 lo = w[0];
  const float4 hi = w[1];
  uint4 o;
  o.x = em_bf16_rne(lo.x) | (em_bf16_rne(lo.y) << 16);
  o.y = em_bf16_rne(lo.z) | (em_bf16_rne(lo.w) << 16);
  o.z = em_bf16_rne(hi.x) | (em_bf16_rne(hi.y) << 16);
  o.w = em_bf16_rne(hi.z) | (em_bf16_rne(hi.w) << 16);
  out[start + threadIdx.x] = o;
  if (widx != nullptr && part == 0) widx[row * T + t] = (int32_t)i;
}

template <int D>
EMBED_KERNEL void __launch_bounds__(EM_THREADS)
    embed_bwd_onehot_kernel(const EmbedBwdArgs a,
                            const int32_t* __restrict__ widx,
                            const uint16_t* __restrict__ dout,
                            float* __restrict__ part, int64_t B, int32_t T,
                            int32_t S) {
  // Columns this workgroup stages and multiplies: all D up to 32, else the
  // 32-column slice blockIdx.z. W = D and z = 0 leave the narrow widths
  // what they were.
  constexpr int W = D < 32 ? D : 32;
  constexpr int PPT = W / 8;
  static_assert(D % W == 0, "whole column slices");
  extern __shared__ __attribute__((aligned(16))) uint8_t em_smem[];
  int32_t* sidx = reinterpret_cast<int32_t*>(em_smem);            // [S]
  uint16_t* sg = reinterpret_cast<uint16_t*>(em_smem + S * 4);    // [W][LS]
  const int32_t LS = S + 8;

  const int32_t e = blockIdx.x;
  const int32_t slab = blockIdx.y;
  const int32_t c0 = D > 32 ? (int32_t)blockIdx.z * W : 0;  // first column
  const int32_t tid = threadIdx.x;
  const int32_t t = a.t[e];
  const int32_t card = a.card[e];
  const int64_t b0 = (int64_t)slab * S;
  const int32_t nb = (int32_t)((B - b0) < S ? (B - b0) : S);
  const int32_t TD = T * D;

  // Rows past the batch match no table row (-1) and carry zeros.
  for (int32_t i = tid; i < S; i += EM_THREADS) {
    sidx[i] = i < nb ? widx[(b0 + i) * T + t] : -1;
  }
  for (int32_t i = tid; i < S * PPT; i += EM_THREADS) {
    const int32_t r = i / PPT;
    const int32_t p = i % PPT;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (r < nb) {
      v = *reinterpret_cast<const uint4*>(
          &dout[(b0 + r) * TD + t * D + c0 + p * 8]);
    }
    uint16_t* col = &sg[(p * 8) * LS + r];
    col[0 * LS] = (uint16_t)v.x;
    col[1 * LS] = (uint16_t)(v.x >> 16);
    col[2 * LS] = (uint16_t)v.y;
    col[3 * LS] = (uint16_t)(v.y >> 16);
    col[4 * LS] = (uint16_t)v.z;
    col[5 * LS] = (uint16_t)(v.z >> 16);
    col[6 * LS] = (uint16_t)v.w;
    col[7 * LS] = (uint16_t)(v.w >> 16);
  }
  __syncthreads();

  const int32_t wave = tid >> 6;
  const int32_t lane = tid & 63;
  const int32_t n = lane & 31;
  const int32_t kh = (lane >> 5) * 8;
  const int32_t ntiles = (card + 31) >> 5;
  const int32_t kend = (nb + 15) & ~15;
  float* my_part =
      part + a.part_off[e] + (int64_t)slab * ntiles * 32 * D;

  for (int32_t g = wave; g * 4 < ntiles; g += EM_THREADS / 64) {
    em_f32x16 acc[4];
    #pragma unroll
    for (int tt = 0; tt < 4; tt++) {
      #pragma unroll
      for (int r = 0; r < 16; r++) acc[tt][r] = 0.f;
    }
    const int32_t live = ntiles - g * 4;  // tiles of this group, >= 1
    const int32_t rbase = g * 128 + n;
    for (int32_t k0 = 0; k0 < kend; k0 += 16) {
      const int4 i0 = *reinterpret_cast<const int4*>(&sidx[k0 + kh]);
      const int4 i1 = *reinterpret_cast<const int4*>(&sidx[k0 + kh + 4]);
      em_bf16x8 bfr = {0, 0, 0, 0, 0, 0, 0, 0};
      if (n < W) {
        bfr = *reinterpret_cast<const em_bf16x8*>(&sg[n * LS + k0 + kh]);
      }
      const int32_t d[8] = {i0.x - rbase, i0.y - rbase, i0.z - rbase,
                            i0.w - rbase, i1.x - rbase, i1.y - rbase,
                            i1.z - rbase, i1.w - rbase};
      #pragma unroll
      for (int tt = 0; tt < 4; tt++) {
        if (tt < live) {
          em_bf16x8 afr;
          #pragma unroll
          for (int j = 0; j < 8; j++) {
            afr[j] = d[j] == tt * 32 ? (short)0x3f80 : (short)0;
          }
          acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr, bfr, acc[tt],
                                                            0, 0, 0);
        }
      }
    }
    #pragma unroll
    for (int tt = 0; tt < 4; tt++) {
      if (tt < live && n < W) {
        #pragma unroll
        for (int reg = 0; reg < 16; reg++) {
          const int32_t row = g * 128 + tt * 32 + (reg & 3) + 8 * (reg >> 2) +
                              4 * (lane >> 5);
          my_part[(int64_t)row * D + c0 + n] = acc[tt][reg];
        }
      }
    }
  }
}

// grad rows of entry e = its slabs' partials summed in ascending slab order.
template <int D>
EMBED_KERNEL void __launch_bounds__(EM_THREADS)
    embed_bwd_fold_kernel(const EmbedBwdArgs a, const float* __restrict__ part,
                          float* __restrict__ grad, int32_t nslab) {
  const int32_t e = blockIdx.y;
  const int32_t card = a.card[e];
  const int32_t n4 = card * (D / 4);
  const int32_t i = blockIdx.x * EM_THREADS + threadIdx.x;
  if (i >= n4) return;
  const int64_t stride4 = (int64_t)((card + 31) & ~31) * (D / 4);
  const float4* p = reinterpret_cast<const float4*>(part + a.part_off[e]) + i;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  #pragma unroll 8
  for (int32_t sl = 0; sl < nslab; sl++) {
    const float4 v = p[sl * stride4];
    s.x += v.x;
    s.y += v.y;
    s.z += v.z;
    s.w += v.w;
  }
  reinterpret_cast<float4*>(grad + a.row_off[e] * D)[i] = s;
}

template <int D>
EMBED_KERNEL void __launch_bounds__(EM_THREADS)
    embed_bwd_runs_kernel(const EmbedBwdArgs a,
                          const int32_t* __restrict__ keys,
                          const int64_t* __restrict__ pos,
                          const uint16_t* __restrict__ dout,
                          float* __restrict__ grad, int64_t N, int64_t B,
                          int32_t T) {
  constexpr int G = D / 4;  // lanes per position, one float4 each
  const int64_t gid = (int64_t)blockIdx.x * EM_THREADS + threadIdx.x;
  const int64_t p = gid / G;
  const int32_t l = (int32_t)(gid % G);
  if (p >= N) return;
  const int32_t key = keys[p];
  if (p > 0 && keys[p - 1] == key) return;  // not the head of a run
  // A run lies inside one table: one division for all of it.
  const int64_t e = pos[p] / B;
  const int64_t base = e * B;
  const int64_t TD = (int64_t)T * D;
  const uint16_t* src = dout + a.t[e] * D + l * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t q = p; q < N && keys[q] == key; q++) {
    const int64_t b = pos[q] - base;
    const uint2 g = *reinterpret_cast<const uint2*>(&src[b * TD]);
    s.x += em_bf16_f32(g.x & 0xffffu);
    s.y += em_bf16_f32(g.x >> 16);
    s.z += em_bf16_f32(g.y & 0xffffu);
    s.w += em_bf16_f32(g.y >> 16);
  }
  *reinterpret_cast<float4*>(&grad[(int64_t)key * D + l * 4]) = s;
}

#define EMBED_BY_WIDTH(D, CALL) \
  switch (D) {                  \
    case 8: { CALL(8); break; } \
    case 16: { CALL(16); break; } \
    case 64: { CALL(64); break; } \
    case 128: { CALL(128); break; } \
    default: { CALL(32); break; } \
  }

void launch_embed_concat_fwd(const EmbedFwdArgs& a, void* out, int32_t* widx,
                             int64_t B, int32_t T, int32_t D,
                             hipStream_t stream) {
  const int64_t pieces = B * T * (D / 8);
  const uint32_t grid = (uint32_t)((pieces + EM_THREADS - 1) / EM_THREADS);
#define EM_FWD(W)                                                        \
  hipLaunchKernelGGL(embed_concat_fwd_kernel<W>, dim3(grid),             \
                     dim3(EM_THREADS), 0, stream, a,                     \
                     reinterpret_cast<uint4*>(out), widx, B, T)
  EMBED_BY_WIDTH(D, EM_FWD)
#undef EM_FWD
}

void launch_embed_bwd_onehot(const EmbedBwdArgs& a, int32_t n,
                             const int32_t* widx, const void* dout,
                             float* part, float* grad, int64_t B, int32_t T,
                             int32_t D, int32_t S, int32_t nslab,
                             int32_t nslice, int32_t max_card,
                             hipStream_t stream) {
  const size_t lds = (size_t)S * 4 + (size_t)(D / nslice) * (S + 8) * 2;
  const uint32_t fold_x =
      (uint32_t)((max_card * (D / 4) + EM_THREADS - 1) / EM_THREADS);
#define EM_ONEHOT(W)                                                      \
  hipLaunchKernelGGL(embed_bwd_onehot_kernel<W>, dim3(n, nslab, nslice),  \
                     dim3(EM_THREADS), lds, stream, a, widx,              \
                     reinterpret_cast<const uint16_t*>(dout), part, B, T, \
                     S);                                                  \
  hipLaunchKernelGGL(embed_bwd_fold_kernel<W>, dim3(fold_x, n),           \
                     dim3(EM_THREADS), 0, stream, a, part, grad, nslab)
  EMBED_BY_WIDTH(D, EM_ONEHOT)
#undef EM_ONEHOT
}

void launch_embed_onehot_partials(const EmbedBwdArgs& a, int32_t n,
                                  const int32_t* widx, const void* dout,
                                  float* part, int64_t B, int32_t T,
                                  int32_t D, int32_t S, int32_t nslab,
                                  int32_t nslice, hipStream_t stream) {
  const size_t lds = (size_t)S * 4 + (size_t)(D / nslice) * (S + 8) * 2;
#define EM_PARTIALS(W)                                                    \
  hipLaunchKernelGGL(embed_bwd_onehot_kernel<W>, dim3(n, nslab, nslice),  \
                     dim3(EM_THREADS), lds, stream, a, widx,              \
                     reinterpret_cast<const uint16_t*>(dout), part, B, T, \
                     S)
  EMBED_BY_WIDTH(D, EM_PARTIALS)
#undef EM_PARTIALS
}

void launch_embed_bwd_runs(const EmbedBwdArgs& a, const int32_t* keys,
                           const int64_t* pos, const void* dout, float* grad,
                           int64_t N, int64_t B, int32_t T, int32_t D,
                           hipStream_t stream) {
  const int64_t threads = N * (D / 4);
  const uint32_t grid = (uint32_t)((threads + EM_THREADS - 1) / EM_THREADS);
#define EM_RUNS(W)                                                         \
  hipLaunchKernelGGL(embed_bwd_runs_kernel<W>, dim3(grid),                 \
                     dim3(EM_THREADS), 0, stream, a, keys, pos,            \
                     reinterpret_cast<const uint16_t*>(dout), grad, N, B, T)
  EMBED_BY_WIDTH(D, EM_RUNS)
#undef EM_RUNS
}

}  // namespace rsdl
