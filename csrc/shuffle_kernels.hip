// MI355X (gfx950, CDNA4) shuffle kernels.
//
// These are the native replacements for the reference's pandas/numpy hot ops
// (reference: ray_shuffling_data_loader/shuffle.py:156-194 random assignment +
// mask-partition + concat + sample(frac=1); torch_dataset.py:204-236 column
// cast/pack):
//
//   * gather_rows_u4     — full row permutation of a packed row-major byte
//                          matrix (the reducer-side `sample(frac=1)` +
//                          implicit `pd.concat`, fused into ONE gather pass).
//   * unpack_permute     — fused gather-permute + per-column cast + pack of
//                          packed rows into contiguous per-column torch
//                          tensors (the `convert_to_tensor` replacement).
//   * pack_columns       — inverse: per-column cast + interleave into packed
//                          rows (map-side, feeds the RCCL all-to-all).
//
// Design notes (see /opt/skills/guides/cdna_hip_programming.md):
//   - All three are memory-bound; the job is coalescing + enough waves in
//     flight to hide HBM latency (~900 cyc misses on the random-row gathers).
//   - Rows are padded to 16 B (Schema.row_stride), so row copies are uint4
//     (dwordx4) moves: 16 B/lane/instruction.
//   - Writes are always coalesced (consecutive lanes -> consecutive output
//     addresses); reads on the permuted side are row-random but contiguous
//     within a row, which the L2/L3 absorb at dataset-shard scale.
//   - Grids are sized ≫ 256 workgroups so all 8 XCDs fill; the default
//     blockIdx -> data mapping already round-robins XCDs (block b runs on
//     XCD b%8), which spreads the random-gather traffic across all 8 L2s.
//   - Wave width 64 is assumed (gfx950); no warp-32 idioms.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>

#include <cstdint>

#define RSDL_MAX_COLS 128

namespace rsdl {

// ---------------------------------------------------------------------------
// gather_rows: dst[i][:] = src[perm[i]][:], row_stride multiple of 16 B.
// One uint4 (16 B) per thread; consecutive threads cover one row then the
// next, so global stores are perfectly coalesced and loads are contiguous
// segments of row_stride bytes at a random row base.
// ---------------------------------------------------------------------------
__global__ void gather_rows_u4_kernel(
    const uint4* __restrict__ src,
    uint4* __restrict__ dst,
    const int64_t* __restrict__ perm,
    int64_t n_rows,
    int64_t row_u4) {
  const int64_t total = n_rows * row_u4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const int64_t row = i / row_u4;
    const int64_t j = i - row * row_u4;
    dst[i] = src[perm[row] * row_u4 + j];
  }
}

// Identity-permutation variant (pure packed copy, used for the exchange
// staging path): dst[i] = src[sel[i]] with sel given as 32-bit indices.
__global__ void gather_rows_u4_idx32_kernel(
    const uint4* __restrict__ src,
    uint4* __restrict__ dst,
    const int32_t* __restrict__ perm,
    int64_t n_rows,
    int64_t row_u4) {
  const int64_t total = n_rows * row_u4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const int64_t row = i / row_u4;
    const int64_t j = i - row * row_u4;
    dst[i] = src[(int64_t)perm[row] * row_u4 + j];
  }
}

// ---------------------------------------------------------------------------
// Fused unpack+permute+cast and pack+cast.
//
// Column descriptors are passed as a kernel argument struct (lands in
// scalar registers / constant memory — no extra global loads).
// ---------------------------------------------------------------------------

enum DType : int32_t {
  DT_F32 = 0,
  DT_F64 = 1,
  DT_I32 = 2,
  DT_I64 = 3,
  DT_F16 = 4,
  DT_BF16 = 5,
  DT_U8 = 6,
};

struct ColDesc {
  int64_t col_ptr;     // device pointer to the contiguous column tensor
  int32_t packed_off;  // byte offset of this column inside a packed row
  int32_t src_dtype;   // dtype inside the packed row
  int32_t dst_dtype;   // dtype of the column tensor
  int32_t numel;       // elements per row for this column
};

struct ColTable {
  ColDesc cols[RSDL_MAX_COLS];
};

template <typename S, typename D>
__device__ __forceinline__ D cast_elem(S v) {
  return (D)v;
}
template <>
__device__ __forceinline__ __hip_bfloat16 cast_elem(float v) {
  return __float2bfloat16(v);
}
// ONE rounding, double -> bf16. Written as __float2bfloat16((float)v) this
// always compiled to the same thing (the compiler folds two adjacent
// truncations into one), so the bits are what they were; spelling it out
// keeps them from depending on whether the two casts stay adjacent in a
// caller. It differs from rounding to fp32 first only where the fp32 value
// is a bf16 tie (about 2^-17 of random inputs). The standardized paths do
// round to fp32 first: affine_f32 returns a float by definition.
template <>
__device__ __forceinline__ __hip_bfloat16 cast_elem(double v) {
  return __double2bfloat16(v);
}
template <>
__device__ __forceinline__ __hip_bfloat16 cast_elem(int32_t v) {
  return __float2bfloat16((float)v);
}
template <>
__device__ __forceinline__ __hip_bfloat16 cast_elem(int64_t v) {
  return __float2bfloat16((float)v);
}
template <>
__device__ __forceinline__ float cast_elem(__hip_bfloat16 v) {
  return __bfloat162float(v);
}
template <>
__device__ __forceinline__ double cast_elem(__hip_bfloat16 v) {
  return (double)__bfloat162float(v);
}

// Vectorized unpack specializations for the hot flagship combos: the
// feature-matrix column is (f32 -> f32) or (f32 -> bf16) with numel % 4 == 0
// and a 16-B-aligned packed offset, so each lane moves one float4 (16 B
// load) instead of four scalar dwords. ~2x on the fused unpack
// (profiles/microbench: scalar 2.6 TB/s vs gather roofline 4.8 TB/s).
__device__ __forceinline__ void unpack_vec4_f32_f32(
    const uint8_t* __restrict__ packed, int64_t row_stride,
    const int64_t* __restrict__ perm, float* __restrict__ dst,
    int32_t packed_off, int32_t numel, int64_t n_rows, int64_t tid,
    int64_t nthreads) {
  const int32_t groups = numel >> 2;
  const int64_t total = n_rows * groups;
  for (int64_t i = tid; i < total; i += nthreads) {
    const int64_t row = i / groups;
    const int64_t g = i - row * groups;
    const int64_t srow = perm ? perm[row] : row;
    const float4 v = *reinterpret_cast<const float4*>(
        packed + srow * row_stride + packed_off + (g << 4));
    *reinterpret_cast<float4*>(dst + row * numel + (g << 2)) = v;
  }
}

__device__ __forceinline__ void unpack_vec4_f32_bf16(
    const uint8_t* __restrict__ packed, int64_t row_stride,
    const int64_t* __restrict__ perm, __hip_bfloat16* __restrict__ dst,
    int32_t packed_off, int32_t numel, int64_t n_rows, int64_t tid,
    int64_t nthreads) {
  const int32_t groups = numel >> 2;
  const int64_t total = n_rows * groups;
  for (int64_t i = tid; i < total; i += nthreads) {
    const int64_t row = i / groups;
    const int64_t g = i - row * groups;
    const int64_t srow = perm ? perm[row] : row;
    const float4 v = *reinterpret_cast<const float4*>(
        packed + srow * row_stride + packed_off + (g << 4));
    union {
      __hip_bfloat16 h[4];
      uint2 u;
    } o;
    o.h[0] = __float2bfloat16(v.x);
    o.h[1] = __float2bfloat16(v.y);
    o.h[2] = __float2bfloat16(v.z);
    o.h[3] = __float2bfloat16(v.w);
    *reinterpret_cast<uint2*>(dst + row * numel + (g << 2)) = o.u;
  }
}

// Unpack direction: column[i*numel + e] = cast(packed[perm[i]*stride + off +
// e*sizeof(S)]). Writes coalesced; reads random-row.
template <typename S, typename D>
__device__ void unpack_col_loop(
    const uint8_t* __restrict__ packed,
    int64_t row_stride,
    const int64_t* __restrict__ perm,
    D* __restrict__ dst,
    int32_t packed_off,
    int32_t numel,
    int64_t n_rows,
    int64_t tid,
    int64_t nthreads) {
  const int64_t total = n_rows * numel;
  for (int64_t i = tid; i < total; i += nthreads) {
    const int64_t row = i / numel;
    const int64_t e = i - row * numel;
    const int64_t srow = perm ? perm[row] : row;
    const S* sp = reinterpret_cast<const S*>(
        packed + srow * row_stride + packed_off);
    dst[i] = cast_elem<S, D>(sp[e]);
  }
}

// Pack direction: packed[perm[i]*stride + off + e] = cast(column[i*numel+e])
// (perm==null => packed[i*...]). Reads coalesced; writes strided by row.
template <typename S, typename D>
__device__ void pack_col_loop(
    uint8_t* __restrict__ packed,
    int64_t row_stride,
    const int64_t* __restrict__ perm,
    const S* __restrict__ src,
    int32_t packed_off,
    int32_t numel,
    int64_t n_rows,
    int64_t tid,
    int64_t nthreads) {
  const int64_t total = n_rows * numel;
  for (int64_t i = tid; i < total; i += nthreads) {
    const int64_t row = i / numel;
    const int64_t e = i - row * numel;
    const int64_t drow = perm ? perm[row] : row;
    D* dp = reinterpret_cast<D*>(packed + drow * row_stride + packed_off);
    dp[e] = cast_elem<S, D>(src[i]);
  }
}

// Same-dtype column (src_dtype == dst_dtype): a byte copy, whatever the
// dtype — this is how bf16/f16 columns of a narrowed source block (see
// narrow_rows_kernel) are unpacked. Every address is base + row * pitch +
// j * sizeof(V), so V may be as wide as the two bases, the two pitches and
// the column's byte width all prove, and no wider. The flagship narrow row
// (200 B of bf16 features at offset 8 of a 208-B row -> a 200-B pitch
// matrix) proves 8 B: 25 lanes per row.
template <typename V>
__device__ __forceinline__ void copy_col_loop(
    const uint8_t* __restrict__ src, int64_t src_pitch,
    const int64_t* __restrict__ perm, uint8_t* __restrict__ dst,
    int64_t dst_pitch, int32_t col_bytes, int64_t n_rows, int64_t tid,
    int64_t nthreads) {
  const int32_t lanes = col_bytes / (int32_t)sizeof(V);
  const int64_t total = n_rows * lanes;
  for (int64_t i = tid; i < total; i += nthreads) {
    const int64_t row = i / lanes;
    const int64_t j = i - row * lanes;
    const int64_t srow = perm ? perm[row] : row;
    const V v = *reinterpret_cast<const V*>(
        src + srow * src_pitch + j * (int64_t)sizeof(V));
    *reinterpret_cast<V*>(dst + row * dst_pitch + j * (int64_t)sizeof(V)) = v;
  }
}

__device__ __forceinline__ void copy_col(
    const uint8_t* __restrict__ src, int64_t src_pitch,
    const int64_t* __restrict__ perm, uint8_t* __restrict__ dst,
    int64_t dst_pitch, int32_t col_bytes, int64_t n_rows, int64_t tid,
    int64_t nthreads) {
  const uintptr_t m = reinterpret_cast<uintptr_t>(src) |
                      reinterpret_cast<uintptr_t>(dst) |
                      (uintptr_t)src_pitch | (uintptr_t)dst_pitch |
                      (uintptr_t)col_bytes;
  if ((m & 15) == 0)
    copy_col_loop<uint4>(src, src_pitch, perm, dst, dst_pitch, col_bytes,
                         n_rows, tid, nthreads);
  else if ((m & 7) == 0)
    copy_col_loop<uint2>(src, src_pitch, perm, dst, dst_pitch, col_bytes,
                         n_rows, tid, nthreads);
  else if ((m & 3) == 0)
    copy_col_loop<uint32_t>(src, src_pitch, perm, dst, dst_pitch, col_bytes,
                            n_rows, tid, nthreads);
  else if ((m & 1) == 0)
    copy_col_loop<uint16_t>(src, src_pitch, perm, dst, dst_pitch, col_bytes,
                            n_rows, tid, nthreads);
  else
    copy_col_loop<uint8_t>(src, src_pitch, perm, dst, dst_pitch, col_bytes,
                           n_rows, tid, nthreads);
}

__device__ __forceinline__ int32_t dtype_size(int32_t dt) {
  switch (dt) {
    case DT_F64: case DT_I64: return 8;
    case DT_F32: case DT_I32: return 4;
    case DT_F16: case DT_BF16: return 2;
    default: return 1;
  }
}

#define RSDL_DISPATCH_DST(S_CTYPE, SRC_DT, DST_DT, CALL)                   \
  switch (DST_DT) {                                                        \
    case DT_F32: { using D = float; CALL; break; }                         \
    case DT_F64: { using D = double; CALL; break; }                        \
    case DT_I32: { using D = int32_t; CALL; break; }                       \
    case DT_I64: { using D = int64_t; CALL; break; }                       \
    case DT_BF16: { using D = __hip_bfloat16; CALL; break; }               \
    default: break;                                                        \
  }

#define RSDL_DISPATCH_PAIR(SRC_DT, DST_DT, CALL)                           \
  switch (SRC_DT) {                                                        \
    case DT_F32: { using S = float; RSDL_DISPATCH_DST(float, SRC_DT,       \
                   DST_DT, CALL); break; }                                 \
    case DT_F64: { using S = double; RSDL_DISPATCH_DST(double, SRC_DT,     \
                   DST_DT, CALL); break; }                                 \
    case DT_I32: { using S = int32_t; RSDL_DISPATCH_DST(int32_t, SRC_DT,   \
                   DST_DT, CALL); break; }                                 \
    case DT_I64: { using S = int64_t; RSDL_DISPATCH_DST(int64_t, SRC_DT,   \
                   DST_DT, CALL); break; }                                 \
    default: break;                                                        \
  }

// Work is partitioned by column via blockIdx.y; blockIdx.x strides within a
// column. Columns have very different sizes, but the grid-stride loop keeps
// all blocks busy until their column is finished; with >=1024 blocks per
// column the chip stays full.
__global__ void unpack_permute_kernel(
    const uint8_t* __restrict__ packed,
    int64_t row_stride,
    const int64_t* __restrict__ perm,
    ColTable table,
    int32_t num_cols,
    int64_t n_rows) {
  const int32_t c = blockIdx.y;
  if (c >= num_cols) return;
  const ColDesc d = table.cols[c];
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  // Hot-path vector specializations (flagship feature matrix).
  if (d.src_dtype == DT_F32 && (d.numel & 3) == 0 &&
      (d.packed_off & 15) == 0) {
    if (d.dst_dtype == DT_F32) {
      unpack_vec4_f32_f32(packed, row_stride, perm,
                          reinterpret_cast<float*>(d.col_ptr), d.packed_off,
                          d.numel, n_rows, tid, nthreads);
      return;
    }
    if (d.dst_dtype == DT_BF16) {
      unpack_vec4_f32_bf16(packed, row_stride, perm,
                           reinterpret_cast<__hip_bfloat16*>(d.col_ptr),
                           d.packed_off, d.numel, n_rows, tid, nthreads);
      return;
    }
  }
  if (d.src_dtype == d.dst_dtype) {
    const int32_t col_bytes = d.numel * dtype_size(d.src_dtype);
    copy_col(packed + d.packed_off, row_stride, perm,
             reinterpret_cast<uint8_t*>(d.col_ptr), col_bytes, col_bytes,
             n_rows, tid, nthreads);
    return;
  }
  RSDL_DISPATCH_PAIR(
      d.src_dtype, d.dst_dtype,
      (unpack_col_loop<S, D>(packed, row_stride, perm,
                             reinterpret_cast<D*>(d.col_ptr), d.packed_off,
                             d.numel, n_rows, tid, nthreads)));
}

// Row-major sweep for a block whose columns are all same-dtype copies made
// of whole 8-B lanes (the narrowed source block): one pass over the rows
// serves every column, as gather_rows does, so a narrow scalar column (the
// 8-B label) does not fetch the sectors of its row a second time in a pass
// of its own. Lane j of a row belongs to the column whose [lane0, lane0 +
// lanes) holds it; lanes in no column (padding) are skipped.
#define RSDL_SWEEP_MAX_COLS 8

struct SweepCol {
  int64_t col_ptr;  // contiguous column tensor, 8-B aligned
  int32_t lane0;    // packed offset / 8
  int32_t lanes;    // column bytes per row / 8
};

struct SweepTable {
  SweepCol cols[RSDL_SWEEP_MAX_COLS];
};

__global__ void unpack_rows_sweep_kernel(
    const uint2* __restrict__ packed,
    int64_t row_u2,  // row stride in 8-B lanes
    const int64_t* __restrict__ perm,
    SweepTable table,
    int32_t num_cols,
    int32_t lanes_per_row,  // lanes up to the end of the last column
    int64_t n_rows) {
  const int64_t total = n_rows * lanes_per_row;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const int64_t row = i / lanes_per_row;
    const int32_t j = (int32_t)(i - row * lanes_per_row);
    const int64_t srow = perm ? perm[row] : row;
#pragma unroll
    for (int32_t c = 0; c < RSDL_SWEEP_MAX_COLS; ++c) {
      if (c < num_cols) {
        const SweepCol d = table.cols[c];
        const int32_t k = j - d.lane0;
        if ((uint32_t)k < (uint32_t)d.lanes) {
          reinterpret_cast<uint2*>(d.col_ptr)[row * d.lanes + k] =
              packed[srow * row_u2 + j];
        }
      }
    }
  }
}

__global__ void pack_columns_kernel(
    uint8_t* __restrict__ packed,
    int64_t row_stride,
    const int64_t* __restrict__ perm,
    ColTable table,
    int32_t num_cols,
    int64_t n_rows) {
  const int32_t c = blockIdx.y;
  if (c >= num_cols) return;
  const ColDesc d = table.cols[c];
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  // A 2-B or 1-B column (f16, bf16, u8) that keeps its dtype is outside the
  // cast dispatch: its elements move as bit patterns, as copy_col moves
  // them on the unpack side. The host refuses every other pair the
  // dispatch does not know (check_col_pair in shuffle_ops.cpp).
  if (d.src_dtype == d.dst_dtype && d.src_dtype >= DT_F16) {
    if (dtype_size(d.src_dtype) == 2)
      pack_col_loop<uint16_t, uint16_t>(
          packed, row_stride, perm,
          reinterpret_cast<const uint16_t*>(d.col_ptr), d.packed_off,
          d.numel, n_rows, tid, nthreads);
    else
      pack_col_loop<uint8_t, uint8_t>(
          packed, row_stride, perm,
          reinterpret_cast<const uint8_t*>(d.col_ptr), d.packed_off,
          d.numel, n_rows, tid, nthreads);
    return;
  }
  RSDL_DISPATCH_PAIR(
      d.dst_dtype, d.src_dtype,
      (pack_col_loop<S, D>(packed, row_stride, perm,
                           reinterpret_cast<const S*>(d.col_ptr),
                           d.packed_off, d.numel, n_rows, tid, nthreads)));
}

// ---------------------------------------------------------------------------
// Radix partition by destination id (replaces torch argsort+bincount on the
// map side; reference shuffle.py:156-161 boolean-mask loop). Three phases:
//   1. per-block LDS histogram of dest ids -> block_counts[B][T]
//   2. exclusive scan on host side (tiny [B,T] tensor, torch cumsum)
//   3. rank+scatter: per-block LDS running counters assign each row its
//      output slot; writes the GATHER permutation (perm[dst] = src row),
//      which then drives the roofline-speed gather_rows kernel.
// Within-destination order is block-local-nondeterministic, which is fine:
// a full random permutation is applied downstream either way.
// ---------------------------------------------------------------------------

#define RSDL_PART_MAX_DESTS 1024

__global__ void partition_hist_kernel(
    const int32_t* __restrict__ dest,
    int32_t* __restrict__ block_counts,  // [gridDim.x][num_dests]
    int64_t n,
    int32_t num_dests) {
  extern __shared__ int32_t lds_counts[];
  for (int32_t d = threadIdx.x; d < num_dests; d += blockDim.x)
    lds_counts[d] = 0;
  __syncthreads();
  const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = min(lo + chunk, n);
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
    atomicAdd(&lds_counts[dest[i]], 1);
  __syncthreads();
  for (int32_t d = threadIdx.x; d < num_dests; d += blockDim.x)
    block_counts[(int64_t)blockIdx.x * num_dests + d] = lds_counts[d];
}

__global__ void partition_scatter_kernel(
    const int32_t* __restrict__ dest,
    const int32_t* __restrict__ block_base,  // [gridDim.x][num_dests]
    int32_t* __restrict__ perm_out,          // [n] gather indices
    int64_t n,
    int32_t num_dests) {
  extern __shared__ int32_t lds_next[];
  for (int32_t d = threadIdx.x; d < num_dests; d += blockDim.x)
    lds_next[d] = block_base[(int64_t)blockIdx.x * num_dests + d];
  __syncthreads();
  const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = min(lo + chunk, n);
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const int32_t pos = atomicAdd(&lds_next[dest[i]], 1);
    perm_out[pos] = (int32_t)i;
  }
}

// ---------------------------------------------------------------------------
// Tiled pack for the map side: C scalar/vector columns -> packed rows.
// The naive per-element kernel stores 4-8 B at row_stride intervals
// (~0.5 TB/s); this one stages a TILE_R-row tile in LDS (per-column
// coalesced loads, conflict-spread by the padded row stride) and then
// streams the tile out as one contiguous row-major block (16-B lanes,
// perfectly coalesced).
// ---------------------------------------------------------------------------

__global__ void pack_tiled_kernel(
    uint8_t* __restrict__ packed,
    int64_t row_stride,
    ColTable table,
    int32_t num_cols,
    int64_t n_rows,
    int32_t tile_rows,
    int32_t n8) {  // n8 >= 0: fast path; first n8 columns are 8-B scalars,
                   // the rest 4-B scalars, no casts. n8 < 0: generic path.
  extern __shared__ uint8_t lds_tile[];  // [tile_rows][lds_stride]
  // +8 B pad keeps 8-B column alignment inside LDS and makes the dword
  // stride ≡ 2 (mod 4): per-column lane strides cover 16 of 32 banks
  // (gcd=2 -> at worst 2-way, which is free for ds_write_b32).
  const int64_t lds_stride = row_stride + 8;
  const int64_t row0 = (int64_t)blockIdx.x * tile_rows;
  const int32_t rows_here =
      (int32_t)min((int64_t)tile_rows, n_rows - row0);
  if (rows_here <= 0) return;

  if (n8 >= 0) {
    // Fast phase 1: column plan staged in LDS-adjacent static shared
    // memory; flat (column-major) element loop, no per-element dispatch.
    // Loads are perfectly coalesced (consecutive lanes -> consecutive rows
    // of one column); each wave stays within one column.
    __shared__ int64_t s_ptr[RSDL_MAX_COLS];
    __shared__ int32_t s_off[RSDL_MAX_COLS];
    for (int32_t c = threadIdx.x; c < num_cols; c += blockDim.x) {
      s_ptr[c] = table.cols[c].col_ptr;
      s_off[c] = table.cols[c].packed_off;
    }
    __syncthreads();
    const int64_t total8 = (int64_t)rows_here * n8;
    for (int64_t t = threadIdx.x; t < total8; t += blockDim.x) {
      const int32_t c = (int32_t)(t / rows_here);
      const int32_t r = (int32_t)(t - (int64_t)c * rows_here);
      const uint64_t v =
          reinterpret_cast<const uint64_t*>(s_ptr[c])[row0 + r];
      *reinterpret_cast<uint64_t*>(
          lds_tile + (int64_t)r * lds_stride + s_off[c]) = v;
    }
    const int32_t n4 = num_cols - n8;
    const int64_t total4 = (int64_t)rows_here * n4;
    for (int64_t t = threadIdx.x; t < total4; t += blockDim.x) {
      const int32_t c = n8 + (int32_t)(t / rows_here);
      const int32_t r = (int32_t)(t - (int64_t)(c - n8) * rows_here);
      const uint32_t v =
          reinterpret_cast<const uint32_t*>(s_ptr[c])[row0 + r];
      *reinterpret_cast<uint32_t*>(
          lds_tile + (int64_t)r * lds_stride + s_off[c]) = v;
    }
  } else {
    // Generic phase 1: per-column loop with dtype-cast dispatch.
    for (int32_t c = 0; c < num_cols; ++c) {
      const ColDesc d = table.cols[c];
      const int64_t elems = (int64_t)rows_here * d.numel;
      if (d.src_dtype == d.dst_dtype && d.src_dtype >= DT_F16) {
        // Same-dtype f16 / bf16 / u8: a bit copy (see pack_columns_kernel).
        const bool two = dtype_size(d.src_dtype) == 2;
        for (int64_t t = threadIdx.x; t < elems; t += blockDim.x) {
          const int32_t r = (int32_t)(t / d.numel);
          const int32_t e = (int32_t)(t - (int64_t)r * d.numel);
          uint8_t* dst_base =
              lds_tile + (int64_t)r * lds_stride + d.packed_off;
          if (two)
            reinterpret_cast<uint16_t*>(dst_base)[e] =
                reinterpret_cast<const uint16_t*>(
                    d.col_ptr)[row0 * d.numel + t];
          else
            dst_base[e] = reinterpret_cast<const uint8_t*>(
                d.col_ptr)[row0 * d.numel + t];
        }
        continue;
      }
      for (int64_t t = threadIdx.x; t < elems; t += blockDim.x) {
        const int32_t r = (int32_t)(t / d.numel);
        const int32_t e = (int32_t)(t - (int64_t)r * d.numel);
        uint8_t* dst_base = lds_tile + (int64_t)r * lds_stride + d.packed_off;
        RSDL_DISPATCH_PAIR(
            d.dst_dtype, d.src_dtype,
            (reinterpret_cast<D*>(dst_base)[e] = cast_elem<S, D>(
                 reinterpret_cast<const S*>(d.col_ptr)[row0 * d.numel + t])));
      }
    }
  }
  __syncthreads();

  // Phase 2: stream the tile to global as contiguous row-major dwords
  // (consecutive lanes -> consecutive banks and fully coalesced stores;
  // the padded LDS stride rules out 16-B-aligned reads).
  const int64_t row_dw = row_stride >> 2;
  const int64_t lds_stride_dw = lds_stride >> 2;
  const int64_t total_dw = (int64_t)rows_here * row_dw;
  uint32_t* gout = reinterpret_cast<uint32_t*>(packed + row0 * row_stride);
  const uint32_t* lin = reinterpret_cast<const uint32_t*>(lds_tile);
  for (int64_t t = threadIdx.x; t < total_dw; t += blockDim.x) {
    const int64_t r = t / row_dw;
    const int64_t o = t - r * row_dw;
    gout[t] = lin[r * lds_stride_dw + o];
  }
}

// ---------------------------------------------------------------------------
// Host-side launchers (called from shuffle_ops.cpp).
// ---------------------------------------------------------------------------

void launch_partition_hist(
    const int32_t* dest, int32_t* block_counts, int64_t n,
    int32_t num_dests, int32_t num_blocks, hipStream_t stream) {
  hipLaunchKernelGGL(partition_hist_kernel, dim3(num_blocks), dim3(256),
                     num_dests * sizeof(int32_t), stream, dest, block_counts,
                     n, num_dests);
}

void launch_partition_scatter(
    const int32_t* dest, const int32_t* block_base, int32_t* perm_out,
    int64_t n, int32_t num_dests, int32_t num_blocks, hipStream_t stream) {
  hipLaunchKernelGGL(partition_scatter_kernel, dim3(num_blocks), dim3(256),
                     num_dests * sizeof(int32_t), stream, dest, block_base,
                     perm_out, n, num_dests);
}

void launch_pack_tiled(
    void* packed, int64_t row_stride, const ColTable& table,
    int32_t num_cols, int64_t n_rows, int32_t tile_rows, int64_t lds_bytes,
    int32_t n8, hipStream_t stream) {
  const int64_t blocks = (n_rows + tile_rows - 1) / tile_rows;
  hipLaunchKernelGGL(pack_tiled_kernel, dim3((uint32_t)blocks), dim3(256),
                     (uint32_t)lds_bytes, stream,
                     reinterpret_cast<uint8_t*>(packed), row_stride, table,
                     num_cols, n_rows, tile_rows, n8);
}

void launch_gather_rows(
    const void* src, void* dst, const int64_t* perm, int64_t n_rows,
    int64_t row_bytes, hipStream_t stream) {
  const int64_t row_u4 = row_bytes / 16;
  const int64_t total = n_rows * row_u4;
  const int threads = 256;
  int64_t blocks = (total + threads - 1) / threads;
  if (blocks > 65535 * 16) blocks = 65535 * 16;  // grid-stride covers rest
  hipLaunchKernelGGL(gather_rows_u4_kernel, dim3((uint32_t)blocks),
                     dim3(threads), 0, stream,
                     reinterpret_cast<const uint4*>(src),
                     reinterpret_cast<uint4*>(dst), perm, n_rows, row_u4);
}

void launch_gather_rows_idx32(
    const void* src, void* dst, const int32_t* perm, int64_t n_rows,
    int64_t row_bytes, hipStream_t stream) {
  const int64_t row_u4 = row_bytes / 16;
  const int64_t total = n_rows * row_u4;
  const int threads = 256;
  int64_t blocks = (total + threads - 1) / threads;
  if (blocks > 65535 * 16) blocks = 65535 * 16;
  hipLaunchKernelGGL(gather_rows_u4_idx32_kernel, dim3((uint32_t)blocks),
                     dim3(threads), 0, stream,
                     reinterpret_cast<const uint4*>(src),
                     reinterpret_cast<uint4*>(dst), perm, n_rows, row_u4);
}

void launch_unpack_permute(
    const void* packed, int64_t row_stride, const int64_t* perm,
    const ColTable& table, int32_t num_cols, int64_t n_rows,
    hipStream_t stream) {
  const int threads = 256;
  // ~4096 blocks per column keeps 256 CUs busy even for a single column.
  int64_t bx = (n_rows + threads - 1) / threads;
  if (bx > 4096) bx = 4096;
  if (bx < 1) bx = 1;
  dim3 grid((uint32_t)bx, (uint32_t)num_cols);
  hipLaunchKernelGGL(unpack_permute_kernel, grid, dim3(threads), 0, stream,
                     reinterpret_cast<const uint8_t*>(packed), row_stride,
                     perm, table, num_cols, n_rows);
}

void launch_pack_columns(
    void* packed, int64_t row_stride, const int64_t* perm,
    const ColTable& table, int32_t num_cols, int64_t n_rows,
    hipStream_t stream) {
  const int threads = 256;
  int64_t bx = (n_rows + threads - 1) / threads;
  if (bx > 4096) bx = 4096;
  if (bx < 1) bx = 1;
  dim3 grid((uint32_t)bx, (uint32_t)num_cols);
  hipLaunchKernelGGL(pack_columns_kernel, grid, dim3(threads), 0, stream,
                     reinterpret_cast<uint8_t*>(packed), row_stride, perm,
                     table, num_cols, n_rows);
}

// ---------------------------------------------------------------------------
// Feature standardization (opt-in, ShuffleEngine(normalize=...)).
//
//   * column_stats_kernel   — the FIT: one read-only pass over the packed
//                             source block, per-element (count, Σ(x-p),
//                             Σ(x-p)²) in fp64 about a pivot p (the first
//                             finite value of the element, row 0 as a rule).
//   * unpack_permute_affine — the APPLY: the fused unpack with
//                             y = cast((float)((double(x) - shift) * scale))
//                             evaluated in fp64 BEFORE the narrowing cast.
//
// The fit must be bitwise reproducible (a resumed job has to rebuild the
// same batches), so there are no float atomics anywhere: a fixed grid, each
// block owns a contiguous row slab and writes ONE partial per element to a
// [blocks, elems] slab, and a second tiny kernel folds the slab in block
// order. Every reduction (lane tree, wave order, block order) is fixed by
// the launch shape alone.
// ---------------------------------------------------------------------------

#define RSDL_STATS_THREADS 256
#define RSDL_STATS_WAVES (RSDL_STATS_THREADS / 64)
// Columns at least this wide put lanes across the elements of a row
// (coalesced along the row, no cross-lane reduction); narrower ones put
// lanes across rows.
#define RSDL_STATS_WIDE 64

struct StatsCol {
  int32_t packed_off;  // byte offset of the column inside a packed row
  int32_t src_dtype;   // dtype inside the packed row
  int32_t numel;       // elements per row
  int32_t elem_base;   // index of element 0 in the flat [elems] outputs
};

struct StatsTable {
  StatsCol cols[RSDL_MAX_COLS];
};

__device__ __forceinline__ bool finite_f64(double v) {
  // Bit test: independent of any fast-math treatment of isfinite().
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

__device__ __forceinline__ bool isnan_f64(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
}

// Element e of a column in source row `row`, widened to double.
__device__ __forceinline__ double load_as_f64(
    const uint8_t* __restrict__ packed, int64_t row_stride, int64_t row,
    int32_t packed_off, int32_t src_dtype, int32_t e) {
  const uint8_t* p = packed + row * row_stride + packed_off;
  switch (src_dtype) {
    case DT_F64: return reinterpret_cast<const double*>(p)[e];
    case DT_F32: return (double)reinterpret_cast<const float*>(p)[e];
    case DT_I64: return (double)reinterpret_cast<const int64_t*>(p)[e];
    default: return (double)reinterpret_cast<const int32_t*>(p)[e];
  }
}

// Pivot of one element: its first finite value among the leading
// RSDL_STATS_PIVOT_ROWS rows (row 0 whenever that is finite), else 0.0. A
// pivot near the data keeps Σ(x-p)² - (Σ(x-p))²/n from cancelling; falling
// straight back to 0.0 on a NaN in row 0 would give that up for a
// `1e9 + noise` column. Every block derives the same pivot (cached reads).
#define RSDL_STATS_PIVOT_ROWS 64

__device__ __forceinline__ double stats_pivot(
    const uint8_t* __restrict__ packed, int64_t row_stride, int64_t n_rows,
    int32_t packed_off, int32_t src_dtype, int32_t e) {
  const int64_t lim = min(n_rows, (int64_t)RSDL_STATS_PIVOT_ROWS);
  for (int64_t r = 0; r < lim; ++r) {
    const double v =
        load_as_f64(packed, row_stride, r, packed_off, src_dtype, e);
    if (finite_f64(v)) return v;
  }
  return 0.0;
}

struct StatsAcc {
  double s;
  double ss;
  int32_t n;  // a block's slab is far below 2^31 rows
};

__device__ __forceinline__ void stats_add(StatsAcc& a, double x, double p) {
  if (finite_f64(x)) {
    const double d = x - p;
    a.s += d;
    a.ss += d * d;
    a.n += 1;
  }
}

__global__ __launch_bounds__(RSDL_STATS_THREADS) void column_stats_kernel(
    const uint8_t* __restrict__ packed,
    int64_t row_stride,
    int64_t n_rows,
    StatsTable table,
    int32_t num_cols,
    int32_t total_elems,
    int64_t* __restrict__ part_n,    // [gridDim.x][total_elems]
    double* __restrict__ part_s,     // [gridDim.x][total_elems]
    double* __restrict__ part_ss,    // [gridDim.x][total_elems]
    double* __restrict__ pivot_out)  // [total_elems]
{
  __shared__ double lds_s[RSDL_STATS_WAVES][64];
  __shared__ double lds_ss[RSDL_STATS_WAVES][64];
  __shared__ int32_t lds_n[RSDL_STATS_WAVES][64];

  const int32_t lane = threadIdx.x & 63;
  const int32_t wave = threadIdx.x >> 6;
  // Contiguous row slab of this block (may be empty for trailing blocks).
  const int64_t chunk = (n_rows + gridDim.x - 1) / gridDim.x;
  const int64_t lo = min((int64_t)blockIdx.x * chunk, n_rows);
  const int64_t hi = min(lo + chunk, n_rows);
  const int64_t out_base = (int64_t)blockIdx.x * total_elems;

  for (int32_t c = 0; c < num_cols; ++c) {
    const StatsCol d = table.cols[c];
    if (d.numel >= RSDL_STATS_WIDE) {
      // Lanes across the elements of a row, one wave per row; 64-element
      // chunks of the row are taken in turn so the accumulators stay in
      // registers whatever the column width.
      for (int32_t e0 = 0; e0 < d.numel; e0 += 64) {
        const int32_t e = e0 + lane;
        const bool live = e < d.numel;
        double p = 0.0;
        if (live) {
          p = stats_pivot(packed, row_stride, n_rows, d.packed_off,
                          d.src_dtype, e);
        }
        StatsAcc a{0.0, 0.0, 0};
        if (live) {
          int64_t r = lo + wave;
          // 4 independent row loads in flight per wave.
          for (; r + 3 * RSDL_STATS_WAVES < hi; r += 4 * RSDL_STATS_WAVES) {
            const double x0 = load_as_f64(packed, row_stride, r,
                                          d.packed_off, d.src_dtype, e);
            const double x1 = load_as_f64(
                packed, row_stride, r + RSDL_STATS_WAVES, d.packed_off,
                d.src_dtype, e);
            const double x2 = load_as_f64(
                packed, row_stride, r + 2 * RSDL_STATS_WAVES, d.packed_off,
                d.src_dtype, e);
            const double x3 = load_as_f64(
                packed, row_stride, r + 3 * RSDL_STATS_WAVES, d.packed_off,
                d.src_dtype, e);
            stats_add(a, x0, p);
            stats_add(a, x1, p);
            stats_add(a, x2, p);
            stats_add(a, x3, p);
          }
          for (; r < hi; r += RSDL_STATS_WAVES) {
            stats_add(a, load_as_f64(packed, row_stride, r, d.packed_off,
                                     d.src_dtype, e), p);
          }
        }
        lds_s[wave][lane] = a.s;
        lds_ss[wave][lane] = a.ss;
        lds_n[wave][lane] = a.n;
        __syncthreads();
        if (wave == 0 && live) {
          double s = lds_s[0][lane], ss = lds_ss[0][lane];
          int64_t n = lds_n[0][lane];
          for (int32_t w = 1; w < RSDL_STATS_WAVES; ++w) {  // fixed order
            s += lds_s[w][lane];
            ss += lds_ss[w][lane];
            n += lds_n[w][lane];
          }
          const int64_t o = out_base + d.elem_base + e;
          part_n[o] = n;
          part_s[o] = s;
          part_ss[o] = ss;
          if (blockIdx.x == 0) pivot_out[d.elem_base + e] = p;
        }
        __syncthreads();
      }
    } else {
      // Lanes across rows; fixed shuffle tree inside the wave, then the
      // waves in order through LDS.
      for (int32_t e = 0; e < d.numel; ++e) {
        const double p = stats_pivot(packed, row_stride, n_rows,
                                     d.packed_off, d.src_dtype, e);
        StatsAcc a{0.0, 0.0, 0};
        for (int64_t r = lo + threadIdx.x; r < hi; r += RSDL_STATS_THREADS) {
          stats_add(a, load_as_f64(packed, row_stride, r, d.packed_off,
                                   d.src_dtype, e), p);
        }
        for (int32_t off = 32; off > 0; off >>= 1) {
          a.s += __shfl_down(a.s, off, 64);
          a.ss += __shfl_down(a.ss, off, 64);
          a.n += __shfl_down(a.n, off, 64);
        }
        if (lane == 0) {
          lds_s[wave][0] = a.s;
          lds_ss[wave][0] = a.ss;
          lds_n[wave][0] = a.n;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
          double s = lds_s[0][0], ss = lds_ss[0][0];
          int64_t n = lds_n[0][0];
          for (int32_t w = 1; w < RSDL_STATS_WAVES; ++w) {  // fixed order
            s += lds_s[w][0];
            ss += lds_ss[w][0];
            n += lds_n[w][0];
          }
          const int64_t o = out_base + d.elem_base + e;
          part_n[o] = n;
          part_s[o] = s;
          part_ss[o] = ss;
          if (blockIdx.x == 0) pivot_out[d.elem_base + e] = p;
        }
        __syncthreads();
      }
    }
  }
}

// Fold the [blocks, elems] partial slab in block order: one thread per
// element, a serial fp64 sum (the slab is a few MB at most).
__global__ void column_stats_combine_kernel(
    const int64_t* __restrict__ part_n,
    const double* __restrict__ part_s,
    const double* __restrict__ part_ss,
    int32_t num_blocks,
    int32_t total_elems,
    int64_t* __restrict__ out_n,
    double* __restrict__ out_s,
    double* __restrict__ out_ss) {
  const int32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total_elems) return;
  int64_t n = 0;
  double s = 0.0, ss = 0.0;
  for (int32_t b = 0; b < num_blocks; ++b) {
    const int64_t o = (int64_t)b * total_elems + e;
    n += part_n[o];
    s += part_s[o];
    ss += part_ss[o];
  }
  out_n[e] = n;
  out_s[e] = s;
  out_ss[e] = ss;
}

// ----- apply ---------------------------------------------------------------

// Per-column index of element 0 in the interleaved (shift, scale) table, or
// -1 for a column that is not standardized (it takes the plain paths).
struct AffineBase {
  int32_t base[RSDL_MAX_COLS];
};

// The one place the affine arithmetic lives. Pinned fp64 subtract and
// multiply (no contraction, no reassociation), round-to-nearest to fp32;
// the caller applies the project's fp32 -> dst conversion.
__device__ __forceinline__ float affine_f32(double x, double2 a, bool fill,
                                            float fill_f) {
  if (fill && isnan_f64(x)) return fill_f;
  return (float)__dmul_rn(__dsub_rn(x, a.x), a.y);
}

template <typename D>
__device__ __forceinline__ void store4(D* dst, float y0, float y1, float y2,
                                       float y3);
template <>
__device__ __forceinline__ void store4<float>(float* dst, float y0, float y1,
                                              float y2, float y3) {
  *reinterpret_cast<float4*>(dst) = make_float4(y0, y1, y2, y3);
}
template <>
__device__ __forceinline__ void store4<__hip_bfloat16>(
    __hip_bfloat16* dst, float y0, float y1, float y2, float y3) {
  union {
    __hip_bfloat16 h[4];
    uint2 u;
  } o;
  o.h[0] = __float2bfloat16(y0);
  o.h[1] = __float2bfloat16(y1);
  o.h[2] = __float2bfloat16(y2);
  o.h[3] = __float2bfloat16(y3);
  *reinterpret_cast<uint2*>(dst) = o.u;
}

// f64 source, numel % 4 == 0: four elements per lane, packed 8-B (bf16) or
// 16-B (f32) stores. ALIGNED16: the element address is 16-B aligned, so the
// four doubles arrive as two 16-B loads; otherwise (e.g. the feature matrix
// behind an int64 key, offset 8) as four 8-B loads.
template <typename D, bool ALIGNED16>
__device__ __forceinline__ void unpack_affine_vec4_f64(
    const uint8_t* __restrict__ packed, int64_t row_stride,
    const int64_t* __restrict__ perm, D* __restrict__ dst,
    const double2* __restrict__ aff, int32_t packed_off, int32_t numel,
    int64_t n_rows, int64_t tid, int64_t nthreads, bool fill, float fill_f) {
  const int32_t groups = numel >> 2;
  const int64_t total = n_rows * groups;
  for (int64_t i = tid; i < total; i += nthreads) {
    const int64_t row = i / groups;
    const int64_t g = i - row * groups;
    const int64_t srow = perm ? perm[row] : row;
    const uint8_t* sp = packed + srow * row_stride + packed_off + (g << 5);
    double x0, x1, x2, x3;
    if (ALIGNED16) {
      const double2 v0 = reinterpret_cast<const double2*>(sp)[0];
      const double2 v1 = reinterpret_cast<const double2*>(sp)[1];
      x0 = v0.x; x1 = v0.y; x2 = v1.x; x3 = v1.y;
    } else {
      const double* dp = reinterpret_cast<const double*>(sp);
      x0 = dp[0]; x1 = dp[1]; x2 = dp[2]; x3 = dp[3];
    }
    const double2* ap = aff + (g << 2);
    store4<D>(dst + row * numel + (g << 2),
              affine_f32(x0, ap[0], fill, fill_f),
              affine_f32(x1, ap[1], fill, fill_f),
              affine_f32(x2, ap[2], fill, fill_f),
              affine_f32(x3, ap[3], fill, fill_f));
  }
}

// f32 source, numel % 4 == 0, 16-B-aligned element address: the float4
// pattern of the plain kernel.
template <typename D>
__device__ __forceinline__ void unpack_affine_vec4_f32(
    const uint8_t* __restrict__ packed, int64_t row_stride,
    const int64_t* __restrict__ perm, D* __restrict__ dst,
    const double2* __restrict__ aff, int32_t packed_off, int32_t numel,
    int64_t n_rows, int64_t tid, int64_t nthreads, bool fill, float fill_f) {
  const int32_t groups = numel >> 2;
  const int64_t total = n_rows * groups;
  for (int64_t i = tid; i < total; i += nthreads) {
    const int64_t row = i / groups;
    const int64_t g = i - row * groups;
    const int64_t srow = perm ? perm[row] : row;
    const float4 v = *reinterpret_cast<const float4*>(
        packed + srow * row_stride + packed_off + (g << 4));
    const double2* ap = aff + (g << 2);
    store4<D>(dst + row * numel + (g << 2),
              affine_f32((double)v.x, ap[0], fill, fill_f),
              affine_f32((double)v.y, ap[1], fill, fill_f),
              affine_f32((double)v.z, ap[2], fill, fill_f),
              affine_f32((double)v.w, ap[3], fill, fill_f));
  }
}

// Scalar generic path: any source dtype, any numel, any alignment.
template <typename S, typename D>
__device__ void unpack_affine_col_loop(
    const uint8_t* __restrict__ packed, int64_t row_stride,
    const int64_t* __restrict__ perm, D* __restrict__ dst,
    const double2* __restrict__ aff, int32_t packed_off, int32_t numel,
    int64_t n_rows, int64_t tid, int64_t nthreads, bool fill, float fill_f) {
  const int64_t total = n_rows * numel;
  for (int64_t i = tid; i < total; i += nthreads) {
    const int64_t row = i / numel;
    const int64_t e = i - row * numel;
    const int64_t srow = perm ? perm[row] : row;
    const S* sp = reinterpret_cast<const S*>(
        packed + srow * row_stride + packed_off);
    dst[i] = cast_elem<float, D>(
        affine_f32((double)sp[e], aff[e], fill, fill_f));
  }
}

// Same grid shape and column partitioning as unpack_permute_kernel; a
// column without a table entry runs exactly the plain code.
__global__ void unpack_permute_affine_kernel(
    const uint8_t* __restrict__ packed,
    int64_t row_stride,
    const int64_t* __restrict__ perm,
    ColTable table,
    AffineBase abase,
    const double2* __restrict__ aff_table,
    int32_t num_cols,
    int64_t n_rows,
    int32_t has_fill,
    float fill_f) {
  const int32_t c = blockIdx.y;
  if (c >= num_cols) return;
  const ColDesc d = table.cols[c];
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  // Alignment of element 0 of this column in row 0; row_stride is a
  // multiple of 16, so it holds for every row.
  const bool al16 =
      ((reinterpret_cast<uintptr_t>(packed) + (uintptr_t)d.packed_off) &
       15) == 0;
  const int32_t ab = abase.base[c];
  if (ab < 0) {
    // Not standardized: the plain kernel's paths, unchanged.
    if (d.src_dtype == DT_F32 && (d.numel & 3) == 0 &&
        (d.packed_off & 15) == 0) {
      if (d.dst_dtype == DT_F32) {
        unpack_vec4_f32_f32(packed, row_stride, perm,
                            reinterpret_cast<float*>(d.col_ptr),
                            d.packed_off, d.numel, n_rows, tid, nthreads);
        return;
      }
      if (d.dst_dtype == DT_BF16) {
        unpack_vec4_f32_bf16(packed, row_stride, perm,
                             reinterpret_cast<__hip_bfloat16*>(d.col_ptr),
                             d.packed_off, d.numel, n_rows, tid, nthreads);
        return;
      }
    }
    if (d.src_dtype == d.dst_dtype) {
      const int32_t col_bytes = d.numel * dtype_size(d.src_dtype);
      copy_col(packed + d.packed_off, row_stride, perm,
               reinterpret_cast<uint8_t*>(d.col_ptr), col_bytes, col_bytes,
               n_rows, tid, nthreads);
      return;
    }
    RSDL_DISPATCH_PAIR(
        d.src_dtype, d.dst_dtype,
        (unpack_col_loop<S, D>(packed, row_stride, perm,
                               reinterpret_cast<D*>(d.col_ptr),
                               d.packed_off, d.numel, n_rows, tid,
                               nthreads)));
    return;
  }
  const double2* aff = aff_table + ab;
  const bool fill = has_fill != 0;
  const bool vec_dst = d.dst_dtype == DT_F32 || d.dst_dtype == DT_BF16;
  if (vec_dst && (d.numel & 3) == 0 && d.src_dtype == DT_F64) {
    if (d.dst_dtype == DT_BF16) {
      __hip_bfloat16* o = reinterpret_cast<__hip_bfloat16*>(d.col_ptr);
      if (al16)
        unpack_affine_vec4_f64<__hip_bfloat16, true>(
            packed, row_stride, perm, o, aff, d.packed_off, d.numel, n_rows,
            tid, nthreads, fill, fill_f);
      else
        unpack_affine_vec4_f64<__hip_bfloat16, false>(
            packed, row_stride, perm, o, aff, d.packed_off, d.numel, n_rows,
            tid, nthreads, fill, fill_f);
    } else {
      float* o = reinterpret_cast<float*>(d.col_ptr);
      if (al16)
        unpack_affine_vec4_f64<float, true>(
            packed, row_stride, perm, o, aff, d.packed_off, d.numel, n_rows,
            tid, nthreads, fill, fill_f);
      else
        unpack_affine_vec4_f64<float, false>(
            packed, row_stride, perm, o, aff, d.packed_off, d.numel, n_rows,
            tid, nthreads, fill, fill_f);
    }
    return;
  }
  if (vec_dst && (d.numel & 3) == 0 && d.src_dtype == DT_F32 && al16) {
    if (d.dst_dtype == DT_BF16)
      unpack_affine_vec4_f32<__hip_bfloat16>(
          packed, row_stride, perm,
          reinterpret_cast<__hip_bfloat16*>(d.col_ptr), aff, d.packed_off,
          d.numel, n_rows, tid, nthreads, fill, fill_f);
    else
      unpack_affine_vec4_f32<float>(
          packed, row_stride, perm, reinterpret_cast<float*>(d.col_ptr),
          aff, d.packed_off, d.numel, n_rows, tid, nthreads, fill, fill_f);
    return;
  }
  RSDL_DISPATCH_PAIR(
      d.src_dtype, d.dst_dtype,
      (unpack_affine_col_loop<S, D>(packed, row_stride, perm,
                                    reinterpret_cast<D*>(d.col_ptr), aff,
                                    d.packed_off, d.numel, n_rows, tid,
                                    nthreads, fill, fill_f)));
}

// ---------------------------------------------------------------------------
// Narrowed source cache (ShuffleEngine, RSDL_NARROW_CACHE).
//
// The cast (and the affine) of the fused unpack is per element and the
// source block never changes, so cast(row[perm[i]]) every epoch equals
// cast(row)[perm[i]] with the cast done ONCE. narrow_rows_kernel converts
// the wide packed block to a packed block of the OUTPUT dtypes in identity
// row order; each epoch then unpacks the narrow block with plain same-dtype
// copies (copy_col / unpack_rows_sweep_kernel above). The arithmetic is the
// unpack kernels' own (affine_f32, cast_elem, store4), so the bits are too.
// ---------------------------------------------------------------------------

struct NarrowCol {
  int32_t src_off;    // byte offset inside a wide row
  int32_t dst_off;    // byte offset inside a narrow row
  int32_t src_dtype;
  int32_t dst_dtype;
  int32_t numel;
  int32_t aff_base;   // element 0 in the (shift, scale) table, or -1
};

struct NarrowTable {
  NarrowCol cols[RSDL_MAX_COLS];
};

// Four source elements of one lane. WIDE: 16-B loads (the address is 16-B
// aligned); otherwise 8-B loads (it is 8-B aligned).
template <typename S, bool WIDE>
__device__ __forceinline__ void load4(const uint8_t* __restrict__ sp,
                                      S (&x)[4]) {
  if constexpr (sizeof(S) == 8) {
    if constexpr (WIDE) {
      const double2 v0 = reinterpret_cast<const double2*>(sp)[0];
      const double2 v1 = reinterpret_cast<const double2*>(sp)[1];
      x[0] = v0.x; x[1] = v0.y; x[2] = v1.x; x[3] = v1.y;
    } else {
      const double* dp = reinterpret_cast<const double*>(sp);
      x[0] = dp[0]; x[1] = dp[1]; x[2] = dp[2]; x[3] = dp[3];
    }
  } else {
    if constexpr (WIDE) {
      const float4 v = *reinterpret_cast<const float4*>(sp);
      x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
      const float2 v0 = reinterpret_cast<const float2*>(sp)[0];
      const float2 v1 = reinterpret_cast<const float2*>(sp)[1];
      x[0] = v0.x; x[1] = v0.y; x[2] = v1.x; x[3] = v1.y;
    }
  }
}

// f64 / f32 source, f32 / bf16 destination, numel % 4 == 0: four elements
// per lane, one packed 8-B (bf16) or 16-B (f32) store. AFF: the affine and
// then the fp32 -> dst conversion, as unpack_affine_vec4_*; otherwise
// cast_elem<S, D> on the source element itself, as unpack_col_loop (the two
// are separate instantiations on purpose: a double -> bf16 cast must stay
// the single rounding it is there).
template <typename S, typename D, bool WIDE, bool AFF>
__device__ __forceinline__ void narrow_vec4_loop(
    const uint8_t* __restrict__ src, int64_t src_stride,
    uint8_t* __restrict__ dst, int64_t dst_stride,
    const double2* __restrict__ aff, int32_t numel, int64_t n_rows,
    int64_t tid, int64_t nthreads, bool fill, float fill_f) {
  const int32_t groups = numel >> 2;
  const int64_t total = n_rows * groups;
  for (int64_t i = tid; i < total; i += nthreads) {
    const int64_t row = i / groups;
    const int64_t g = i - row * groups;
    S x[4];
    load4<S, WIDE>(src + row * src_stride + g * (int64_t)(4 * sizeof(S)), x);
    D* dp = reinterpret_cast<D*>(dst + row * dst_stride) + (g << 2);
    if constexpr (AFF) {
      const double2* ap = aff + (g << 2);
      store4<D>(dp, affine_f32((double)x[0], ap[0], fill, fill_f),
                affine_f32((double)x[1], ap[1], fill, fill_f),
                affine_f32((double)x[2], ap[2], fill, fill_f),
                affine_f32((double)x[3], ap[3], fill, fill_f));
    } else {
      union {
        D h[4];
        uint32_t u[sizeof(D)];  // 4 * sizeof(D) bytes
      } o;
#pragma unroll
      for (int32_t k = 0; k < 4; ++k) o.h[k] = cast_elem<S, D>(x[k]);
      if constexpr (sizeof(D) == 2)
        *reinterpret_cast<uint2*>(dp) = make_uint2(o.u[0], o.u[1]);
      else
        *reinterpret_cast<uint4*>(dp) =
            make_uint4(o.u[0], o.u[1], o.u[2], o.u[3]);
    }
  }
}

template <typename S, typename D>
__device__ __forceinline__ void narrow_vec4(
    const uint8_t* __restrict__ src, int64_t src_stride,
    uint8_t* __restrict__ dst, int64_t dst_stride,
    const double2* __restrict__ aff, int32_t numel, int64_t n_rows,
    int64_t tid, int64_t nthreads, bool fill, float fill_f, bool wide) {
  if (aff != nullptr) {
    if (wide)
      narrow_vec4_loop<S, D, true, true>(src, src_stride, dst, dst_stride,
                                         aff, numel, n_rows, tid, nthreads,
                                         fill, fill_f);
    else
      narrow_vec4_loop<S, D, false, true>(src, src_stride, dst, dst_stride,
                                          aff, numel, n_rows, tid, nthreads,
                                          fill, fill_f);
  } else {
    if (wide)
      narrow_vec4_loop<S, D, true, false>(src, src_stride, dst, dst_stride,
                                          aff, numel, n_rows, tid, nthreads,
                                          fill, fill_f);
    else
      narrow_vec4_loop<S, D, false, false>(src, src_stride, dst, dst_stride,
                                           aff, numel, n_rows, tid, nthreads,
                                           fill, fill_f);
  }
}

// Scalar fallback: any supported dtype pair, any numel, any alignment.
template <typename S, typename D>
__device__ void narrow_col_loop(
    const uint8_t* __restrict__ src, int64_t src_stride,
    uint8_t* __restrict__ dst, int64_t dst_stride,
    const double2* __restrict__ aff, int32_t numel, int64_t n_rows,
    int64_t tid, int64_t nthreads, bool fill, float fill_f) {
  const int64_t total = n_rows * numel;
  for (int64_t i = tid; i < total; i += nthreads) {
    const int64_t row = i / numel;
    const int64_t e = i - row * numel;
    const S x = reinterpret_cast<const S*>(src + row * src_stride)[e];
    D* dp = reinterpret_cast<D*>(dst + row * dst_stride);
    if (aff != nullptr)
      dp[e] = cast_elem<float, D>(
          affine_f32((double)x, aff[e], fill, fill_f));
    else
      dp[e] = cast_elem<S, D>(x);
  }
}

// One launch over the whole block: blockIdx.y picks the column, as in the
// unpack kernels; the extra y == num_cols pass (launched only when the
// narrow row has padding) zeroes the padding bytes.
__global__ void narrow_rows_kernel(
    const uint8_t* __restrict__ src,
    int64_t src_stride,
    uint8_t* __restrict__ dst,
    int64_t dst_stride,
    NarrowTable table,
    const double2* __restrict__ aff_table,
    int32_t num_cols,
    int64_t n_rows,
    int32_t has_fill,
    float fill_f,
    int32_t pad_off) {  // first padding byte of a narrow row
  const int32_t c = blockIdx.y;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  if (c >= num_cols) {
    const int32_t pad = (int32_t)dst_stride - pad_off;
    const int64_t total = n_rows * pad;
    for (int64_t i = tid; i < total; i += nthreads) {
      const int64_t row = i / pad;
      dst[row * dst_stride + pad_off + (i - row * pad)] = 0;
    }
    return;
  }
  const NarrowCol d = table.cols[c];
  const uint8_t* sp = src + d.src_off;
  uint8_t* dp = dst + d.dst_off;
  if (d.src_dtype == d.dst_dtype && d.aff_base < 0) {
    // The dtype does not change: a byte copy.
    copy_col(sp, src_stride, nullptr, dp, dst_stride,
             d.numel * dtype_size(d.src_dtype), n_rows, tid, nthreads);
    return;
  }
  const double2* aff = d.aff_base < 0 ? nullptr : aff_table + d.aff_base;
  const bool fill = has_fill != 0;
  // Alignment of element 0 in row 0 of either side; both strides are
  // multiples of 16, so it holds for every row.
  const uintptr_t sa = reinterpret_cast<uintptr_t>(sp);
  const uintptr_t da = reinterpret_cast<uintptr_t>(dp);
  const bool vec_src = (d.src_dtype == DT_F64 || d.src_dtype == DT_F32) &&
                       (d.numel & 3) == 0 && (sa & 7) == 0;
  const bool wide = (sa & 15) == 0;
  if (vec_src && d.dst_dtype == DT_BF16 && (da & 7) == 0) {
    if (d.src_dtype == DT_F64)
      narrow_vec4<double, __hip_bfloat16>(sp, src_stride, dp, dst_stride, aff,
                                          d.numel, n_rows, tid, nthreads,
                                          fill, fill_f, wide);
    else
      narrow_vec4<float, __hip_bfloat16>(sp, src_stride, dp, dst_stride, aff,
                                         d.numel, n_rows, tid, nthreads,
                                         fill, fill_f, wide);
    return;
  }
  if (vec_src && d.dst_dtype == DT_F32 && (da & 15) == 0) {
    if (d.src_dtype == DT_F64)
      narrow_vec4<double, float>(sp, src_stride, dp, dst_stride, aff,
                                 d.numel, n_rows, tid, nthreads, fill,
                                 fill_f, wide);
    else
      narrow_vec4<float, float>(sp, src_stride, dp, dst_stride, aff, d.numel,
                                n_rows, tid, nthreads, fill, fill_f, wide);
    return;
  }
  RSDL_DISPATCH_PAIR(
      d.src_dtype, d.dst_dtype,
      (narrow_col_loop<S, D>(sp, src_stride, dp, dst_stride, aff, d.numel,
                             n_rows, tid, nthreads, fill, fill_f)));
}

void launch_narrow_rows(
    const void* src, int64_t src_stride, void* dst, int64_t dst_stride,
    const NarrowTable& table, const void* aff_table, int32_t num_cols,
    int64_t n_rows, int32_t has_fill, float fill_f, int32_t pad_off,
    hipStream_t stream) {
  const int threads = 256;
  int64_t bx = (n_rows + threads - 1) / threads;
  if (bx > 4096) bx = 4096;
  if (bx < 1) bx = 1;
  dim3 grid((uint32_t)bx,
            (uint32_t)(num_cols + (pad_off < dst_stride ? 1 : 0)));
  hipLaunchKernelGGL(narrow_rows_kernel, grid, dim3(threads), 0, stream,
                     reinterpret_cast<const uint8_t*>(src), src_stride,
                     reinterpret_cast<uint8_t*>(dst), dst_stride, table,
                     reinterpret_cast<const double2*>(aff_table), num_cols,
                     n_rows, has_fill, fill_f, pad_off);
}

void launch_unpack_rows_sweep(
    const void* packed, int64_t row_stride, const int64_t* perm,
    const SweepTable& table, int32_t num_cols, int32_t lanes_per_row,
    int64_t n_rows, hipStream_t stream) {
  const int64_t total = n_rows * lanes_per_row;
  const int threads = 256;
  int64_t blocks = (total + threads - 1) / threads;
  if (blocks > 65535 * 16) blocks = 65535 * 16;  // grid-stride covers rest
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(unpack_rows_sweep_kernel, dim3((uint32_t)blocks),
                     dim3(threads), 0, stream,
                     reinterpret_cast<const uint2*>(packed), row_stride / 8,
                     perm, table, num_cols, lanes_per_row, n_rows);
}

void launch_column_stats(
    const void* packed, int64_t row_stride, int64_t n_rows,
    const StatsTable& table, int32_t num_cols, int32_t total_elems,
    int32_t num_blocks, int64_t* part_n, double* part_s, double* part_ss,
    double* pivot, int64_t* out_n, double* out_s, double* out_ss,
    hipStream_t stream) {
  hipLaunchKernelGGL(column_stats_kernel, dim3(num_blocks),
                     dim3(RSDL_STATS_THREADS), 0, stream,
                     reinterpret_cast<const uint8_t*>(packed), row_stride,
                     n_rows, table, num_cols, total_elems, part_n, part_s,
                     part_ss, pivot);
  const int threads = 64;
  hipLaunchKernelGGL(column_stats_combine_kernel,
                     dim3((total_elems + threads - 1) / threads),
                     dim3(threads), 0, stream, part_n, part_s, part_ss,
                     num_blocks, total_elems, out_n, out_s, out_ss);
}

void launch_unpack_permute_affine(
    const void* packed, int64_t row_stride, const int64_t* perm,
    const ColTable& table, const AffineBase& abase, const void* aff_table,
    int32_t num_cols, int64_t n_rows, int32_t has_fill, float fill_f,
    hipStream_t stream) {
  const int threads = 256;
  int64_t bx = (n_rows + threads - 1) / threads;
  if (bx > 4096) bx = 4096;
  if (bx < 1) bx = 1;
  dim3 grid((uint32_t)bx, (uint32_t)num_cols);
  hipLaunchKernelGGL(unpack_permute_affine_kernel, grid, dim3(threads), 0,
                     stream, reinterpret_cast<const uint8_t*>(packed),
                     row_stride, perm, table, abase,
                     reinterpret_cast<const double2*>(aff_table), num_cols,
                     n_rows, has_fill, fill_f);
}

}  // namespace rsdl
