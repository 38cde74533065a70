// Sparse in-place optimizer update of the fused embedding tables for MI355X
// (gfx950): the rows a batch touched get their new weights (and optimizer
// state) straight from the gradient sum in registers. No dense gradient is
// ever written, and rows the batch did not touch are neither read nor
// written (large tables) or come out bit-identical (small tables).
//
//   sgd              p' = p - lr * g
//   adagrad          h' = h + g * g                       (per element)
//                    p' = p - lr * (g / (sqrt(h') + eps))
//   rowwise_adagrad  s_l = ((gx*gx + gy*gy) + gz*gz) + gw*gw   per lane
//                    s   = xor-butterfly sum of s_l over the row's
//                          G = D/4 lanes, distances 1 .. G/2 ascending
//                          (1, 2, 4 at D = 32; 1 .. 16 at D = 128)
//                    h' = h + s * (1/D)                   (one float per row)
//                    p' = p - lr * (g / (sqrt(h') + eps))
//
// One fp32 IEEE operation per line, contraction off (as csrc/step_glue.hip).
// g is the row's sum of dOut segments in the fixed order given below.
//
// Large tables. The caller's stable sort of the int32 keys (flat row of
// every (table, batch row)) is cut into fixed chunks of C = 16 positions,
// whatever the launch geometry.
//
// embed_runs_update (pass 1): D/4 lanes per chunk, one float4 of the row
// each. The group loads its 16 keys and 16 pos, then issues all 16 dOut
// gathers (8 B per lane) before the first add: their addresses depend on no
// key comparison, so 16 loads are in flight per group where the dense
// backward's run walk has one dependent load per iteration. It then walks
// the 16 positions in order and closes a segment at every key change. A run
// that begins and ends inside the chunk is complete: the group reads the
// row of W and its state, applies the update and stores both. A chunk has
// at most two open segments, a head (the run came in from the previous
// chunk; a segment that covers the whole chunk without beginning in it
// counts as one) and a tail (the run begins here and goes on into the next
// chunk). Each is written as an fp32 partial to carry[chunk][0 | 1][D];
// carry is not cleared, pass 2 reads only slots pass 1 wrote.
//
// embed_carry_update (pass 2): one lane group per chunk, which acts only if
// the chunk's tail opens a crossing run. It starts from that tail partial,
// adds the head partials of the following chunks in ascending order until
// the run ends (the run goes on past chunk c' iff keys[16 * (c' + 1)] is
// still its key) and applies the update once.
//
// The summation order of a row is therefore: ascending batch row inside a
// chunk, then chunks ascending.
//
// Small tables. embed_bwd_onehot_kernel (csrc/embed.hip) writes its slab
// partials as for the dense gradient; embed_fold_update has the grid and
// the ascending-slab sum of embed_bwd_fold and applies the update to every
// row of the table. A row no batch row names has g = +0 and comes out
// bit-identical under all three kinds (eps > 0).

#include <hip/hip_runtime.h>

#include <cstdint>

#include "embed.h"

namespace rsdl {

// As in csrc/embed.hip: the packed fp32 forms are kept out of these kernels.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(EMBED_ALLOW_PACKED_FP32)
#define EMBED_KERNEL \
  __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define EMBED_KERNEL __global__
#endif

#define EM_THREADS 256
#define EM_CHUNK 16

namespace {

__device__ __forceinline__ float eo_bf16_f32(uint32_t h) {
  return __uint_as_float(h << 16);
}

__device__ __forceinline__ void eo_add(float4& s, const uint2 g) {
  s.x += eo_bf16_f32(g.x & 0xffffu);
  s.y += eo_bf16_f32(g.x >> 16);
  s.z += eo_bf16_f32(g.y & 0xffffu);
  s.w += eo_bf16_f32(g.y >> 16);
}

__device__ __forceinline__ void eo_add(float4& s, const float4 v) {
  s.x += v.x;
  s.y += v.y;
  s.z += v.z;
  s.w += v.w;
}

__device__ __forceinline__ void eo_sgd(float g, float& p, float lr) {
  #pragma clang fp contract(off)
  const float u = lr * g;
  p = p - u;
}

// p' = p - lr * (g / (sqrt(h) + eps)), h already updated
__device__ __forceinline__ void eo_scaled(float g, float& p, float h,
                                          float lr, float eps) {
  #pragma clang fp contract(off)
  const float sv = __builtin_sqrtf(h);
  const float den = sv + eps;
  const float r = g / den;
  const float u = lr * r;
  p = p - u;
}

__device__ __forceinline__ void eo_adagrad(float g, float& p, float& h,
                                           float lr, float eps) {
  #pragma clang fp contract(off)
  const float gg = g * g;
  h = h + gg;
  eo_scaled(g, p, h, lr, eps);
}

// h' = h + mean of g^2 over the row; every lane of the row's group is
// active here and gets the same bits (each butterfly level adds the same
// two values on both sides).
template <int D>
__device__ __forceinline__ float eo_row_state(const float4 g, float h) {
  #pragma clang fp contract(off)
  constexpr int G = D / 4;
  // __shfl_xor's width: a power of two inside one wave, and the groups
  // tile the workgroup, so a group never straddles two waves.
  static_assert(G >= 2 && G <= 32 && (G & (G - 1)) == 0 &&
                    EM_THREADS % G == 0,
                "a row's lanes are a power-of-two group of at most 32");
  const float xx = g.x * g.x;
  const float yy = g.y * g.y;
  const float zz = g.z * g.z;
  const float ww = g.w * g.w;
  const float xy = xx + yy;
  const float xyz = xy + zz;
  float s = xyz + ww;
  #pragma unroll
  for (int d = 1; d < G; d <<= 1) {
    const float o = __shfl_xor(s, d, G);
    s = s + o;
  }
  const float m = s * (1.0f / D);
  return h + m;
}

// Update lane l's float4 of row ``row`` of entry e from its gradient g.
template <int D, int KIND>
__device__ __forceinline__ void eo_apply(const EmbedOptArgs& a, int32_t e,
                                         int32_t row, int32_t l,
                                         const float4 g) {
  float4* wp = reinterpret_cast<float4*>(a.W[e] + (int64_t)row * D) + l;
  float4 p = *wp;
  if (KIND == kEmbedSgd) {
    eo_sgd(g.x, p.x, a.lr);
    eo_sgd(g.y, p.y, a.lr);
    eo_sgd(g.z, p.z, a.lr);
    eo_sgd(g.w, p.w, a.lr);
  } else if (KIND == kEmbedAdagrad) {
    float4* hp = reinterpret_cast<float4*>(a.state[e] + (int64_t)row * D) + l;
    float4 h = *hp;
    eo_adagrad(g.x, p.x, h.x, a.lr, a.eps);
    eo_adagrad(g.y, p.y, h.y, a.lr, a.eps);
    eo_adagrad(g.z, p.z, h.z, a.lr, a.eps);
    eo_adagrad(g.w, p.w, h.w, a.lr, a.eps);
    *hp = h;
  } else {
    float* hp = a.state[e] + row;
    const float h = eo_row_state<D>(g, *hp);
    if (l == 0) *hp = h;
    eo_scaled(g.x, p.x, h, a.lr, a.eps);
    eo_scaled(g.y, p.y, h, a.lr, a.eps);
    eo_scaled(g.z, p.z, h, a.lr, a.eps);
    eo_scaled(g.w, p.w, h, a.lr, a.eps);
  }
  *wp = p;
}

}  // namespace

template <int D, int KIND>
EMBED_KERNEL void __launch_bounds__(EM_THREADS)
    embed_runs_update_kernel(const EmbedOptArgs a,
                             const int32_t* __restrict__ keys,
                             const int64_t* __restrict__ pos,
                             const uint16_t* __restrict__ dout,
                             float* __restrict__ carry, int64_t N, int64_t B,
                             int32_t T) {
  constexpr int G = D / 4;  // lanes per chunk, one float4 each
  constexpr int C = EM_CHUNK;
  const int64_t gid = (int64_t)blockIdx.x * EM_THREADS + threadIdx.x;
  const int64_t c = gid / G;
  const int32_t l = (int32_t)(gid % G);
  const int64_t p0 = c * C;
  if (p0 >= N) return;
  const int32_t cnt = (int32_t)((N - p0) < C ? (N - p0) : C);

  int32_t k[C];
  int64_t ps[C];
  if (cnt == C) {
    const int4* k4 = reinterpret_cast<const int4*>(keys + p0);
    const longlong2* p2 = reinterpret_cast<const longlong2*>(pos + p0);
    #pragma unroll
    for (int i = 0; i < C / 4; i++) {
      const int4 v = k4[i];
      k[4 * i] = v.x;
      k[4 * i + 1] = v.y;
      k[4 * i + 2] = v.z;
      k[4 * i + 3] = v.w;
    }
    #pragma unroll
    for (int i = 0; i < C / 2; i++) {
      const longlong2 v = p2[i];
      ps[2 * i] = v.x;
      ps[2 * i + 1] = v.y;
    }
  } else {
    // positions past the end repeat the last one's key and are never added
    #pragma unroll
    for (int i = 0; i < C; i++) {
      const int64_t q = p0 + (i < cnt ? i : cnt - 1);
      k[i] = keys[q];
      ps[i] = pos[q];
    }
  }

  // A run lies inside one table, and so does nearly every chunk: two
  // divisions, and one per position only where the chunk spans tables.
  const int64_t TD = (int64_t)T * D;
  const int32_t e0 = (int32_t)(ps[0] / B);
  const int32_t e1 = (int32_t)(ps[cnt - 1] / B);
  int32_t en[C];
  uint2 g[C];
  #pragma unroll
  for (int i = 0; i < C; i++) {
    en[i] = e0 == e1 ? e0 : (int32_t)(ps[i] / B);
    const int64_t b = ps[i] - (int64_t)en[i] * B;
    g[i] = make_uint2(0u, 0u);
    if (i < cnt) {
      g[i] = *reinterpret_cast<const uint2*>(
          &dout[b * TD + a.t[en[i]] * D + l * 4]);
    }
  }

  const bool head_open = p0 > 0 && keys[p0 - 1] == k[0];
  const bool tail_open = p0 + cnt < N && keys[p0 + cnt] == k[cnt - 1];
  float4* cr = reinterpret_cast<float4*>(carry + c * 2 * D) + l;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  bool first = true;  // the segment being summed began at position 0
  #pragma unroll
  for (int i = 0; i < C; i++) {
    if (i < cnt) {
      eo_add(s, g[i]);
      const bool last = i == cnt - 1;
      if (last || k[i + 1 < C ? i + 1 : i] != k[i]) {
        const bool began = !(first && head_open);
        const bool ended = !(last && tail_open);
        if (began && ended) {
          eo_apply<D, KIND>(a, en[i], k[i] - (int32_t)a.row_off[en[i]], l, s);
        } else {
          cr[began ? G : 0] = s;
        }
        s = make_float4(0.f, 0.f, 0.f, 0.f);
        first = false;
      }
    }
  }
}

template <int D, int KIND>
EMBED_KERNEL void __launch_bounds__(EM_THREADS)
    embed_carry_update_kernel(const EmbedOptArgs a,
                              const int32_t* __restrict__ keys,
                              const int64_t* __restrict__ pos,
                              const float* __restrict__ carry, int64_t N,
                              int64_t B) {
  constexpr int G = D / 4;
  constexpr int C = EM_CHUNK;
  const int64_t gid = (int64_t)blockIdx.x * EM_THREADS + threadIdx.x;
  const int64_t c = gid / G;
  const int32_t l = (int32_t)(gid % G);
  const int64_t p0 = c * C;
  const int64_t end = p0 + C;
  if (end >= N) return;  // the last chunk's tail is never open
  const int32_t key = keys[end - 1];
  if (keys[end] != key) return;  // the tail ends with the chunk
  // Keys ascend: the first key equals the last iff the chunk is one
  // segment, and then the run begins here only if it did not come in.
  if (keys[p0] == key && p0 > 0 && keys[p0 - 1] == key) return;

  const float4* cr = reinterpret_cast<const float4*>(carry) + l;
  float4 s = cr[(c * 2 + 1) * G];
  for (int64_t c2 = c + 1;; c2++) {
    eo_add(s, cr[c2 * 2 * G]);
    const int64_t next = (c2 + 1) * C;
    if (next >= N || keys[next] != key) break;
  }
  const int32_t e = (int32_t)(pos[end - 1] / B);
  eo_apply<D, KIND>(a, e, key - (int32_t)a.row_off[e], l, s);
}

// Rows of entry e: the slabs' partials summed in ascending slab order (as
// embed_bwd_fold), then the update of the row in place.
template <int D, int KIND>
EMBED_KERNEL void __launch_bounds__(EM_THREADS)
    embed_fold_update_kernel(const EmbedOptArgs a,
                             const float* __restrict__ part, int32_t nslab) {
  constexpr int G = D / 4;
  const int32_t e = blockIdx.y;
  const int32_t card = a.card[e];
  const int32_t n4 = card * G;
  const int32_t i = blockIdx.x * EM_THREADS + threadIdx.x;
  if (i >= n4) return;  // whole lane groups: n4 is a multiple of G
  const int64_t stride4 = (int64_t)((card + 31) & ~31) * G;
  const float4* p = reinterpret_cast<const float4*>(part + a.part_off[e]) + i;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  #pragma unroll 8
  for (int32_t sl = 0; sl < nslab; sl++) {
    eo_add(s, p[sl * stride4]);
  }
  eo_apply<D, KIND>(a, e, i / G, i % G, s);
}

#define EMBED_BY_WIDTH_KIND(D, KIND, CALL)            \
  switch ((D) * 4 + (KIND)) {                         \
    case 8 * 4 + 0: { CALL(8, 0); break; }            \
    case 8 * 4 + 1: { CALL(8, 1); break; }            \
    case 8 * 4 + 2: { CALL(8, 2); break; }            \
    case 16 * 4 + 0: { CALL(16, 0); break; }          \
    case 16 * 4 + 1: { CALL(16, 1); break; }          \
    case 16 * 4 + 2: { CALL(16, 2); break; }          \
    case 32 * 4 + 0: { CALL(32, 0); break; }          \
    case 32 * 4 + 1: { CALL(32, 1); break; }          \
    case 64 * 4 + 0: { CALL(64, 0); break; }          \
    case 64 * 4 + 1: { CALL(64, 1); break; }          \
    case 64 * 4 + 2: { CALL(64, 2); break; }          \
    case 128 * 4 + 0: { CALL(128, 0); break; }        \
    case 128 * 4 + 1: { CALL(128, 1); break; }        \
    case 128 * 4 + 2: { CALL(128, 2); break; }        \
    default: { CALL(32, 2); break; }                  \
  }

void launch_embed_runs_update(const EmbedOptArgs& a, const int32_t* keys,
                              const int64_t* pos, const void* dout,
                              float* carry, int64_t N, int64_t B, int32_t T,
                              int32_t D, hipStream_t stream) {
  const int64_t chunks = (N + EM_CHUNK - 1) / EM_CHUNK;
  const int64_t threads = chunks * (D / 4);
  const uint32_t grid = (uint32_t)((threads + EM_THREADS - 1) / EM_THREADS);
#define EM_RUNS_UPDATE(W, K)                                                \
  hipLaunchKernelGGL((embed_runs_update_kernel<W, K>), dim3(grid),          \
                     dim3(EM_THREADS), 0, stream, a, keys, pos,             \
                     reinterpret_cast<const uint16_t*>(dout), carry, N, B,  \
                     T);                                                    \
  if (chunks > 1) {                                                         \
    hipLaunchKernelGGL((embed_carry_update_kernel<W, K>), dim3(grid),       \
                       dim3(EM_THREADS), 0, stream, a, keys, pos, carry, N, \
                       B);                                                  \
  }
  EMBED_BY_WIDTH_KIND(D, a.kind, EM_RUNS_UPDATE)
#undef EM_RUNS_UPDATE
}

void launch_embed_fold_update(const EmbedOptArgs& a, int32_t n,
                              const float* part, int32_t D, int32_t nslab,
                              int32_t max_card, hipStream_t stream) {
  const uint32_t fold_x =
      (uint32_t)((max_card * (D / 4) + EM_THREADS - 1) / EM_THREADS);
#define EM_FOLD_UPDATE(W, K)                                               \
  hipLaunchKernelGGL((embed_fold_update_kernel<W, K>), dim3(fold_x, n),    \
                     dim3(EM_THREADS), 0, stream, a, part, nslab)
  EMBED_BY_WIDTH_KIND(D, a.kind, EM_FOLD_UPDATE)
#undef EM_FOLD_UPDATE
}

}  // namespace rsdl
