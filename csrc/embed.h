// Launch arguments of the fused multi-table embedding kernels
// (csrc/embed.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rsdl {

constexpr int kEmbedMaxTables = 64;

// Forward: one entry per table, by value in the kernel arguments.
struct EmbedFwdArgs {
  const int64_t* idx[kEmbedMaxTables];  // first index of table t's column
  int64_t stride[kEmbedMaxTables];      // elements between batch rows
  const float* W[kEmbedMaxTables];      // [card, D] fp32, 16-byte aligned
  int32_t card[kEmbedMaxTables];
};

// Backward: one entry per table of the regime the kernel serves. The
// gradients of all tables are one flat fp32 [R, D] buffer; table t owns the
// rows [row_off, row_off + card).
struct EmbedBwdArgs {
  int32_t t[kEmbedMaxTables];         // table number (column block of dOut)
  int32_t card[kEmbedMaxTables];
  int64_t row_off[kEmbedMaxTables];
  int64_t part_off[kEmbedMaxTables];  // floats; onehot partials of the entry
};

// In-place optimizer update (csrc/embed_optim.hip): one entry per table of
// the regime the kernel serves. row_off is the entry's first key in the flat
// row numbering of the sorted regime; state is [card, D] (adagrad), [card]
// (rowwise adagrad) or unused (sgd).
enum EmbedOptKind : int32_t {
  kEmbedSgd = 0,
  kEmbedAdagrad = 1,
  kEmbedRowwiseAdagrad = 2,
};

struct EmbedOptArgs {
  int32_t t[kEmbedMaxTables];         // table number (column block of dOut)
  int32_t card[kEmbedMaxTables];
  int64_t row_off[kEmbedMaxTables];
  int64_t part_off[kEmbedMaxTables];  // floats; onehot partials of the entry
  float* W[kEmbedMaxTables];          // [card, D] fp32, 16-byte aligned
  float* state[kEmbedMaxTables];
  int32_t kind;
  float lr;
  float eps;
};

// embed_bwd_onehot stages at most 32 columns of dOut: wider tables are cut
// into D / 32 column slices, one workgroup each (the grid's z axis).
inline int32_t embed_slices(int32_t D) { return D > 32 ? D / 32 : 1; }

// Rows of a batch slab of embed_bwd_onehot at width D: the largest whose
// staged indices and transposed dOut slice (of min(D, 32) columns) fit
// 64 KB of LDS.
inline int32_t embed_max_slab(int32_t D) {
  return 16384 / (D / embed_slices(D));
}

// out bf16 [B, T*D]; widx int32 [B, T] wrapped indices, or nullptr.
void launch_embed_concat_fwd(const EmbedFwdArgs& a, void* out, int32_t* widx,
                             int64_t B, int32_t T, int32_t D,
                             hipStream_t stream);
// n entries, nslab slabs of S rows (S a multiple of 16, at most
// embed_max_slab(D)), nslice = embed_slices(D) column slices; part holds
// [nslab, card_pad, D] per entry at part_off, card_pad = card rounded up to
// 32, and slice z writes its columns [z * D / nslice, (z + 1) * D / nslice)
// of it. Then the fixed-order fold into grad.
void launch_embed_bwd_onehot(const EmbedBwdArgs& a, int32_t n,
                             const int32_t* widx, const void* dout,
                             float* part, float* grad, int64_t B, int32_t T,
                             int32_t D, int32_t S, int32_t nslab,
                             int32_t nslice, int32_t max_card,
                             hipStream_t stream);
// keys int32 [N] ascending (flat grad row of each position), pos int64 [N]
// (entry * B + batch row, ascending inside equal keys); a.t holds the n
// entries' table numbers.
void launch_embed_bwd_runs(const EmbedBwdArgs& a, const int32_t* keys,
                           const int64_t* pos, const void* dout, float* grad,
                           int64_t N, int64_t B, int32_t T, int32_t D,
                           hipStream_t stream);

// The first half of launch_embed_bwd_onehot alone: the slab partials.
void launch_embed_onehot_partials(const EmbedBwdArgs& a, int32_t n,
                                  const int32_t* widx, const void* dout,
                                  float* part, int64_t B, int32_t T,
                                  int32_t D, int32_t S, int32_t nslab,
                                  int32_t nslice, hipStream_t stream);
// keys, pos as for launch_embed_bwd_runs, both 16-byte aligned; carry holds
// ceil(N / 16) * 2 * D floats and need not be cleared. Updates the rows the
// keys name (key - row_off of the entry) and their state, nothing else.
void launch_embed_runs_update(const EmbedOptArgs& a, const int32_t* keys,
                              const int64_t* pos, const void* dout,
                              float* carry, int64_t N, int64_t B, int32_t T,
                              int32_t D, hipStream_t stream);
// part as launch_embed_onehot_partials left it: folds it in ascending slab
// order and updates every row of the n entries.
void launch_embed_fold_update(const EmbedOptArgs& a, int32_t n,
                              const float* part, int32_t D, int32_t nslab,
                              int32_t max_card, hipStream_t stream);

}  // namespace rsdl
