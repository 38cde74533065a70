// Torch bindings for the MI355X shuffle kernels (csrc/shuffle_kernels.hip).
//
// Exposes the fused reducer-side ops (gather-permute / unpack+cast+pack /
// pack) to Python as ray_shuffling_data_loader_amd._rsdl_hip. All ops run on
// the CALLER's current HIP stream, so the shuffle engine's side-stream
// discipline (double-buffering against the trainer step) is controlled from
// Python via torch.cuda.Stream.

#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <tuple>
#include <vector>

#include "chain.h"
#include "step_glue.h"

namespace rsdl {

// Mirror of the definitions in shuffle_kernels.hip.
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
  int64_t col_ptr;
  int32_t packed_off;
  int32_t src_dtype;
  int32_t dst_dtype;
  int32_t numel;
};

struct ColTable {
  ColDesc cols[128];
};

void launch_gather_rows(const void* src, void* dst, const int64_t* perm,
                        int64_t n_rows, int64_t row_bytes, hipStream_t stream);
void launch_gather_rows_idx32(const void* src, void* dst, const int32_t* perm,
                              int64_t n_rows, int64_t row_bytes,
                              hipStream_t stream);
void launch_unpack_permute(const void* packed, int64_t row_stride,
                           const int64_t* perm, const ColTable& table,
                           int32_t num_cols, int64_t n_rows,
                           hipStream_t stream);
void launch_pack_columns(void* packed, int64_t row_stride, const int64_t* perm,
                         const ColTable& table, int32_t num_cols,
                         int64_t n_rows, hipStream_t stream);
struct StatsCol {
  int32_t packed_off;
  int32_t src_dtype;
  int32_t numel;
  int32_t elem_base;
};

struct StatsTable {
  StatsCol cols[128];
};

struct AffineBase {
  int32_t base[128];
};

void launch_column_stats(const void* packed, int64_t row_stride,
                         int64_t n_rows, const StatsTable& table,
                         int32_t num_cols, int32_t total_elems,
                         int32_t num_blocks, int64_t* part_n, double* part_s,
                         double* part_ss, double* pivot, int64_t* out_n,
                         double* out_s, double* out_ss, hipStream_t stream);
void launch_unpack_permute_affine(const void* packed, int64_t row_stride,
                                  const int64_t* perm, const ColTable& table,
                                  const AffineBase& abase,
                                  const void* aff_table, int32_t num_cols,
                                  int64_t n_rows, int32_t has_fill,
                                  float fill_f, hipStream_t stream);
struct NarrowCol {
  int32_t src_off;
  int32_t dst_off;
  int32_t src_dtype;
  int32_t dst_dtype;
  int32_t numel;
  int32_t aff_base;
};

struct NarrowTable {
  NarrowCol cols[128];
};

struct SweepCol {
  int64_t col_ptr;
  int32_t lane0;
  int32_t lanes;
};

struct SweepTable {
  SweepCol cols[8];
};

void launch_narrow_rows(const void* src, int64_t src_stride, void* dst,
                        int64_t dst_stride, const NarrowTable& table,
                        const void* aff_table, int32_t num_cols,
                        int64_t n_rows, int32_t has_fill, float fill_f,
                        int32_t pad_off, hipStream_t stream);
void launch_unpack_rows_sweep(const void* packed, int64_t row_stride,
                              const int64_t* perm, const SweepTable& table,
                              int32_t num_cols, int32_t lanes_per_row,
                              int64_t n_rows, hipStream_t stream);
void launch_partition_hist(const int32_t* dest, int32_t* block_counts,
                           int64_t n, int32_t num_dests, int32_t num_blocks,
                           hipStream_t stream);
void launch_partition_scatter(const int32_t* dest, const int32_t* block_base,
                              int32_t* perm_out, int64_t n, int32_t num_dests,
                              int32_t num_blocks, hipStream_t stream);
void launch_pack_tiled(void* packed, int64_t row_stride, const ColTable& table,
                       int32_t num_cols, int64_t n_rows, int32_t tile_rows,
                       int64_t lds_bytes, int32_t n8, hipStream_t stream);
void launch_wgrad_bf16(const void* dy, const void* x, float* dW, float* db,
                       int64_t M, int32_t N, int32_t K, int32_t split_m,
                       hipStream_t stream);
void launch_wgrad_wide(const void* dy, const void* x, float* dW, float* db,
                       int64_t M, int32_t N, int32_t K, int32_t split_m,
                       hipStream_t stream);
void launch_relu_bwd_bias(const void* dy, const void* y, void* dx,
                          float* db_part, int64_t nvec, int32_t N,
                          int32_t grid, hipStream_t stream);

namespace {

int32_t dtype_code(at::ScalarType st) {
  switch (st) {
    case at::kFloat: return DT_F32;
    case at::kDouble: return DT_F64;
    case at::kInt: return DT_I32;
    case at::kLong: return DT_I64;
    case at::kHalf: return DT_F16;
    case at::kBFloat16: return DT_BF16;
    case at::kByte: return DT_U8;
    default:
      TORCH_CHECK(false, "unsupported dtype for shuffle ops: ", st);
  }
}

const char* dtype_name(int64_t code) {
  switch (code) {
    case DT_F32: return "float32";
    case DT_F64: return "float64";
    case DT_I32: return "int32";
    case DT_I64: return "int64";
    case DT_F16: return "float16";
    case DT_BF16: return "bfloat16";
    case DT_U8: return "uint8";
    default: return "unknown";
  }
}

// What pack_columns, pack_columns_tiled and unpack_permute can do with one
// column: keep its dtype (a byte copy, any of the seven dtypes), or one of
// the casts RSDL_DISPATCH_PAIR knows ({f32, f64, i32, i64} to the same four
// or bf16). Any other pair would leave the destination unwritten, so it is
// refused here, before the launch.
void check_col_pair(const char* who, size_t col, int64_t from, int64_t to) {
  TORCH_CHECK(from >= DT_F32 && from <= DT_U8 && to >= DT_F32 && to <= DT_U8,
              who, ": column ", col, ": unknown dtype code (", from, " -> ",
              to, ")");
  const bool cast_src =
      from == DT_F32 || from == DT_F64 || from == DT_I32 || from == DT_I64;
  const bool cast_dst = to == DT_F32 || to == DT_F64 || to == DT_I32 ||
                        to == DT_I64 || to == DT_BF16;
  TORCH_CHECK(from == to || (cast_src && cast_dst), who, ": column ", col,
              ": no kernel converts ", dtype_name(from), " to ",
              dtype_name(to),
              " (a column keeps its dtype, or goes from float32, float64, "
              "int32 or int64 to one of those or to bfloat16)");
}

hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

int64_t row_bytes_of(const at::Tensor& t) {
  TORCH_CHECK(t.dim() == 2, "packed tensor must be 2-D [rows, row_bytes]");
  TORCH_CHECK(t.is_contiguous(), "packed tensor must be contiguous");
  int64_t rb = t.size(1) * t.element_size();
  TORCH_CHECK(rb % 16 == 0,
              "packed row byte width must be a multiple of 16, got ", rb);
  return rb;
}

// dst[i,:] = src[perm[i],:]
at::Tensor gather_rows(const at::Tensor& src, const at::Tensor& perm) {
  TORCH_CHECK(src.is_cuda() && perm.is_cuda(), "gather_rows: inputs on GPU");
  TORCH_CHECK(perm.scalar_type() == at::kLong || perm.scalar_type() == at::kInt,
              "perm must be int64 or int32");
  TORCH_CHECK(perm.is_contiguous(), "perm must be contiguous");
  int64_t rb = row_bytes_of(src);
  int64_t n = perm.numel();
  auto dst = at::empty({n, src.size(1)}, src.options());
  if (n == 0) return dst;
  if (perm.scalar_type() == at::kLong) {
    launch_gather_rows(src.data_ptr(), dst.data_ptr(),
                       perm.data_ptr<int64_t>(), n, rb, current_stream());
  } else {
    launch_gather_rows_idx32(src.data_ptr(), dst.data_ptr(),
                             perm.data_ptr<int32_t>(), n, rb,
                             current_stream());
  }
  return dst;
}

void gather_rows_out(const at::Tensor& src, const at::Tensor& perm,
                     at::Tensor& dst) {
  TORCH_CHECK(src.is_cuda() && perm.is_cuda() && dst.is_cuda(),
              "gather_rows_out: inputs on GPU");
  int64_t rb = row_bytes_of(src);
  TORCH_CHECK(row_bytes_of(dst) == rb, "dst row width mismatch");
  TORCH_CHECK(dst.size(0) >= perm.numel(), "dst too small");
  TORCH_CHECK(perm.is_contiguous(), "perm must be contiguous");
  int64_t n = perm.numel();
  if (n == 0) return;
  if (perm.scalar_type() == at::kLong) {
    launch_gather_rows(src.data_ptr(), dst.data_ptr(),
                       perm.data_ptr<int64_t>(), n, rb, current_stream());
  } else if (perm.scalar_type() == at::kInt) {
    launch_gather_rows_idx32(src.data_ptr(), dst.data_ptr(),
                             perm.data_ptr<int32_t>(), n, rb,
                             current_stream());
  } else {
    TORCH_CHECK(false, "perm must be int64 or int32");
  }
}

// outs[c][i*numel+e] = cast(packed[perm[i]*stride + off_c + e*esz])
void unpack_permute(const at::Tensor& packed,
                    const c10::optional<at::Tensor>& perm,
                    const std::vector<at::Tensor>& outs,
                    const std::vector<int64_t>& packed_offsets,
                    const std::vector<int64_t>& src_dtype_codes) {
  TORCH_CHECK(packed.is_cuda(), "packed must be on GPU");
  TORCH_CHECK(packed.scalar_type() == at::kByte, "packed must be uint8");
  TORCH_CHECK(outs.size() == packed_offsets.size() &&
                  outs.size() == src_dtype_codes.size(),
              "descriptor length mismatch");
  TORCH_CHECK(outs.size() <= 128, "at most 128 columns per launch");
  int64_t stride = packed.size(1);
  int64_t n_rows;
  const int64_t* perm_ptr = nullptr;
  if (perm.has_value()) {
    TORCH_CHECK(perm->is_cuda() && perm->scalar_type() == at::kLong &&
                    perm->is_contiguous(),
                "perm must be contiguous int64 on GPU");
    n_rows = perm->numel();
    perm_ptr = perm->data_ptr<int64_t>();
  } else {
    n_rows = packed.size(0);
  }
  if (n_rows == 0 || outs.empty()) return;
  ColTable table{};
  for (size_t c = 0; c < outs.size(); ++c) {
    const auto& o = outs[c];
    TORCH_CHECK(o.is_cuda() && o.is_contiguous(),
                "output column must be contiguous GPU tensor");
    TORCH_CHECK(o.size(0) == n_rows, "output rows mismatch");
    check_col_pair("unpack_permute", c, src_dtype_codes[c],
                   dtype_code(o.scalar_type()));
    table.cols[c] = ColDesc{
        reinterpret_cast<int64_t>(o.data_ptr()),
        (int32_t)packed_offsets[c],
        (int32_t)src_dtype_codes[c],
        dtype_code(o.scalar_type()),
        (int32_t)(o.numel() / n_rows),
    };
  }
  launch_unpack_permute(packed.data_ptr(), stride, perm_ptr, table,
                        (int32_t)outs.size(), n_rows, current_stream());
}

int64_t src_elem_bytes(int64_t code) {
  switch (code) {
    case DT_F64: case DT_I64: return 8;
    case DT_F32: case DT_I32: return 4;
    default:
      TORCH_CHECK(false, "unsupported packed source dtype code ", code);
  }
}

// Affine variant of unpack_permute: a column c with aff_base[c] >= 0 comes
// out as cast((float)((double(x) - shift[e]) * scale[e])), (shift, scale)
// interleaved per element in aff_table[aff_base[c] + e]; the others exactly
// as unpack_permute gives them. With nan_fill, a NaN source element of a
// standardized column becomes cast((float)nan_fill).
void unpack_permute_affine(const at::Tensor& packed,
                           const c10::optional<at::Tensor>& perm,
                           const std::vector<at::Tensor>& outs,
                           const std::vector<int64_t>& packed_offsets,
                           const std::vector<int64_t>& src_dtype_codes,
                           const at::Tensor& aff_table,
                           const std::vector<int64_t>& aff_base,
                           const c10::optional<double>& nan_fill) {
  TORCH_CHECK(packed.is_cuda(), "packed must be on GPU");
  TORCH_CHECK(packed.scalar_type() == at::kByte && packed.dim() == 2 &&
                  packed.is_contiguous(),
              "packed must be contiguous uint8 [rows, row_stride]");
  TORCH_CHECK(outs.size() == packed_offsets.size() &&
                  outs.size() == src_dtype_codes.size() &&
                  outs.size() == aff_base.size(),
              "descriptor length mismatch");
  TORCH_CHECK(outs.size() <= 128, "at most 128 columns per launch");
  TORCH_CHECK(aff_table.is_cuda() && aff_table.scalar_type() == at::kDouble &&
                  aff_table.is_contiguous() && aff_table.dim() == 2 &&
                  aff_table.size(1) == 2,
              "aff_table must be contiguous float64 [elems, 2] on GPU");
  int64_t stride = packed.size(1);
  TORCH_CHECK(stride % 16 == 0, "row stride must be a multiple of 16");
  int64_t n_rows;
  const int64_t* perm_ptr = nullptr;
  if (perm.has_value()) {
    TORCH_CHECK(perm->is_cuda() && perm->scalar_type() == at::kLong &&
                    perm->is_contiguous(),
                "perm must be contiguous int64 on GPU");
    n_rows = perm->numel();
    perm_ptr = perm->data_ptr<int64_t>();
  } else {
    n_rows = packed.size(0);
  }
  if (n_rows == 0 || outs.empty()) return;
  ColTable table{};
  AffineBase abase{};
  for (size_t c = 0; c < outs.size(); ++c) {
    const auto& o = outs[c];
    TORCH_CHECK(o.is_cuda() && o.is_contiguous(),
                "output column must be contiguous GPU tensor");
    TORCH_CHECK(o.size(0) == n_rows, "output rows mismatch");
    const int64_t numel = o.numel() / n_rows;
    const int64_t esz = src_elem_bytes(src_dtype_codes[c]);
    check_col_pair("unpack_permute_affine", c, src_dtype_codes[c],
                   dtype_code(o.scalar_type()));
    TORCH_CHECK(packed_offsets[c] >= 0 && packed_offsets[c] % esz == 0 &&
                    packed_offsets[c] + numel * esz <= stride,
                "column ", c, " does not fit the packed row");
    TORCH_CHECK(aff_base[c] < 0 ||
                    aff_base[c] + numel <= aff_table.size(0),
                "affine table too short for column ", c);
    table.cols[c] = ColDesc{
        reinterpret_cast<int64_t>(o.data_ptr()),
        (int32_t)packed_offsets[c],
        (int32_t)src_dtype_codes[c],
        dtype_code(o.scalar_type()),
        (int32_t)numel,
    };
    abase.base[c] = aff_base[c] < 0 ? -1 : (int32_t)aff_base[c];
  }
  launch_unpack_permute_affine(
      packed.data_ptr(), stride, perm_ptr, table, abase,
      aff_table.data_ptr(), (int32_t)outs.size(), n_rows,
      nan_fill.has_value() ? 1 : 0,
      nan_fill.has_value() ? (float)*nan_fill : 0.0f, current_stream());
}

int64_t any_elem_bytes(int64_t code) {
  switch (code) {
    case DT_F64: case DT_I64: return 8;
    case DT_F32: case DT_I32: return 4;
    case DT_F16: case DT_BF16: return 2;
    case DT_U8: return 1;
    default:
      TORCH_CHECK(false, "unsupported packed dtype code ", code);
  }
}

// The one-off narrowing pass of the source cache: wide packed rows ->
// packed rows of the output dtypes, identity row order. Column c moves from
// src_offsets[c] (dtype src_codes[c]) to dst_offsets[c] (dtype
// dst_codes[c]): a byte copy when the dtype stays, else the unpack kernels'
// cast, after the affine of aff_table[aff_base[c] + e] when aff_base[c] >=
// 0 (nan_fill as in unpack_permute_affine). Bytes of a narrow row from
// pad_off on are written as zero. Returns the [rows, dst_stride] block.
at::Tensor narrow_rows(const at::Tensor& packed, int64_t dst_stride,
                       int64_t pad_off,
                       const std::vector<int64_t>& src_offsets,
                       const std::vector<int64_t>& src_codes,
                       const std::vector<int64_t>& dst_offsets,
                       const std::vector<int64_t>& dst_codes,
                       const std::vector<int64_t>& numels,
                       const c10::optional<at::Tensor>& aff_table,
                       const std::vector<int64_t>& aff_base,
                       const c10::optional<double>& nan_fill) {
  TORCH_CHECK(packed.is_cuda(), "packed must be on GPU");
  TORCH_CHECK(packed.scalar_type() == at::kByte && packed.dim() == 2 &&
                  packed.is_contiguous(),
              "packed must be contiguous uint8 [rows, row_stride]");
  const size_t nc = numels.size();
  TORCH_CHECK(src_offsets.size() == nc && src_codes.size() == nc &&
                  dst_offsets.size() == nc && dst_codes.size() == nc &&
                  aff_base.size() == nc,
              "descriptor length mismatch");
  TORCH_CHECK(nc >= 1 && nc <= 128, "1..128 columns per launch");
  const int64_t n_rows = packed.size(0);
  const int64_t src_stride = packed.size(1);
  TORCH_CHECK(src_stride % 16 == 0 && dst_stride > 0 && dst_stride % 16 == 0,
              "row strides must be multiples of 16");
  TORCH_CHECK(pad_off >= 0 && pad_off <= dst_stride,
              "pad_off outside the narrow row");
  int64_t aff_rows = 0;
  if (aff_table.has_value()) {
    TORCH_CHECK(aff_table->is_cuda() &&
                    aff_table->scalar_type() == at::kDouble &&
                    aff_table->is_contiguous() && aff_table->dim() == 2 &&
                    aff_table->size(1) == 2,
                "aff_table must be contiguous float64 [elems, 2] on GPU");
    aff_rows = aff_table->size(0);
  }
  NarrowTable table{};
  for (size_t c = 0; c < nc; ++c) {
    const int64_t ssz = any_elem_bytes(src_codes[c]);
    const int64_t dsz = any_elem_bytes(dst_codes[c]);
    const bool same = src_codes[c] == dst_codes[c] && aff_base[c] < 0;
    if (!same) {
      // what the cast dispatch of the kernels knows
      TORCH_CHECK(src_codes[c] == DT_F32 || src_codes[c] == DT_F64 ||
                      src_codes[c] == DT_I32 || src_codes[c] == DT_I64,
                  "column ", c, ": unsupported source dtype for a cast");
      TORCH_CHECK(dst_codes[c] == DT_F32 || dst_codes[c] == DT_F64 ||
                      dst_codes[c] == DT_I32 || dst_codes[c] == DT_I64 ||
                      dst_codes[c] == DT_BF16,
                  "column ", c, ": unsupported destination dtype for a cast");
    }
    TORCH_CHECK(numels[c] >= 1 && src_offsets[c] >= 0 &&
                    src_offsets[c] % ssz == 0 &&
                    src_offsets[c] + numels[c] * ssz <= src_stride,
                "column ", c, " does not fit the wide row");
    TORCH_CHECK(dst_offsets[c] >= 0 && dst_offsets[c] % dsz == 0 &&
                    dst_offsets[c] + numels[c] * dsz <= pad_off,
                "column ", c, " does not fit the narrow row");
    TORCH_CHECK(aff_base[c] < 0 || aff_base[c] + numels[c] <= aff_rows,
                "affine table too short for column ", c);
    table.cols[c] = NarrowCol{
        (int32_t)src_offsets[c], (int32_t)dst_offsets[c],
        (int32_t)src_codes[c],   (int32_t)dst_codes[c],
        (int32_t)numels[c],      aff_base[c] < 0 ? -1 : (int32_t)aff_base[c],
    };
  }
  auto out = at::empty({n_rows, dst_stride}, packed.options());
  if (n_rows == 0) return out;
  launch_narrow_rows(packed.data_ptr(), src_stride, out.data_ptr(),
                     dst_stride, table,
                     aff_table.has_value() ? aff_table->data_ptr() : nullptr,
                     (int32_t)nc, n_rows, nan_fill.has_value() ? 1 : 0,
                     nan_fill.has_value() ? (float)*nan_fill : 0.0f,
                     (int32_t)pad_off, current_stream());
  return out;
}

// unpack_permute for a block whose columns all keep their dtype and are
// made of whole 8-B lanes (at most 8 columns): one row-major sweep instead
// of one grid pass per column. Same outputs as unpack_permute.
void unpack_permute_sweep(const at::Tensor& packed,
                          const c10::optional<at::Tensor>& perm,
                          const std::vector<at::Tensor>& outs,
                          const std::vector<int64_t>& packed_offsets,
                          const std::vector<int64_t>& src_dtype_codes) {
  TORCH_CHECK(packed.is_cuda(), "packed must be on GPU");
  TORCH_CHECK(packed.scalar_type() == at::kByte && packed.dim() == 2 &&
                  packed.is_contiguous(),
              "packed must be contiguous uint8 [rows, row_stride]");
  TORCH_CHECK(outs.size() == packed_offsets.size() &&
                  outs.size() == src_dtype_codes.size(),
              "descriptor length mismatch");
  TORCH_CHECK(outs.size() >= 1 && outs.size() <= 8,
              "1..8 columns per sweep");
  const int64_t stride = packed.size(1);
  TORCH_CHECK(stride % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(packed.data_ptr()) % 8 == 0,
              "packed rows must be 8-B aligned");
  int64_t n_rows;
  const int64_t* perm_ptr = nullptr;
  if (perm.has_value()) {
    TORCH_CHECK(perm->is_cuda() && perm->scalar_type() == at::kLong &&
                    perm->is_contiguous(),
                "perm must be contiguous int64 on GPU");
    n_rows = perm->numel();
    perm_ptr = perm->data_ptr<int64_t>();
  } else {
    n_rows = packed.size(0);
  }
  if (n_rows == 0) return;
  SweepTable table{};
  int64_t lanes_per_row = 0;
  for (size_t c = 0; c < outs.size(); ++c) {
    const auto& o = outs[c];
    TORCH_CHECK(o.is_cuda() && o.is_contiguous(),
                "output column must be contiguous GPU tensor");
    TORCH_CHECK(o.size(0) == n_rows, "output rows mismatch");
    TORCH_CHECK(dtype_code(o.scalar_type()) == src_dtype_codes[c],
                "sweep: column ", c, " changes dtype");
    const int64_t bytes =
        o.numel() / n_rows * any_elem_bytes(src_dtype_codes[c]);
    TORCH_CHECK(packed_offsets[c] >= 0 && packed_offsets[c] % 8 == 0 &&
                    bytes % 8 == 0 && packed_offsets[c] + bytes <= stride &&
                    reinterpret_cast<uintptr_t>(o.data_ptr()) % 8 == 0,
                "sweep: column ", c, " is not made of whole 8-B lanes");
    table.cols[c] = SweepCol{reinterpret_cast<int64_t>(o.data_ptr()),
                             (int32_t)(packed_offsets[c] / 8),
                             (int32_t)(bytes / 8)};
    lanes_per_row = std::max(lanes_per_row, (packed_offsets[c] + bytes) / 8);
  }
  launch_unpack_rows_sweep(packed.data_ptr(), stride, perm_ptr, table,
                           (int32_t)outs.size(), (int32_t)lanes_per_row,
                           n_rows, current_stream());
}

// One read-only pass over a packed block: per element of the listed columns
// (count of finite values, sum(x - p), sum((x - p)^2), p) in fp64 about the
// pivot p = the element's first finite value among the leading 64 rows
// (row 0 as a rule; 0 if there is none). Fixed grid sized
// from the CU count, per-block partial slab folded in block order: the same
// input gives the same bits on every call. Returns (count int64 [E],
// sum [E], sumsq [E], pivot [E]) on the device.
std::vector<at::Tensor> column_stats(
    const at::Tensor& packed, const std::vector<int64_t>& packed_offsets,
    const std::vector<int64_t>& src_dtype_codes,
    const std::vector<int64_t>& numels) {
  TORCH_CHECK(packed.is_cuda(), "packed must be on GPU");
  TORCH_CHECK(packed.scalar_type() == at::kByte && packed.dim() == 2 &&
                  packed.is_contiguous(),
              "packed must be contiguous uint8 [rows, row_stride]");
  TORCH_CHECK(packed_offsets.size() == src_dtype_codes.size() &&
                  packed_offsets.size() == numels.size(),
              "descriptor length mismatch");
  TORCH_CHECK(!numels.empty() && numels.size() <= 128,
              "1..128 columns per launch");
  const int64_t n_rows = packed.size(0);
  const int64_t stride = packed.size(1);
  TORCH_CHECK(n_rows > 0, "column_stats needs at least one row");
  StatsTable table{};
  int64_t total = 0;
  for (size_t c = 0; c < numels.size(); ++c) {
    const int64_t esz = src_elem_bytes(src_dtype_codes[c]);
    TORCH_CHECK(numels[c] >= 1 && packed_offsets[c] >= 0 &&
                    packed_offsets[c] % esz == 0 &&
                    packed_offsets[c] + numels[c] * esz <= stride,
                "column ", c, " does not fit the packed row");
    table.cols[c] = StatsCol{(int32_t)packed_offsets[c],
                             (int32_t)src_dtype_codes[c],
                             (int32_t)numels[c], (int32_t)total};
    total += numels[c];
  }
  TORCH_CHECK(total < (1 << 24), "too many elements");
  int cus = 0;
  C10_HIP_CHECK(hipDeviceGetAttribute(
      &cus, hipDeviceAttributeMultiprocessorCount, packed.get_device()));
  const int32_t num_blocks = std::max(1, cus) * 8;
  auto opt_d = packed.options().dtype(at::kDouble);
  auto opt_l = packed.options().dtype(at::kLong);
  auto part_n = at::empty({num_blocks, total}, opt_l);
  auto part_s = at::empty({num_blocks, total}, opt_d);
  auto part_ss = at::empty({num_blocks, total}, opt_d);
  auto pivot = at::empty({total}, opt_d);
  auto out_n = at::empty({total}, opt_l);
  auto out_s = at::empty({total}, opt_d);
  auto out_ss = at::empty({total}, opt_d);
  launch_column_stats(packed.data_ptr(), stride, n_rows, table,
                      (int32_t)numels.size(), (int32_t)total, num_blocks,
                      part_n.data_ptr<int64_t>(), part_s.data_ptr<double>(),
                      part_ss.data_ptr<double>(), pivot.data_ptr<double>(),
                      out_n.data_ptr<int64_t>(), out_s.data_ptr<double>(),
                      out_ss.data_ptr<double>(), current_stream());
  return {out_n, out_s, out_ss, pivot};
}

// packed[perm[i]*stride + off_c + e*esz] = cast(cols[c][i*numel+e])
at::Tensor pack_columns(const std::vector<at::Tensor>& cols,
                        const std::vector<int64_t>& packed_offsets,
                        const std::vector<int64_t>& packed_dtype_codes,
                        int64_t row_stride,
                        const c10::optional<at::Tensor>& perm) {
  TORCH_CHECK(!cols.empty(), "need at least one column");
  TORCH_CHECK(cols.size() <= 128, "at most 128 columns per launch");
  TORCH_CHECK(cols.size() == packed_offsets.size() &&
                  cols.size() == packed_dtype_codes.size(),
              "descriptor length mismatch");
  TORCH_CHECK(row_stride % 16 == 0, "row_stride must be multiple of 16");
  int64_t n_rows = cols[0].size(0);
  const int64_t* perm_ptr = nullptr;
  if (perm.has_value()) {
    TORCH_CHECK(perm->is_cuda() && perm->scalar_type() == at::kLong &&
                    perm->is_contiguous(),
                "perm must be contiguous int64 on GPU");
    TORCH_CHECK(perm->numel() == n_rows, "perm length mismatch");
    perm_ptr = perm->data_ptr<int64_t>();
  }
  auto packed = at::empty(
      {n_rows, row_stride},
      cols[0].options().dtype(at::kByte));
  ColTable table{};
  for (size_t c = 0; c < cols.size(); ++c) {
    const auto& t = cols[c];
    TORCH_CHECK(t.is_cuda() && t.is_contiguous(),
                "input column must be contiguous GPU tensor");
    TORCH_CHECK(t.size(0) == n_rows, "column rows mismatch");
    check_col_pair("pack_columns", c, dtype_code(t.scalar_type()),
                   packed_dtype_codes[c]);
    table.cols[c] = ColDesc{
        reinterpret_cast<int64_t>(t.data_ptr()),
        (int32_t)packed_offsets[c],
        (int32_t)packed_dtype_codes[c],
        dtype_code(t.scalar_type()),
        (int32_t)(t.numel() / n_rows),
    };
  }
  if (n_rows > 0) {
    launch_pack_columns(packed.data_ptr(), row_stride, perm_ptr, table,
                        (int32_t)cols.size(), n_rows, current_stream());
  }
  return packed;
}

// Build the gather permutation that groups rows by destination id.
// Returns (perm int32 [n], counts int64 [num_dests]).
std::vector<at::Tensor> partition_build_perm(const at::Tensor& dest,
                                             int64_t num_dests) {
  TORCH_CHECK(dest.is_cuda() && dest.is_contiguous(),
              "dest must be contiguous GPU tensor");
  TORCH_CHECK(num_dests >= 1 && num_dests <= 1024,
              "num_dests must be in [1, 1024]");
  auto dest32 = dest.scalar_type() == at::kInt ? dest : dest.to(at::kInt);
  int64_t n = dest32.numel();
  int32_t num_blocks = 1024;
  if (n < (int64_t)num_blocks * 256) {
    num_blocks = (int32_t)std::max<int64_t>(1, (n + 255) / 256);
  }
  auto opts32 = dest32.options();
  auto block_counts = at::empty({num_blocks, num_dests}, opts32);
  auto stream = current_stream();
  if (n > 0) {
    launch_partition_hist(dest32.data_ptr<int32_t>(),
                          block_counts.data_ptr<int32_t>(), n,
                          (int32_t)num_dests, num_blocks, stream);
  } else {
    block_counts.zero_();
  }
  // Exclusive scan (dest-major, then block-major within a dest), done with
  // torch ops on the same stream: tiny [B, T] tensor.
  auto counts64 = block_counts.to(at::kLong);
  auto per_dest = counts64.sum(0);                    // [T]
  auto dest_base = per_dest.cumsum(0) - per_dest;     // exclusive [T]
  auto within = counts64.cumsum(0) - counts64;        // exclusive over blocks
  auto base = (within + dest_base.unsqueeze(0)).to(at::kInt).contiguous();
  auto perm = at::empty({n}, opts32);
  if (n > 0) {
    launch_partition_scatter(dest32.data_ptr<int32_t>(),
                             base.data_ptr<int32_t>(),
                             perm.data_ptr<int32_t>(), n, (int32_t)num_dests,
                             num_blocks, stream);
  }
  return {perm, per_dest};
}

// LDS-tiled pack (no scatter perm): cols -> packed rows. ``out`` may be a
// contiguous [n_rows, row_stride] uint8 view (e.g. a row-slice of a larger
// preallocated source tensor) to pack in place.
at::Tensor pack_columns_tiled(const std::vector<at::Tensor>& cols,
                              const std::vector<int64_t>& packed_offsets,
                              const std::vector<int64_t>& packed_dtype_codes,
                              int64_t row_stride,
                              const c10::optional<at::Tensor>& out) {
  TORCH_CHECK(!cols.empty() && cols.size() <= 128, "1..128 columns");
  TORCH_CHECK(cols.size() == packed_offsets.size() &&
                  cols.size() == packed_dtype_codes.size(),
              "descriptor length mismatch");
  TORCH_CHECK(row_stride % 16 == 0, "row_stride must be multiple of 16");
  int64_t n_rows = cols[0].size(0);
  at::Tensor packed;
  if (out.has_value()) {
    packed = *out;
    TORCH_CHECK(packed.is_cuda() && packed.is_contiguous() &&
                    packed.scalar_type() == at::kByte &&
                    packed.size(0) == n_rows &&
                    packed.size(1) == row_stride,
                "out must be contiguous uint8 [n_rows, row_stride]");
  } else {
    packed =
        at::empty({n_rows, row_stride}, cols[0].options().dtype(at::kByte));
  }
  ColTable table{};
  for (size_t c = 0; c < cols.size(); ++c) {
    const auto& t = cols[c];
    TORCH_CHECK(t.is_cuda() && t.is_contiguous(),
                "input column must be contiguous GPU tensor");
    TORCH_CHECK(t.size(0) == n_rows, "column rows mismatch");
    check_col_pair("pack_columns_tiled", c, dtype_code(t.scalar_type()),
                   packed_dtype_codes[c]);
    table.cols[c] = ColDesc{
        reinterpret_cast<int64_t>(t.data_ptr()),
        (int32_t)packed_offsets[c],
        (int32_t)packed_dtype_codes[c],
        dtype_code(t.scalar_type()),
        (int32_t)(t.numel() / n_rows),
    };
  }
  const int64_t lds_stride = row_stride + 8;
  int32_t tile_rows = (int32_t)std::min<int64_t>(128, 65536 / lds_stride);
  TORCH_CHECK(tile_rows >= 1, "row_stride too large for tiled pack");
  // Fast-path eligibility: scalar columns, no casts, 8-B columns first
  // (guaranteed by Schema's descending-size packing) then 4-B columns.
  int32_t n8 = 0;
  bool fast = true;
  bool in8 = true;
  for (size_t c = 0; c < cols.size(); ++c) {
    const ColDesc& d = table.cols[c];
    if (d.numel != 1 || d.src_dtype != d.dst_dtype) { fast = false; break; }
    int esz = (d.src_dtype == DT_F64 || d.src_dtype == DT_I64) ? 8
              : (d.src_dtype == DT_F32 || d.src_dtype == DT_I32) ? 4 : 0;
    if (esz == 0) { fast = false; break; }
    if (esz == 8) {
      if (!in8) { fast = false; break; }
      n8++;
    } else {
      in8 = false;
    }
  }
  if (n_rows > 0) {
    launch_pack_tiled(packed.data_ptr(), row_stride, table,
                      (int32_t)cols.size(), n_rows, tile_rows,
                      lds_stride * tile_rows, fast ? n8 : -1,
                      current_stream());
  }
  return packed;
}

// MFMA split-M weight gradient: dW = dy^T @ x (+ db = dy.sum(0)).
// Returns (dW fp32 [N,K], db fp32 [N] or empty).
std::vector<at::Tensor> wgrad_bf16(const at::Tensor& dy, const at::Tensor& x,
                                   bool with_bias) {
  TORCH_CHECK(dy.is_cuda() && x.is_cuda(), "wgrad: inputs on GPU");
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 &&
                  x.scalar_type() == at::kBFloat16,
              "wgrad: bf16 inputs only");
  TORCH_CHECK(dy.dim() == 2 && x.dim() == 2 && dy.size(0) == x.size(0),
              "wgrad: dy [M,N], x [M,K]");
  TORCH_CHECK(dy.is_contiguous() && x.is_contiguous(),
              "wgrad: contiguous inputs");
  int64_t M = dy.size(0);
  int32_t N = (int32_t)dy.size(1);
  int32_t K = (int32_t)x.size(1);
  bool wide = getenv("RSDL_WGRAD_WIDE") != nullptr && N >= 64 && K >= 64 &&
              M >= 4096;
  if (wide) {
    // Wide-tile kernel wants 128-multiples; pad (cheap relative to the
    // re-read amplification it removes) and narrow the result.
    auto dyp = (N % 128) ? at::constant_pad_nd(dy, {0, 128 - N % 128})
                         : dy.contiguous();
    auto xp = (K % 128) ? at::constant_pad_nd(x, {0, 128 - K % 128})
                        : x.contiguous();
    int32_t Np = (int32_t)dyp.size(1), Kp = (int32_t)xp.size(1);
    auto dWp = at::zeros({Np, Kp}, dy.options().dtype(at::kFloat));
    auto dbp = with_bias ? at::zeros({Np}, dy.options().dtype(at::kFloat))
                         : at::Tensor();
    int32_t tiles = (Np / 128) * (Kp / 128);
    int32_t split = (int32_t)std::min<int64_t>(
        std::max<int64_t>(1, 2048 / std::max(1, tiles)),
        std::max<int64_t>(1, M / 64));
    launch_wgrad_wide(dyp.data_ptr(), xp.data_ptr(), dWp.data_ptr<float>(),
                      with_bias ? dbp.data_ptr<float>() : nullptr, M, Np, Kp,
                      split, current_stream());
    auto dW = dWp.narrow(0, 0, N).narrow(1, 0, K).contiguous();
    auto db = with_bias ? dbp.narrow(0, 0, N).contiguous() : at::Tensor();
    return {dW, db};
  }
  // 64-tile kernel: pad N/K to 64-multiples so the hot loop runs only the
  // unguarded vector-load stages (per-element guards serialize loads).
  auto dyp = (N % 64) ? at::constant_pad_nd(dy, {0, 64 - N % 64})
                      : dy.contiguous();
  auto xp = (K % 64) ? at::constant_pad_nd(x, {0, 64 - K % 64})
                     : x.contiguous();
  int32_t Np = (int32_t)dyp.size(1), Kp = (int32_t)xp.size(1);
  auto dWp = at::zeros({Np, Kp}, dy.options().dtype(at::kFloat));
  auto dbp = with_bias ? at::zeros({Np}, dy.options().dtype(at::kFloat))
                       : at::Tensor();
  int32_t tiles = (Np / 64) * (Kp / 64);
  int32_t split = (int32_t)std::min<int64_t>(
      std::max<int64_t>(1, 2048 / tiles), std::max<int64_t>(1, M / 64));
  if (const char* ov = getenv("RSDL_WGRAD_SPLIT")) {
    split = std::max(1, atoi(ov));
  }
  if (M > 0) {
    launch_wgrad_bf16(dyp.data_ptr(), xp.data_ptr(), dWp.data_ptr<float>(),
                      with_bias ? dbp.data_ptr<float>() : nullptr, M, Np, Kp,
                      split, current_stream());
  }
  auto dW = (Np == N && Kp == K)
                ? dWp
                : dWp.narrow(0, 0, N).narrow(1, 0, K).contiguous();
  auto db = with_bias
                ? ((Np == N) ? dbp : dbp.narrow(0, 0, N).contiguous())
                : at::Tensor();
  return {dW, db};
}


// Fused ReLU-backward + bias gradient: dx = dy * (y > 0), db = dx.sum(0).
// One pass over HBM instead of threshold_backward + a separate column
// reduce (csrc/relu_bwd.hip). Requires bf16, contiguous, N a power of two
// >= 8 (the LinearReLU widths); callers fall back to torch otherwise.
std::vector<at::Tensor> relu_bwd_bias(const at::Tensor& dy,
                                      const at::Tensor& y) {
  TORCH_CHECK(dy.is_cuda() && y.is_cuda(), "relu_bwd_bias: inputs on GPU");
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 &&
                  y.scalar_type() == at::kBFloat16,
              "relu_bwd_bias: bf16 inputs only");
  TORCH_CHECK(dy.dim() == 2 && dy.sizes() == y.sizes(),
              "relu_bwd_bias: dy and y must be equal 2-D shapes");
  TORCH_CHECK(dy.is_contiguous() && y.is_contiguous(),
              "relu_bwd_bias: contiguous inputs");
  const int64_t M = dy.size(0);
  const int64_t N = dy.size(1);
  TORCH_CHECK(N >= 8 && N <= 2048 && (N & (N - 1)) == 0,
              "relu_bwd_bias: N must be a power of two in [8, 2048]");
  auto dx = at::empty_like(dy);
  const int64_t nvec = M * N / 8;
  int32_t grid = (int32_t)std::min<int64_t>(
      1024, std::max<int64_t>(1, nvec / (256 * 8)));
  auto db_part = at::empty({grid, N}, dy.options().dtype(at::kFloat));
  if (nvec > 0) {
    launch_relu_bwd_bias(dy.data_ptr(), y.data_ptr(), dx.data_ptr(),
                         db_part.data_ptr<float>(), nvec, (int32_t)N, grid,
                         current_stream());
  } else {
    db_part.zero_();
  }
  return {dx, db_part.sum(0)};
}


// EXPERIMENTAL round-2 fused forward chain (csrc/fwd_chain.hip): fixed
// TabularMLP(100-512-256-128-1) architecture, bf16. Returns
// (a1, a2, a3, out). Exercised only by the RSDL_EXPERIMENTAL=1 GPU test.
// Fragment-major weight swizzle for the chain kernels (see
// csrc/fwd_chain.hip): [N,K] -> [N/32][K/16][2][32][8] flat, so one
// wave's B-fragment load is a contiguous 1 KB block.
static at::Tensor swizzle_frag(const at::Tensor& W) {
  int64_t N = W.size(0), K = W.size(1);
  TORCH_CHECK(N % 32 == 0 && K % 16 == 0, "swizzle_frag: bad shape");
  return W.view({N / 32, 32, K / 16, 2, 8})
      .permute({0, 2, 3, 1, 4})
      .contiguous()
      .view({-1});
}

// Rows per workgroup slab of the chain kernels (csrc/fwd_chain.hip,
// csrc/bwd_chain.hip): 32 or 64. The bindings' ``rows`` argument picks
// per call; 0 means the default, which is RSDL_CHAIN_ROWS if set (read
// once) and the build's default otherwise. Only the grouping of the
// loss/db partials depends on it; every per-row output is bit-identical.
#ifndef RSDL_CHAIN_ROWS_DEFAULT
#define RSDL_CHAIN_ROWS_DEFAULT 64
#endif
static int chain_rows(int64_t rows) {
  if (rows == 0) {
    static const int64_t latched = [] {
      const char* e = std::getenv("RSDL_CHAIN_ROWS");
      return (e != nullptr && *e != '\0')
                 ? static_cast<int64_t>(std::atoll(e))
                 : static_cast<int64_t>(RSDL_CHAIN_ROWS_DEFAULT);
    }();
    rows = latched;
  }
  TORCH_CHECK(rows == 32 || rows == 64,
              "chain rows must be 32 or 64 (argument or RSDL_CHAIN_ROWS), "
              "got ", rows);
  return static_cast<int>(rows);
}

// Objective of the fused head epilogue (csrc/fwd_chain.hip): the ``loss``
// argument of fwd_chain_bf16 / fused_step_bf16 and the ``task`` argument
// of eval_chain_bf16. Exported as LOSS_MSE / LOSS_BCE.
constexpr int64_t kLossMse = 0;
constexpr int64_t kLossBce = 1;
static int chain_loss(int64_t loss, const char* who, const char* what) {
  TORCH_CHECK(loss == kLossMse || loss == kLossBce, who, ": ", what,
              " must be 0 (MSE / regression) or 1 (BCE / binary), got ",
              loss);
  return static_cast<int>(loss);
}

// The feature batch every chain binding takes.
static void check_x(const char* who, const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
                  x.dim() == 2 && x.size(1) == 100 && x.is_contiguous(),
              who, ": x must be contiguous bf16 [M,100]");
}

// fp32 ``biases`` [b1..b4] read in place; with ``on`` (x's device index)
// they must also sit on that GPU.
static void check_biases(const char* who,
                         const std::vector<at::Tensor>& biases, int on = -1) {
  TORCH_CHECK(biases.size() == 4, who, ": biases must be [b1..b4]");
  const int64_t bn[4] = {512, 256, 128, 1};
  for (int i = 0; i < 4; i++) {
    TORCH_CHECK(biases[i].is_cuda() &&
                    biases[i].scalar_type() == at::kFloat &&
                    biases[i].is_contiguous() && biases[i].numel() == bn[i] &&
                    (on < 0 || biases[i].get_device() == on),
                who, ": bias ", i, " must be contiguous fp32 [", bn[i],
                on < 0 ? "] on GPU" : "] on x's GPU");
  }
}

// Sample weights and pos_weight of the fused head (csrc/fwd_chain.hip),
// validated for ``who``: ``weight`` fp32 [M] on x's GPU or absent (every
// w = 1), ``pos_weight`` finite and > 0, and != 1 only with LOSS_BCE.
// ``on`` says whether the weighted kernel is needed at all: with no weight
// and pos_weight == 1 the bindings launch what they always launched.
struct HeadWeights {
  bool on = false;
  const float* weight = nullptr;
  float pos_weight = 1.f;
};

static HeadWeights head_weights(const char* who, const at::Tensor& x,
                                const c10::optional<at::Tensor>& weight,
                                double pos_weight, int loss) {
  HeadWeights h;
  TORCH_CHECK(std::isfinite(pos_weight) && pos_weight > 0.0, who,
              ": pos_weight must be finite and > 0, got ", pos_weight);
  TORCH_CHECK(pos_weight == 1.0 || loss == kLossBce, who,
              ": pos_weight needs loss=1 (BCE)");
  if (weight.has_value()) {
    TORCH_CHECK(weight->is_cuda() &&
                    weight->get_device() == x.get_device() &&
                    weight->scalar_type() == at::kFloat &&
                    weight->is_contiguous() && weight->numel() == x.size(0),
                who, ": weight must be contiguous fp32 with ", x.size(0),
                " elements on x's GPU");
    h.weight = weight->data_ptr<float>();
  }
  h.pos_weight = static_cast<float>(pos_weight);
  h.on = weight.has_value() || h.pos_weight != 1.f;
  return h;
}

// Buffers + launches of the forward chain, shared by fwd_chain_bf16 and
// fused_step_bf16. Weights arrive fragment-major (W1 with K padded to
// 112), biases fp32, ``tgt`` fp32 [M] or nullptr. Nothing is launched for
// M == 0 (the weight tensors may then be undefined).
struct FwdChainOut {
  at::Tensor a1t, mask1, a2t, mask2, a3, out, dyb, loss_part;
};

FwdChainOut run_fwd_chain(const at::Tensor& x, const at::Tensor& W1s,
                          const at::Tensor& W2s, const at::Tensor& W3s,
                          const at::Tensor& w4, const at::Tensor& b1f,
                          const at::Tensor& b2f, const at::Tensor& b3f,
                          const at::Tensor& b4f, const at::Tensor* tgt,
                          const c10::optional<at::Tensor>& xt_out,
                          bool pi16, int rows, int loss,
                          const HeadWeights& hw = HeadWeights()) {
  FwdChainOut f;
  const int64_t M = x.size(0);
  // a1/a2 exist only TRANSPOSED in wgrad fragment-major layout (plus
  // 32-bit relu-mask words per column) — the backward chain consumes
  // masks, the wgrad kernel consumes the fragments; nothing reads
  // row-major a1/a2.
  const int64_t mtiles = std::max<int64_t>((M + 31) / 32, 1);
  const int64_t mchunks = mtiles * 2;
  f.a1t = at::empty({16 * mchunks * 512}, x.options());
  f.a2t = at::empty({8 * mchunks * 512}, x.options());
  f.mask1 = at::empty({mtiles, 512}, x.options().dtype(at::kInt));
  f.mask2 = at::empty({mtiles, 256}, x.options().dtype(at::kInt));
  f.a3 = at::empty({M, 128}, x.options());
  f.out = at::empty({M, 1}, x.options());
  FwdChainArgs p{};
  if (tgt != nullptr) {
    f.dyb = at::empty({M, 1}, x.options());
    f.loss_part = at::empty({std::max<int64_t>(fwd_chain_grid(M, rows), 1)},
                            x.options().dtype(at::kFloat));
    p.target = tgt->data_ptr<float>();
    p.dyb = f.dyb.data_ptr();
    p.loss_part = f.loss_part.data_ptr<float>();
  }
  if (M > 0) {
    // x pre-swizzled to the same fragment-major layout (per 32-row
    // m-tile): layer 1's A fragments then come straight from global,
    // coalesced, and the kernel needs no x LDS tile (occupancy 2 -> 3
    // workgroups/CU). Pads are zeroed by the swizzle kernel
    // (uninitialized bf16 could be NaN; NaN * W1pad(0) would poison
    // real rows).
    const int64_t Mp = (M + 31) / 32 * 32;
    auto xs = at::empty({Mp * 112}, x.options());
    if (xt_out.has_value()) {
      // one pass over x emits both the forward and the wgrad layouts
      launch_swizzle_x_both(x.data_ptr(), xs.data_ptr(),
                            xt_out->data_ptr(), M, pi16 ? 1 : 0,
                            current_stream());
    } else {
      launch_swizzle_x(x.data_ptr(), xs.data_ptr(), M, current_stream());
    }
    p.x0s = xs.data_ptr();
    p.w = {W1s.data_ptr(), b1f.data_ptr<float>(), W2s.data_ptr(),
           b2f.data_ptr<float>(), W3s.data_ptr(), b3f.data_ptr<float>(),
           w4.data_ptr(), b4f.data_ptr<float>()};
    p.a1t = f.a1t.data_ptr();
    p.mask1 = reinterpret_cast<uint32_t*>(f.mask1.data_ptr<int32_t>());
    p.a2t = f.a2t.data_ptr();
    p.mask2 = reinterpret_cast<uint32_t*>(f.mask2.data_ptr<int32_t>());
    p.a3 = f.a3.data_ptr();
    p.out = f.out.data_ptr();
    p.M = M;
    p.pi16 = pi16 ? 1 : 0;
    p.rows = rows;
    p.loss = loss;
    // the weighted head has nothing to weigh without a target
    p.weighted = hw.on && tgt != nullptr;
    p.weight = hw.weight;
    p.pos_weight = hw.pos_weight;
    launch_fwd_chain(p, current_stream());
  }
  return f;
}

std::vector<at::Tensor> fwd_chain_bf16(
    const at::Tensor& x, const at::Tensor& W1, const at::Tensor& b1,
    const at::Tensor& W2, const at::Tensor& b2, const at::Tensor& W3,
    const at::Tensor& b3, const at::Tensor& w4, const at::Tensor& b4,
    const c10::optional<at::Tensor>& target,
    const c10::optional<at::Tensor>& xt_out, bool pi16, int64_t rows,
    int64_t loss, const c10::optional<at::Tensor>& weight,
    double pos_weight) {
  const int crows = chain_rows(rows);
  const int closs = chain_loss(loss, "fwd_chain", "loss");
  // Sample weights / pos_weight of the loss epilogue (need a target).
  const HeadWeights hw =
      head_weights("fwd_chain", x, weight, pos_weight, closs);
  TORCH_CHECK(!hw.on || target.has_value(),
              "fwd_chain: weight / pos_weight need a target");
  check_x("fwd_chain", x);
  auto chk_w = [](const at::Tensor& W, int64_t n, int64_t k,
                  const char* nm) {
    TORCH_CHECK(W.is_cuda() && W.scalar_type() == at::kBFloat16 &&
                    W.dim() == 2 && W.size(0) == n && W.size(1) == k &&
                    W.is_contiguous(),
                "fwd_chain: ", nm, " must be contiguous bf16 [", n, ",", k,
                "]");
  };
  // W1 may arrive pre-padded [512,112] (cached by the fused-step driver)
  // or raw [512,100] (padded here, one kernel per call).
  const bool w1_padded = W1.size(1) == 112;
  chk_w(W1, 512, w1_padded ? 112 : 100, "W1");
  chk_w(W2, 256, 512, "W2");
  chk_w(W3, 128, 256, "W3");
  TORCH_CHECK(w4.numel() == 128 && w4.scalar_type() == at::kBFloat16 &&
                  w4.is_contiguous(),
              "fwd_chain: w4 must be contiguous bf16 [128]");
  auto fb = [](const at::Tensor& b, int64_t n) {
    TORCH_CHECK(b.numel() == n, "fwd_chain: bias size mismatch");
    return b.to(at::kFloat).contiguous();
  };
  auto b1f = fb(b1, 512), b2f = fb(b2, 256), b3f = fb(b3, 128),
       b4f = fb(b4, 1);
  const int64_t M = x.size(0);
  // The kernel's A-fragment loads need W1's k-dim padded 100 -> 112.
  auto W1p = w1_padded ? W1 : at::constant_pad_nd(W1, {0, 12}).contiguous();
  // Fused loss epilogue: with a target, the kernel also emits the bf16
  // loss gradient dyb and per-block loss partials (loss =
  // loss_part.sum()/M) — no eager loss/grad kernels. LOSS_MSE: dyb =
  // (2/M)(out - target), squared errors; LOSS_BCE: dyb = (1/M)
  // (sigmoid(out) - target), logistic losses (out is the logit).
  const bool with_loss = target.has_value();
  at::Tensor tgt;
  if (with_loss) {
    tgt = target->reshape({-1}).to(at::kFloat).contiguous();
    TORCH_CHECK(tgt.numel() == M, "fwd_chain: target size mismatch");
  }
  at::Tensor W1s, W2s, W3s;
  if (M > 0) {
    W1s = swizzle_frag(W1p);
    W2s = swizzle_frag(W2);
    W3s = swizzle_frag(W3);
  }
  auto f = run_fwd_chain(x, W1s, W2s, W3s, w4, b1f, b2f, b3f, b4f,
                         with_loss ? &tgt : nullptr, xt_out, pi16, crows,
                         closs, hw);
  if (with_loss) {
    return {f.a1t, f.mask1, f.a2t, f.mask2, f.a3, f.out, f.dyb,
            f.loss_part};
  }
  return {f.a1t, f.mask1, f.a2t, f.mask2, f.a3, f.out};
}


// EXPERIMENTAL round-2 fused backward chain (csrc/bwd_chain.hip):
// dgrad + relu mask + bias partials for the fixed TabularMLP
// architecture. Returns (dz1, dz2, dz3, db1, db2, db3, db4); the wgrads
// (dW_l = dz_l^T @ a_{l-1}) remain the caller's streaming kernels.
// Swizzle of W^T computed directly from model-layout W [K,N] (single
// strided copy, no intermediate transpose materialization).
static at::Tensor swizzle_frag_T(const at::Tensor& W) {
  int64_t K = W.size(0), N = W.size(1);
  TORCH_CHECK(K % 16 == 0 && N % 32 == 0, "swizzle_frag_T: bad shape");
  return W.view({K / 16, 2, 8, N / 32, 32})
      .permute({3, 0, 1, 4, 2})
      .contiguous()
      .view({-1});
}

constexpr int64_t kPartW = 512 + 256 + 128 + 1 + 256;
// Width padded to a 4-multiple for the float4 slab reduce; the 3 pad
// columns are never read back.
constexpr int64_t kPartWPad = (kPartW + 3) / 4 * 4;

// Buffers + launch of the backward chain, shared by bwd_chain_bf16 and
// fused_step_bf16. W3Ts/W2Ts are the fragment-major transposed weights.
struct BwdChainOut {
  at::Tensor dz1t, dz2t, dz3t, db_part;
};

BwdChainOut run_bwd_chain(const at::Tensor& dy, const at::Tensor& a3,
                          const at::Tensor& mask1, const at::Tensor& mask2,
                          const at::Tensor& w4c, const at::Tensor& W3Ts,
                          const at::Tensor& W2Ts, bool pi16, int rows) {
  BwdChainOut b;
  const int64_t M = dy.size(0);
  const int64_t mtiles = std::max<int64_t>((M + 31) / 32, 1);
  // dz outputs exist only transposed, in wgrad fragment-major layout.
  const int64_t mchunks = mtiles * 2;
  b.dz1t = at::empty({16 * mchunks * 512}, dy.options());
  b.dz2t = at::empty({8 * mchunks * 512}, dy.options());
  b.dz3t = at::empty({4 * mchunks * 512}, dy.options());
  const int64_t grid = bwd_chain_grid(M, rows);
  b.db_part = at::empty({std::max<int64_t>(grid, 1), kPartWPad},
                        dy.options().dtype(at::kFloat));
  if (M == 0) b.db_part.zero_();
  if (M > 0) {
    BwdChainArgs p{};
    p.dy = dy.data_ptr();
    p.a3 = a3.data_ptr();
    p.mask1 = mask1.data_ptr();
    p.mask2 = mask2.data_ptr();
    p.w4 = w4c.data_ptr();
    p.W3T = W3Ts.data_ptr();
    p.W2T = W2Ts.data_ptr();
    p.dz1t = b.dz1t.data_ptr();
    p.dz2t = b.dz2t.data_ptr();
    p.dz3t = b.dz3t.data_ptr();
    p.db_part = b.db_part.data_ptr<float>();
    p.M = M;
    p.pi16 = pi16 ? 1 : 0;
    p.rows = rows;
    launch_bwd_chain(p, current_stream());
  }
  return b;
}

std::vector<at::Tensor> bwd_chain_bf16(
    const at::Tensor& dy, const at::Tensor& a3, const at::Tensor& mask1,
    const at::Tensor& mask2, const at::Tensor& w4, const at::Tensor& W3,
    const at::Tensor& W2, bool pi16, int64_t rows) {
  const int crows = chain_rows(rows);
  const int64_t M = dy.size(0);
  const int64_t mtiles = std::max<int64_t>((M + 31) / 32, 1);
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16 &&
                  dy.numel() == M && dy.is_contiguous(),
              "bwd_chain: dy must be contiguous bf16 [M] or [M,1]");
  auto chk_a = [M](const at::Tensor& a, int64_t n, const char* nm) {
    TORCH_CHECK(a.is_cuda() && a.scalar_type() == at::kBFloat16 &&
                    a.dim() == 2 && a.size(0) == M && a.size(1) == n &&
                    a.is_contiguous(),
                "bwd_chain: ", nm, " must be contiguous bf16 [M,", n, "]");
  };
  chk_a(a3, 128, "a3");
  TORCH_CHECK(mask1.is_cuda() && mask1.scalar_type() == at::kInt &&
                  mask1.is_contiguous() && mask1.numel() == mtiles * 512,
              "bwd_chain: mask1 must be int32 [mtiles,512]");
  TORCH_CHECK(mask2.is_cuda() && mask2.scalar_type() == at::kInt &&
                  mask2.is_contiguous() && mask2.numel() == mtiles * 256,
              "bwd_chain: mask2 must be int32 [mtiles,256]");
  TORCH_CHECK(w4.numel() == 128 && w4.scalar_type() == at::kBFloat16,
              "bwd_chain: w4 must be bf16 [128]");
  // Weights may arrive pre-transposed ([256,128] / [512,256], cached by
  // the fused-step driver) or in model layout (transposed here per call).
  // The shapes are unambiguous between the two layouts.
  TORCH_CHECK(W3.scalar_type() == at::kBFloat16 &&
                  ((W3.size(0) == 128 && W3.size(1) == 256) ||
                   (W3.size(0) == 256 && W3.size(1) == 128)),
              "bwd_chain: W3 must be bf16 [128,256] or W3^T [256,128]");
  TORCH_CHECK(W2.scalar_type() == at::kBFloat16 &&
                  ((W2.size(0) == 256 && W2.size(1) == 512) ||
                   (W2.size(0) == 512 && W2.size(1) == 256)),
              "bwd_chain: W2 must be bf16 [256,512] or W2^T [512,256]");
  auto w4c = w4.contiguous();
  // Swizzled W^T fragments, computed directly from whichever layout was
  // passed (model [out,in] or pre-transposed [in,out]).
  auto W3Ts = (W3.size(0) == 128) ? swizzle_frag_T(W3.contiguous())
                                  : swizzle_frag(W3.contiguous());
  auto W2Ts = (W2.size(0) == 256) ? swizzle_frag_T(W2.contiguous())
                                  : swizzle_frag(W2.contiguous());
  auto bo = run_bwd_chain(dy, a3, mask1, mask2, w4c, W3Ts, W2Ts, pi16,
                          crows);
  auto& dz1t = bo.dz1t;
  auto& dz2t = bo.dz2t;
  auto& dz3t = bo.dz3t;
  auto& db_part = bo.db_part;
  // Column reduction with the split-slab reduce kernel (the GEMV ran at
  // ~0.9 TB/s; this streams the 28 MB slab near roofline). Pad columns
  // may sum garbage; they are never read.
  auto db_full = at::zeros({kPartWPad}, dy.options().dtype(at::kFloat));
  launch_slab_reduce(db_part.data_ptr<float>(), db_full.data_ptr<float>(),
                     kPartWPad, db_part.size(0), current_stream());
  auto db = db_full.narrow(0, 0, kPartW);
  auto dw4 = (db.narrow(0, 897, 128) + db.narrow(0, 897 + 128, 128))
                 .reshape({1, 128});
  return {dz1t,
          dz2t,
          dz3t,
          db.narrow(0, 0, 512),
          db.narrow(0, 512, 256),
          db.narrow(0, 512 + 256, 128),
          db.narrow(0, 512 + 256 + 128, 1),
          dw4};
}

// Per-slab fp32 partials of one fragment-major wgrad, [nslabs, N*K]:
// buffer + launch, shared by wgrad_frag_bf16 and fused_step_bf16.
// Requires mchunks > 0 and a tile config launch_wgrad_frag dispatches.
// ``variant``: 0 default, 1 direct kernel, 2 LDS-ring kernel.
at::Tensor run_wgrad_frag(const at::Tensor& AT, const at::Tensor& BT,
                          int64_t N, int64_t K, int64_t mchunks,
                          int64_t nt_w, int64_t kt_w, int64_t variant) {
  const int64_t nslabs = wgrad_frag_nslabs(mchunks, (int32_t)N, (int32_t)K,
                                           (int32_t)nt_w, (int32_t)kt_w);
  auto part = at::empty({nslabs, N * K}, AT.options().dtype(at::kFloat));
  launch_wgrad_frag(AT.data_ptr(), BT.data_ptr(), part.data_ptr<float>(),
                    (int32_t)N, (int32_t)K, mchunks, (int32_t)nt_w,
                    (int32_t)kt_w, (int32_t)variant, current_stream());
  return part;
}

// The step's three wgrads as one grouped launch (launch_wgrad_grouped):
// (part1, part2, part3), each [ns_i, N*K] fp32. Requires mchunks > 0.
std::vector<at::Tensor> run_wgrad_grouped(
    const at::Tensor& dz1t, const at::Tensor& xt, const at::Tensor& dz2t,
    const at::Tensor& a1t, const at::Tensor& dz3t, const at::Tensor& a2t,
    int64_t mchunks) {
  const WgradGroupedSlabs ns = wgrad_grouped_nslabs(mchunks);
  auto f32 = dz1t.options().dtype(at::kFloat);
  auto p1 = at::empty({ns.ns[0], 512 * 128}, f32);
  auto p2 = at::empty({ns.ns[1], 256 * 512}, f32);
  auto p3 = at::empty({ns.ns[2], 128 * 256}, f32);
  launch_wgrad_grouped(dz1t.data_ptr(), xt.data_ptr(), p1.data_ptr<float>(),
                       dz2t.data_ptr(), a1t.data_ptr(), p2.data_ptr<float>(),
                       dz3t.data_ptr(), a2t.data_ptr(), p3.data_ptr<float>(),
                       mchunks, current_stream());
  return {p1, p2, p3};
}

void check_wgrad_frag(const at::Tensor& AT, const at::Tensor& BT, int64_t N,
                      int64_t K, int64_t mchunks, int64_t nt_w, int64_t kt_w,
                      int64_t variant) {
  TORCH_CHECK(AT.is_cuda() && AT.scalar_type() == at::kBFloat16 &&
                  AT.is_contiguous() && BT.is_cuda() &&
                  BT.scalar_type() == at::kBFloat16 && BT.is_contiguous(),
              "wgrad_frag: inputs must be contiguous bf16 on GPU");
  TORCH_CHECK(AT.numel() == (N / 32) * mchunks * 512,
              "wgrad_frag: AT numel mismatch");
  TORCH_CHECK(BT.numel() == (K / 32) * mchunks * 512,
              "wgrad_frag: BT numel mismatch");
  // Must list every config launch_wgrad_frag dispatches (an unlisted one
  // would fall through its if-chain and leave the partials unwritten).
  TORCH_CHECK((nt_w == 2 && kt_w == 4) || (nt_w == 1 && kt_w == 8) ||
                  (nt_w == 1 && kt_w == 4),
              "wgrad_frag: unsupported tile config");
  TORCH_CHECK(N % (nt_w * 128) == 0 && K % (kt_w * 32) == 0,
              "wgrad_frag: N/K not divisible by block shape");
  TORCH_CHECK(variant >= 0 && variant <= 2,
              "wgrad_frag: variant must be 0 (default), 1 (direct) or 2 "
              "(LDS ring), got ", variant);
  TORCH_CHECK(variant != 2 ||
                  wgrad_frag_has_lds((int32_t)nt_w, (int32_t)kt_w),
              "wgrad_frag: no LDS-ring kernel for tile config (", nt_w, ",",
              kt_w, ")");
}

}  // namespace
// x [M,100] -> wgrad fragment-major x^T ([128/32][mchunks][2][32][8],
// zero-padded cols 100..127 and rows past M) for the dW1 wgrad.
at::Tensor swizzle_xt_bf16(const at::Tensor& x, bool pi16) {
  check_x("swizzle_xt", x);
  const int64_t M = x.size(0);
  const int64_t mtiles = std::max<int64_t>((M + 31) / 32, 1);
  auto out = at::empty({4 * mtiles * 2 * 512}, x.options());
  if (M > 0) {
    launch_swizzle_xt(x.data_ptr(), out.data_ptr(), M, pi16 ? 1 : 0,
                      current_stream());
  }
  return out;
}

// Fragment-major wgrad (csrc/wgrad_frag.hip): dW = dz^T @ src with both
// inputs pre-swizzled to [C/32][Mp/16][2][32][8] fragment layout.
at::Tensor wgrad_frag_bf16(const at::Tensor& AT, const at::Tensor& BT,
                           int64_t N, int64_t K, int64_t mchunks,
                           int64_t nt_w, int64_t kt_w, int64_t variant) {
  check_wgrad_frag(AT, BT, N, K, mchunks, nt_w, kt_w, variant);
  auto dW = at::zeros({N, K}, AT.options().dtype(at::kFloat));
  if (mchunks > 0) {
    // Per-slab fp32 partials + split-slab reduce (atomic combine over
    // <= a handful of writers per line).
    auto part = run_wgrad_frag(AT, BT, N, K, mchunks, nt_w, kt_w, variant);
    const int64_t nslabs = part.size(0);
    launch_slab_reduce(part.data_ptr<float>(), dW.data_ptr<float>(),
                       N * K, nslabs, current_stream());
  }
  return dW;
}

// The raw per-slab partials [nslabs, N*K] of the same launch, unreduced:
// unlike the atomically combined output above they are bit-stable, so two
// kernel variants can be compared with torch.equal.
at::Tensor wgrad_frag_partials_bf16(const at::Tensor& AT,
                                    const at::Tensor& BT, int64_t N,
                                    int64_t K, int64_t mchunks, int64_t nt_w,
                                    int64_t kt_w, int64_t variant) {
  check_wgrad_frag(AT, BT, N, K, mchunks, nt_w, kt_w, variant);
  TORCH_CHECK(mchunks > 0, "wgrad_frag_partials: mchunks must be positive");
  return run_wgrad_frag(AT, BT, N, K, mchunks, nt_w, kt_w, variant);
}

// The per-slab partials (part1 [ns1, 512*128], part2 [ns2, 256*512], part3
// [ns3, 128*256]) of the train step's three wgrads run as ONE grouped
// launch (csrc/wgrad_frag.hip, wgrad_grouped_kernel): dW1 = dz1^T x,
// dW2 = dz2^T a1, dW3 = dz3^T a2, every input in the fragment layout of
// wgrad_frag_bf16. Slab s of problem i covers chunks [s * cps_i,
// min((s + 1) * cps_i, mchunks)) with cps_i = ceil(mchunks / ns_i).
std::vector<at::Tensor> wgrad_grouped_partials_bf16(
    const at::Tensor& dz1t, const at::Tensor& xt, const at::Tensor& dz2t,
    const at::Tensor& a1t, const at::Tensor& dz3t, const at::Tensor& a2t,
    int64_t mchunks) {
  TORCH_CHECK(mchunks > 0, "wgrad_grouped_partials: mchunks must be positive");
  check_wgrad_frag(dz1t, xt, 512, 128, mchunks, 2, 4, 0);
  check_wgrad_frag(dz2t, a1t, 256, 512, mchunks, 1, 8, 0);
  check_wgrad_frag(dz3t, a2t, 128, 256, mchunks, 1, 8, 0);
  return run_wgrad_grouped(dz1t, xt, dz2t, a1t, dz3t, a2t, mchunks);
}

// ---------------------------------------------------------------------
// Fused-step glue (csrc/step_glue.hip): one prep launch ahead of the
// chain kernels, one finalize launch behind the wgrads.
// ---------------------------------------------------------------------
namespace {

void check_master(const std::vector<at::Tensor>& w, const char* who) {
  TORCH_CHECK(w.size() == 4, who, ": weights must be [W1, W2, W3, w4]");
  const int64_t shp[4][2] = {{512, 100}, {256, 512}, {128, 256}, {1, 128}};
  for (int i = 0; i < 4; i++) {
    TORCH_CHECK(w[i].is_cuda() && w[i].scalar_type() == at::kFloat &&
                    w[i].is_contiguous() &&
                    w[i].numel() == shp[i][0] * shp[i][1] &&
                    (i == 3 || (w[i].dim() == 2 && w[i].size(0) == shp[i][0])),
                who, ": weight ", i, " must be contiguous fp32 [", shp[i][0],
                ",", shp[i][1], "] on GPU");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(w[i].data_ptr()) % 16 == 0,
                who, ": weight ", i, " must be 16-byte aligned");
  }
}

struct PrepOut {
  at::Tensor W1s, W2s, W3s, W2Ts, W3Ts, w4b, tgt;
};

// ``bufs``: optional caller buffers for the six bf16 outputs. ``target``
// fp32 passes through untouched (no launch work); fp64 is cast in-kernel.
// ``bufs_valid``: the caller's buffers already hold the images of ``w``
// (kept so by the update kernels), so only the target is cast, and
// nothing is launched for an fp32 one.
PrepOut run_step_prep(const std::vector<at::Tensor>& w,
                      const c10::optional<at::Tensor>& target,
                      const c10::optional<std::vector<at::Tensor>>& bufs,
                      bool bufs_valid = false) {
  check_master(w, "step_prep");
  TORCH_CHECK(!bufs_valid || bufs.has_value(),
              "step_prep: bufs_valid needs the caller's buffers");
  const int64_t numel[6] = {512 * 112, 256 * 512, 128 * 256,
                            256 * 512, 128 * 256, 128};
  at::Tensor o[6];
  auto bf = w[0].options().dtype(at::kBFloat16);
  if (bufs.has_value()) {
    TORCH_CHECK(bufs->size() == 6, "step_prep: need six output buffers");
  }
  for (int i = 0; i < 6; i++) {
    if (bufs.has_value()) {
      o[i] = (*bufs)[i];
      TORCH_CHECK(o[i].is_cuda() && o[i].scalar_type() == at::kBFloat16 &&
                      o[i].is_contiguous() && o[i].numel() == numel[i] &&
                      reinterpret_cast<uintptr_t>(o[i].data_ptr()) % 16 == 0,
                  "step_prep: output buffer ", i,
                  " must be contiguous aligned bf16 with ", numel[i],
                  " elements");
    } else {
      o[i] = at::empty({numel[i]}, bf);
    }
  }
  PrepOut r{o[0], o[1], o[2], o[3], o[4], o[5], at::Tensor()};
  StepPrepArgs p{};
  p.b0 = bufs_valid ? step_prep_target_only() : 0;
  p.W1 = w[0].data_ptr<float>();
  p.W2 = w[1].data_ptr<float>();
  p.W3 = w[2].data_ptr<float>();
  p.w4 = w[3].data_ptr<float>();
  p.W1s = reinterpret_cast<uint16_t*>(o[0].data_ptr());
  p.W2s = reinterpret_cast<uint16_t*>(o[1].data_ptr());
  p.W3s = reinterpret_cast<uint16_t*>(o[2].data_ptr());
  p.W2Ts = reinterpret_cast<uint16_t*>(o[3].data_ptr());
  p.W3Ts = reinterpret_cast<uint16_t*>(o[4].data_ptr());
  p.w4b = reinterpret_cast<uint16_t*>(o[5].data_ptr());
  if (target.has_value()) {
    TORCH_CHECK(target->is_cuda() &&
                    (target->scalar_type() == at::kFloat ||
                     target->scalar_type() == at::kDouble),
                "step_prep: target must be fp32 or fp64 on GPU");
    auto t = target->reshape({-1}).contiguous();
    if (t.scalar_type() == at::kDouble) {
      r.tgt = at::empty({t.numel()}, t.options().dtype(at::kFloat));
      p.tgt64 = t.data_ptr<double>();
      p.tgt32 = r.tgt.data_ptr<float>();
      p.M = t.numel();
    } else {
      r.tgt = t;
    }
  }
  launch_step_prep(p, current_stream());
  return r;
}

// outs (optional): [dW1, dW2, dW3, dW4, db1, db2, db3, db4] contiguous
// fp32. Returns [loss, dW1, dW2, dW3, dW4, db1, db2, db3, db4]. With
// ``opt`` (validated by make_step_opt) the launch is step_finalize_update
// of that kind.
std::vector<at::Tensor> run_step_finalize(
    const at::Tensor& part1, const at::Tensor& part2,
    const at::Tensor& part3, const at::Tensor& db_part,
    const at::Tensor& loss_part, int64_t M,
    const c10::optional<std::vector<at::Tensor>>& outs,
    const StepOptArgs* opt = nullptr, int kind = 0) {
  auto chk = [](const at::Tensor& t, int64_t w, const char* nm) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                    t.is_contiguous() && t.dim() == 2 && t.size(1) == w &&
                    t.size(0) >= 1 &&
                    reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                "step_finalize: ", nm, " must be contiguous fp32 [rows>=1, ",
                w, "] on GPU");
  };
  chk(part1, 512 * 128, "part1");
  chk(part2, 256 * 512, "part2");
  chk(part3, 128 * 256, "part3");
  chk(db_part, kPartWPad, "db_part");
  TORCH_CHECK(loss_part.is_cuda() && loss_part.scalar_type() == at::kFloat &&
                  loss_part.is_contiguous(),
              "step_finalize: loss_part must be contiguous fp32 on GPU");
  TORCH_CHECK(M >= 1, "step_finalize: M must be positive");
  const std::vector<std::vector<int64_t>> shp = {
      {512, 100}, {256, 512}, {128, 256}, {1, 128},
      {512},      {256},      {128},      {1}};
  std::vector<at::Tensor> o(8);
  auto f32 = part1.options();
  if (outs.has_value()) {
    TORCH_CHECK(outs->size() == 8, "step_finalize: need eight outputs");
  }
  for (int i = 0; i < 8; i++) {
    if (outs.has_value()) {
      o[i] = (*outs)[i];
      int64_t n = 1;
      for (auto d : shp[i]) n *= d;
      TORCH_CHECK(o[i].is_cuda() && o[i].scalar_type() == at::kFloat &&
                      o[i].is_contiguous() && o[i].numel() == n,
                  "step_finalize: output ", i,
                  " must be contiguous fp32 with ", n, " elements");
      TORCH_CHECK(i >= 3 ||
                      reinterpret_cast<uintptr_t>(o[i].data_ptr()) % 16 == 0,
                  "step_finalize: output ", i, " must be 16-byte aligned");
    } else {
      o[i] = at::empty(shp[i], f32);
    }
  }
  auto loss = at::empty({}, f32);
  StepFinArgs p{};
  p.part1 = part1.data_ptr<float>();
  p.part2 = part2.data_ptr<float>();
  p.part3 = part3.data_ptr<float>();
  p.db_part = db_part.data_ptr<float>();
  p.loss_part = loss_part.data_ptr<float>();
  p.ns1 = part1.size(0);
  p.ns2 = part2.size(0);
  p.ns3 = part3.size(0);
  p.db_rows = db_part.size(0);
  p.loss_n = loss_part.numel();
  p.M = M;
  p.dw1 = o[0].data_ptr<float>();
  p.dw2 = o[1].data_ptr<float>();
  p.dw3 = o[2].data_ptr<float>();
  p.dw4 = o[3].data_ptr<float>();
  p.db1 = o[4].data_ptr<float>();
  p.db2 = o[5].data_ptr<float>();
  p.db3 = o[6].data_ptr<float>();
  p.db4 = o[7].data_ptr<float>();
  p.loss = loss.data_ptr<float>();
  if (opt != nullptr) {
    launch_step_finalize_update(p, *opt, kind, current_stream());
  } else {
    launch_step_finalize(p, current_stream());
  }
  return {loss, o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]};
}

// Element counts in the parameter order of StepOptArgs.
constexpr int64_t kParamNumel[8] = {512 * 100, 256 * 512, 128 * 256, 128,
                                    512,       256,       128,       1};

// One of the eight fp32 tensors of ``what`` (gradients, a state slot):
// contiguous, the parameter's element count, on ``dev``; the three large
// matrices are accessed as float4.
void check_param_like(const char* who, const char* what, int64_t idx, int i,
                      const at::Tensor& t, int dev) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                  t.is_contiguous() && t.numel() == kParamNumel[i] &&
                  t.get_device() == dev,
              who, ": ", what, " ", idx, " must be contiguous fp32 with ",
              kParamNumel[i], " elements on the weights' GPU");
  TORCH_CHECK(i >= 3 || reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              who, ": ", what, " ", idx, " must be 16-byte aligned");
}

// Validated launch arguments of the update kernels (csrc/step_glue.hip).
// ``state``: 8 momentum buffers for SGD with momentum, none without, and
// 8 first then 8 second moments for AdamW, in parameter order. ``staged``:
// the six bf16 buffers of step_prep. ``hyper``: the h[] of step_glue.h,
// each rounded to fp32 here.
StepOptArgs make_step_opt(const char* who,
                          const std::vector<at::Tensor>& weights,
                          const std::vector<at::Tensor>& biases,
                          const std::vector<at::Tensor>& state,
                          const std::vector<at::Tensor>& staged,
                          int64_t kind, const std::vector<double>& hyper) {
  TORCH_CHECK(kind == kOptSgd || kind == kOptAdamW, who,
              ": kind must be OPT_SGD or OPT_ADAMW, got ", kind);
  const size_t nh = kind == kOptSgd ? 5 : 8;
  TORCH_CHECK(hyper.size() == nh, who, ": hyper must hold ", nh,
              " values for this kind, got ", hyper.size());
  check_master(weights, who);
  const int dev = weights[0].get_device();
  for (int i = 1; i < 4; i++) {
    TORCH_CHECK(weights[i].get_device() == dev, who, ": weight ", i,
                " must be on weight 0's GPU");
  }
  check_biases(who, biases, dev);
  StepOptArgs a{};
  for (size_t i = 0; i < nh; i++) a.h[i] = (float)hyper[i];
  const size_t ns = kind == kOptAdamW ? 16 : a.h[2] != 0.f ? 8 : 0;
  TORCH_CHECK(state.size() == ns, who, ": state must hold ", ns,
              " tensors for this kind and momentum, got ", state.size());
  for (size_t s = 0; s < ns; s++) {
    const int i = (int)(s % 8);
    check_param_like(who, "state", (int64_t)s, i, state[s], dev);
    (s < 8 ? a.s1 : a.s2)[i] = state[s].data_ptr<float>();
  }
  const int64_t sn[6] = {512 * 112, 256 * 512, 128 * 256,
                         256 * 512, 128 * 256, 128};
  TORCH_CHECK(staged.size() == 6, who, ": need six staged buffers");
  for (int i = 0; i < 6; i++) {
    const at::Tensor& t = staged[i];
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                    t.is_contiguous() && t.numel() == sn[i] &&
                    t.get_device() == dev &&
                    reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                who, ": staged buffer ", i,
                " must be contiguous aligned bf16 with ", sn[i],
                " elements on the weights' GPU");
    a.stg[i] = reinterpret_cast<uint16_t*>(t.data_ptr());
  }
  for (int i = 0; i < 4; i++) {
    a.prm[i] = weights[i].data_ptr<float>();
    a.prm[4 + i] = biases[i].data_ptr<float>();
  }
  return a;
}

// The update kernels write masters and state behind autograd's back: bump
// the version counters (shared with the parameters the detached views
// came from), so caches keyed on ``_version`` see the write.
void bump_versions(const std::vector<at::Tensor>& a,
                   const std::vector<at::Tensor>& b,
                   const std::vector<at::Tensor>& c) {
  for (const auto* v : {&a, &b, &c}) {
    for (const auto& t : *v) t.unsafeGetTensorImpl()->bump_version();
  }
}

}  // namespace

// [W1s, W2s, W3s, W2Ts, W3Ts, w4 bf16] (+ fp32 target when one is given).
std::vector<at::Tensor> step_prep(
    const std::vector<at::Tensor>& weights,
    const c10::optional<at::Tensor>& target,
    const c10::optional<std::vector<at::Tensor>>& outs) {
  auto r = run_step_prep(weights, target, outs);
  std::vector<at::Tensor> v = {r.W1s, r.W2s, r.W3s, r.W2Ts, r.W3Ts, r.w4b};
  if (target.has_value()) v.push_back(r.tgt);
  return v;
}

std::vector<at::Tensor> step_finalize(
    const at::Tensor& part1, const at::Tensor& part2,
    const at::Tensor& part3, const at::Tensor& db_part,
    const at::Tensor& loss_part, int64_t M,
    const c10::optional<std::vector<at::Tensor>>& outs) {
  return run_step_finalize(part1, part2, part3, db_part, loss_part, M, outs);
}

// step_finalize, then the SGD / AdamW update of every parameter from the
// gradient just stored, in the same launch: masters ``weights`` /
// ``biases`` and ``state`` in place, plus the bf16 images of the new
// weights in ``staged`` (make_step_opt). Returns what step_finalize does.
std::vector<at::Tensor> step_finalize_update(
    const at::Tensor& part1, const at::Tensor& part2,
    const at::Tensor& part3, const at::Tensor& db_part,
    const at::Tensor& loss_part, int64_t M,
    const c10::optional<std::vector<at::Tensor>>& outs,
    const std::vector<at::Tensor>& weights,
    const std::vector<at::Tensor>& biases,
    const std::vector<at::Tensor>& state,
    const std::vector<at::Tensor>& staged, int64_t kind,
    const std::vector<double>& hyper) {
  const StepOptArgs a = make_step_opt("step_finalize_update", weights,
                                      biases, state, staged, kind, hyper);
  TORCH_CHECK(part1.is_cuda() && part1.get_device() == weights[0].get_device(),
              "step_finalize_update: part1 must be on the weights' GPU");
  auto r = run_step_finalize(part1, part2, part3, db_part, loss_part, M, outs,
                             &a, (int)kind);
  bump_versions(weights, biases, state);
  return r;
}

// The same update from already folded gradients ``grads`` = [dW1, dW2,
// dW3, dW4, db1..db4] (finalize -> all-reduce -> update, grad_hook steps,
// gradients from elsewhere). One launch; outputs as step_finalize_update.
void step_update(const std::vector<at::Tensor>& grads,
                 const std::vector<at::Tensor>& weights,
                 const std::vector<at::Tensor>& biases,
                 const std::vector<at::Tensor>& state,
                 const std::vector<at::Tensor>& staged, int64_t kind,
                 const std::vector<double>& hyper) {
  StepOptArgs a = make_step_opt("step_update", weights, biases, state,
                                staged, kind, hyper);
  TORCH_CHECK(grads.size() == 8, "step_update: need eight gradients");
  for (int i = 0; i < 8; i++) {
    check_param_like("step_update", "grad", i, i, grads[i],
                     weights[0].get_device());
    a.grad[i] = grads[i].data_ptr<float>();
  }
  launch_step_update(a, (int)kind, current_stream());
  bump_versions(weights, biases, state);
}

// ``opt=`` of fused_step_bf16: (state, staged, staged_valid, kind, hyper),
// the arguments of step_finalize_update plus whether ``staged`` already
// holds the images of ``weights``.
using StepOpt = std::tuple<std::vector<at::Tensor>, std::vector<at::Tensor>,
                           bool, int64_t, std::vector<double>>;

// The whole fused train step of the stock TabularMLP(100-512-256-128-1)
// in 6 launches: prep -> x swizzle -> fwd chain -> bwd chain -> the three
// fragment wgrads into slab partials as one grouped launch (three
// launches, 8 in all, with wgrad_variant 1 or 2 or the grouped launch
// off) -> finalize. fp32 master
// ``weights`` [W1, W2, W3, w4] and ``biases`` [b1..b4] are read
// directly. Returns [loss, dW1, dW2, dW3, dW4, db1, db2, db3, db4];
// with ``outs`` the eight gradients are written into the caller's
// tensors (same order). No sync, no host read: graph-capture safe.
//
// With ``opt`` (StepOpt) the step also applies the optimizer: the weights
// are staged into the caller's persistent ``staged`` buffers, by step_prep
// only when ``staged_valid`` is false (an fp64 target is still cast), and
// the step ends in step_finalize_update, which keeps them current.
// Without ``opt`` the launches are exactly those above.
std::vector<at::Tensor> fused_step_bf16(
    const at::Tensor& x, const at::Tensor& target,
    const std::vector<at::Tensor>& weights,
    const std::vector<at::Tensor>& biases, bool pi16,
    const c10::optional<std::vector<at::Tensor>>& outs, int64_t rows,
    int64_t loss, const c10::optional<at::Tensor>& weight,
    double pos_weight, int64_t wgrad_variant, int64_t wgrad_grouped,
    const c10::optional<StepOpt>& opt) {
  const int crows = chain_rows(rows);
  const int closs = chain_loss(loss, "fused_step", "loss");
  TORCH_CHECK(wgrad_variant >= 0 && wgrad_variant <= 2,
              "fused_step: wgrad_variant must be 0, 1 or 2, got ",
              wgrad_variant);
  TORCH_CHECK(wgrad_grouped >= -1 && wgrad_grouped <= 1,
              "fused_step: wgrad_grouped must be -1 (default), 0 or 1, got ",
              wgrad_grouped);
  TORCH_CHECK(wgrad_grouped != 1 || wgrad_variant == 0,
              "fused_step: wgrad_grouped=1 needs wgrad_variant 0");
  const HeadWeights hw =
      head_weights("fused_step", x, weight, pos_weight, closs);
  check_x("fused_step", x);
  const int64_t M = x.size(0);
  TORCH_CHECK(M > 0, "fused_step: empty batch");
  TORCH_CHECK(target.numel() == M, "fused_step: target size mismatch");
  check_biases("fused_step", biases);
  StepOptArgs oa{};
  c10::optional<std::vector<at::Tensor>> stage_bufs;
  if (opt.has_value()) {
    oa = make_step_opt("fused_step", weights, biases, std::get<0>(*opt),
                       std::get<1>(*opt), std::get<3>(*opt),
                       std::get<4>(*opt));
    TORCH_CHECK(weights[0].get_device() == x.get_device(),
                "fused_step: weight 0 must be on x's GPU");
    stage_bufs = std::get<1>(*opt);
  }
  const StepOptArgs* oap = opt.has_value() ? &oa : nullptr;
  const int okind = opt.has_value() ? (int)std::get<3>(*opt) : 0;
  auto finalize = [&](const at::Tensor& p1, const at::Tensor& p2,
                      const at::Tensor& p3, const at::Tensor& db_part,
                      const at::Tensor& loss_part) {
    auto r = run_step_finalize(p1, p2, p3, db_part, loss_part, M, outs, oap,
                               okind);
    if (opt.has_value()) bump_versions(weights, biases, std::get<0>(*opt));
    return r;
  };
  auto pr = run_step_prep(weights, target, stage_bufs,
                          opt.has_value() && std::get<2>(*opt));
  const int64_t mchunks = 2 * ((M + 31) / 32);
  c10::optional<at::Tensor> xt =
      at::empty({4 * mchunks * 512}, x.options());
  auto f = run_fwd_chain(x, pr.W1s, pr.W2s, pr.W3s, pr.w4b, biases[0],
                         biases[1], biases[2], biases[3], &pr.tgt, xt, pi16,
                         crows, closs, hw);
  auto b = run_bwd_chain(f.dyb, f.a3, f.mask1, f.mask2, pr.w4b, pr.W3Ts,
                         pr.W2Ts, pi16, crows);
  // Same tile-config choice as ops.shuffle_ops.wgrad_frag.
  const char* st = std::getenv("RSDL_WGRAD_SMALL_TILES");
  const int64_t kt23 = (st != nullptr && std::strcmp(st, "1") == 0) ? 4 : 8;
  // wgrad_variant 0 (what callers pass outside tests) = the default of
  // launch_wgrad_frag. The small tiles have the direct kernel only, and
  // the launcher keeps them on it whatever the variant.
  const int64_t wv = wgrad_variant;  // 0 | 1 | 2, checked above
  // At variant 0 the three wgrads are one grouped launch, unless
  // RSDL_WGRAD_GROUPED=0 or a tuning knob of the separate launches asks
  // for those (wgrad_grouped_default); wgrad_grouped 0 / 1 decides it for
  // this call. Only the slab partition, so the grouping of the fp32 sums
  // of dW1-dW3, differs between the two.
  if (wv == 0 &&
      (wgrad_grouped < 0 ? wgrad_grouped_default() : wgrad_grouped == 1)) {
    auto p = run_wgrad_grouped(b.dz1t, *xt, b.dz2t, f.a1t, b.dz3t, f.a2t,
                               mchunks);
    return finalize(p[0], p[1], p[2], b.db_part, f.loss_part);
  }
  auto p1 = run_wgrad_frag(b.dz1t, *xt, 512, 128, mchunks, 2, 4, wv);
  auto p2 = run_wgrad_frag(b.dz2t, f.a1t, 256, 512, mchunks, 1, kt23, wv);
  auto p3 = run_wgrad_frag(b.dz3t, f.a2t, 128, 256, mchunks, 1, kt23, wv);
  return finalize(p1, p2, p3, b.db_part, f.loss_part);
}

// Forward-only evaluation of the stock TabularMLP (csrc/fwd_chain.hip,
// eval_chain_kernel): x swizzle + one chain launch that writes fp32
// predictions and/or four metric partials per workgroup, and none of the
// training by-products. ``Wstage`` = [W1s, W2s, W3s, w4b], the bf16
// fragment-major buffers step_prep produces (staged once by the caller,
// not per call); ``biases`` fp32, read directly. ``target`` fp32 or fp64
// (cast to fp32 first) with M elements -> part fp32 [grid, 4] =
// {sum (o-t)^2, sum |o-t|, sum t, sum t^2} per slab of ``rows`` rows;
// column 0 is bit-identical to fwd_chain_bf16's loss_part. ``pred_out``:
// caller-owned contiguous fp32 with M elements (may be a view into a
// larger buffer). ``task`` = 1 (binary classification, the head value is
// a logit): part = {sum logloss, sum (sigmoid - t)^2, sum t, sum correct},
// column 0 bit-identical to fwd_chain_bf16(loss=LOSS_BCE)'s loss_part;
// with ``hist`` (int64 [2,65536] on x's GPU, caller-owned and persistent)
// each row also adds 1 to hist[t >= 0.5][key of the logit] with integer
// atomics — the streaming-AUC histogram (csrc/fwd_chain.hip).
// ``weight`` (fp32 [M] on x's GPU, needs a target): the weighted kernel —
// every term scaled by w, part fp32 [grid, 8] = {the four sums, sum w, 0,
// 0, 0}, and the histogram adds llrintf(w * 2^20) in place of 1.
// Returns (pred or None, part or None). No sync, no host
// read: graph-capture safe.
std::tuple<c10::optional<at::Tensor>, c10::optional<at::Tensor>>
eval_chain_bf16(const at::Tensor& x, const std::vector<at::Tensor>& Wstage,
                const std::vector<at::Tensor>& biases,
                const c10::optional<at::Tensor>& target,
                const c10::optional<at::Tensor>& pred_out, bool want_pred,
                int64_t rows, int64_t task,
                const c10::optional<at::Tensor>& hist,
                const c10::optional<at::Tensor>& weight) {
  const int crows = chain_rows(rows);
  const int ctask = chain_loss(task, "eval_chain", "task");
  check_x("eval_chain", x);
  const int64_t M = x.size(0);
  TORCH_CHECK(Wstage.size() == 4,
              "eval_chain: Wstage must be [W1s, W2s, W3s, w4b]");
  const int64_t wn[4] = {512 * 112, 256 * 512, 128 * 256, 128};
  for (int i = 0; i < 4; i++) {
    TORCH_CHECK(Wstage[i].is_cuda() &&
                    Wstage[i].scalar_type() == at::kBFloat16 &&
                    Wstage[i].is_contiguous() && Wstage[i].numel() == wn[i] &&
                    Wstage[i].get_device() == x.get_device() &&
                    reinterpret_cast<uintptr_t>(Wstage[i].data_ptr()) % 16 ==
                        0,
                "eval_chain: staged weight ", i,
                " must be contiguous aligned bf16 with ", wn[i],
                " elements on x's GPU");
  }
  check_biases("eval_chain", biases, x.get_device());
  const bool with_pred = want_pred || pred_out.has_value();
  TORCH_CHECK(with_pred || target.has_value(),
              "eval_chain: nothing to compute (no target, no predictions)");
  at::Tensor tgt, pred, part;
  if (target.has_value()) {
    TORCH_CHECK(target->is_cuda() &&
                    target->get_device() == x.get_device() &&
                    (target->scalar_type() == at::kFloat ||
                     target->scalar_type() == at::kDouble),
                "eval_chain: target must be fp32 or fp64 on x's GPU");
    TORCH_CHECK(target->numel() == M, "eval_chain: target size mismatch");
    tgt = target->reshape({-1}).to(at::kFloat).contiguous();
  }
  if (pred_out.has_value()) {
    TORCH_CHECK(pred_out->is_cuda() &&
                    pred_out->get_device() == x.get_device() &&
                    pred_out->scalar_type() == at::kFloat &&
                    pred_out->is_contiguous() && pred_out->numel() == M,
                "eval_chain: pred_out must be contiguous fp32 with ", M,
                " elements on x's GPU");
    pred = *pred_out;
  } else if (with_pred) {
    pred = at::empty({M}, x.options().dtype(at::kFloat));
  }
  if (hist.has_value()) {
    TORCH_CHECK(ctask == kLossBce && target.has_value(),
                "eval_chain: hist needs task=1 and a target");
    TORCH_CHECK(hist->is_cuda() && hist->get_device() == x.get_device() &&
                    hist->scalar_type() == at::kLong &&
                    hist->is_contiguous() && hist->dim() == 2 &&
                    hist->size(0) == 2 && hist->size(1) == 65536,
                "eval_chain: hist must be contiguous int64 [2,65536] on "
                "x's GPU");
  }
  // ``weight`` (fp32 [M]): the weighted kernel, part fp32 [grid, 8] =
  // {the four sums with every term scaled by w, sum w, 0, 0, 0}, and the
  // histogram adds llrintf(w * 2^20) in place of 1.
  TORCH_CHECK(!weight.has_value() || target.has_value(),
              "eval_chain: weight needs a target");
  const HeadWeights hw = head_weights("eval_chain", x, weight, 1.0, ctask);
  const int64_t pcols = hw.on ? 8 : 4;
  const int64_t grid = M > 0 ? fwd_chain_grid(M, crows) : 0;
  if (target.has_value()) {
    part = M > 0 ? at::empty({grid, pcols}, x.options().dtype(at::kFloat))
                 : at::zeros({1, pcols}, x.options().dtype(at::kFloat));
  }
  if (M > 0) {
    const int64_t Mp = (M + 31) / 32 * 32;
    auto xs = at::empty({Mp * 112}, x.options());
    launch_swizzle_x(x.data_ptr(), xs.data_ptr(), M, current_stream());
    EvalChainArgs p{};
    p.x0s = xs.data_ptr();
    p.w = {Wstage[0].data_ptr(), biases[0].data_ptr<float>(),
           Wstage[1].data_ptr(), biases[1].data_ptr<float>(),
           Wstage[2].data_ptr(), biases[2].data_ptr<float>(),
           Wstage[3].data_ptr(), biases[3].data_ptr<float>()};
    if (with_pred) p.pred = pred.data_ptr<float>();
    if (target.has_value()) {
      p.target = tgt.data_ptr<float>();
      p.part = part.data_ptr<float>();
    }
    p.M = M;
    p.rows = crows;
    p.task = ctask;
    if (hist.has_value()) p.hist = hist->data_ptr<int64_t>();
    p.weighted = hw.on;
    p.weight = hw.weight;
    launch_eval_chain(p, current_stream());
  }
  c10::optional<at::Tensor> po, pa;
  if (with_pred) po = pred;
  if (target.has_value()) pa = part;
  return {po, pa};
}

// acc[5] = {rows, sse, sae, sum_t, sum_tt} (fp64, persistent) += M and
// the column sums of ``part`` [n, 4], in place, one launch, fixed order
// (csrc/step_glue.hip). The weighted chain's ``part`` [n, 8] folds into
// acc[6] = {rows, c0..c3, sum w} the same way.
void eval_accumulate(const at::Tensor& part, const at::Tensor& acc,
                     int64_t M) {
  TORCH_CHECK(part.is_cuda() && part.scalar_type() == at::kFloat &&
                  part.is_contiguous() && part.dim() == 2 &&
                  (part.size(1) == 4 || part.size(1) == 8) &&
                  reinterpret_cast<uintptr_t>(part.data_ptr()) % 16 == 0,
              "eval_accumulate: part must be contiguous aligned fp32 [n,4] "
              "(or [n,8], weighted) on GPU");
  const bool wide = part.size(1) == 8;
  TORCH_CHECK(acc.is_cuda() && acc.scalar_type() == at::kDouble &&
                  acc.is_contiguous() && acc.numel() == (wide ? 6 : 5) &&
                  acc.get_device() == part.get_device(),
              "eval_accumulate: acc must be contiguous fp64 [",
              wide ? 6 : 5, "] on part's GPU");
  TORCH_CHECK(M >= 0, "eval_accumulate: M must not be negative");
  launch_eval_accumulate(part.data_ptr<float>(), part.size(0), M,
                         acc.data_ptr<double>(), wide ? 5 : 4,
                         current_stream());
}

}  // namespace rsdl

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X (gfx950) fused shuffle kernels";
  m.def("gather_rows", &rsdl::gather_rows,
        "dst[i, :] = src[perm[i], :] for int64 or int32 perm; rows are a "
        "multiple of 16 B wide. Precondition, NOT checked: every index lies "
        "in [0, src rows); an index outside reads out of bounds.",
        py::arg("src"), py::arg("perm"));
  m.def("gather_rows_out", &rsdl::gather_rows_out,
        "gather_rows into the first perm.numel() rows of dst; further rows "
        "of dst are left alone. Same unchecked precondition on perm.",
        py::arg("src"), py::arg("perm"), py::arg("dst"));
  m.def("unpack_permute", &rsdl::unpack_permute,
        "outs[c][i] = cast(column c of packed row perm[i]). Each column "
        "keeps its dtype or takes a cast from float32/float64/int32/int64 "
        "to one of those or bfloat16; any other pair raises before the "
        "launch. Precondition, NOT checked: perm indices lie in [0, packed "
        "rows); an index outside reads out of bounds.",
        py::arg("packed"), py::arg("perm"), py::arg("outs"),
        py::arg("packed_offsets"), py::arg("src_dtype_codes"));
  m.def("unpack_permute_affine", &rsdl::unpack_permute_affine,
        py::arg("packed"), py::arg("perm"), py::arg("outs"),
        py::arg("packed_offsets"), py::arg("src_dtype_codes"),
        py::arg("aff_table"), py::arg("aff_base"),
        py::arg("nan_fill") = c10::nullopt);
  m.def("narrow_rows", &rsdl::narrow_rows, py::arg("packed"),
        py::arg("dst_stride"), py::arg("pad_off"), py::arg("src_offsets"),
        py::arg("src_dtype_codes"), py::arg("dst_offsets"),
        py::arg("dst_dtype_codes"), py::arg("numels"),
        py::arg("aff_table") = c10::nullopt,
        py::arg("aff_base") = std::vector<int64_t>(),
        py::arg("nan_fill") = c10::nullopt);
  m.def("unpack_permute_sweep", &rsdl::unpack_permute_sweep,
        py::arg("packed"), py::arg("perm"), py::arg("outs"),
        py::arg("packed_offsets"), py::arg("src_dtype_codes"));
  m.def("column_stats", &rsdl::column_stats, py::arg("packed"),
        py::arg("packed_offsets"), py::arg("src_dtype_codes"),
        py::arg("numels"));
  m.def("pack_columns", &rsdl::pack_columns,
        "packed[perm[i]] column c = cast(cols[c][i]) (perm None: row i). "
        "Dtype pairs as unpack_permute, from the tensor's dtype to the "
        "packed one; any other pair raises before the launch. Padding bytes "
        "are not written. Precondition, NOT checked: perm is a permutation "
        "of [0, rows); an index outside writes out of bounds.",
        py::arg("cols"), py::arg("packed_offsets"),
        py::arg("packed_dtype_codes"), py::arg("row_stride"),
        py::arg("perm") = c10::nullopt);
  m.def("pack_columns_tiled", &rsdl::pack_columns_tiled,
        "pack_columns without perm through an LDS tile, optionally into "
        "``out``. Same dtype pairs; padding bytes are undefined.",
        py::arg("cols"), py::arg("packed_offsets"),
        py::arg("packed_dtype_codes"), py::arg("row_stride"),
        py::arg("out") = c10::nullopt);
  m.def("partition_build_perm", &rsdl::partition_build_perm,
        "(perm int32 [n], counts int64 [num_dests]): the gather permutation "
        "that groups rows by destination, for int32 or int64 dest and "
        "num_dests in [1, 1024]. Precondition, NOT checked: every id lies "
        "in [0, num_dests); an id outside indexes LDS out of bounds.",
        py::arg("dest"), py::arg("num_dests"));
  m.def("wgrad_bf16", &rsdl::wgrad_bf16, py::arg("dy"), py::arg("x"),
        py::arg("with_bias") = true);
  m.def("relu_bwd_bias", &rsdl::relu_bwd_bias, py::arg("dy"), py::arg("y"));
  m.def("swizzle_xt_bf16", &rsdl::swizzle_xt_bf16, py::arg("x"),
        py::arg("pi16") = false);
  m.def("wgrad_frag_bf16", &rsdl::wgrad_frag_bf16, py::arg("AT"),
        py::arg("BT"), py::arg("N"), py::arg("K"), py::arg("mchunks"),
        py::arg("nt_w"), py::arg("kt_w"), py::arg("variant") = 0);
  m.def("wgrad_frag_partials_bf16", &rsdl::wgrad_frag_partials_bf16,
        py::arg("AT"), py::arg("BT"), py::arg("N"), py::arg("K"),
        py::arg("mchunks"), py::arg("nt_w"), py::arg("kt_w"),
        py::arg("variant") = 0);
  m.def("fwd_chain_bf16", &rsdl::fwd_chain_bf16, py::arg("x"),
        py::arg("W1"), py::arg("b1"), py::arg("W2"), py::arg("b2"),
        py::arg("W3"), py::arg("b3"), py::arg("w4"), py::arg("b4"),
        py::arg("target") = c10::nullopt,
        py::arg("xt_out") = c10::nullopt, py::arg("pi16") = false,
        py::arg("rows") = 0, py::arg("loss") = 0,
        py::arg("weight") = c10::nullopt, py::arg("pos_weight") = 1.0);
  m.def("bwd_chain_bf16", &rsdl::bwd_chain_bf16, py::arg("dy"),
        py::arg("a3"), py::arg("mask1"), py::arg("mask2"), py::arg("w4"),
        py::arg("W3"), py::arg("W2"), py::arg("pi16") = false,
        py::arg("rows") = 0);
  m.def("step_prep", &rsdl::step_prep, py::arg("weights"),
        py::arg("target") = c10::nullopt, py::arg("outs") = c10::nullopt);
  m.def("step_finalize", &rsdl::step_finalize, py::arg("part1"),
        py::arg("part2"), py::arg("part3"), py::arg("db_part"),
        py::arg("loss_part"), py::arg("M"), py::arg("outs") = c10::nullopt);
  m.def("fused_step_bf16", &rsdl::fused_step_bf16, py::arg("x"),
        py::arg("target"), py::arg("weights"), py::arg("biases"),
        py::arg("pi16") = false, py::arg("outs") = c10::nullopt,
        py::arg("rows") = 0, py::arg("loss") = 0,
        py::arg("weight") = c10::nullopt, py::arg("pos_weight") = 1.0,
        py::arg("wgrad_variant") = 0, py::arg("wgrad_grouped") = -1,
        py::arg("opt") = c10::nullopt);
  m.def("step_finalize_update", &rsdl::step_finalize_update,
        py::arg("part1"), py::arg("part2"), py::arg("part3"),
        py::arg("db_part"), py::arg("loss_part"), py::arg("M"),
        py::arg("outs"), py::arg("weights"), py::arg("biases"),
        py::arg("state"), py::arg("staged"), py::arg("kind"),
        py::arg("hyper"));
  m.def("step_update", &rsdl::step_update, py::arg("grads"),
        py::arg("weights"), py::arg("biases"), py::arg("state"),
        py::arg("staged"), py::arg("kind"), py::arg("hyper"));
  m.def("wgrad_grouped_partials_bf16", &rsdl::wgrad_grouped_partials_bf16,
        py::arg("dz1t"), py::arg("xt"), py::arg("dz2t"), py::arg("a1t"),
        py::arg("dz3t"), py::arg("a2t"), py::arg("mchunks"));
  m.def("eval_chain_bf16", &rsdl::eval_chain_bf16, py::arg("x"),
        py::arg("Wstage"), py::arg("biases"),
        py::arg("target") = c10::nullopt, py::arg("pred_out") = c10::nullopt,
        py::arg("want_pred") = true, py::arg("rows") = 0,
        py::arg("task") = 0, py::arg("hist") = c10::nullopt,
        py::arg("weight") = c10::nullopt);
  m.def("eval_accumulate", &rsdl::eval_accumulate, py::arg("part"),
        py::arg("acc"), py::arg("M"));
  m.attr("LOSS_MSE") = (int)rsdl::kLossMse;
  m.attr("LOSS_BCE") = (int)rsdl::kLossBce;
  // the heads take sample weights / pos_weight (weight=, pos_weight=)
  m.attr("HEAD_WEIGHTS") = 1;
  // step_update / step_finalize_update and opt= of fused_step_bf16
  m.attr("STEP_OPTIM") = 1;
  m.attr("OPT_SGD") = (int)rsdl::kOptSgd;
  m.attr("OPT_ADAMW") = (int)rsdl::kOptAdamW;
  m.attr("DT_F32") = (int)rsdl::DT_F32;
  m.attr("DT_F64") = (int)rsdl::DT_F64;
  m.attr("DT_I32") = (int)rsdl::DT_I32;
  m.attr("DT_I64") = (int)rsdl::DT_I64;
  m.attr("DT_F16") = (int)rsdl::DT_F16;
  m.attr("DT_BF16") = (int)rsdl::DT_BF16;
  m.attr("DT_U8") = (int)rsdl::DT_U8;
}
