// Launch arguments of the fused-step glue kernels (csrc/step_glue.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rsdl {

struct StepPrepArgs {
  const float* W1;   // [512,100] fp32 master weights, row-major
  const float* W2;   // [256,512]
  const float* W3;   // [128,256]
  const float* w4;   // [128]
  uint16_t* W1s;     // bf16 fragment-major, K padded to 112
  uint16_t* W2s;
  uint16_t* W3s;
  uint16_t* W2Ts;    // fragment-major W2^T [512,256]
  uint16_t* W3Ts;    // fragment-major W3^T [256,128]
  uint16_t* w4b;     // bf16 [128]
  const double* tgt64;  // fp64 target [M], or nullptr (no cast needed)
  float* tgt32;
  int64_t M;
};

struct StepFinArgs {
  const float* part1;  // [ns1, 512*128] dW1 slab partials (K pad included)
  const float* part2;  // [ns2, 256*512]
  const float* part3;  // [ns3, 128*256]
  const float* db_part;    // [db_rows, 1156]
  const float* loss_part;  // [loss_n]
  int64_t ns1, ns2, ns3, db_rows, loss_n, M;
  float* dw1;  // [512,100]
  float* dw2;
  float* dw3;
  float* dw4;  // [128]
  float* db1;
  float* db2;
  float* db3;
  float* db4;
  float* loss;  // [1]
};

void launch_step_prep(const StepPrepArgs& p, hipStream_t stream);
void launch_step_finalize(const StepFinArgs& p, hipStream_t stream);
// ncol = 4: part fp32 [nrows, 4] (16-byte aligned) -> acc fp64 [5] +=
// {M, column sums}; ncol = 5: part fp32 [nrows, 8] (columns 0..4 used) ->
// acc fp64 [6]
void launch_eval_accumulate(const float* part, int64_t nrows, int64_t M,
                            double* acc, int ncol, hipStream_t stream);

}  // namespace rsdl
