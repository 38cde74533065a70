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
  // First block index to run: 0 = everything, step_prep_target_only() =
  // skip the weight blocks (the caller's staged buffers are already
  // valid) and only cast the target.
  int32_t b0;
};

// Optimizer kinds of the update kernels and the layout of ``h``, the fp32
// hyper-parameters. Scalars that depend on the step count are formed by
// the caller in fp64 and rounded to fp32 once.
//   SGD    h = {grad_scale, lr, momentum, weight_decay, nesterov (0|1)}
//   AdamW  h = {grad_scale, c1 = 1 - lr*wd, a1 = 1 - beta1, beta2,
//               a2 = 1 - beta2, s = lr / (1 - beta1^t),
//               q = sqrt(1 - beta2^t), eps}
constexpr int kOptSgd = 0;
constexpr int kOptAdamW = 1;

// Parameter order of every array below: W1, W2, W3, w4, b1, b2, b3, b4.
struct StepOptArgs {
  float* prm[8];         // fp32 masters, updated in place
  float* s1[8];          // SGD momentum buffer (null when momentum == 0) /
                         // AdamW first moment
  float* s2[8];          // AdamW second moment (null for SGD)
  const float* grad[8];  // folded gradients (step_update only)
  uint16_t* stg[6];      // W1s, W2s, W3s, W2Ts, W3Ts, w4b of StepPrepArgs
  float h[8];
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
// step_finalize, then the optimizer update of every element where its
// gradient was just stored (``o.grad`` is not read).
void launch_step_finalize_update(const StepFinArgs& p, const StepOptArgs& o,
                                 int kind, hipStream_t stream);
// The same update from the gradients in ``o.grad``.
void launch_step_update(const StepOptArgs& o, int kind, hipStream_t stream);
int32_t step_prep_target_only();  // StepPrepArgs::b0 that skips the weights
// ncol = 4: part fp32 [nrows, 4] (16-byte aligned) -> acc fp64 [5] +=
// {M, column sums}; ncol = 5: part fp32 [nrows, 8] (columns 0..4 used) ->
// acc fp64 [6]
void launch_eval_accumulate(const float* part, int64_t nrows, int64_t M,
                            double* acc, int ncol, hipStream_t stream);

}  // namespace rsdl
