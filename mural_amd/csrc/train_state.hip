// The training loop's step state on the device (include/mural_hip.h: MuralTrainState) and its two kernels (gfx950 / CDNA4).
//
// The reference keeps Adam's step count, the bias corrections, the scheduled learning rate and the epoch's loss sum on the host
// (MuRaL/training.py:432-450: optimizer.step(), total_loss += loss.item(), scheduler.step(), the restart of a rate below min_lr).  A step
// replayed as a HIP graph never comes back to the host, so kernel arguments are frozen at capture: here those values live in one
// 128-byte block that a one-thread tick kernel advances every step and the flat Adam kernel reads.  Per step that is ONE launch more
// than mural_op_adam_flat; the loss is added by the tick, not by a launch of its own.
#include <cmath>
#include <cstddef>

#include "train_ops.h"

static_assert(sizeof(MuralTrainState) == 128, "MuralTrainState is a fixed 128-byte layout (mural_amd/train.py reads it by offset)");
static_assert(offsetof(MuralTrainState, loss_sum) == 24 && offsetof(MuralTrainState, step_size) == 48 &&
              offsetof(MuralTrainState, bc2_sqrt) == 52, "MuralTrainState field offsets");

namespace mural {
namespace {

// One workgroup, one working lane: ~20 dependent double operations, nothing to spread.  Every write to the block is an ordinary store of
// this lane; the order of the statements is the order of the host loop, so the lr sequence is the host's bit for bit.
__global__ __launch_bounds__(64) void train_state_tick_kernel(MuralTrainState* __restrict__ st, const float* __restrict__ loss, int64_t rows,
                                                              double beta1, double beta2, int64_t sched_step_size, double gamma,
                                                              double min_lr, double restart_lr) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t step = st->step + 1;
  double lr = st->lr;
  st->step = step;
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  st->step_size = (float)(lr / bc1);
  st->bc2_sqrt = (float)sqrt(bc2);
  if (loss != nullptr) {
    st->loss_sum = st->loss_sum + (double)loss[0];
    st->rows = st->rows + rows;
  }
  st->steps_done = st->steps_done + 1;
  const int64_t ticks = st->ticks + 1;
  st->ticks = ticks;
  if (sched_step_size > 0 && ticks % sched_step_size == 0) lr = lr * gamma;
  if (lr < min_lr) lr = restart_lr;
  st->lr = lr;
}

__global__ __launch_bounds__(256) void adam_flat_state_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, int64_t n4, const MuralTrainState* __restrict__ st,
                                                              float w1, float beta2, float w2, float eps, float wd) {
  adam_flat_elements(p, g, m, v, n4, w1, beta2, w2, st->step_size, st->bc2_sqrt, eps, wd);
}

// (the block's lr AFTER a tick is the rate the tick's scheduler left for the next update: the rate of this update wherever the scheduler
// did not move it at this tick.  mural_amd/train.py orders its launches accordingly.)
__global__ __launch_bounds__(256) void adamw_amsgrad_flat_state_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                       float* __restrict__ v, float* __restrict__ vmax, int64_t n4,
                                                                       const MuralTrainState* __restrict__ st, double wd, float w1, float beta2,
                                                                       float w2, float eps) {
  adamw_amsgrad_flat_elements(p, g, m, v, vmax, n4, (float)fma(-st->lr, wd, 1.0), w1, beta2, w2, st->step_size, st->bc2_sqrt, eps);
}

__global__ __launch_bounds__(256) void sgd_flat_state_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                             int64_t n4, const MuralTrainState* __restrict__ st, float momentum, float wd) {
  sgd_flat_elements(p, g, buf, n4, (float)st->lr, momentum, wd);
}

}  // namespace
}  // namespace mural

using namespace mural;
#define STREAM ((hipStream_t)stream)
#define CHECK_LAUNCH() MURAL_HIP_CHECK(hipGetLastError()); return MURAL_OK

extern "C" int mural_op_train_state_tick(MuralTrainState* state, const float* loss, int64_t rows, double beta1, double beta2,
                                         int64_t sched_step_size, double gamma, double min_lr, double restart_lr, void* stream) {
  MURAL_REQUIRE(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0, "train_state_tick: the state block must be an 8-byte aligned device pointer");
  MURAL_REQUIRE((reinterpret_cast<uintptr_t>(loss) & 3) == 0, "train_state_tick: the loss must be a 4-byte aligned device float");
  MURAL_REQUIRE(rows >= 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1, "train_state_tick: rows >= 0, 0 <= beta < 1");
  MURAL_REQUIRE(sched_step_size >= 0 && gamma >= 0 && min_lr >= 0 && restart_lr >= 0,
                "train_state_tick: sched_step_size >= 0, gamma >= 0, min_lr >= 0, restart_lr >= 0");
  hipLaunchKernelGGL(train_state_tick_kernel, dim3(1), dim3(64), 0, STREAM, state, loss, rows, beta1, beta2, sched_step_size, gamma, min_lr,
                     restart_lr);
  CHECK_LAUNCH();
}

extern "C" int mural_op_adam_flat_state(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                        const MuralTrainState* state, double beta1, double beta2, double eps, double weight_decay,
                                        void* stream) {
  if (const int rc = adam_flat_check(param, grad, exp_avg, exp_avg_sq, n, beta1, beta2, eps, weight_decay)) return rc;
  MURAL_REQUIRE(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0, "adam_flat_state: the state block must be an 8-byte aligned device pointer");
  if (n == 0) return MURAL_OK;
  hipLaunchKernelGGL(adam_flat_state_kernel, dim3(adam_flat_grid(n / 4)), dim3(256), 0, STREAM, param, grad, exp_avg, exp_avg_sq, n / 4, state,
                     (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay);
  CHECK_LAUNCH();
}

extern "C" int mural_op_adamw_amsgrad_flat_state(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                                                 int64_t n, const MuralTrainState* state, double beta1, double beta2, double eps,
                                                 double weight_decay, void* stream) {
  if (const int rc = adamw_amsgrad_flat_check(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, beta1, beta2, eps, weight_decay)) return rc;
  MURAL_REQUIRE(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0,
                "adamw_amsgrad_flat_state: the state block must be an 8-byte aligned device pointer");
  if (n == 0) return MURAL_OK;
  hipLaunchKernelGGL(adamw_amsgrad_flat_state_kernel, dim3(adam_flat_grid(n / 4)), dim3(256), 0, STREAM, param, grad, exp_avg, exp_avg_sq,
                     max_exp_avg_sq, n / 4, state, weight_decay, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps);
  CHECK_LAUNCH();
}

extern "C" int mural_op_sgd_flat_state(float* param, const float* grad, float* buf, int64_t n, const MuralTrainState* state, double momentum,
                                       double weight_decay, void* stream) {
  if (const int rc = sgd_flat_check(param, grad, buf, n, momentum, weight_decay)) return rc;
  MURAL_REQUIRE(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0, "sgd_flat_state: the state block must be an 8-byte aligned device pointer");
  if (n == 0) return MURAL_OK;
  hipLaunchKernelGGL(sgd_flat_state_kernel, dim3(adam_flat_grid(n / 4)), dim3(256), 0, STREAM, param, grad, buf, n / 4, state, (float)momentum,
                     (float)weight_decay);
  CHECK_LAUNCH();
}
