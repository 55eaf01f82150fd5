// Host entry points of train_ops.hip (with snv_head_train.h and snv_local_train.h, whose kernels that file alone instantiates) for
// the composed SNV training step (snv_train.hip) and the diagnostics (debug_hooks.hip).
#pragma once
#include "snv.h"

namespace mural {

// first layer of a tower with channel-last output (kernels: snv_stage1.hip, launch_first_train)
int train_first_fwd_cl(const uint8_t* sym, int64_t B, int Lwin, int col0, int L1, int pk, int ps, int pp, const float* gamma, const float* beta,
                       const float* W, const float* bias, float eps, float momentum, float* running_mean, float* running_var,
                       unsigned long long* counts, float* tab, float* y, void* arg, double* stat, hipStream_t stream);
int train_first_prepare2(const uint8_t* sym, int64_t B, int Lwin, const int* col0, const int* L1, const float* const* gamma,
                         const float* const* beta, const float* const* W, const float* const* bias, float* const* running_mean,
                         float* const* running_var, unsigned long long* const* counts, float* const* tab, float eps, float momentum,
                         hipStream_t stream);
int train_first_fwd_cl_prepared(const uint8_t* sym, int64_t B, int Lwin, int col0, int L1, int pk, int ps, int pp, const float* tab, float* y,
                                void* arg, double* stat, hipStream_t stream);
int train_first_bwd_cl(const float* dy, const void* arg, const uint8_t* sym, int64_t B, int Lwin, int col0, int L1, int pk, int ps, int pp,
                       const float* tab, const float* W, float* scratch, float* dW, float* dbias, float* dgamma, float* dbeta,
                       const FirstFold* fold, hipStream_t stream);
int train_bn2d_apply_dropout(const float* x, int64_t B, int C, int relu, const double* acc, const float* gamma, const float* beta, float eps,
                             float momentum, float* running_mean, float* running_var, float* state, float p, uint64_t seed,
                             const uint64_t* seed_dev, float* y_bn, float* y, hipStream_t stream);
// snv_head_train.h: a tower's head in two launches per direction
bool head_train_shape_ok(int nc);      // the shapes the fused form serves
bool head_train_fused_ok(int nc);      // ... and MURAL_TRAIN_HEAD_OPS does not ask for the per-op launches
int head_train_fwd(const float* c3, int64_t B, int L, float* feat, int32_t* arg, double* acc, const float* gamma, const float* beta, float eps,
                   float momentum, float* running_mean, float* running_var, float* state, float p, uint64_t seed, const uint64_t* seed_dev,
                   float* fd, const float* W, const float* bias, int nc, float* logits, hipStream_t stream);
int head_train_bwd(const float* dlogits, const float* W, int nc, int64_t B, int L, const float* feat, const float* state, const float* gamma,
                   float p, uint64_t seed, const uint64_t* seed_dev, float* dd, double* acc, const int32_t* arg, const float* c3, float* dx,
                   float* dgamma, float* dbeta, hipStream_t stream);
int head_train_wgrad(const float* dlogits, const float* fd, int64_t B, int nc, float* dW, float* db, hipStream_t stream);
// snv_local_train.h: the local branch in three launches per direction
bool local_train_shape_ok(int in1, int h1, int h2, int nc, int emb_rows, int64_t B);      // the shapes the fused form serves
bool local_train_fused_ok(int in1, int h1, int h2, int nc, int emb_rows, int64_t B);      // ... unless MURAL_TRAIN_LOCAL_OPS is set
int local_train_fwd(const int64_t* cat, const float* E, int cols, int emb_rows, int64_t B, const int* dims, const float* const* W,
                    const float* const* bias, const float* const* gamma, const float* const* beta, float* const* running_mean,
                    float* const* running_var, float* const* state, double* const* acc_f, const float* drop, const uint64_t* seeds,
                    const uint64_t* seed_dev, float eps, float momentum, float* const* xt, float* const* lin, float* logits, hipStream_t stream);
int local_train_bwd(const int64_t* cat, int cols, int emb_rows, int64_t B, const int* dims, const float* dlogits, const float* const* W,
                    const float* const* gamma, const float* const* state, double* const* acc_b, const float* drop, const uint64_t* seeds,
                    const uint64_t* seed_dev, const float* const* xt, const float* const* lin, float* const* dd, float* const* g,
                    float* const* dW, float* const* db, float* const* dgamma, float* const* dbeta, float* dE, hipStream_t stream);
namespace ltrain { extern unsigned long long* g_lt_stamps; }      // diagnostic (mural_debug_lt_set_stamps)

// The flat Adam step behind its two entries: mural_op_adam_flat (train_ops.hip: step_size / bc2_sqrt formed on the host) and
// mural_op_adam_flat_state (train_state.hip: read from a MuralTrainState block).  One argument check, one grid, one element loop.
int adam_flat_check(const float* param, const float* grad, const float* exp_avg, const float* exp_avg_sq, int64_t n, double beta1,
                    double beta2, double eps, double weight_decay);
int adam_flat_grid(int64_t n4);
//   g' = g + weight_decay p;  m = m + (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g' g';
//   p = p - step_size m / (sqrt(v) / bc2_sqrt + eps)          with step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t)
// (torch's fused kernel's update, in float) over n4 float4 groups, grid-strided.
__device__ __forceinline__ void adam_flat_elements(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n4, float w1, float beta2, float w2, float step_size,
                                                   float bc2_sqrt, float eps, float wd) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i], mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float* pp = &pv.x; float* mp = &mv.x; float* vp = &vv.x;
    const float* gp = &gv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gk = gp[k] + wd * pp[k];
      mp[k] = mp[k] + (gk - mp[k]) * w1;
      vp[k] = beta2 * vp[k] + w2 * gk * gk;
      const float denom = sqrtf(vp[k]) / bc2_sqrt + eps;
      pp[k] = pp[k] - step_size * mp[k] / denom;
    }
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
}

// The flat AdamW (amsgrad) and SGD (momentum, nesterov) steps, built like the Adam step above: one argument check and one element loop each
// behind two entries -- mural_op_adamw_amsgrad_flat / mural_op_sgd_flat (train_ops.hip: lr and step from the host) and their _state twins
// (train_state.hip: read from a MuralTrainState block) -- on adam_flat_grid.
int adamw_amsgrad_flat_check(const float* param, const float* grad, const float* exp_avg, const float* exp_avg_sq, const float* max_exp_avg_sq,
                             int64_t n, double beta1, double beta2, double eps, double weight_decay);
int sgd_flat_check(const float* param, const float* grad, const float* buf, int64_t n, double momentum, double weight_decay);
// torch.optim.AdamW(amsgrad=True)'s single-tensor update, in float; decay = (float)(1 - lr weight_decay), formed in double:
//   p = p decay;  m = m + (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g g;  vmax = max(vmax, v);
//   p = p - step_size m / (sqrt(vmax) / bc2_sqrt + eps)       with step_size, bc2_sqrt as in adam_flat_elements
__device__ __forceinline__ void adamw_amsgrad_flat_elements(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, float* __restrict__ vmax, int64_t n4, float decay, float w1,
                                                            float beta2, float w2, float step_size, float bc2_sqrt, float eps) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i], mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    float4 xv = reinterpret_cast<float4*>(vmax)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float* pp = &pv.x; float* mp = &mv.x; float* vp = &vv.x; float* xp = &xv.x;
    const float* gp = &gv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gk = gp[k];
      mp[k] = mp[k] + (gk - mp[k]) * w1;
      vp[k] = beta2 * vp[k] + w2 * gk * gk;
      xp[k] = fmaxf(xp[k], vp[k]);
      const float denom = sqrtf(xp[k]) / bc2_sqrt + eps;
      pp[k] = pp[k] * decay - step_size * mp[k] / denom;
    }
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
    reinterpret_cast<float4*>(vmax)[i] = xv;
  }
}
// torch.optim.SGD(momentum, nesterov=True, dampening=0)'s update with L2 weight decay, in float (a zero buf gives torch's first step):
//   g' = g + weight_decay p;  buf = momentum buf + g';  p = p - lr (g' + momentum buf)
__device__ __forceinline__ void sgd_flat_elements(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int64_t n4,
                                                  float lr, float momentum, float wd) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i], bv = reinterpret_cast<float4*>(buf)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float* pp = &pv.x; float* bp = &bv.x;
    const float* gp = &gv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gk = gp[k] + wd * pp[k];
      bp[k] = momentum * bp[k] + gk;
      pp[k] = pp[k] - lr * (gk + momentum * bp[k]);
    }
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(buf)[i] = bv;
  }
}

}  // namespace mural
