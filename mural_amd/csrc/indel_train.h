// Internal entry points of the INDEL training ops (indel_train.hip, conv_wgrad_mfma.hip) used by the composed step
// (indel_train_step.hip).
#pragma once
#include "common.h"

namespace mural {

// conv_wgrad_mfma.hip: the weight gradient as an implicit GEMM on the matrix cores (nonzero return: shape not covered)
int launch_conv_wgrad_mfma(const float* dy, const float* x, float* part, int64_t B, int Cin, int Lin, int Cout, int Lout, int K, int stride,
                           int pad, int up, int max_chunks, int* chunks_out, hipStream_t st);
// indel_train.hip
void wgrad_defer_begin();                 // collect the weight-gradient partial rows of the layers that follow ...
int wgrad_defer_flush(hipStream_t st);    // ... and reduce them all in one launch
// mural_op_convg_bn_bwd with dx_add (optional, may alias dx): dx = the conv's input gradient + dx_add -- the composed step hands the
// gradient that reaches x through a residual or skip connection here instead of a separate add pass
int convg_bn_bwd_add(const float* dz, const float* x, const float* W, const float* y0, const float* state, const float* gamma, int64_t B,
                     int32_t Cin, int32_t Lin, int32_t Cout, int32_t K, int32_t stride, int32_t pad, int32_t up, int32_t act, double* acc,
                     float* dy0, float* dx, const float* dx_add, float* dW, float* db, float* dgamma, float* dbeta, float* part,
                     size_t part_floats, const float* wt_dgrad, void* stream);
// the two halves of a unit behind / in front of its conv (mural_op_convg_bn_fwd / _bwd call them): batch-statistics BatchNorm,
// activation and residuals of a conv output y0 that is already there; their backward, which leaves the conv output's gradient in dy0
int bn_post_fwd(const float* y0, int64_t B, int32_t Cout, int32_t Lout, const float* gamma, const float* beta, float eps, float momentum,
                float* running_mean, float* running_var, double* acc, float* state, int32_t act, const float* res1, const float* res2, float* z,
                void* stream);
int bn_post_bwd(const float* dz, const float* y0, const float* state, const float* gamma, int64_t B, int32_t Cout, int32_t Lout, int32_t act,
                double* acc, float* dy0, float* dgamma, float* dbeta, void* stream);

// indel_first.hip: the conv of the unit that consumes the window, from one symbol byte per column (MURAL_SYM_*; a byte above 14 counts
// as N).  y [B][Cout][Lout] = bias + conv(dense(sym)); with `rev` (stride 1, pad (K - 1) / 2) y_rev receives the same conv of the
// channel- and length-flipped window, read from the same bytes reversed and complemented.  The weight gradient sums dz (and, with
// dz_rev, the flipped application's gradient) per (channel, tap, symbol) in `part` and contracts with the symbols' columns: dW
// [Cout][4][K] and db [Cout] (optional) are fully written, in a fixed order.  Cout must be a multiple of 4, K <= 63.
size_t indel_first_scratch_floats(int64_t B, int Lout, int Cout, int K, int rev);
int indel_first_fwd(const uint8_t* sym, const float* W, const float* bias, int64_t B, int L, int Cout, int K, int stride, int pad, float* y,
                    float* y_rev, hipStream_t st);
int indel_first_bwd(const uint8_t* sym, const float* dz, const float* dz_rev, int64_t B, int L, int Cout, int K, int stride, int pad, float* dW,
                    float* db, float* part, size_t part_floats, hipStream_t st);

}  // namespace mural
