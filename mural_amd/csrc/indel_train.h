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

}  // namespace mural
