// Reduction of the weight / bias gradient partial rows of the 32->32, k=3 training convolutions.  The backward kernels of a step
// (conv32_wave.hip, conv32_cl.hip) leave one partial row [32*32*3 + 32] per workgroup; one launch at the end of the backward
// (snv_train.hip) turns the rows of every layer into dW / db in a fixed summation order -> reproducible gradients.
#include <cstdlib>
#include <cstring>

#include "conv32_jobs.h"

namespace mural {

constexpr int C32 = 32;

// 64 outputs x 16 slices of the partial rows per workgroup, for up to PR_MAXJOBS layers in one launch (blockIdx.y = layer)
constexpr int PR_MAXJOBS = 24;
struct PartJobs {
  const float* part[PR_MAXJOBS];
  float* dW[PR_MAXJOBS];
  float* db[PR_MAXJOBS];
  int nrow[PR_MAXJOBS];
};

__global__ __launch_bounds__(1024) void part_reduce_multi_kernel(const PartJobs jobs, int nW, int nB) {
  __shared__ float sh[16][64];
  const int job = blockIdx.y;
  const float* __restrict__ part = jobs.part[job];
  const int nrow = jobs.nrow[job];
  const int o = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + o;
  float s = 0.f;
  if (i < nW + nB) {
    // eight rows in flight per thread (the loop is latency-bound: 49 workgroups read 6 MB); the order of the adds is fixed
    const size_t rs = (size_t)(nW + nB);
    const float* p = part + i;
    int b = slice;
    float s0 = 0.f, s1 = 0.f;
    for (; b + 7 * 16 < nrow; b += 8 * 16) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = p[(size_t)(b + 16 * q) * rs];
      s0 += (v[0] + v[1]) + (v[2] + v[3]);
      s1 += (v[4] + v[5]) + (v[6] + v[7]);
    }
    for (; b < nrow; b += 16) s0 += p[(size_t)b * rs];
    s = s0 + s1;
  }
  sh[slice][o] = s;
  __syncthreads();
  if (slice == 0 && i < nW + nB) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) t += sh[q][o];
    if (i < nW) jobs.dW[job][i] = t;
    else if (jobs.db[job]) jobs.db[job][i - nW] = t;
  }
}

int train_reduce_parts(const float* const* part, const int* nrow, float* const* dW, float* const* db, int njobs, hipStream_t stream) {
  for (int j0 = 0; j0 < njobs; j0 += PR_MAXJOBS) {
    PartJobs jobs;
    std::memset(&jobs, 0, sizeof(jobs));
    const int n = njobs - j0 < PR_MAXJOBS ? njobs - j0 : PR_MAXJOBS;
    // validation only (tests/test_gpu_train.py): MURAL_DEBUG_DROP_PART_ROW=<job> leaves the last partial row of that job out of
    // its sum -- the fault the parity tests of the training step must be able to see
    int drop_job = -1;
    if (const char* e = dev_env("MURAL_DEBUG_DROP_PART_ROW")) drop_job = atoi(e);
    for (int j = 0; j < n; ++j) {
      jobs.part[j] = part[j0 + j];
      jobs.nrow[j] = nrow[j0 + j] - ((j0 + j == drop_job && nrow[j0 + j] > 1) ? 1 : 0);
      jobs.dW[j] = dW[j0 + j];
      jobs.db[j] = db[j0 + j];
    }
    hipLaunchKernelGGL(part_reduce_multi_kernel, dim3((C32 * C32 * 3 + C32 + 63) / 64, n), dim3(1024), 0, stream, jobs, C32 * C32 * 3, C32);
    MURAL_HIP_CHECK(hipGetLastError());
  }
  return MURAL_OK;
}

}  // namespace mural
