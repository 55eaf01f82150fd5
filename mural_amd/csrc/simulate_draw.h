// The stateless draw of the simulation kernels, shared by csrc/simulate.hip (counts per named interval set, mutation lists),
// csrc/simulate_conseq.hip, csrc/simulate_txstruct.hip and csrc/simulate_txindel.hip (counts per transcript and bin) so that their draws
// cannot drift: the rows' argument block, the check kernel (the status bits of every row), the Philox4x32-10 round, a row's cumulative
// class bounds and the last counter word, with the loop bounds all four files plan their launches on.
// summaries.simulate_rows_host is the specification; DESIGN.md section 3.20.
#pragma once
#include "common.h"
#include "kmer_key.h"

namespace mural {

constexpr int SIM_MAX_CLASS = 8;
constexpr int SIM_THREADS = 256;
constexpr int SIM_WAVES = SIM_THREADS / 64;
constexpr int SIM_SCAN_THREADS = 1024;
constexpr int64_t SIM_CHUNK_ROWS = 1024;          // rows of one unit of the draw kernels: 16 tiles of 64
constexpr int64_t SIM_GRID_WAVES = 8192;          // waves of the draw kernels' grid; they stride over the units
constexpr int32_t SIM_MAX_REP = 1 << 20;
constexpr u64 SIM_ONE = 1ull << 32;

struct SimRows {
  const void* prob;
  const int64_t* start;
  const uint8_t* strand;      // or nullptr: all '+'
  int64_t prob_stride;
  int32_t n_class;
  uint32_t chrom_key, seed_lo, seed_hi;
  int32_t* status;
};

inline SimRows sim_rows(const void* prob, int64_t prob_stride, const int64_t* start, const uint8_t* strand, int32_t n_class,
                        uint32_t chrom_key, uint64_t seed, int32_t* status) {
  SimRows A{};
  A.prob = prob, A.start = start, A.strand = strand, A.prob_stride = prob_stride, A.n_class = n_class;
  A.chrom_key = chrom_key, A.seed_lo = (uint32_t)seed, A.seed_hi = (uint32_t)(seed >> 32), A.status = status;
  return A;
}

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// cum[c - 1] of row i for c = 1 .. n_class - 1 (0 beyond, and 0 everywhere for a bad row); returns the row's status bits
template <typename T>
__device__ __forceinline__ int32_t row_cum(const SimRows& A, int64_t i, u64 (&cum)[SIM_MAX_CLASS - 1]) {
  const T* __restrict__ p_row = static_cast<const T*>(A.prob) + i * A.prob_stride;
  int32_t bad = A.start[i] < 0 ? (int32_t)SM_BAD_START : 0;
  u64 run = 0;
#pragma unroll
  for (int c = 1; c < SIM_MAX_CLASS; ++c) {
    cum[c - 1] = 0;
    if (c < A.n_class) {
      const double p = (double)p_row[c];      // (float -> double is exact)
      // finite and not negative, on the bit pattern -- non-negative doubles order like their bits --, so that NaN is caught whatever
      // the compiler assumes about comparisons; -0.0 counts as 0
      const u64 bits = (u64)__double_as_longlong(p);
      if (bits >= 0x7FF0000000000000ull && bits != 0x8000000000000000ull) {
        bad |= SM_BAD_PROB;
      } else {
        double s = p * 4294967296.0;          // exact: a power of two
        if (s > 4294967296.0) s = 4294967296.0;
        run += (u64)(long long)floor(s);
        cum[c - 1] = run < SIM_ONE ? run : SIM_ONE;
      }
    }
  }
  if (bad) {
#pragma unroll
    for (int c = 0; c < SIM_MAX_CLASS - 1; ++c) cum[c] = 0;
  }
  return bad;
}

// a thread per row: the status bits (a bad probability, a negative start and, with check_order, a start below the row before it)
template <typename T>
__global__ __launch_bounds__(SIM_THREADS) void simulate_check_kernel(SimRows A, int64_t n, int check_order) {
  const int64_t i = (int64_t)blockIdx.x * SIM_THREADS + threadIdx.x;
  int32_t bad = 0;
  if (i < n) {
    u64 cum[SIM_MAX_CLASS - 1];
    bad = row_cum<T>(A, i, cum);
    if (check_order && i > 0 && A.start[i] < A.start[i - 1]) bad |= SM_BAD_ORDER;
  }
  if (bad) atomicOr(A.status, bad);
}

// the check kernel on `st`; MURAL_OK or the error code of the launch
inline int launch_simulate_check(hipStream_t st, const SimRows& A, int64_t n, bool prob_f64, int check_order) {
  const dim3 grid((unsigned)((n + SIM_THREADS - 1) / SIM_THREADS)), block(SIM_THREADS);
  if (prob_f64)
    hipLaunchKernelGGL(simulate_check_kernel<double>, grid, block, 0, st, A, n, check_order);
  else
    hipLaunchKernelGGL(simulate_check_kernel<float>, grid, block, 0, st, A, n, check_order);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

__device__ __forceinline__ uint32_t last_counter_word(const SimRows& A, int64_t i, uint32_t block) {
  return block | ((A.strand != nullptr && A.strand[i] != 0) ? 0x80000000u : 0u);
}

}  // namespace mural
