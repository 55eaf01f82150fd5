// The row checks and the two-limb quantisation of the integer-sum summaries, shared by csrc/summary_kmer.hip (k-mer and motif tables)
// csrc/summary_annot.hip (annotation tables) and csrc/summary_conseq.hip (consequence tables) so that their cells cannot drift:
// q = rne(p * 2^71) carried as
// hi = floor(p * 2^31) and lo = rint((p * 2^31 - hi) * 2^40), each step exact in float64.
#pragma once
#include "common.h"
#include "kmer_key.h"

namespace mural {

constexpr int SK_MAX_CLASS = 8;
constexpr int SK_LO_BITS = 40;
typedef unsigned long long u64;

// One probability as the two limbs; false (and hi = lo = 0) where it is NaN, negative or above 1.
__device__ __forceinline__ bool quantise_prob(double p, u64& hi, u64& lo) {
  hi = 0, lo = 0;
  // 0 <= p <= 1 on the bit pattern -- non-negative doubles order like their bits --, so that NaN is caught whatever the compiler
  // assumes about comparisons; -0.0 counts as 0
  const u64 bits = (u64)__double_as_longlong(p);
  if (bits > 0x3FF0000000000000ull && bits != 0x8000000000000000ull) return false;
  const double s = p * 2147483648.0;                       // p * 2^31
  const double h = floor(s);
  hi = (u64)(long long)h;
  lo = (u64)(long long)rint((s - h) * 1099511627776.0);      // * 2^40, half to even
  return true;
}

// The checks of a row (status bits, 0 if it counts) and its probabilities as the two limbs.
template <typename T>
__device__ __forceinline__ int32_t quantise_row(const T* __restrict__ prob, int nc, int64_t st, int lab, u64 (&hi)[SK_MAX_CLASS],
                                                u64 (&lo)[SK_MAX_CLASS]) {
  int32_t bad_row = 0;
  if (st < 0) bad_row |= SM_BAD_START;
  if (lab < 0 || lab >= nc) bad_row |= SM_BAD_LABEL;
#pragma unroll
  for (int c = 0; c < SK_MAX_CLASS; ++c) {
    hi[c] = 0, lo[c] = 0;
    if (c < nc && !quantise_prob((double)prob[c], hi[c], lo[c])) bad_row |= SM_BAD_PROB;      // (float -> double is exact)
  }
  return bad_row;
}

}  // namespace mural
