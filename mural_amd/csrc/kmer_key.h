// The k-mer key of a prediction-table row, shared by csrc/tables.hip (mural_table_kmer_keys: the table read back from a file) and
// csrc/summary_kmer.hip (mural_summary_kmer_rows: the same tables reduced while the rows are on the device), so that the two cannot
// drift.  Also the row checks the two summary reductions share (label decoding, status bits).
#pragma once
#include "common.h"

namespace mural {

// Python's slice bounds of chrom[s0:s1] on a chromosome of L bases: a negative index counts from the end, both are clamped to 0 .. L
__device__ __forceinline__ void kmer_slice_clip(int64_t L, int64_t s0, int64_t s1, int64_t& lo, int64_t& hi) {
  lo = s0 < 0 ? max(L + s0, (int64_t)0) : min(s0, L);
  hi = s1 < 0 ? max(L + s1, (int64_t)0) : min(s1, L);
}

// 2-bit code of base q (A0 C1 G2 T3); `bad` is set where the base is none of them (an nmask bit).  0 <= q < length.
__device__ __forceinline__ int32_t kmer_base(const MuralGenome& g, int64_t q, bool& bad) {
  bad |= ((static_cast<const uint32_t*>(g.nmask)[q >> 5] >> (q & 31)) & 1u) != 0;
  return (int32_t)((static_cast<const uint32_t*>(g.packed2)[q >> 4] >> (2 * (q & 15))) & 3u);
}

// the keys of the Python slice chrom[s0:s1]: fwd = base-4 number of its k bases (A0 C1 G2 T3), rev = that of their reverse complement;
// both -1 when the slice is not exactly k bases long or holds a base other than A/C/G/T.  1 <= k <= 15.
__device__ __forceinline__ void kmer_window_decode(const MuralGenome& g, int64_t s0, int64_t s1, int k, int32_t& fwd, int32_t& rev) {
  int64_t lo, hi;
  kmer_slice_clip(g.length, s0, s1, lo, hi);
  fwd = -1, rev = -1;
  if (hi - lo == k) {
    int32_t f = 0, rv = 0;
    bool bad = false;
    for (int j = 0; j < k; ++j) {
      const int32_t code = kmer_base(g, lo + j, bad);
      f = f * 4 + code;
      rv += (3 - code) << (2 * j);
    }
    if (!bad) {
      fwd = f;
      rev = rv;
    }
  }
}

// k-mer of a row (get_expanded_region, MuRaL/data/preprocessing.py:524-567, and the slice of calc_kmer_corr.py:246-251 with Python's
// slice semantics at both ends of the chromosome): the window is [start - k/2 (+1 indel), end + k/2).
__device__ __forceinline__ void kmer_key_decode(const MuralGenome& g, int64_t start, int64_t end, int k, int indel, int32_t& fwd,
                                                int32_t& rev) {
  const int64_t r = k / 2;
  kmer_window_decode(g, start - r + (indel ? 1 : 0), end + r, k, fwd, rev);
}

// strand mode 0: the row's strand; 1 '+'; 2 '-' (3: both keys count, the caller takes fwd and rev)
__device__ __forceinline__ bool kmer_key_minus(int mode, const uint8_t* __restrict__ strand, int64_t i) {
  return mode == 2 || (mode == 0 && strand[i] != 0);
}

// status bits of the summary reductions (summary.hip, summary_kmer.hip); rows that set one are skipped
enum : int32_t { SM_BAD_START = 1, SM_BAD_LABEL = 2, SM_BAD_ORDER = 4, SM_BAD_PROB = 8 };

// label of row i as an int, -1 if it is no whole number
__device__ __forceinline__ int load_label(const void* label, int kind, int64_t i) {
  if (kind == 0) {
    const float f = static_cast<const float*>(label)[i];
    const int v = (f >= -1.0f && f < 1024.0f) ? (int)f : -1;
    return (float)v == f ? v : -1;
  }
  if (kind == 1) return static_cast<const int32_t*>(label)[i];
  const int64_t v = static_cast<const int64_t*>(label)[i];
  return (v >= 0 && v < 1024) ? (int)v : -1;
}

}  // namespace mural
