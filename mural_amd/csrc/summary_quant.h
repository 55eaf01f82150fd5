// The row checks, the two-limb quantisation and the limb fold of the integer-sum summaries, shared by csrc/summary_kmer.hip (k-mer and
// motif tables), csrc/summary_annot.hip (annotation tables) and the per-transcript tables (csrc/summary_conseq.hip,
// csrc/summary_txstruct.hip, csrc/summary_txindel.hip) so that their cells cannot drift: q = rne(p * 2^71) carried as hi = floor(p * 2^31)
// and lo = rint((p * 2^31 - hi) * 2^40), each step exact in float64.  The SNV rows of the consequence and structure tables (SnvRows),
// their row function and their check kernel are here as well.
// (csrc/summary_calib.hip carries 46-bit limbs at irregular cell positions: it has a quantisation, a fold and bounds of its own.)
#pragma once
#include "common.h"
#include "kmer_key.h"

namespace mural {

constexpr int SK_MAX_CLASS = 8;
constexpr int SK_LO_BITS = 40;
constexpr u64 SK_LO_MASK = (1ull << SK_LO_BITS) - 1;

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

// The SNV rows (4 classes) of a per-transcript table, as its kernels read them.
struct SnvRows {
  const void* prob;
  const int64_t* start;
  const uint8_t* strand;      // or nullptr: all '+'
  const void* label;
  int64_t prob_stride, n;
  int32_t label_kind;
  int32_t* status;
};

// X from the row fields of a public argument struct
template <typename Pub>
inline SnvRows snv_rows(const Pub* s) {
  SnvRows X{};
  X.prob = s->prob, X.start = s->start, X.strand = s->strand, X.label = s->label, X.prob_stride = s->prob_stride, X.n = s->n;
  X.label_kind = s->label_kind, X.status = s->status;
  return X;
}

// The checks of SNV row i (status bits, 0 if it counts) and the limbs of its classes 1 .. 3; class 0's probability is not read.
template <typename T>
__device__ __forceinline__ int32_t snv_row(const SnvRows& A, int64_t i, int& lab, u64 (&hi)[3], u64 (&lo)[3]) {
  const T* __restrict__ p_row = static_cast<const T*>(A.prob) + i * A.prob_stride;
  lab = load_label(A.label, A.label_kind, i);
  int32_t bad = 0;
  if (A.start[i] < 0) bad |= SM_BAD_START;
  if (lab < 0 || lab >= 4) bad |= SM_BAD_LABEL;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (!quantise_prob((double)p_row[c + 1], hi[c], lo[c])) bad |= SM_BAD_PROB;      // (float -> double is exact)
  return bad;
}

// a thread per SNV row: the status bits, a start below the row before it among them
template <typename T, int THREADS>
__global__ __launch_bounds__(THREADS) void snv_check_kernel(SnvRows A) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  int32_t bad = 0;
  if (i < A.n) {
    int lab;
    u64 hi[3], lo[3];
    bad = snv_row<T>(A, i, lab, hi, lo);
    if (i > 0 && A.start[i] < A.start[i - 1]) bad |= SM_BAD_ORDER;
  }
  if (bad) atomicOr(A.status, bad);
}

// the check kernel on `st`; MURAL_OK or the error code of the launch
template <int THREADS>
inline int launch_snv_check(hipStream_t st, const SnvRows& A, bool prob_f64) {
  const dim3 grid((unsigned)((A.n + THREADS - 1) / THREADS)), block(THREADS);
  if (prob_f64)
    hipLaunchKernelGGL((snv_check_kernel<double, THREADS>), grid, block, 0, st, A);
  else
    hipLaunchKernelGGL((snv_check_kernel<float, THREADS>), grid, block, 0, st, A);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

// The fold: the overflow of a sum of lo limbs goes into the sum of hi limbs; the pair's value hi * 2^40 + lo does not change.
// THE LIMB BOUND.  A lo limb is at most 2^40 (2^40 itself where the fraction rounds up: the pair's value stays right), and a folded
// lo is below 2^40.  A TERM is a lo limb or a folded sum of lo limbs; unfolded sums count as the terms they hold.  A cell that takes at
// most X terms between two folds holds lo <= 2^40 (1 + X) before the next fold: below 2^63 while X <= 2^23 - 2, and below 2^40 on
// return from an entry that folds last.  Each file that adds to such cells gives its X in its head comment; with this rule that is
// all a reader needs.  A hi limb is at most 2^31 and a row's carry at most 1: a cell's hi is exact for 2^32 - 2 additions.
__device__ __forceinline__ void fold_limbs(u64& hi, u64& lo) {
  hi += lo >> SK_LO_BITS;
  lo &= SK_LO_MASK;
}

// The tables whose lo limbs one launch folds: table blockIdx.y is [n_groups][3][nc] -- label counts | sums of hi | sums of lo.
struct FoldTables {
  u64* table[MURAL_SUMMARY_MAX_KMERS];
  int64_t n_groups[MURAL_SUMMARY_MAX_KMERS];
  int32_t nc;
};

// carry the overflow of the tables' lo limbs into their hi limbs: a thread per (group, class), plain loads and stores
template <int THREADS>
__global__ __launch_bounds__(THREADS) void summary_fold_kernel(FoldTables F) {
  const int j = blockIdx.y, nc = F.nc;
  const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (t >= F.n_groups[j] * nc) return;
  u64* __restrict__ cell = F.table[j] + (t / nc) * (3 * nc) + t % nc;
  u64 lo = cell[2 * nc];
  if (lo >> SK_LO_BITS) {
    u64 hi = cell[nc];
    fold_limbs(hi, lo);
    cell[nc] = hi, cell[2 * nc] = lo;
  }
}

// the fold of a per-transcript table [n_cells][3][1] at the end of a call, on `st`; MURAL_OK or the error code of the launch
template <int THREADS>
inline int launch_cell_fold(hipStream_t st, u64* table, int64_t n_cells) {
  FoldTables F{};
  F.table[0] = table, F.n_groups[0] = n_cells, F.nc = 1;      // [transcript][bin][3] = [cell][3][1]
  hipLaunchKernelGGL(summary_fold_kernel<THREADS>, dim3((unsigned)((n_cells + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, F);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

}  // namespace mural
