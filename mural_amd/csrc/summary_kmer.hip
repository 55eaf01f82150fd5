// k-mer rate tables of a prediction shard while it is on the device (mural_amd/predict.py: SummarySink(kmers=...)): what
// `evaluate --kmer_only` (tables.kmer_table) reads back from the written table and the re-packed genome, reduced in one pass over the
// rows from the resident chromosome and the probabilities before '%.4g' rounds them.
//
// A k-mer table is a scatter: rows of one key lie anywhere in the part, so unlike the window tables (summary.hip) there is no segment to
// scan.  The sums are made order-free instead: every probability is quantised ONCE to an integer q = rne(p * 2^71), carried as two
// int64 limbs  hi = floor(p * 2^31)  and  lo = rint((p * 2^31 - hi) * 2^40)  (each step exact in float64: scaling by a power of two, a
// difference of two numbers of one binade or below, one rounding to an integer), and the table cells -- per key the per-label row
// counts, the per-class sums of hi and of lo -- are 64-bit integers added with integer atomics.  Integer addition commutes: the table
// is a function of the SET of rows, bit for bit the same for any split into parts, any launch geometry, any run.  No floating-point
// atomics anywhere.
//   * rows kernel, one launch per k-mer length (each with the LDS its table needs): a workgroup takes a fixed range of rows.  Where the k's table
//     (4^k keys x (3 n_class + 1) cells of 8 bytes, the last the first-appearance word) fits the workgroup's LDS it is accumulated there
//     with LDS atomics and flushed once -- the non-zero cells only -- with global atomics; otherwise every row adds to the global table.
//   * fold kernel (summary_quant.h, with the limb bound), after every slice of at most SK_FOLD_ROWS rows: a slice adds at most
//     X = 2 * SK_FOLD_ROWS = 2^22 terms to a cell (mode 3 counts a palindrome twice).  hi stays exact for 2^32 - 2 additions to one
//     cell, more than a genome of 2^32 rows can make in modes 0 .. 2 (and in mode 3 unless over half of its rows share one palindrome).
//
// Motif rate tables (`evaluate --motif_only`, MuRaL/scripts/calc_motif_corr.py:191-261; SummarySink(motifs=...) and tables.motif_table)
// are the same cells under another key rule: a row adds to EVERY window of m bases (m odd) that contains its site -- m windows of an
// SNV row (i = 0 .. m-1: chrom[start - i : end + m-1 - i]), m - 1 of an INDEL row (i = 1 .. m-1, the SNV windows 0 .. m-2) --, all on
// the reference strand, and a motif shares its cell with its reverse complement: the cell is that of min(key, revcomp(key)) in a table
// indexed by all 4^m keys, of which the half that is the larger of its pair stays zero.
//   * one read per row: the windows of a row of one base (end = start + 1) away from the chromosome's ends are the m-grams of 2m - 1
//     consecutive bases; these are decoded once, the forward and the reverse-complement key rolled across them (two shifts and a mask per
//     base) with a count of the bases since the last non-ACGT one.  Any other row -- within m - 1 bases of an end, or longer than a base,
//     whose unclipped windows all have the wrong length -- clips every window as a Python slice and decodes the few that are m long
//     (kmer_key.h: the clipping, the base decode and the window decode are the k-mer key's).
//   * first[key] = min over the windows of ((order_base + pos) << 5 | i << 1 | o): pos the row's start (or its index in the call,
//     order_by_row), i the window, o = 1 where the window's own key is the larger of the pair.  The minimum is the first window in the
//     reference's order (rows ascending, i ascending within a row) AND says under which orientation the reference names the entry.
//   * fold: a row adds up to m <= 15 times to one cell (a homopolymer run), so the slice between two folds is SM_FOLD_ROWS = 2^18 rows:
//     X = 15 * 2^18 < 2^22 terms.  hi is exact for floor((2^32 - 2) / m) rows in one cell.
#include "common.h"
#include "kmer_key.h"
#include "summary_quant.h"      // quantise_row, SK_MAX_CLASS, the fold: the cells' limbs, shared with the other integer-sum tables

namespace mural {
namespace {

constexpr int SK_THREADS = 256;
constexpr int64_t SK_FOLD_ROWS = 1ll << 21;       // rows between two folds (the bound above)
constexpr int64_t SM_FOLD_ROWS = 1ll << 18;       // ... of the motif tables: up to 15 additions of a row to one cell
constexpr int64_t SK_BLOCK_ROWS = 1ll << 14;      // rows of a workgroup: one LDS table is zeroed and flushed per that many rows
constexpr size_t SK_LDS_BYTES = 160 * 1024;       // LDS of a CU (a single workgroup may take all of it)
constexpr unsigned long long SK_NEVER = ~0ull;

struct KmerArgs {
  MuralGenome g;
  const void* prob;
  const int64_t* start;
  const int64_t* end;
  const uint8_t* strand;
  const void* label;
  int64_t prob_stride, n, order_base;
  int32_t label_kind, n_class, indel, mode, n_k, by_row;      // (k-mer: mode; motif: by_row)
  int32_t k[MURAL_SUMMARY_MAX_KMERS], in_lds[MURAL_SUMMARY_MAX_KMERS];
  u64* table[MURAL_SUMMARY_MAX_KMERS];      // [4^k][3][n_class]: label counts | sums of hi | sums of lo
  u64* first[MURAL_SUMMARY_MAX_KMERS];      // [4^k]
  int32_t* status;
};

size_t lds_bytes_of(int k, int n_class) { return ((size_t)1 << (2 * k)) * (size_t)(3 * n_class + 1) * 8; }

// first[key] = min(first[key], ord).  The plain read may be stale, but the word only ever falls: a stale value is too large and costs an
// atomic that was not needed, never one that was.
__device__ __forceinline__ void global_first(u64* __restrict__ first, int64_t key, u64 ord) {
  if (first[key] > ord) atomicMin(&first[key], ord);
}

// One row into the cell of `key`: cells = an LDS table's [3 n_class + 1] per key (the last the first-appearance word) when in_lds,
// the global table's [3 n_class] otherwise, with the word in first[].  (Two instantiations, each called with its own pointer, so that
// the LDS one keeps LDS atomics.)
template <bool in_lds>
__device__ __forceinline__ void add_row(u64* __restrict__ cells, u64* __restrict__ first, int64_t key, int nc, int lab,
                                        const u64 (&hi)[SK_MAX_CLASS], const u64 (&lo)[SK_MAX_CLASS], u64 ord) {
  u64* cell = cells + key * (in_lds ? 3 * nc + 1 : 3 * nc);
  atomicAdd(&cell[lab], 1ull);
#pragma unroll
  for (int c = 0; c < SK_MAX_CLASS; ++c) {
    if (c < nc) {
      if (hi[c]) atomicAdd(&cell[nc + c], hi[c]);
      if (lo[c]) atomicAdd(&cell[2 * nc + c], lo[c]);
    }
  }
  if (in_lds)
    atomicMin(&cell[3 * nc], ord);
  else
    global_first(first, key, ord);
}

// The prologue and the epilogue of a rows kernel whose table lives in LDS: all cells zero and the words at "never"; the non-zero cells
// added to the global table once.
__device__ __forceinline__ void lds_table_clear(u64* __restrict__ cells, int64_t groups, int n_cells) {
  for (int64_t c = threadIdx.x; c < groups * n_cells; c += SK_THREADS) cells[c] = (c % n_cells == n_cells - 1) ? SK_NEVER : 0ull;
  __syncthreads();
}

__device__ __forceinline__ void lds_table_flush(const u64* __restrict__ cells, int64_t groups, int nc, u64* __restrict__ table,
                                                u64* __restrict__ first) {
  const int n_cells = 3 * nc + 1;
  __syncthreads();
  for (int64_t c = threadIdx.x; c < groups * n_cells; c += SK_THREADS) {
    const u64 v = cells[c];
    const int64_t key = c / n_cells;
    const int col = (int)(c % n_cells);
    if (col == n_cells - 1) {
      if (v != SK_NEVER) global_first(first, key, v);
    } else if (v) {
      atomicAdd(&table[key * (3 * nc) + col], v);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(SK_THREADS) void summary_kmer_rows_kernel(KmerArgs A, int j, int64_t row0, int64_t row1) {
  extern __shared__ u64 sk_cells[];
  const int k = A.k[j], nc = A.n_class;
  const bool in_lds = A.in_lds[j] != 0;
  const int cells = 3 * nc + 1;
  const int64_t groups = (int64_t)1 << (2 * k);
  u64* __restrict__ table = A.table[j];
  u64* __restrict__ first = A.first[j];
  if (in_lds) lds_table_clear(sk_cells, groups, cells);
  const T* __restrict__ prob = static_cast<const T*>(A.prob);
  const int64_t b0 = row0 + (int64_t)blockIdx.x * SK_BLOCK_ROWS, b1 = min(b0 + SK_BLOCK_ROWS, row1);
  int32_t bad = 0;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += SK_THREADS) {
    const int64_t st = A.start[i];
    const int lab = load_label(A.label, A.label_kind, i);
    u64 hi[SK_MAX_CLASS], lo[SK_MAX_CLASS];
    const int32_t bad_row = quantise_row(prob + i * A.prob_stride, nc, st, lab, hi, lo);
    if (bad_row) {
      bad |= bad_row;
      continue;
    }
    int32_t fwd, rev;
    kmer_key_decode(A.g, st, A.end[i], k, A.indel, fwd, rev);
    const u64 ord = (u64)(A.order_base + 2 * st);
    int32_t key[2] = {fwd, rev};
    if (A.mode != 3) key[0] = kmer_key_minus(A.mode, A.strand, i) ? rev : fwd, key[1] = -1;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (key[sub] < 0) continue;
      if (in_lds)
        add_row<true>(sk_cells, first, key[sub], nc, lab, hi, lo, ord + sub);
      else
        add_row<false>(table, first, key[sub], nc, lab, hi, lo, ord + sub);
    }
  }
  if (in_lds) lds_table_flush(sk_cells, groups, nc, table, first);
  if (bad) atomicOr(A.status, bad);
}

// The motif windows of a row: see the head of the file.
template <typename T>
__global__ __launch_bounds__(SK_THREADS) void summary_motif_rows_kernel(KmerArgs A, int j, int64_t row0, int64_t row1) {
  extern __shared__ u64 sk_cells[];
  const int m = A.k[j], nc = A.n_class;
  const bool in_lds = A.in_lds[j] != 0;
  const int64_t groups = (int64_t)1 << (2 * m);
  u64* __restrict__ table = A.table[j];
  u64* __restrict__ first = A.first[j];
  if (in_lds) lds_table_clear(sk_cells, groups, 3 * nc + 1);
  const T* __restrict__ prob = static_cast<const T*>(A.prob);
  const int64_t b0 = row0 + (int64_t)blockIdx.x * SK_BLOCK_ROWS, b1 = min(b0 + SK_BLOCK_ROWS, row1);
  const int n_win = m - A.indel;                    // window w = 0 .. n_win - 1 is chrom[start - w : end + m-1 - w], the reference's i = w + indel
  const uint32_t mask = (uint32_t)(groups - 1);
  int32_t bad = 0;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += SK_THREADS) {
    const int64_t st = A.start[i], en = A.end[i];
    const int lab = load_label(A.label, A.label_kind, i);
    u64 hi[SK_MAX_CLASS], lo[SK_MAX_CLASS];
    const int32_t bad_row = quantise_row(prob + i * A.prob_stride, nc, st, lab, hi, lo);
    if (bad_row) {
      bad |= bad_row;
      continue;
    }
    const u64 ord = (u64)(A.order_base + (A.by_row ? i : st)) << 5;
    auto add = [&](int32_t fwd, int32_t rev, int w) {
      const u64 word = ord | (u64)((w + A.indel) << 1) | (fwd > rev ? 1u : 0u);
      if (in_lds)
        add_row<true>(sk_cells, first, min(fwd, rev), nc, lab, hi, lo, word);
      else
        add_row<false>(table, first, min(fwd, rev), nc, lab, hi, lo, word);
    };
    if (en - st == 1 && st >= n_win - 1 && en + (m - 1) <= A.g.length) {
      // no window is clipped: the m-grams of bases start - (n_win-1) .. start + m-1, the one that ends at base q being window
      // w = start + m-1 - q
      uint32_t fwd = 0, rev = 0;
      int run = 0;                                  // bases since the last one that is not A/C/G/T
      for (int64_t q = st - (n_win - 1); q < st + m; ++q) {
        bool n_base = false;
        const uint32_t code = (uint32_t)kmer_base(A.g, q, n_base);
        fwd = ((fwd << 2) | code) & mask;
        rev = (rev >> 2) | ((3u - code) << (2 * (m - 1)));
        run = n_base ? 0 : run + 1;
        if (run >= m) add((int32_t)fwd, (int32_t)rev, (int)(st + (m - 1) - q));
      }
    } else {
      for (int w = 0; w < n_win; ++w) {
        int32_t fwd, rev;
        kmer_window_decode(A.g, st - w, en + (m - 1) - w, m, fwd, rev);
        if (fwd >= 0) add(fwd, rev, w);
      }
    }
  }
  if (in_lds) lds_table_flush(sk_cells, groups, nc, table, first);
  if (bad) atomicOr(A.status, bad);
}

// the k-mer (or motif) tables of a call as the fold kernel takes them, and its grid
int launch_fold(const KmerArgs& A, hipStream_t stream) {
  FoldTables F{};
  int64_t fold_threads = 0;
  for (int j = 0; j < A.n_k; ++j) {
    F.table[j] = A.table[j], F.n_groups[j] = (int64_t)1 << (2 * A.k[j]);
    fold_threads = std::max(fold_threads, F.n_groups[j] * A.n_class);
  }
  F.nc = A.n_class;
  const dim3 fold_grid((unsigned)((fold_threads + SK_THREADS - 1) / SK_THREADS), (unsigned)A.n_k);
  hipLaunchKernelGGL(summary_fold_kernel<SK_THREADS>, fold_grid, dim3(SK_THREADS), 0, stream, F);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

}  // namespace
}  // namespace mural

using namespace mural;

extern "C" int32_t mural_summary_kmer_in_lds(int32_t k, int32_t n_class) {
  if (k < 1 || k > 15 || n_class < 1 || n_class > SK_MAX_CLASS) return 0;
  return lds_bytes_of(k, n_class) <= SK_LDS_BYTES ? 1 : 0;
}

extern "C" int mural_summary_kmer_rows(const MuralSummaryKmerRows* s, void* stream) {
  MURAL_REQUIRE(s && s->genome, "summary_kmer_rows: NULL argument");
  MURAL_REQUIRE(s->n >= 0 && s->n_class >= 1 && s->n_class <= SK_MAX_CLASS, "summary_kmer_rows: n >= 0 and 1 <= n_class <= %d required",
                SK_MAX_CLASS);
  MURAL_REQUIRE(s->n_k >= 1 && s->n_k <= MURAL_SUMMARY_MAX_KMERS, "summary_kmer_rows: 1 .. %d k-mer lengths per call",
                MURAL_SUMMARY_MAX_KMERS);
  MURAL_REQUIRE(s->label_kind >= 0 && s->label_kind <= 2, "summary_kmer_rows: label_kind is 0 (float32), 1 (int32) or 2 (int64)");
  MURAL_REQUIRE(s->mode >= 0 && s->mode <= 3 && (s->mode != 0 || s->strand || s->n == 0), "summary_kmer_rows: bad strand mode");
  MURAL_REQUIRE(s->order_base >= 0, "summary_kmer_rows: order_base < 0");
  for (int j = 0; j < s->n_k; ++j)
    MURAL_REQUIRE(s->k[j] >= 1 && s->k[j] <= 15 && s->table[j] && s->first[j], "summary_kmer_rows: bad k-mer table %d (1 <= k <= 15)", j);
  if (s->n == 0) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->start && s->end && s->label && s->status, "summary_kmer_rows: NULL argument");
  MURAL_REQUIRE(s->genome->packed2 && s->genome->nmask && s->genome->length >= 0, "summary_kmer_rows: empty genome");
  MURAL_REQUIRE(s->prob_stride >= s->n_class, "summary_kmer_rows: prob_stride < n_class");
  KmerArgs A{};
  A.g = *s->genome;
  A.prob = s->prob, A.start = s->start, A.end = s->end, A.strand = s->strand, A.label = s->label;
  A.prob_stride = s->prob_stride, A.n = s->n, A.order_base = s->order_base;
  A.label_kind = s->label_kind, A.n_class = s->n_class, A.indel = s->indel ? 1 : 0, A.mode = s->mode, A.n_k = s->n_k;
  for (int j = 0; j < s->n_k; ++j) {
    A.k[j] = s->k[j];
    A.in_lds[j] = mural_summary_kmer_in_lds(s->k[j], s->n_class);
    A.table[j] = reinterpret_cast<u64*>(s->table[j]), A.first[j] = reinterpret_cast<u64*>(s->first[j]);
  }
  A.status = s->status;
  static DynLdsOnce once;
  if (const int rc = once.ensure(summary_kmer_rows_kernel<float>, summary_kmer_rows_kernel<double>)) return rc;
  for (int64_t r0 = 0; r0 < s->n; r0 += SK_FOLD_ROWS) {
    const int64_t r1 = std::min(r0 + SK_FOLD_ROWS, s->n);
    const dim3 grid((unsigned)((r1 - r0 + SK_BLOCK_ROWS - 1) / SK_BLOCK_ROWS));
    for (int j = 0; j < s->n_k; ++j) {
      const size_t lds = A.in_lds[j] ? lds_bytes_of(A.k[j], A.n_class) : 0;
      if (s->prob_f64)
        hipLaunchKernelGGL(summary_kmer_rows_kernel<double>, grid, dim3(SK_THREADS), lds, (hipStream_t)stream, A, j, r0, r1);
      else
        hipLaunchKernelGGL(summary_kmer_rows_kernel<float>, grid, dim3(SK_THREADS), lds, (hipStream_t)stream, A, j, r0, r1);
      MURAL_HIP_CHECK(hipGetLastError());
    }
    if (const int rc = launch_fold(A, (hipStream_t)stream)) return rc;
  }
  return MURAL_OK;
}

extern "C" int32_t mural_summary_motif_in_lds(int32_t m, int32_t n_class) {
  if (m < 3 || m > 15 || m % 2 == 0) return 0;
  return mural_summary_kmer_in_lds(m, n_class);
}

extern "C" int mural_summary_motif_rows(const MuralSummaryMotifRows* s, void* stream) {
  MURAL_REQUIRE(s && s->genome, "summary_motif_rows: NULL argument");
  MURAL_REQUIRE(s->n >= 0 && s->n_class >= 1 && s->n_class <= SK_MAX_CLASS, "summary_motif_rows: n >= 0 and 1 <= n_class <= %d required",
                SK_MAX_CLASS);
  MURAL_REQUIRE(s->n_m >= 1 && s->n_m <= MURAL_SUMMARY_MAX_KMERS, "summary_motif_rows: 1 .. %d motif lengths per call",
                MURAL_SUMMARY_MAX_KMERS);
  MURAL_REQUIRE(s->label_kind >= 0 && s->label_kind <= 2, "summary_motif_rows: label_kind is 0 (float32), 1 (int32) or 2 (int64)");
  MURAL_REQUIRE(s->order_base >= 0 && s->order_base < (1ll << 58), "summary_motif_rows: order_base outside 0 .. 2^58 - 1");
  for (int j = 0; j < s->n_m; ++j)
    MURAL_REQUIRE(s->m[j] >= 3 && s->m[j] <= 15 && s->m[j] % 2 == 1 && s->table[j] && s->first[j],
                  "summary_motif_rows: bad motif table %d (m odd, 3 <= m <= 15)", j);
  if (s->n == 0) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->start && s->end && s->label && s->status, "summary_motif_rows: NULL argument");
  MURAL_REQUIRE(s->genome->packed2 && s->genome->nmask && s->genome->length >= 0, "summary_motif_rows: empty genome");
  MURAL_REQUIRE(s->prob_stride >= s->n_class, "summary_motif_rows: prob_stride < n_class");
  KmerArgs A{};
  A.g = *s->genome;
  A.prob = s->prob, A.start = s->start, A.end = s->end, A.label = s->label;
  A.prob_stride = s->prob_stride, A.n = s->n, A.order_base = s->order_base;
  A.label_kind = s->label_kind, A.n_class = s->n_class, A.indel = s->indel ? 1 : 0, A.n_k = s->n_m, A.by_row = s->order_by_row ? 1 : 0;
  for (int j = 0; j < s->n_m; ++j) {
    A.k[j] = s->m[j];
    A.in_lds[j] = mural_summary_motif_in_lds(s->m[j], s->n_class);
    A.table[j] = reinterpret_cast<u64*>(s->table[j]), A.first[j] = reinterpret_cast<u64*>(s->first[j]);
  }
  A.status = s->status;
  static DynLdsOnce once;
  if (const int rc = once.ensure(summary_motif_rows_kernel<float>, summary_motif_rows_kernel<double>)) return rc;
  for (int64_t r0 = 0; r0 < s->n; r0 += SM_FOLD_ROWS) {
    const int64_t r1 = std::min(r0 + SM_FOLD_ROWS, s->n);
    const dim3 grid((unsigned)((r1 - r0 + SK_BLOCK_ROWS - 1) / SK_BLOCK_ROWS));
    for (int j = 0; j < s->n_m; ++j) {
      const size_t lds = A.in_lds[j] ? lds_bytes_of(A.k[j], A.n_class) : 0;
      if (s->prob_f64)
        hipLaunchKernelGGL(summary_motif_rows_kernel<double>, grid, dim3(SK_THREADS), lds, (hipStream_t)stream, A, j, r0, r1);
      else
        hipLaunchKernelGGL(summary_motif_rows_kernel<float>, grid, dim3(SK_THREADS), lds, (hipStream_t)stream, A, j, r0, r1);
      MURAL_HIP_CHECK(hipGetLastError());
    }
    if (const int rc = launch_fold(A, (hipStream_t)stream)) return rc;
  }
  return MURAL_OK;
}
