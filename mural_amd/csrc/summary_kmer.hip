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
//   * fold kernel, a thread per (key, class), no atomics: hi += lo >> 40, lo &= 2^40 - 1, after every slice of at most SK_FOLD_ROWS
//     rows.  Bound: lo < 2^40 after a fold; a slice adds at most 2 * SK_FOLD_ROWS terms (mode 3 counts a palindrome twice) of at most
//     2^40 each, so lo < 2^40 + 2^22 * 2^40 < 2^63 before the next fold.  hi is at most (2^31 + 1) per addition: below 2^64 -- the
//     cells are read as UNSIGNED 64-bit numbers -- for 2^32 - 2 additions to one cell, more than a genome of 2^32 rows can make in
//     modes 0 .. 2 (and in mode 3 unless over half of its rows share one palindrome).
#include "common.h"
#include "kmer_key.h"

namespace mural {
namespace {

constexpr int SK_THREADS = 256;
constexpr int SK_MAX_CLASS = 8;
constexpr int64_t SK_FOLD_ROWS = 1ll << 21;       // rows between two folds (the bound above)
constexpr int64_t SK_BLOCK_ROWS = 1ll << 14;      // rows of a workgroup: one LDS table is zeroed and flushed per that many rows
constexpr size_t SK_LDS_BYTES = 160 * 1024;       // LDS of a CU (a single workgroup may take all of it)
constexpr int SK_LO_BITS = 40;
constexpr unsigned long long SK_NEVER = ~0ull;
typedef unsigned long long u64;

struct KmerArgs {
  MuralGenome g;
  const void* prob;
  const int64_t* start;
  const int64_t* end;
  const uint8_t* strand;
  const void* label;
  int64_t prob_stride, n, order_base;
  int32_t label_kind, n_class, indel, mode, n_k;
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

template <typename T>
__global__ __launch_bounds__(SK_THREADS) void summary_kmer_rows_kernel(KmerArgs A, int j, int64_t row0, int64_t row1) {
  extern __shared__ u64 sk_cells[];
  const int k = A.k[j], nc = A.n_class;
  const bool in_lds = A.in_lds[j] != 0;
  const int cells = 3 * nc + 1;
  const int64_t groups = (int64_t)1 << (2 * k);
  u64* __restrict__ table = A.table[j];
  u64* __restrict__ first = A.first[j];
  if (in_lds) {
    for (int64_t c = threadIdx.x; c < groups * cells; c += SK_THREADS) sk_cells[c] = (c % cells == cells - 1) ? SK_NEVER : 0ull;
    __syncthreads();
  }
  const T* __restrict__ prob = static_cast<const T*>(A.prob);
  const int64_t b0 = row0 + (int64_t)blockIdx.x * SK_BLOCK_ROWS, b1 = min(b0 + SK_BLOCK_ROWS, row1);
  int32_t bad = 0;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += SK_THREADS) {
    const int64_t st = A.start[i];
    const int lab = load_label(A.label, A.label_kind, i);
    int32_t bad_row = 0;
    if (st < 0) bad_row |= SM_BAD_START;
    if (lab < 0 || lab >= nc) bad_row |= SM_BAD_LABEL;
    u64 hi[SK_MAX_CLASS], lo[SK_MAX_CLASS];
#pragma unroll
    for (int c = 0; c < SK_MAX_CLASS; ++c) {
      hi[c] = 0, lo[c] = 0;
      if (c < nc) {
        const double p = (double)prob[i * A.prob_stride + c];      // (float -> double is exact)
        // 0 <= p <= 1 on the bit pattern -- non-negative doubles order like their bits --, so that NaN is caught whatever the
        // compiler assumes about comparisons; -0.0 counts as 0
        const u64 bits = (u64)__double_as_longlong(p);
        if (bits > 0x3FF0000000000000ull && bits != 0x8000000000000000ull) {
          bad_row |= SM_BAD_PROB;
        } else {
          const double s = p * 2147483648.0;                       // p * 2^31
          const double h = floor(s);
          hi[c] = (u64)(long long)h;
          lo[c] = (u64)(long long)rint((s - h) * 1099511627776.0);      // * 2^40, half to even
        }
      }
    }
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
      if (in_lds) {
        u64* cell = sk_cells + (int64_t)key[sub] * cells;
        atomicAdd(&cell[lab], 1ull);
#pragma unroll
        for (int c = 0; c < SK_MAX_CLASS; ++c) {
          if (c < nc) {
            if (hi[c]) atomicAdd(&cell[nc + c], hi[c]);
            if (lo[c]) atomicAdd(&cell[2 * nc + c], lo[c]);
          }
        }
        atomicMin(&cell[3 * nc], ord + sub);
      } else {
        u64* cell = table + (int64_t)key[sub] * (3 * nc);
        atomicAdd(&cell[lab], 1ull);
#pragma unroll
        for (int c = 0; c < SK_MAX_CLASS; ++c) {
          if (c < nc) {
            if (hi[c]) atomicAdd(&cell[nc + c], hi[c]);
            if (lo[c]) atomicAdd(&cell[2 * nc + c], lo[c]);
          }
        }
        global_first(first, key[sub], ord + sub);
      }
    }
  }
  if (in_lds) {
    __syncthreads();
    for (int64_t c = threadIdx.x; c < groups * cells; c += SK_THREADS) {
      const u64 v = sk_cells[c];
      const int64_t key = c / cells;
      const int col = (int)(c % cells);
      if (col == cells - 1) {
        if (v != SK_NEVER) global_first(first, key, v);
      } else if (v) {
        atomicAdd(&table[key * (3 * nc) + col], v);
      }
    }
  }
  if (bad) atomicOr(A.status, bad);
}

// carry the overflow of the lo limbs into the hi limbs: a thread per (key, class), plain loads and stores
__global__ __launch_bounds__(SK_THREADS) void summary_kmer_fold_kernel(KmerArgs A) {
  const int j = blockIdx.y, nc = A.n_class;
  const int64_t t = (int64_t)blockIdx.x * SK_THREADS + threadIdx.x;
  if (t >= ((int64_t)nc << (2 * A.k[j]))) return;
  u64* __restrict__ cell = A.table[j] + (t / nc) * (3 * nc) + t % nc;
  const u64 lo = cell[2 * nc];
  if (lo >> SK_LO_BITS) {
    cell[nc] += lo >> SK_LO_BITS;
    cell[2 * nc] = lo & ((1ull << SK_LO_BITS) - 1);
  }
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
  int64_t fold_threads = 0;
  for (int j = 0; j < s->n_k; ++j) {
    A.k[j] = s->k[j];
    A.in_lds[j] = mural_summary_kmer_in_lds(s->k[j], s->n_class);
    A.table[j] = reinterpret_cast<u64*>(s->table[j]), A.first[j] = reinterpret_cast<u64*>(s->first[j]);
    fold_threads = std::max(fold_threads, (int64_t)s->n_class << (2 * s->k[j]));
  }
  A.status = s->status;
  static DynLdsOnce once;
  if (const int rc = once.ensure(summary_kmer_rows_kernel<float>, summary_kmer_rows_kernel<double>)) return rc;
  const dim3 fold_grid((unsigned)((fold_threads + SK_THREADS - 1) / SK_THREADS), (unsigned)s->n_k);
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
    hipLaunchKernelGGL(summary_kmer_fold_kernel, fold_grid, dim3(SK_THREADS), 0, (hipStream_t)stream, A);
    MURAL_HIP_CHECK(hipGetLastError());
  }
  return MURAL_OK;
}
