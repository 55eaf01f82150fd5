// Expected and observed mutations per annotated interval set while a prediction shard is on the device
// (mural_amd/summaries.py: SummarySink(annotations=...); tables.annotation_table from a written table): per NAME -- a gene's exons, an
// enhancer set -- the label counts and the sums of the probabilities of the rows whose start lies in one of the name's intervals.
//
// The intervals are arbitrary: unsorted, overlapping, nested, many per name.  The host (tables.read_annotations) merges each name's
// intervals per chromosome into disjoint PIECES [b0, b1) with the name's index as their group; pieces of different names overlap
// freely.  A per-row stabbing query would do unbounded work under nesting.  The rows of a part ascend in start instead, so the rows of
// a piece are ONE contiguous range [i0, i1) -- both ends lower bounds, the first row with start >= b -- and its sums are the
// difference of two row prefix sums.  The cells are the k-mer tables' (summary_quant.h: q = rne(p * 2^71) as two integer limbs), so
// every sum is an integer sum: the table is a function of the SET of rows alone, bit for bit, whatever the parts, slices or tiles.
// Per slice of at most SA_SLICE_ROWS rows:
//   * tile kernel, a wave per tile of SA_TILE = 64 consecutive rows (a row per lane): quantise, reduce the 3 n_class words -- label
//     counts by ballot, the limbs by a wave butterfly -- and store them with plain vector stores; rows that fail a check quantise to
//     nothing and set status; start[i] < start[i - 1] sets bit 2.
//   * scan kernel, a workgroup per word (common.h: run_excl_scan): the exclusive prefix over the tiles in place, per limb and WITHOUT
//     folding: a slice adds at most 2^23 terms of at most 2^40 to a lo word, so the prefixes do not wrap and their differences are exact.
//   * piece kernel, a wave per piece: two 64-ary searches in start (common.h: wave_partition_point; 4 rounds of one probe per lane for
//     2^23 rows), prefix(i) = the tile prefix + a masked reduce over the at most 63 rows of the partial tile, re-read and re-quantised
//     (mostly L2 hits: at most 2 * n_pieces * 64 rows); the difference is folded and its non-zero words are added to the group's cells
//     with 64-bit INTEGER atomics, one wave-instruction of 3 n_class contiguous words.  Empty pieces add nothing.
//   * fold kernel (summary_quant.h, with the limb bound), after every SA_FOLD_PIECES pieces: a piece adds one folded term to a cell,
//     X = SA_FOLD_PIECES = 2^20 terms between two folds.
// No floating-point atomics, no synchronisation, no read-back.
#include "common.h"
#include "kmer_key.h"
#include "summary_quant.h"

namespace mural {
namespace {

constexpr int SA_TILE = 64;                       // rows of a tile = lanes of a wave
constexpr int SA_THREADS = 256;                   // tile and piece kernels: 4 waves, a tile / a piece each
constexpr int SA_WAVES = SA_THREADS / 64;
constexpr int SA_SCAN_THREADS = 1024;
constexpr int64_t SA_SLICE_ROWS = 1ll << 23;      // rows whose unfolded lo prefixes stay below 2^63
constexpr int64_t SA_FOLD_PIECES = 1ll << 20;     // pieces between two folds of the table

struct AnnotArgs {
  const void* prob;
  const int64_t* start;
  const void* label;
  int64_t prob_stride;
  int32_t label_kind, n_class, n_groups;
  const int64_t* b0;
  const int64_t* b1;
  const int32_t* group;
  u64* tiles;           // [n_tiles + 1][3 n_class]: the tile sums, then their exclusive prefixes
  u64* table;
  int32_t* status;
};

// The 3 n_class words of rows row .. row + cnt - 1 (0 <= cnt <= 64, a row per lane): word j -- label counts | sums of hi | sums of
// lo -- comes back in lane j, 0 in the lanes from 3 n_class on.  `bad`: the status bits of the rows.
template <typename T>
__device__ __forceinline__ u64 tile_words(const AnnotArgs& A, int64_t row, int cnt, int32_t& bad) {
  const int lane = threadIdx.x & 63, nc = A.n_class;
  u64 hi[SK_MAX_CLASS], lo[SK_MAX_CLASS];
  int lab = -1;
  bool live = false;
#pragma unroll
  for (int c = 0; c < SK_MAX_CLASS; ++c) hi[c] = 0, lo[c] = 0;
  if (lane < cnt) {
    const int64_t i = row + lane;
    lab = load_label(A.label, A.label_kind, i);
    const int32_t bad_row = quantise_row(static_cast<const T*>(A.prob) + i * A.prob_stride, nc, A.start[i], lab, hi, lo);
    bad |= bad_row;
    live = bad_row == 0;
    if (!live) {
#pragma unroll
      for (int c = 0; c < SK_MAX_CLASS; ++c) hi[c] = 0, lo[c] = 0;
    }
  }
  u64 word = 0;
#pragma unroll
  for (int c = 0; c < SK_MAX_CLASS; ++c) {
    if (c < nc) {      // (wave-uniform)
      const u64 n_lab = (u64)__popcll(__ballot(live && lab == c));
      const u64 h = wave_sum(hi[c]), l = wave_sum(lo[c]);
      if (lane == c) word = n_lab;
      if (lane == nc + c) word = h;
      if (lane == 2 * nc + c) word = l;
    }
  }
  return word;
}

template <typename T>
__global__ __launch_bounds__(SA_THREADS) void summary_annot_tile_kernel(AnnotArgs A, int64_t s0, int64_t s1, int64_t n_tiles) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * SA_WAVES + (threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const int64_t row = s0 + t * SA_TILE;
  const int cnt = (int)min((int64_t)SA_TILE, s1 - row);
  int32_t bad = 0;
  if (lane < cnt && row + lane > 0 && A.start[row + lane] < A.start[row + lane - 1]) bad |= SM_BAD_ORDER;
  const u64 word = tile_words<T>(A, row, cnt, bad);
  if (lane < 3 * A.n_class) A.tiles[t * (3 * A.n_class) + lane] = word;
  if (bad) atomicOr(A.status, bad);
}

// exclusive prefix over the tiles of word blockIdx.x, in place; entry n_tiles gets the total.  A thread owns a run of consecutive tiles.
__global__ __launch_bounds__(SA_SCAN_THREADS) void summary_annot_scan_kernel(AnnotArgs A, int64_t n_tiles) {
  const int words = 3 * A.n_class;
  u64* __restrict__ col = A.tiles + blockIdx.x;
  const u64 total = run_excl_scan<SA_SCAN_THREADS, u64>(n_tiles, [&](int64_t t) { return col[t * words]; },
                                                        [&](int64_t t, u64 x) { col[t * words] = x; });
  if (threadIdx.x == 0) col[n_tiles * words] = total;
}

// lane j: word j of the sums over rows s0 .. i - 1 of the slice
template <typename T>
__device__ __forceinline__ u64 prefix_words(const AnnotArgs& A, int64_t s0, int64_t i) {
  const int lane = threadIdx.x & 63, words = 3 * A.n_class;
  const int64_t tile = (i - s0) / SA_TILE;
  const int rem = (int)((i - s0) % SA_TILE);
  u64 word = lane < words ? A.tiles[tile * words + lane] : 0;
  int32_t bad = 0;      // (reported by the tile kernel)
  if (rem) word += tile_words<T>(A, s0 + tile * SA_TILE, rem, bad);
  return word;
}

template <typename T>
__global__ __launch_bounds__(SA_THREADS) void summary_annot_piece_kernel(AnnotArgs A, int64_t s0, int64_t s1, int64_t p0, int64_t p1) {
  const int lane = threadIdx.x & 63, nc = A.n_class;
  const int64_t p = p0 + (int64_t)blockIdx.x * SA_WAVES + (threadIdx.x >> 6);
  if (p >= p1) return;
  const int32_t g = A.group[p];
  if (g < 0 || g >= A.n_groups) return;
  // both ends are lower bounds: the first row with start >= b (the rows ascend: the rows below the bound come first)
  const int64_t* __restrict__ start = A.start;
  const int64_t b0 = A.b0[p], b1 = A.b1[p];
  const int64_t i0 = wave_partition_point(s0, s1, [&](int64_t i) { return start[i] < b0; });
  const int64_t i1 = wave_partition_point(i0, s1, [&](int64_t i) { return start[i] < b1; });
  if (i1 <= i0) return;
  const u64 sum = prefix_words<T>(A, s0, i1) - prefix_words<T>(A, s0, i0);
  const u64 above = __shfl(sum, (lane + nc) & 63, 64);      // a hi lane reads its lo lane
  u64 word = sum;
  if (lane >= nc && lane < 2 * nc) word += above >> SK_LO_BITS;      // (fold_limbs, the two limbs in two lanes)
  if (lane >= 2 * nc) word &= SK_LO_MASK;
  if (lane < 3 * nc && word) atomicAdd(&A.table[(int64_t)g * (3 * nc) + lane], word);
}

int64_t tiles_of(int64_t rows) { return (rows + SA_TILE - 1) / SA_TILE; }

}  // namespace
}  // namespace mural

using namespace mural;

extern "C" int32_t mural_summary_annot_tile_rows(void) { return SA_TILE; }
extern "C" int64_t mural_summary_annot_slice_rows(void) { return SA_SLICE_ROWS; }
extern "C" int64_t mural_summary_annot_fold_pieces(void) { return SA_FOLD_PIECES; }

extern "C" size_t mural_summary_annot_workspace_bytes(int64_t n, int32_t n_class) {
  if (n <= 0 || n_class < 1 || n_class > SK_MAX_CLASS) return 0;
  return (size_t)(tiles_of(std::min(n, SA_SLICE_ROWS)) + 1) * (size_t)(3 * n_class) * sizeof(u64);
}

extern "C" int mural_summary_annot_rows(const MuralSummaryAnnotRows* s, void* ws, size_t ws_bytes, void* stream) {
  MURAL_REQUIRE(s, "summary_annot_rows: NULL argument");
  MURAL_REQUIRE(s->n >= 0 && s->n_class >= 1 && s->n_class <= SK_MAX_CLASS, "summary_annot_rows: n >= 0 and 1 <= n_class <= %d required",
                SK_MAX_CLASS);
  MURAL_REQUIRE(s->label_kind >= 0 && s->label_kind <= 2, "summary_annot_rows: label_kind is 0 (float32), 1 (int32) or 2 (int64)");
  MURAL_REQUIRE(s->n_pieces >= 0 && s->n_groups >= 0, "summary_annot_rows: n_pieces < 0 or n_groups < 0");
  if (s->n == 0 || s->n_pieces == 0) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->start && s->label && s->status && s->table, "summary_annot_rows: NULL argument");
  MURAL_REQUIRE(s->piece_b0 && s->piece_b1 && s->piece_group && s->n_groups >= 1, "summary_annot_rows: pieces without groups");
  MURAL_REQUIRE(s->prob_stride >= s->n_class, "summary_annot_rows: prob_stride < n_class");
  MURAL_REQUIRE(ws && ws_bytes >= mural_summary_annot_workspace_bytes(s->n, s->n_class) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                "summary_annot_rows: the workspace is NULL, misaligned or smaller than mural_summary_annot_workspace_bytes");
  AnnotArgs A{};
  A.prob = s->prob, A.start = s->start, A.label = s->label, A.prob_stride = s->prob_stride;
  A.label_kind = s->label_kind, A.n_class = s->n_class, A.n_groups = s->n_groups;
  A.b0 = s->piece_b0, A.b1 = s->piece_b1, A.group = s->piece_group;
  A.tiles = static_cast<u64*>(ws), A.table = reinterpret_cast<u64*>(s->table), A.status = s->status;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(SA_THREADS);
  const dim3 fold_grid((unsigned)(((int64_t)s->n_groups * s->n_class + SA_THREADS - 1) / SA_THREADS));
  FoldTables F{};
  F.table[0] = A.table, F.n_groups[0] = s->n_groups, F.nc = s->n_class;
  for (int64_t s0 = 0; s0 < s->n; s0 += SA_SLICE_ROWS) {
    const int64_t s1 = std::min(s0 + SA_SLICE_ROWS, s->n);
    const int64_t n_tiles = tiles_of(s1 - s0);
    const dim3 tile_grid((unsigned)((n_tiles + SA_WAVES - 1) / SA_WAVES));
    if (s->prob_f64)
      hipLaunchKernelGGL(summary_annot_tile_kernel<double>, tile_grid, block, 0, st, A, s0, s1, n_tiles);
    else
      hipLaunchKernelGGL(summary_annot_tile_kernel<float>, tile_grid, block, 0, st, A, s0, s1, n_tiles);
    MURAL_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(summary_annot_scan_kernel, dim3(3 * s->n_class), dim3(SA_SCAN_THREADS), 0, st, A, n_tiles);
    MURAL_HIP_CHECK(hipGetLastError());
    for (int64_t p0 = 0; p0 < s->n_pieces; p0 += SA_FOLD_PIECES) {
      const int64_t p1 = std::min(p0 + SA_FOLD_PIECES, s->n_pieces);
      const dim3 piece_grid((unsigned)((p1 - p0 + SA_WAVES - 1) / SA_WAVES));
      if (s->prob_f64)
        hipLaunchKernelGGL(summary_annot_piece_kernel<double>, piece_grid, block, 0, st, A, s0, s1, p0, p1);
      else
        hipLaunchKernelGGL(summary_annot_piece_kernel<float>, piece_grid, block, 0, st, A, s0, s1, p0, p1);
      MURAL_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(summary_fold_kernel<SA_THREADS>, fold_grid, block, 0, st, F);
      MURAL_HIP_CHECK(hipGetLastError());
    }
  }
  return MURAL_OK;
}
