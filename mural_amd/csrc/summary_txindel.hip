// Expected and observed INDEL events per transcript by what they do to the transcript's STRUCTURE while a prediction shard is on the
// device (mural_amd/summaries.py: SummarySink(indel_transcripts=...); tables.indel_structure_table from a written table): per transcript
// of a BED12 file the label counts and the sums of the probabilities of the INDEL rows whose home base lies inside [chromStart,
// chromEnd), split into utr5, utr3, noncoding_exon, splice, splice_utr, intron, start_lost, frameshift, inframe and cds_mixed.
// summaries.summary_txindel_host is the specification; DESIGN.md section 3.25.  No genome is read: nothing here depends on sequence.
// The bin rule itself -- an item as a transcript sees it, an insertion's site, the bin of a class with the deletion's walk -- lives in
// txindel_bins.h, which csrc/simulate_txindel.hip shares.
//
// The items are those of csrc/summary_txstruct.hip (tables.read_transcript_structure) with two link arrays, feat_prev / feat_next, the
// same transcript's neighbouring items in genomic order (tables.structure_links).  The stages are those of csrc/summary_txstruct.hip:
//   * check kernel, a thread per row: the status bits;
//   * the plan (row_chunks.h: plan_row_chunks with a shift): an item's rows are those whose HOME BASE -- start + breakpoint_offset - 1
//     for an insertion and a deletion end, start + breakpoint_offset for a deletion start -- lies in it, cut into chunks of at most
//     TI_CHUNK_ROWS rows;
//   * reduce kernel, a grid of at most TI_GRID_WAVES waves striding over the chunks, a row per lane.  An insertion looks at the home
//     item and, on its last boundary, at the item behind it (wave-uniform: loaded once per chunk).  A deletion of class c removes L =
//     lo(c) <= 64 bases: the lane walks from the home item over feat_next (deletion start) or feat_prev (deletion end) while the items
//     meet the deleted bases, one O(1) overlap per item; a link that is out of range, names another transcript or does not abut ends
//     the walk, so every step moves on by at least one base and a walk has at most 64 steps.  A lane carries 10 bins x (hi | count <<
//     48, lo); after the chunk 20 wave butterflies, the fold of lo into hi, and ONE wave-instruction of 64-bit INTEGER atomics over the
//     transcript's 30 contiguous cells + its two row counters, zero words skipped;
//   * fold kernel (summary_quant.h, with the limb bound): the table as [transcript * bin][3][1], at the end of every call.
// Terms.  A lane adds at most n_class - 1 <= 15 limbs per row and TI_CHUNK_ROWS / 64 = 16 rows per chunk: 240 terms per lane (lo < 2^48,
// hi < 2^39, count < 2^8 above bit 48) and 64 * 240 < 2^14 terms in a wave's sum before its fold (lo < 2^54, hi < 2^45, count < 2^14).
// A chunk then adds one folded term to a cell; the items of one transcript are disjoint and a row has one home item per transcript,
// so one call adds at most n / TI_CHUNK_ROWS + n_features chunks to a cell; the entry refuses n > 2^31 or n_features > 2^22: X <= 2^21
// + 2^22 terms per call.  No per-row bin is stored; no floating-point atomics, no synchronisation, no read-back.
#include "common.h"
#include "kmer_key.h"
#include "row_chunks.h"
#include "summary_quant.h"
#include "txindel_bins.h"

namespace mural {
namespace {

constexpr int TI_THREADS = 256;
constexpr int TI_WAVES = TI_THREADS / 64;
constexpr int TI_SCAN_THREADS = 1024;
constexpr int64_t TI_CHUNK_ROWS = 1024;           // rows of one unit of the reduce kernel: 16 tiles of 64
constexpr int64_t TI_GRID_WAVES = 8192;           // waves of the reduce kernel's grid; they stride over the chunks
constexpr int64_t TI_MAX_ROWS = 1ll << 31;        // per call (the fold bound above)
constexpr int64_t TI_MAX_FEATURES = 1ll << 22;    // per call
constexpr int TI_MAX_CLASS = 16;
constexpr int TI_CELL_WORDS = 3 * TI_BINS;        // per transcript: [bin][label count | sum of hi | sum of lo]
constexpr int TI_COUNT_SHIFT = 48;                // a lane's label count rides above its sum of hi limbs

struct TxindelArgs {
  const void* prob;
  const int64_t* start;
  const void* label;
  int64_t prob_stride, n, chrom_len;      // chrom_len < 0: not known, a deletion is clipped to the span alone
  int32_t label_kind, n_tx, n_class, kind, off;
  const int64_t* seg_b0;
  const int64_t* seg_b1;
  const int64_t* seg_cds0;
  const int32_t* seg_tx;
  int64_t n_seg;
  const int64_t* feat_b0;
  const int64_t* feat_b1;
  const int32_t* feat_tx;
  const uint8_t* feat_kind;
  const int32_t* feat_seg;
  const int32_t* feat_prev;
  const int32_t* feat_next;
  int64_t n_feat;
  const uint8_t* tx_strand;
  const int64_t* tx_cds_len;
  uint32_t cls[TI_MAX_CLASS];      // class c: lo | frame mode << 8
  u64* table;
  u64* rows;
  int32_t* status;
};

// 0 <= p <= 1, summary_quant.h's test (quantise_prob returns it): on the bit pattern, so that NaN is caught whatever the compiler assumes
__device__ __forceinline__ bool txindel_prob_ok(double p) {
  const u64 bits = (u64)__double_as_longlong(p);
  return !(bits > 0x3FF0000000000000ull && bits != 0x8000000000000000ull);
}

// The checks of row i (status bits, 0 if it counts); class 0's probability is not read.  Nothing is quantised here: the reduce kernel
// quantises a class once, where it adds it.
template <typename T>
__device__ __forceinline__ int32_t txindel_row(const TxindelArgs& A, int64_t i, int& lab) {
  const T* __restrict__ p_row = static_cast<const T*>(A.prob) + i * A.prob_stride;
  lab = load_label(A.label, A.label_kind, i);
  int32_t bad = 0;
  if (A.start[i] < 0) bad |= SM_BAD_START;
  if (lab < 0 || lab >= A.n_class) bad |= SM_BAD_LABEL;
  for (int c = 1; c < A.n_class; ++c)
    if (!txindel_prob_ok((double)p_row[c])) bad |= SM_BAD_PROB;      // (float -> double is exact)
  return bad;
}

template <typename T>
__global__ __launch_bounds__(TI_THREADS) void summary_txindel_check_kernel(TxindelArgs A) {
  const int64_t i = (int64_t)blockIdx.x * TI_THREADS + threadIdx.x;
  int32_t bad = 0;
  if (i < A.n) {
    int lab;
    bad = txindel_row<T>(A, i, lab);
    if (i > 0 && A.start[i] < A.start[i - 1]) bad |= SM_BAD_ORDER;
  }
  if (bad) atomicOr(A.status, bad);
}

template <typename T>
__global__ __launch_bounds__(TI_THREADS) void summary_txindel_reduce_kernel(TxindelArgs A, const int64_t* __restrict__ row0,
                                                                            const int64_t* __restrict__ row1,
                                                                            const int64_t* __restrict__ pre, int64_t n_waves) {
  __shared__ uint32_t cls_words[TI_MAX_CLASS];
#pragma unroll
  for (int j = 0; j < TI_MAX_CLASS; ++j)      // (constant indices: the words stay scalar arguments)
    if (threadIdx.x == j) cls_words[j] = A.cls[j];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * TI_WAVES + (threadIdx.x >> 6);
  const int64_t units = pre[A.n_feat];
  const int64_t home_shift = A.off - (A.kind == TI_DELETION_START ? 0 : 1);
  for (int64_t unit = wave; unit < units; unit += n_waves) {
    const int64_t f = row_chunk_item(pre, A.n_feat, unit);
    const int64_t r0 = row0[f] + (unit - pre[f]) * TI_CHUNK_ROWS;
    const int64_t r1 = min(r0 + TI_CHUNK_ROWS, row1[f]);
    const int32_t tx = A.feat_tx[f];      // (0 <= tx < n_tx: the range kernel gave other items no chunk)
    const TiItem home = txindel_item(A, f, tx);
    if (!home.ok) continue;      // (an item of an unknown kind or a CDS part without its segment: skipped)
    const bool minus = A.tx_strand[tx] != 0;
    const int64_t cds_len = A.tx_cds_len[tx];
    TiItem behind{0, 0, 0, 0, false};      // an insertion on the home item's last boundary: the item of base j
    if (A.kind == TI_INSERTION) {
      behind = txindel_item(A, A.feat_next[f], tx);
      behind.ok = behind.ok && behind.b0 == home.b1;
    }
    u64 acc_hi[TI_BINS], acc_lo[TI_BINS];
#pragma unroll
    for (int b = 0; b < TI_BINS; ++b) acc_hi[b] = 0, acc_lo[b] = 0;
    uint32_t n_rows = 0, n_lab0 = 0;
    for (int64_t row = r0; row < r1; row += 64) {
      const int64_t i = row + lane;
      int lab = -1;
      bool live = false;
      int64_t j = 0;
      if (i < r1) {
        j = A.start[i] + A.off;
        const int64_t h = A.start[i] + home_shift;
        // (the status is the check kernel's; h lies in the item unless the rows do not ascend: then the row is skipped here)
        live = txindel_row<T>(A, i, lab) == 0 && h >= home.b0 && h < home.b1;
      }
      int site = 5;      // an insertion's bin, or TI_FRAME
      if (A.kind == TI_INSERTION) site = txindel_insertion_site(home, behind, minus, cds_len, j, live);
      const T* __restrict__ p_row = static_cast<const T*>(A.prob) + i * A.prob_stride;      // (read in live lanes only)
      for (int c = 1; c < A.n_class; ++c) {
        const uint32_t w = cls_words[c];
        u64 hi = 0, lo = 0;
        int bin = TI_BINS;      // not counted
        if (live) {
          quantise_prob((double)p_row[c], hi, lo);
          bin = txindel_class_bin(A, f, tx, home, minus, site, j, w);
          hi |= (u64)(lab == c) << TI_COUNT_SHIFT;
        }
#pragma unroll
        for (int b = 0; b < TI_BINS; ++b) {
          acc_hi[b] += bin == b ? hi : 0;
          acc_lo[b] += bin == b ? lo : 0;
        }
      }
      n_rows += (uint32_t)__popcll(__ballot(live));
      n_lab0 += (uint32_t)__popcll(__ballot(live && lab == 0));
    }
    u64 word = 0;      // lane 3 b + w: word w of bin b; lanes 30, 31: the row counters
    const int my_bin = lane / 3, my_word = lane - 3 * my_bin;
#pragma unroll
    for (int b = 0; b < TI_BINS; ++b) {
      u64 l = wave_sum(acc_lo[b]), h = wave_sum(acc_hi[b]);
      const u64 cnt = h >> TI_COUNT_SHIFT;
      h &= (1ull << TI_COUNT_SHIFT) - 1;
      fold_limbs(h, l);
      if (my_bin == b) word = my_word == 0 ? cnt : my_word == 1 ? h : l;
    }
    if (lane == TI_CELL_WORDS) word = n_rows;
    if (lane == TI_CELL_WORDS + 1) word = n_lab0;
    if (word) {      // (0 in the lanes from 32 on)
      if (lane < TI_CELL_WORDS) atomicAdd(&A.table[(int64_t)tx * TI_CELL_WORDS + lane], word);
      else atomicAdd(&A.rows[(int64_t)tx * 2 + (lane - TI_CELL_WORDS)], word);
    }
  }
}

}  // namespace
}  // namespace mural

using namespace mural;

extern "C" int64_t mural_summary_txindel_chunk_rows(void) { return TI_CHUNK_ROWS; }
extern "C" int64_t mural_summary_txindel_grid_waves(void) { return TI_GRID_WAVES; }
extern "C" int32_t mural_summary_txindel_scan_threads(void) { return TI_SCAN_THREADS; }

extern "C" size_t mural_summary_txindel_workspace_bytes(int64_t n_features) {
  return row_chunks_bytes(n_features);
}

extern "C" int mural_summary_txindel_rows(const MuralSummaryTxindelRows* s, void* ws_ptr, size_t ws_bytes, void* stream) {
  MURAL_REQUIRE(s, "summary_txindel_rows: NULL argument");
  MURAL_REQUIRE(s->n_class >= 2 && s->n_class <= TI_MAX_CLASS, "summary_txindel_rows: 2 <= n_class <= 16 required (n_class = %d)", s->n_class);
  MURAL_REQUIRE(s->kind >= 0 && s->kind <= 2, "summary_txindel_rows: kind is 0 (insertion), 1 (deletion start) or 2 (deletion end)");
  MURAL_REQUIRE(s->breakpoint_offset == 0 || s->breakpoint_offset == 1, "summary_txindel_rows: breakpoint_offset is 0 or 1");
  MURAL_REQUIRE(s->n >= 0 && s->n <= TI_MAX_ROWS, "summary_txindel_rows: 0 <= n <= 2^31 required");
  MURAL_REQUIRE(s->n_features >= 0 && s->n_features <= TI_MAX_FEATURES, "summary_txindel_rows: 0 <= n_features <= 2^22 required");
  MURAL_REQUIRE(s->n_segments >= 0, "summary_txindel_rows: n_segments < 0");
  MURAL_REQUIRE(s->n_transcripts >= 0, "summary_txindel_rows: n_transcripts < 0");
  MURAL_REQUIRE(s->label_kind >= 0 && s->label_kind <= 2, "summary_txindel_rows: label_kind is 0 (float32), 1 (int32) or 2 (int64)");
  for (int c = 1; c < s->n_class; ++c)
    MURAL_REQUIRE(1 <= s->class_len[c][0] && s->class_len[c][0] <= s->class_len[c][1] && s->class_len[c][1] <= TI_MAX_LEN,
                  "summary_txindel_rows: class_len[%d] must be 1 <= lo <= hi <= 64", c);
  if (s->n == 0 || s->n_features == 0) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->start && s->label && s->status && s->table && s->rows, "summary_txindel_rows: NULL argument");
  MURAL_REQUIRE(s->feat_b0 && s->feat_b1 && s->feat_tx && s->feat_kind && s->feat_seg && s->feat_prev && s->feat_next && s->tx_strand &&
                    s->tx_cds_len && s->n_transcripts >= 1,
                "summary_txindel_rows: items without links or transcripts");
  MURAL_REQUIRE(s->n_segments == 0 || (s->seg_b0 && s->seg_b1 && s->seg_cds0 && s->seg_tx),
                "summary_txindel_rows: n_segments without the segment arrays");
  MURAL_REQUIRE(s->prob_stride >= s->n_class, "summary_txindel_rows: prob_stride < n_class");
  if (const int rc = check_workspace("summary_txindel_rows", "mural_summary_txindel_workspace_bytes", ws_ptr, ws_bytes,
                                     mural_summary_txindel_workspace_bytes(s->n_features)))
    return rc;
  TxindelArgs A{};
  A.prob = s->prob, A.start = s->start, A.label = s->label, A.prob_stride = s->prob_stride, A.n = s->n, A.chrom_len = s->chrom_length;
  A.label_kind = s->label_kind, A.n_tx = s->n_transcripts, A.n_class = s->n_class, A.kind = s->kind, A.off = s->breakpoint_offset;
  A.seg_b0 = s->seg_b0, A.seg_b1 = s->seg_b1, A.seg_cds0 = s->seg_cds0, A.seg_tx = s->seg_tx, A.n_seg = s->n_segments;
  A.feat_b0 = s->feat_b0, A.feat_b1 = s->feat_b1, A.feat_tx = s->feat_tx, A.feat_kind = s->feat_kind, A.feat_seg = s->feat_seg;
  A.feat_prev = s->feat_prev, A.feat_next = s->feat_next, A.n_feat = s->n_features;
  A.tx_strand = s->tx_strand, A.tx_cds_len = s->tx_cds_len;
  for (int c = 1; c < s->n_class; ++c) {
    A.cls[c] = txindel_class_word(s->class_len[c][0], s->class_len[c][1]);
  }
  A.table = reinterpret_cast<u64*>(s->table), A.rows = reinterpret_cast<u64*>(s->rows), A.status = s->status;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(TI_THREADS);
  const dim3 row_grid((unsigned)((s->n + TI_THREADS - 1) / TI_THREADS));
  if (s->prob_f64)
    hipLaunchKernelGGL(summary_txindel_check_kernel<double>, row_grid, block, 0, st, A);
  else
    hipLaunchKernelGGL(summary_txindel_check_kernel<float>, row_grid, block, 0, st, A);
  MURAL_HIP_CHECK(hipGetLastError());
  WsArena ws(ws_ptr);
  RowChunks w;
  const int64_t home_shift = A.off - (A.kind == TI_DELETION_START ? 0 : 1);
  if (const int rc = plan_row_chunks<TI_THREADS, TI_SCAN_THREADS>(st, A.start, A.n, A.feat_b0, A.feat_b1, A.feat_tx, A.n_tx, A.n_feat,
                                                                  home_shift, TI_CHUNK_ROWS, ws, w))
    return rc;
  const int64_t n_waves = row_chunk_grid_waves(s->n, TI_CHUNK_ROWS, 1, s->n_features, TI_GRID_WAVES, TI_WAVES);
  const dim3 reduce_grid((unsigned)(n_waves / TI_WAVES));
  if (s->prob_f64)
    hipLaunchKernelGGL(summary_txindel_reduce_kernel<double>, reduce_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  else
    hipLaunchKernelGGL(summary_txindel_reduce_kernel<float>, reduce_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  MURAL_HIP_CHECK(hipGetLastError());
  return launch_cell_fold<TI_THREADS>(st, A.table, (int64_t)s->n_transcripts * TI_BINS);
}
