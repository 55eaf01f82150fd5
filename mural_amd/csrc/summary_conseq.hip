// Expected and observed mutations per transcript by consequence while a prediction shard is on the device (mural_amd/summaries.py:
// SummarySink(transcripts=...); tables.consequence_table from a written table): per transcript of a BED12 file the label counts and the
// sums of the probabilities of the SNV rows inside its CDS, split by what each of a row's three substitutions does to the codon it falls
// in -- synonymous, missense, stop gained, stop lost, or unresolved (an incomplete or masked codon).  summaries.summary_conseq_host is
// the specification; DESIGN.md section 3.21.  The codon and the class-to-bin rule live in conseq_bins.h, which csrc/simulate_conseq.hip
// includes as well.
//
// The host (tables.read_transcripts) turns every transcript into its CDS SEGMENTS [b0, b1) with the CDS offset of the segment's first
// base in transcript orientation and the indices of the transcript's neighbouring segments; transcripts overlap and nest freely, so a
// per-row stabbing query is unbounded, and a row's bin depends on the transcript, so row prefix sums do not apply.  The rows of a part
// ascend in start, so the rows of a segment are ONE range [i0, i1); the work is cut per segment, as csrc/simulate.hip cuts it per piece:
//   * check kernel (summary_quant.h: snv_check_kernel), a thread per row: the status bits;
//   * the plan (row_chunks.h: plan_row_chunks): the segments' rows cut into chunks of at most SC_CHUNK_ROWS rows;
//   * reduce kernel, a grid of at most SC_GRID_WAVES waves striding over the chunks: the wave finds the chunk's segment and walks the
//     chunk 64 rows at a time, a row per lane: the row's CDS offset, its codon's three genomic positions (at most two hops over
//     seg_prev / seg_next each: exons may be 1 bp long), the two amino acids from a 64-byte table in LDS, a bin per class.  The limbs
//     (summary_quant.h: q = rne(p * 2^71) as hi, lo) add up per lane and bin over the chunk, the label counts per bin by ballot +
//     popcount; after the chunk 10 wave butterflies, the fold of lo into hi, and ONE wave-instruction of 64-bit INTEGER atomics over
//     the transcript's 15 contiguous cells + its two row counters, zero words skipped;
//   * fold kernel (summary_quant.h, with the limb bound): the table as [transcript * bin][3][1], at the end of every call.
// Terms.  A lane adds at most 3 limbs per row and SC_CHUNK_ROWS / 64 = 16 rows per chunk: X = 3 * 16 * 64 < 2^12 terms in a wave's sum
// before its fold.  A chunk then adds one folded term to a cell; the segments of one transcript are disjoint, so one call adds at most
// n / SC_CHUNK_ROWS + n_segments chunks to a cell; the entry refuses n > 2^31 or n_segments > 2^22: X <= 2^21 + 2^22 terms per call.
// No per-row bin is stored (the check and the reduce kernel both recompute a row); no floating-point atomics, no synchronisation, no
// read-back.
#include "common.h"
#include "conseq_bins.h"
#include "kmer_key.h"
#include "row_chunks.h"
#include "summary_quant.h"

namespace mural {
namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_SCAN_THREADS = 1024;
constexpr int64_t SC_CHUNK_ROWS = 1024;           // rows of one unit of the reduce kernel: 16 tiles of 64
constexpr int64_t SC_GRID_WAVES = 8192;           // waves of the reduce kernel's grid; they stride over the chunks
constexpr int64_t SC_MAX_ROWS = 1ll << 31;        // per call (the fold bound above)
constexpr int64_t SC_MAX_SEGMENTS = 1ll << 22;    // per call
constexpr int SC_CELL_WORDS = 3 * SC_BINS;        // per transcript: [bin][label count | sum of hi | sum of lo]

struct ConseqArgs {
  SnvRows snv;
  TxSegments tx;
  u64* table;
  u64* rows;
};

template <typename T>
__global__ __launch_bounds__(SC_THREADS) void summary_conseq_reduce_kernel(ConseqArgs A, const int64_t* __restrict__ row0,
                                                                           const int64_t* __restrict__ row1, const int64_t* __restrict__ pre,
                                                                           int64_t n_waves) {
  __shared__ uint32_t aa_words[16];
  const uint8_t* aa = stage_aa(A.tx, aa_words);
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * SC_WAVES + (threadIdx.x >> 6);
  const int64_t units = pre[A.tx.n_seg];
  for (int64_t unit = wave; unit < units; unit += n_waves) {
    const int64_t s = row_chunk_item(pre, A.tx.n_seg, unit);
    const int64_t r0 = row0[s] + (unit - pre[s]) * SC_CHUNK_ROWS;
    const int64_t r1 = min(r0 + SC_CHUNK_ROWS, row1[s]);
    const int64_t b0 = A.tx.seg_b0[s], b1 = A.tx.seg_b1[s], cds0 = A.tx.seg_cds0[s];
    const int32_t tx = A.tx.seg_tx[s];      // (0 <= tx < n_tx: the range kernel gave other segments no chunk)
    const bool minus = A.tx.tx_strand[tx] != 0;
    const int64_t cds_len = A.tx.tx_cds_len[tx];
    u64 acc_hi[SC_BINS], acc_lo[SC_BINS];
    uint32_t cnt[SC_BINS];
#pragma unroll
    for (int b = 0; b < SC_BINS; ++b) acc_hi[b] = 0, acc_lo[b] = 0, cnt[b] = 0;
    uint32_t n_rows = 0, n_lab0 = 0;
    for (int64_t row = r0; row < r1; row += 64) {
      const int64_t i = row + lane;
      u64 hi[3] = {0, 0, 0}, lo[3] = {0, 0, 0};
      int bins[3] = {SC_NOWHERE, SC_NOWHERE, SC_NOWHERE};
      int lab = -1;
      bool live = false;
      if (i < r1) {
        const int64_t q = A.snv.start[i];
        // (the status is the check kernel's; q lies in [b0, b1) unless the rows do not ascend: then the row is skipped here)
        live = snv_row<T>(A.snv, i, lab, hi, lo) == 0 && q >= b0 && q < b1;
        if (live) {
          conseq_row_bins(A.tx, A.snv.strand, aa, s, tx, minus, cds_len, b0, b1, cds0, i, q, bins);
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) hi[c] = 0, lo[c] = 0;
        }
      }
      const int lab_bin = lab == 1 ? bins[0] : lab == 2 ? bins[1] : lab == 3 ? bins[2] : SC_NOWHERE;
#pragma unroll
      for (int b = 0; b < SC_BINS; ++b) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          acc_hi[b] += bins[c] == b ? hi[c] : 0;
          acc_lo[b] += bins[c] == b ? lo[c] : 0;
        }
        cnt[b] += (uint32_t)__popcll(__ballot(live && lab_bin == b));
      }
      n_rows += (uint32_t)__popcll(__ballot(live));
      n_lab0 += (uint32_t)__popcll(__ballot(live && lab == 0));
    }
    u64 word = 0;      // lane 3 b + w: word w of bin b; lanes 15, 16: the row counters
#pragma unroll
    for (int b = 0; b < SC_BINS; ++b) {
      u64 l = wave_sum(acc_lo[b]), h = wave_sum(acc_hi[b]);
      fold_limbs(h, l);
      if (lane == 3 * b) word = cnt[b];
      if (lane == 3 * b + 1) word = h;
      if (lane == 3 * b + 2) word = l;
    }
    if (lane == SC_CELL_WORDS) word = n_rows;
    if (lane == SC_CELL_WORDS + 1) word = n_lab0;
    if (word) {      // (0 in the lanes from 17 on)
      if (lane < SC_CELL_WORDS) atomicAdd(&A.table[(int64_t)tx * SC_CELL_WORDS + lane], word);
      else atomicAdd(&A.rows[(int64_t)tx * 2 + (lane - SC_CELL_WORDS)], word);
    }
  }
}

}  // namespace
}  // namespace mural

using namespace mural;

extern "C" int64_t mural_summary_conseq_chunk_rows(void) { return SC_CHUNK_ROWS; }
extern "C" int64_t mural_summary_conseq_grid_waves(void) { return SC_GRID_WAVES; }
extern "C" int32_t mural_summary_conseq_scan_threads(void) { return SC_SCAN_THREADS; }

extern "C" size_t mural_summary_conseq_workspace_bytes(int64_t n_segments) {
  return row_chunks_bytes(n_segments);
}

extern "C" int mural_summary_conseq_rows(const MuralSummaryConseqRows* s, void* ws_ptr, size_t ws_bytes, void* stream) {
  MURAL_REQUIRE(s, "summary_conseq_rows: NULL argument");
  MURAL_REQUIRE(s->n_class == 4, "summary_conseq_rows: SNV rows of 4 classes required (n_class = %d)", s->n_class);
  MURAL_REQUIRE(s->n >= 0 && s->n <= SC_MAX_ROWS, "summary_conseq_rows: 0 <= n <= 2^31 required");
  MURAL_REQUIRE(s->n_segments >= 0 && s->n_segments <= SC_MAX_SEGMENTS, "summary_conseq_rows: 0 <= n_segments <= 2^22 required");
  MURAL_REQUIRE(s->n_transcripts >= 0, "summary_conseq_rows: n_transcripts < 0");
  MURAL_REQUIRE(s->label_kind >= 0 && s->label_kind <= 2, "summary_conseq_rows: label_kind is 0 (float32), 1 (int32) or 2 (int64)");
  ConseqArgs A{};
  const bool live = s->n > 0 && s->n_segments > 0;
  if (const int rc = fill_tx_segments("summary_conseq_rows", s, live, A.tx)) return rc;
  if (!live) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->start && s->label && s->status && s->table && s->rows, "summary_conseq_rows: NULL argument");
  MURAL_REQUIRE(s->seg_b0 && s->seg_b1 && s->seg_cds0 && s->seg_tx && s->seg_prev && s->seg_next && s->tx_strand && s->tx_cds_len &&
                    s->n_transcripts >= 1,
                "summary_conseq_rows: segments without transcripts");
  MURAL_REQUIRE(s->prob_stride >= 4, "summary_conseq_rows: prob_stride < n_class");
  if (const int rc = check_workspace("summary_conseq_rows", "mural_summary_conseq_workspace_bytes", ws_ptr, ws_bytes,
                                     mural_summary_conseq_workspace_bytes(s->n_segments)))
    return rc;
  A.snv = snv_rows(s);
  A.table = reinterpret_cast<u64*>(s->table), A.rows = reinterpret_cast<u64*>(s->rows);
  const hipStream_t st = (hipStream_t)stream;
  if (const int rc = launch_snv_check<SC_THREADS>(st, A.snv, s->prob_f64)) return rc;
  WsArena ws(ws_ptr);
  RowChunks w;
  if (const int rc = plan_row_chunks<SC_THREADS, SC_SCAN_THREADS>(st, s->start, s->n, s->seg_b0, s->seg_b1, s->seg_tx, s->n_transcripts,
                                                                  s->n_segments, 0, SC_CHUNK_ROWS, ws, w))
    return rc;
  const int64_t n_waves = row_chunk_grid_waves(s->n, SC_CHUNK_ROWS, 1, s->n_segments, SC_GRID_WAVES, SC_WAVES);
  const dim3 reduce_grid((unsigned)(n_waves / SC_WAVES)), block(SC_THREADS);
  if (s->prob_f64)
    hipLaunchKernelGGL(summary_conseq_reduce_kernel<double>, reduce_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  else
    hipLaunchKernelGGL(summary_conseq_reduce_kernel<float>, reduce_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  MURAL_HIP_CHECK(hipGetLastError());
  return launch_cell_fold<SC_THREADS>(st, A.table, (int64_t)s->n_transcripts * SC_BINS);
}
