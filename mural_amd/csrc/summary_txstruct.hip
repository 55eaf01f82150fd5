// Expected and observed mutations per transcript by where a row lies in the transcript's STRUCTURE while a prediction shard is on the
// device (mural_amd/summaries.py: SummarySink(transcripts=..., transcript_structure=True); tables.structure_table from a written
// table): per transcript of a BED12 file the label counts and the sums of the probabilities of the SNV rows inside [chromStart,
// chromEnd), split into 5'UTR, 3'UTR, non-coding exon, splice donor, splice acceptor, splice site of a non-coding intron, intron, start
// lost and (other) CDS.  summaries.summary_txstruct_host is the specification; DESIGN.md section 3.23.  The codon and the class-to-bin
// rule of the CDS are conseq_bins.h's: a class is `start lost` where its CDS offset is below 3 and that rule files it as missense, stop
// gained or stop lost.
//
// The host (tables.read_transcript_structure) turns every transcript into ITEMS that tile its span: its blocks cut at thickStart /
// thickEnd and the gaps between them, each with a kind; a CDS item names its CDS segment of tables.read_transcripts.  The stages are
// those of csrc/summary_conseq.hip with the items in the place of the segments:
//   * check kernel (summary_quant.h: snv_check_kernel), a thread per row: the status bits;
//   * the plan (row_chunks.h: plan_row_chunks): the items' rows cut into chunks of at most TS_CHUNK_ROWS rows;
//   * reduce kernel, a grid of at most TS_GRID_WAVES waves striding over the chunks: the wave finds the chunk's item and walks the chunk
//     64 rows at a time, a row per lane.  The rows of one item fall in at most three bins (an intron: donor, acceptor, rest; a CDS part:
//     start lost, cds; every other kind: one), so a lane carries three (hi, lo) SLOTS, mapped to bins by the item's kind at the atomics.
//     Only a CDS item that holds CDS offsets 0 .. 2 reads the genome (conseq_codon), and only in its lanes at those offsets: the branch
//     on the item is wave-uniform, UTR and intron chunks load no base.  After the chunk 6 wave butterflies, the fold of lo into hi, and
//     ONE wave-instruction of 64-bit INTEGER atomics over the transcript's 27 contiguous cells + its two row counters, zero words
//     skipped;
//   * fold kernel (summary_quant.h, with the limb bound): the table as [transcript * bin][3][1], at the end of every call.
// Terms.  A lane adds at most 3 limbs per row and TS_CHUNK_ROWS / 64 = 16 rows per chunk: X = 3 * 16 * 64 < 2^12 terms in a wave's sum
// before its fold.  A chunk then adds one folded term to a cell; the items of one transcript are disjoint, so one call adds at most
// n / TS_CHUNK_ROWS + n_features chunks to a cell; the entry refuses n > 2^31 or n_features > 2^22: X <= 2^21 + 2^22 terms per call.
// No per-row bin is stored (the check and the reduce kernel both recompute a row); no floating-point atomics, no synchronisation, no
// read-back.
#include "common.h"
#include "conseq_bins.h"
#include "kmer_key.h"
#include "row_chunks.h"
#include "summary_quant.h"

namespace mural {
namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_WAVES = TS_THREADS / 64;
constexpr int TS_SCAN_THREADS = 1024;
constexpr int64_t TS_CHUNK_ROWS = 1024;           // rows of one unit of the reduce kernel: 16 tiles of 64
constexpr int64_t TS_GRID_WAVES = 8192;           // waves of the reduce kernel's grid; they stride over the chunks
constexpr int64_t TS_MAX_ROWS = 1ll << 31;        // per call (the fold bound above)
constexpr int64_t TS_MAX_FEATURES = 1ll << 22;    // per call
constexpr int TS_BINS = 9;                        // utr5, utr3, noncoding_exon, splice_donor, splice_acceptor, splice_utr, intron, start_lost, cds
constexpr int TS_CELL_WORDS = 3 * TS_BINS;        // per transcript: [bin][label count | sum of hi | sum of lo]
constexpr int TS_SLOTS = 3;                       // the bins one item's rows can fall in
constexpr int TS_KIND_CODING_INTRON = 3, TS_KIND_INTRON = 4, TS_KIND_CDS = 5;

struct TxstructArgs {
  SnvRows snv;
  TxSegments tx;
  const int64_t* feat_b0;
  const int64_t* feat_b1;
  const int32_t* feat_tx;
  const uint8_t* feat_kind;
  const int32_t* feat_seg;
  int64_t n_feat;
  u64* table;
  u64* rows;
};

template <typename T>
__global__ __launch_bounds__(TS_THREADS) void summary_txstruct_reduce_kernel(TxstructArgs A, const int64_t* __restrict__ row0,
                                                                             const int64_t* __restrict__ row1,
                                                                             const int64_t* __restrict__ pre, int64_t n_waves) {
  __shared__ uint32_t aa_words[16];
  const uint8_t* aa = stage_aa(A.tx, aa_words);
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * TS_WAVES + (threadIdx.x >> 6);
  const int64_t units = pre[A.n_feat];
  for (int64_t unit = wave; unit < units; unit += n_waves) {
    const int64_t f = row_chunk_item(pre, A.n_feat, unit);
    const int64_t r0 = row0[f] + (unit - pre[f]) * TS_CHUNK_ROWS;
    const int64_t r1 = min(r0 + TS_CHUNK_ROWS, row1[f]);
    const int64_t b0 = A.feat_b0[f], b1 = A.feat_b1[f];
    const int32_t tx = A.feat_tx[f];      // (0 <= tx < n_tx: the range kernel gave other items no chunk)
    const int kind = A.feat_kind[f];
    const bool minus = A.tx.tx_strand[tx] != 0;
    // the bins of the item's slots; -1: the slot is not used
    int slot_bin[TS_SLOTS] = {-1, -1, -1};
    int64_t seg = 0, cds0 = 0, cds_len = 0;
    if (kind < TS_KIND_CODING_INTRON) {
      slot_bin[0] = kind;
    } else if (kind == TS_KIND_CODING_INTRON) {
      slot_bin[0] = 3, slot_bin[1] = 4, slot_bin[2] = 6;
    } else if (kind == TS_KIND_INTRON) {
      slot_bin[0] = 5, slot_bin[2] = 6;
    } else if (kind == TS_KIND_CDS) {
      seg = A.feat_seg[f];
      if (seg < 0 || seg >= A.tx.n_seg) continue;      // (a CDS item without its segment: skipped, as an item without its transcript)
      if (A.tx.seg_b0[seg] != b0 || A.tx.seg_b1[seg] != b1 || A.tx.seg_tx[seg] != tx) continue;
      cds0 = A.tx.seg_cds0[seg], cds_len = A.tx.tx_cds_len[tx];
      slot_bin[0] = 7, slot_bin[1] = 8;
    } else {
      continue;      // (an unknown kind)
    }
    const bool has_sites = kind != TS_KIND_CDS && b1 - b0 >= 4;
    const bool has_start = kind == TS_KIND_CDS && cds0 < 3;      // the item holds a base of CDS codon 0
    u64 acc_hi[TS_SLOTS], acc_lo[TS_SLOTS];
    uint32_t cnt[TS_SLOTS];
#pragma unroll
    for (int s = 0; s < TS_SLOTS; ++s) acc_hi[s] = 0, acc_lo[s] = 0, cnt[s] = 0;
    uint32_t n_rows = 0, n_lab0 = 0;
    for (int64_t row = r0; row < r1; row += 64) {
      const int64_t i = row + lane;
      u64 hi[3] = {0, 0, 0}, lo[3] = {0, 0, 0};
      int slots[3] = {TS_SLOTS, TS_SLOTS, TS_SLOTS};      // the slot of classes 1 .. 3; TS_SLOTS: not counted
      int lab = -1;
      bool live = false;
      int64_t q = b0;
      if (i < r1) {
        q = A.snv.start[i];
        // (the status is the check kernel's; q lies in [b0, b1) unless the rows do not ascend: then the row is skipped here)
        live = snv_row<T>(A.snv, i, lab, hi, lo) == 0 && q >= b0 && q < b1;
        if (live) {
          int slot = 0;
          if (kind == TS_KIND_CDS) {
            slot = 1;
          } else if (kind >= TS_KIND_CODING_INTRON) {
            const bool low = has_sites && q < b0 + 2, high = has_sites && q >= b1 - 2;
            const bool donor = minus ? high : low, acceptor = minus ? low : high;
            slot = kind == TS_KIND_CODING_INTRON ? (donor ? 0 : acceptor ? 1 : 2) : ((donor || acceptor) ? 0 : 2);
          }
          slots[0] = slots[1] = slots[2] = slot;
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) hi[c] = 0, lo[c] = 0;
        }
      }
      if (has_start) {      // wave-uniform: the other items read no base
        const int64_t x = cds0 + (minus ? b1 - 1 - q : q - b0);
        if (live && x < 3) {
          int bins[3];
          conseq_row_bins(A.tx, A.snv.strand, aa, seg, tx, minus, cds_len, b0, b1, cds0, i, q, bins);
#pragma unroll
          for (int c = 0; c < 3; ++c) slots[c] = (bins[c] >= 1 && bins[c] <= 3) ? 0 : 1;      // aa_alt != aa_ref on a resolved codon
        }
      }
      const int lab_slot = lab == 1 ? slots[0] : lab == 2 ? slots[1] : lab == 3 ? slots[2] : TS_SLOTS;
#pragma unroll
      for (int s = 0; s < TS_SLOTS; ++s) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          acc_hi[s] += slots[c] == s ? hi[c] : 0;
          acc_lo[s] += slots[c] == s ? lo[c] : 0;
        }
        cnt[s] += (uint32_t)__popcll(__ballot(live && lab_slot == s));
      }
      n_rows += (uint32_t)__popcll(__ballot(live));
      n_lab0 += (uint32_t)__popcll(__ballot(live && lab == 0));
    }
    u64 word = 0;      // lane 3 b + w: word w of bin b; lanes 27, 28: the row counters
    const int my_bin = lane / 3, my_word = lane - 3 * my_bin;
#pragma unroll
    for (int s = 0; s < TS_SLOTS; ++s) {
      u64 l = wave_sum(acc_lo[s]), h = wave_sum(acc_hi[s]);
      fold_limbs(h, l);
      if (my_bin == slot_bin[s]) word = my_word == 0 ? (u64)cnt[s] : my_word == 1 ? h : l;
    }
    if (lane == TS_CELL_WORDS) word = n_rows;
    if (lane == TS_CELL_WORDS + 1) word = n_lab0;
    if (word) {      // (0 in the lanes from 29 on)
      if (lane < TS_CELL_WORDS) atomicAdd(&A.table[(int64_t)tx * TS_CELL_WORDS + lane], word);
      else atomicAdd(&A.rows[(int64_t)tx * 2 + (lane - TS_CELL_WORDS)], word);
    }
  }
}

}  // namespace
}  // namespace mural

using namespace mural;

extern "C" int64_t mural_summary_txstruct_chunk_rows(void) { return TS_CHUNK_ROWS; }
extern "C" int64_t mural_summary_txstruct_grid_waves(void) { return TS_GRID_WAVES; }
extern "C" int32_t mural_summary_txstruct_scan_threads(void) { return TS_SCAN_THREADS; }

extern "C" size_t mural_summary_txstruct_workspace_bytes(int64_t n_features) {
  return row_chunks_bytes(n_features);
}

extern "C" int mural_summary_txstruct_rows(const MuralSummaryTxstructRows* s, void* ws_ptr, size_t ws_bytes, void* stream) {
  MURAL_REQUIRE(s, "summary_txstruct_rows: NULL argument");
  MURAL_REQUIRE(s->n_class == 4, "summary_txstruct_rows: SNV rows of 4 classes required (n_class = %d)", s->n_class);
  MURAL_REQUIRE(s->n >= 0 && s->n <= TS_MAX_ROWS, "summary_txstruct_rows: 0 <= n <= 2^31 required");
  MURAL_REQUIRE(s->n_features >= 0 && s->n_features <= TS_MAX_FEATURES, "summary_txstruct_rows: 0 <= n_features <= 2^22 required");
  MURAL_REQUIRE(s->n_segments >= 0, "summary_txstruct_rows: n_segments < 0");
  MURAL_REQUIRE(s->n_transcripts >= 0, "summary_txstruct_rows: n_transcripts < 0");
  MURAL_REQUIRE(s->label_kind >= 0 && s->label_kind <= 2, "summary_txstruct_rows: label_kind is 0 (float32), 1 (int32) or 2 (int64)");
  TxstructArgs A{};
  const bool live = s->n > 0 && s->n_features > 0;
  if (const int rc = fill_tx_segments("summary_txstruct_rows", s, live, A.tx)) return rc;
  if (!live) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->start && s->label && s->status && s->table && s->rows, "summary_txstruct_rows: NULL argument");
  MURAL_REQUIRE(s->feat_b0 && s->feat_b1 && s->feat_tx && s->feat_kind && s->feat_seg && s->tx_strand && s->tx_cds_len &&
                    s->n_transcripts >= 1,
                "summary_txstruct_rows: items without transcripts");
  MURAL_REQUIRE(s->n_segments == 0 || (s->seg_b0 && s->seg_b1 && s->seg_cds0 && s->seg_tx && s->seg_prev && s->seg_next),
                "summary_txstruct_rows: n_segments without the segment arrays");
  MURAL_REQUIRE(s->prob_stride >= 4, "summary_txstruct_rows: prob_stride < n_class");
  if (const int rc = check_workspace("summary_txstruct_rows", "mural_summary_txstruct_workspace_bytes", ws_ptr, ws_bytes,
                                     mural_summary_txstruct_workspace_bytes(s->n_features)))
    return rc;
  A.snv = snv_rows(s);
  A.feat_b0 = s->feat_b0, A.feat_b1 = s->feat_b1, A.feat_tx = s->feat_tx, A.feat_kind = s->feat_kind, A.feat_seg = s->feat_seg;
  A.n_feat = s->n_features;
  A.table = reinterpret_cast<u64*>(s->table), A.rows = reinterpret_cast<u64*>(s->rows);
  const hipStream_t st = (hipStream_t)stream;
  if (const int rc = launch_snv_check<TS_THREADS>(st, A.snv, s->prob_f64)) return rc;
  WsArena ws(ws_ptr);
  RowChunks w;
  if (const int rc = plan_row_chunks<TS_THREADS, TS_SCAN_THREADS>(st, s->start, s->n, s->feat_b0, s->feat_b1, s->feat_tx, s->n_transcripts,
                                                                  s->n_features, 0, TS_CHUNK_ROWS, ws, w))
    return rc;
  const int64_t n_waves = row_chunk_grid_waves(s->n, TS_CHUNK_ROWS, 1, s->n_features, TS_GRID_WAVES, TS_WAVES);
  const dim3 reduce_grid((unsigned)(n_waves / TS_WAVES)), block(TS_THREADS);
  if (s->prob_f64)
    hipLaunchKernelGGL(summary_txstruct_reduce_kernel<double>, reduce_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  else
    hipLaunchKernelGGL(summary_txstruct_reduce_kernel<float>, reduce_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  MURAL_HIP_CHECK(hipGetLastError());
  return launch_cell_fold<TS_THREADS>(st, A.table, (int64_t)s->n_transcripts * TS_BINS);
}
