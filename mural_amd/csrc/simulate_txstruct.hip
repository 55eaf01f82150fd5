// The simulated null of the structure table while a prediction shard is on the device (mural_amd/summaries.py:
// SummarySink(simulate=R, transcripts=..., transcript_structure=True, simulate_transcripts=True, simulate_structure=True);
// tables.simulate_structure_table from a written table): per transcript of a BED12 file, structure bin and replicate, the SNV rows inside
// [chromStart, chromEnd) whose replicate-r draw is a class c >= 1 that falls in that bin.  The draw is csrc/simulate.hip's
// (simulate_draw.h: Philox key and counter, cum, ties), the items and their bins csrc/summary_txstruct.hip's (kinds, splice sites by
// transcript orientation, start lost through conseq_bins.h); summaries.simulate_txstruct_host is the specification; DESIGN.md section 3.24.
//
// Per call: the check kernel, the plan of the items' rows and the draw kernel, which is simulate_draw.h's draw_count_units() (the
// units, the two walks of a chunk, the counts and their atomics) around this file's policy: items = the parts that tile a transcript's
// span, owners = transcripts.  The rows of one item fall in at most three bins (an intron: donor, acceptor, rest; a CDS part: start lost,
// cds; every other kind: one), so a row's word holds three SLOTS, one per class, two bits each, and "nowhere" after them; there is an
// accumulator per slot, and the item's kind maps the slots to the bins of table[(tx * 9 + b) * n_rep + r].  Only a CDS item that holds
// CDS offsets 0 .. 2 reads the genome (conseq_row_bins), and only in its lanes at those offsets: the branch on the item is
// wave-uniform, UTR and intron chunks load no base.
#include "common.h"
#include "conseq_bins.h"
#include "kmer_key.h"
#include "row_chunks.h"
#include "simulate_draw.h"

namespace mural {
namespace {

constexpr int STX_BINS = 9;                                // utr5, utr3, noncoding_exon, splice_donor, splice_acceptor, splice_utr, intron, start_lost, cds
constexpr int STX_SLOTS = 3;                               // the bins one item's rows can fall in; STX_SLOTS itself: nowhere
constexpr int STX_KIND_CODING_INTRON = 3, STX_KIND_INTRON = 4, STX_KIND_CDS = 5;

struct SimTxstructArgs {
  TxSegments tx;
  const int64_t* feat_b0;
  const int64_t* feat_b1;
  const int32_t* feat_tx;
  const uint8_t* feat_kind;
  const int32_t* feat_seg;
};

struct TxstructDraw {
  using Word = uint16_t;
  static constexpr int BITS = 2, BOUNDS = 3, ACCS = STX_SLOTS, UNIT_BLOCKS = SIM_UNIT_BLOCKS;
  static constexpr uint32_t NOWHERE = STX_SLOTS;
  static constexpr bool ROW_WORDS = true;
  const SimTxstructArgs& A;
  const uint8_t* strand;      // the rows', or nullptr
  const uint8_t* aa;
  int64_t b0, b1, seg, cds0, cds_len;
  int32_t tx;
  int kind;
  bool minus, has_sites, has_start;
  int slot_bin[STX_SLOTS];      // the bins of the item's slots; -1: the slot is not used

  __device__ __forceinline__ bool begin_unit(int64_t f) {
    b0 = A.feat_b0[f], b1 = A.feat_b1[f];
    tx = A.feat_tx[f];      // (0 <= tx < n_tx: the range kernel gave other items no chunk)
    kind = A.feat_kind[f];
    minus = A.tx.tx_strand[tx] != 0;
    slot_bin[0] = slot_bin[1] = slot_bin[2] = -1;
    seg = 0, cds0 = 0, cds_len = 0;
    if (kind < STX_KIND_CODING_INTRON) {
      slot_bin[0] = kind;
    } else if (kind == STX_KIND_CODING_INTRON) {
      slot_bin[0] = 3, slot_bin[1] = 4, slot_bin[2] = 6;
    } else if (kind == STX_KIND_INTRON) {
      slot_bin[0] = 5, slot_bin[2] = 6;
    } else if (kind == STX_KIND_CDS) {
      seg = A.feat_seg[f];
      if (seg < 0 || seg >= A.tx.n_seg) return false;      // (a CDS item without its segment: skipped, as an item without its transcript)
      if (A.tx.seg_b0[seg] != b0 || A.tx.seg_b1[seg] != b1 || A.tx.seg_tx[seg] != tx) return false;
      cds0 = A.tx.seg_cds0[seg], cds_len = A.tx.tx_cds_len[tx];
      slot_bin[0] = 7, slot_bin[1] = 8;
    } else {
      return false;      // (an unknown kind)
    }
    has_sites = kind != STX_KIND_CDS && b1 - b0 >= 4;
    has_start = kind == STX_KIND_CDS && cds0 < 3;      // the item holds a base of CDS codon 0
    return true;
  }
  __device__ __forceinline__ Word row_word(int64_t i, int64_t q) const {
    // (q lies in [b0, b1) unless the rows do not ascend: then the row is skipped here; a bad row draws class 0)
    if (q < b0 || q >= b1) return sim_dead_word<TxstructDraw>();
    uint32_t slot = 0;
    if (kind == STX_KIND_CDS) {
      slot = 1;
    } else if (kind >= STX_KIND_CODING_INTRON) {
      const bool low = has_sites && q < b0 + 2, high = has_sites && q >= b1 - 2;
      const bool donor = minus ? high : low, acceptor = minus ? low : high;
      slot = kind == STX_KIND_CODING_INTRON ? (donor ? 0u : acceptor ? 1u : 2u) : ((donor || acceptor) ? 0u : 2u);
    }
    uint32_t word = slot | slot << 2 | slot << 4;
    if (has_start && cds0 + (minus ? b1 - 1 - q : q - b0) < 3) {      // has_start is wave-uniform: the other items read no base
      int bins[3];
      conseq_row_bins(A.tx, strand, aa, seg, tx, minus, cds_len, b0, b1, cds0, i, q, bins);
      word = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) word |= ((bins[c] >= 1 && bins[c] <= 3) ? 0u : 1u) << (2 * c);      // aa_alt != aa_ref on a resolved codon
    }
    return (Word)(word | NOWHERE << 6);
  }
  __device__ __forceinline__ uint32_t present() const { return ~0u; }
  __device__ __forceinline__ int cell(int s) const { return slot_bin[s]; }
  __device__ __forceinline__ int32_t owner() const { return tx; }
  __device__ __forceinline__ int bins() const { return STX_BINS; }
};

template <typename T>
__global__ __launch_bounds__(SIM_THREADS) void simulate_txstruct_draw_kernel(SimDraw D, SimTxstructArgs A) {
  __shared__ uint32_t aa_words[16];
  __shared__ uint16_t words[SIM_WAVES][SIM_TILES][64];
  TxstructDraw pol{A, D.rows.strand, stage_aa(A.tx, aa_words)};
  draw_count_units<T>(D, pol, words[threadIdx.x >> 6]);
}

}  // namespace
}  // namespace mural

using namespace mural;

extern "C" size_t mural_simulate_txstruct_workspace_bytes(int64_t n_features) {
  return row_chunks_bytes(n_features);
}

extern "C" int mural_simulate_txstruct_rows(const MuralSimulateTxstructRows* s, void* ws_ptr, size_t ws_bytes, void* stream) {
  MURAL_REQUIRE(s, "simulate_txstruct_rows: NULL argument");
  MURAL_REQUIRE(s->n_class == 4, "simulate_txstruct_rows: SNV rows of 4 classes required (n_class = %d)", s->n_class);
  if (const int rc = check_sim_tx_bounds("simulate_txstruct_rows", s->n_rep, s->n, s->n_features, s->n_segments, s->n_transcripts)) return rc;
  SimTxstructArgs A{};
  if (const int rc = fill_tx_segments("simulate_txstruct_rows", s, false, A.tx)) return rc;      // (alt_order alone)
  if (s->n == 0) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->start && s->status, "simulate_txstruct_rows: NULL argument");
  MURAL_REQUIRE(s->prob_stride >= 4, "simulate_txstruct_rows: prob_stride < n_class");
  SimDraw D{};
  D.rows = sim_rows(s->prob, s->prob_stride, s->start, s->strand, 4, s->chrom_key, s->seed, s->status);
  if (s->n_features > 0) {      // (everything is checked before the first launch)
    if (const int rc = fill_tx_segments("simulate_txstruct_rows", s, true, A.tx)) return rc;      // (the genome, and the fill)
    MURAL_REQUIRE(s->feat_b0 && s->feat_b1 && s->feat_tx && s->feat_kind && s->feat_seg && s->tx_strand && s->tx_cds_len &&
                      s->n_transcripts >= 1 && s->table,
                  "simulate_txstruct_rows: items without transcripts or table");
    MURAL_REQUIRE(s->n_segments == 0 || (s->seg_b0 && s->seg_b1 && s->seg_cds0 && s->seg_tx && s->seg_prev && s->seg_next),
                  "simulate_txstruct_rows: n_segments without the segment arrays");
    if (const int rc = check_workspace("simulate_txstruct_rows", "mural_simulate_txstruct_workspace_bytes", ws_ptr, ws_bytes,
                                       mural_simulate_txstruct_workspace_bytes(s->n_features)))
      return rc;
  }
  const hipStream_t st = (hipStream_t)stream;
  if (const int rc = launch_simulate_check(st, D.rows, s->n, s->prob_f64, 1)) return rc;
  if (s->n_features == 0) return MURAL_OK;
  A.feat_b0 = s->feat_b0, A.feat_b1 = s->feat_b1, A.feat_tx = s->feat_tx, A.feat_kind = s->feat_kind, A.feat_seg = s->feat_seg;
  D.n_items = s->n_features, D.n_rep = s->n_rep, D.table = s->table;
  return launch_draw_count(st, D, s->prob_f64, s->n, s->feat_b0, s->feat_b1, s->feat_tx, s->n_transcripts, 0, TxstructDraw::UNIT_BLOCKS, ws_ptr,
                           simulate_txstruct_draw_kernel<float>, simulate_txstruct_draw_kernel<double>, A);
}
