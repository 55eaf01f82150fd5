// The simulated null of the structure table while a prediction shard is on the device (mural_amd/summaries.py:
// SummarySink(simulate=R, transcripts=..., transcript_structure=True, simulate_transcripts=True, simulate_structure=True);
// tables.simulate_structure_table from a written table): per transcript of a BED12 file, structure bin and replicate, the SNV rows inside
// [chromStart, chromEnd) whose replicate-r draw is a class c >= 1 that falls in that bin.  The draw is csrc/simulate.hip's
// (simulate_draw.h: Philox key and counter, cum, ties), the items and their bins csrc/summary_txstruct.hip's (kinds, splice sites by
// transcript orientation, start lost through conseq_bins.h); summaries.simulate_txstruct_host is the specification; DESIGN.md section 3.24.
//
// The loop bounds are csrc/simulate.hip's: SIM_CHUNK_ROWS rows a chunk, SIM_GRID_WAVES waves a grid, SIM_SCAN_THREADS threads in the
// scan (mural_simulate_chunk_rows(), mural_simulate_grid_waves(), mural_simulate_scan_threads()).  Per call:
//   * check kernel (simulate_draw.h), a thread per row: the simulation's status bits;
//   * the plan (row_chunks.h: plan_row_chunks): the items' rows cut into chunks of at most SIM_CHUNK_ROWS rows;
//   * draw kernel, a grid of at most SIM_GRID_WAVES waves striding over the units (chunk of an item, group of up to STX_UNIT_BLOCKS
//     blocks of 64 replicates).  The rows of one item fall in at most three bins (an intron: donor, acceptor, rest; a CDS part: start
//     lost, cds; every other kind: one), so a wave first walks its chunk 64 rows at a time, a row per lane, and forms each row's three
//     SLOTS once, one per class: six bits (and "nowhere" for a dead lane) kept in LDS, a 16-bit word per (tile, lane) that only its own
//     lane reads back.  Only a CDS item that holds CDS offsets 0 .. 2 reads the genome (conseq_row_bins), and only in its lanes at those
//     offsets: the branch on the item is wave-uniform, UTR and intron chunks load no base.  Then per replicate block it walks the chunk
//     again: the lane's cum[3] (row_cum), and per Philox call of four replicates the lane's label, its slot ("nowhere" for label 0), per
//     slot popc(ballot(slot == s)) added in the lane that owns the replicate (lane 4 j + k); after the chunk the slots are mapped to
//     bins by the item's kind and ONE wave-instruction per used slot adds the 64 counts -- 256 contiguous bytes -- with 32-bit INTEGER
//     atomics at table[(tx * 9 + b) * n_rep + rb * 64 + lane], zero counts skipped.
// Draws and bins are recomputed, never stored in memory; no floating-point atomics, no synchronisation, no read-back.
#include "common.h"
#include "conseq_bins.h"
#include "kmer_key.h"
#include "row_chunks.h"
#include "simulate_draw.h"

namespace mural {
namespace {

#ifndef STX_UNIT_BLOCKS
#define STX_UNIT_BLOCKS 16
#endif
constexpr int STX_TILES = (int)(SIM_CHUNK_ROWS / 64);      // tiles of a chunk
constexpr int64_t STX_MAX_ROWS = 1ll << 31;                // per call, as mural_summary_txstruct_rows
constexpr int64_t STX_MAX_FEATURES = 1ll << 22;
constexpr int64_t STX_MAX_SEGMENTS = 1ll << 22;
constexpr int STX_BINS = 9;                                // utr5, utr3, noncoding_exon, splice_donor, splice_acceptor, splice_utr, intron, start_lost, cds
constexpr int STX_SLOTS = 3;                               // the bins one item's rows can fall in; STX_SLOTS itself: nowhere
constexpr int STX_KIND_CODING_INTRON = 3, STX_KIND_INTRON = 4, STX_KIND_CDS = 5;
constexpr uint32_t STX_DEAD = STX_SLOTS | STX_SLOTS << 2 | STX_SLOTS << 4;      // the packed slots of a lane without a row

struct SimTxstructArgs {
  SimRows rows;
  TxSegments tx;
  int32_t n_rep;
  const int64_t* feat_b0;
  const int64_t* feat_b1;
  const int32_t* feat_tx;
  const uint8_t* feat_kind;
  const int32_t* feat_seg;
  int64_t n_feat;
  uint32_t* table;
};

template <typename T>
__global__ __launch_bounds__(SIM_THREADS) void simulate_txstruct_draw_kernel(SimTxstructArgs A, const int64_t* __restrict__ row0,
                                                                             const int64_t* __restrict__ row1,
                                                                             const int64_t* __restrict__ pre, int64_t n_waves) {
  __shared__ uint32_t aa_words[16];
  __shared__ uint16_t packed_slots[SIM_WAVES][STX_TILES][64];
  const uint8_t* aa = stage_aa(A.tx, aa_words);
  const int lane = threadIdx.x & 63;
  uint16_t (&mine)[STX_TILES][64] = packed_slots[threadIdx.x >> 6];      // (a lane reads only what it wrote itself: no barrier)
  const int64_t wave = (int64_t)blockIdx.x * SIM_WAVES + (threadIdx.x >> 6);
  const int n_rep = A.n_rep;
  const int n_rb = (n_rep + 63) / 64;
  const int64_t n_rg = (n_rb + STX_UNIT_BLOCKS - 1) / STX_UNIT_BLOCKS;
  const int64_t units = pre[A.n_feat] * n_rg;
  for (int64_t unit = wave; unit < units; unit += n_waves) {
    const int64_t t = unit / n_rg;
    const int rg = (int)(unit % n_rg);
    const int64_t f = row_chunk_item(pre, A.n_feat, t);
    const int64_t r0 = row0[f] + (t - pre[f]) * SIM_CHUNK_ROWS;
    const int64_t r1 = min(r0 + SIM_CHUNK_ROWS, row1[f]);
    const int64_t b0 = A.feat_b0[f], b1 = A.feat_b1[f];
    const int32_t tx = A.feat_tx[f];      // (0 <= tx < n_tx: the range kernel gave other items no chunk)
    const int kind = A.feat_kind[f];
    const bool minus = A.tx.tx_strand[tx] != 0;
    // the bins of the item's slots; -1: the slot is not used
    int slot_bin[STX_SLOTS] = {-1, -1, -1};
    int64_t seg = 0, cds0 = 0, cds_len = 0;
    if (kind < STX_KIND_CODING_INTRON) {
      slot_bin[0] = kind;
    } else if (kind == STX_KIND_CODING_INTRON) {
      slot_bin[0] = 3, slot_bin[1] = 4, slot_bin[2] = 6;
    } else if (kind == STX_KIND_INTRON) {
      slot_bin[0] = 5, slot_bin[2] = 6;
    } else if (kind == STX_KIND_CDS) {
      seg = A.feat_seg[f];
      if (seg < 0 || seg >= A.tx.n_seg) continue;      // (a CDS item without its segment: skipped, as an item without its transcript)
      if (A.tx.seg_b0[seg] != b0 || A.tx.seg_b1[seg] != b1 || A.tx.seg_tx[seg] != tx) continue;
      cds0 = A.tx.seg_cds0[seg], cds_len = A.tx.tx_cds_len[tx];
      slot_bin[0] = 7, slot_bin[1] = 8;
    } else {
      continue;      // (an unknown kind)
    }
    const bool has_sites = kind != STX_KIND_CDS && b1 - b0 >= 4;
    const bool has_start = kind == STX_KIND_CDS && cds0 < 3;      // the item holds a base of CDS codon 0
    int tile = 0;
    for (int64_t row = r0; row < r1; row += 64, ++tile) {      // (at most STX_TILES tiles: r1 - r0 <= SIM_CHUNK_ROWS)
      const int64_t i = row + lane;
      uint32_t word = STX_DEAD;
      bool live = false;
      int64_t q = b0;
      if (i < r1) {
        q = A.rows.start[i];
        // (q lies in [b0, b1) unless the rows do not ascend: then the row is skipped here; a bad row draws class 0 below)
        live = q >= b0 && q < b1;
        if (live) {
          uint32_t slot = 0;
          if (kind == STX_KIND_CDS) {
            slot = 1;
          } else if (kind >= STX_KIND_CODING_INTRON) {
            const bool low = has_sites && q < b0 + 2, high = has_sites && q >= b1 - 2;
            const bool donor = minus ? high : low, acceptor = minus ? low : high;
            slot = kind == STX_KIND_CODING_INTRON ? (donor ? 0u : acceptor ? 1u : 2u) : ((donor || acceptor) ? 0u : 2u);
          }
          word = slot | slot << 2 | slot << 4;
        }
      }
      if (has_start) {      // wave-uniform: the other items read no base
        const int64_t x = cds0 + (minus ? b1 - 1 - q : q - b0);
        if (live && x < 3) {
          int bins[3];
          conseq_row_bins(A.tx, A.rows.strand, aa, seg, tx, minus, cds_len, b0, b1, cds0, i, q, bins);
          word = 0;
#pragma unroll
          for (int c = 0; c < 3; ++c) word |= ((bins[c] >= 1 && bins[c] <= 3) ? 0u : 1u) << (2 * c);      // aa_alt != aa_ref on a resolved codon
        }
      }
      mine[tile][lane] = (uint16_t)word;
    }
    const int rb_end = min(n_rb, (rg + 1) * STX_UNIT_BLOCKS);
    for (int rb = rg * STX_UNIT_BLOCKS; rb < rb_end; ++rb) {
      const int reps_here = min(64, n_rep - rb * 64);
      const int n_blocks = (reps_here + 3) / 4;
      uint32_t acc[STX_SLOTS];
#pragma unroll
      for (int s = 0; s < STX_SLOTS; ++s) acc[s] = 0;
      tile = 0;
      for (int64_t row = r0; row < r1; row += 64, ++tile) {
        const int64_t i = row + lane;
        u64 cum[SIM_MAX_CLASS - 1];
#pragma unroll
        for (int c = 0; c < SIM_MAX_CLASS - 1; ++c) cum[c] = 0;
        uint32_t s_lo = 0, s_hi = 0, last = 0;
        if (i < r1) {
          row_cum<T>(A.rows, i, cum);      // (the status is the check kernel's)
          const u64 st = (u64)A.rows.start[i];
          s_lo = (uint32_t)st, s_hi = (uint32_t)(st >> 32);
          last = last_counter_word(A.rows, i, 0);
        }
        const uint32_t word = mine[tile][lane];
        for (int j = 0; j < n_blocks; ++j) {
          uint32_t u[4];
          philox4x32_10(s_lo, s_hi, A.rows.chrom_key, last | (uint32_t)(rb * 16 + j), A.rows.seed_lo, A.rows.seed_hi, u);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const u64 mine_u = u[k];
            // cum ascends: the label is the first class whose bound is above u; its two bits of `word`, "nowhere" for label 0
            const uint32_t sh = mine_u < cum[0] ? 0u : mine_u < cum[1] ? 2u : mine_u < cum[2] ? 4u : 6u;
            const uint32_t ls = sh < 6u ? (word >> sh) & 3u : (uint32_t)STX_SLOTS;
#pragma unroll
            for (int s = 0; s < STX_SLOTS; ++s) {
              const uint32_t hits = (uint32_t)__popcll(__ballot(ls == (uint32_t)s));
              if (lane == j * 4 + k) acc[s] += hits;
            }
          }
        }
      }
      if (lane < reps_here) {
#pragma unroll
        for (int s = 0; s < STX_SLOTS; ++s)
          if (slot_bin[s] >= 0 && acc[s])
            atomicAdd(&A.table[((int64_t)tx * STX_BINS + slot_bin[s]) * n_rep + rb * 64 + lane], acc[s]);
      }
    }
  }
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
  MURAL_REQUIRE(s->n_rep >= 1 && s->n_rep <= SIM_MAX_REP, "simulate_txstruct_rows: 1 <= n_rep <= 2^20 required");
  MURAL_REQUIRE(s->n >= 0 && s->n <= STX_MAX_ROWS, "simulate_txstruct_rows: 0 <= n <= 2^31 required");
  MURAL_REQUIRE(s->n_features >= 0 && s->n_features <= STX_MAX_FEATURES, "simulate_txstruct_rows: 0 <= n_features <= 2^22 required");
  MURAL_REQUIRE(s->n_segments >= 0 && s->n_segments <= STX_MAX_SEGMENTS, "simulate_txstruct_rows: 0 <= n_segments <= 2^22 required");
  MURAL_REQUIRE(s->n_transcripts >= 0, "simulate_txstruct_rows: n_transcripts < 0");
  SimTxstructArgs A{};
  if (const int rc = fill_tx_segments("simulate_txstruct_rows", s, false, A.tx)) return rc;      // (alt_order alone)
  if (s->n == 0) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->start && s->status, "simulate_txstruct_rows: NULL argument");
  MURAL_REQUIRE(s->prob_stride >= 4, "simulate_txstruct_rows: prob_stride < n_class");
  A.rows = sim_rows(s->prob, s->prob_stride, s->start, s->strand, 4, s->chrom_key, s->seed, s->status);
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
  if (const int rc = launch_simulate_check(st, A.rows, s->n, s->prob_f64, 1)) return rc;
  if (s->n_features == 0) return MURAL_OK;
  A.n_rep = s->n_rep, A.table = s->table;
  A.feat_b0 = s->feat_b0, A.feat_b1 = s->feat_b1, A.feat_tx = s->feat_tx, A.feat_kind = s->feat_kind, A.feat_seg = s->feat_seg;
  A.n_feat = s->n_features;
  WsArena ws(ws_ptr);
  RowChunks w;
  if (const int rc = plan_row_chunks<SIM_THREADS, SIM_SCAN_THREADS>(st, s->start, s->n, s->feat_b0, s->feat_b1, s->feat_tx, s->n_transcripts,
                                                                    s->n_features, 0, SIM_CHUNK_ROWS, ws, w))
    return rc;
  const int64_t n_rg = ((s->n_rep + 63) / 64 + STX_UNIT_BLOCKS - 1) / STX_UNIT_BLOCKS;
  const int64_t n_waves = row_chunk_grid_waves(s->n, SIM_CHUNK_ROWS, n_rg, s->n_features, SIM_GRID_WAVES, SIM_WAVES);
  const dim3 draw_grid((unsigned)(n_waves / SIM_WAVES)), block(SIM_THREADS);
  if (s->prob_f64)
    hipLaunchKernelGGL(simulate_txstruct_draw_kernel<double>, draw_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  else
    hipLaunchKernelGGL(simulate_txstruct_draw_kernel<float>, draw_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}
