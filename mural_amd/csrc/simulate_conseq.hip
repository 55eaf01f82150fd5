// The simulated null of the consequence table while a prediction shard is on the device (mural_amd/summaries.py:
// SummarySink(simulate=R, transcripts=..., simulate_transcripts=True); tables.simulate_consequence_table from a written table): per
// transcript of a BED12 file, consequence bin and replicate, the SNV rows inside the transcript's CDS whose replicate-r draw is a class
// c >= 1 whose substitution falls in that bin.  The draw is csrc/simulate.hip's (simulate_draw.h: Philox key and counter, cum, ties), the
// bin csrc/summary_conseq.hip's (conseq_bins.h: CDS offset, codon over seg_prev / seg_next, the amino-acid table);
// summaries.simulate_conseq_host is the specification; DESIGN.md section 3.22.
//
// The loop bounds are csrc/simulate.hip's: SIM_CHUNK_ROWS rows a chunk, SIM_GRID_WAVES waves a grid, SIM_SCAN_THREADS threads in the
// scan (mural_simulate_chunk_rows(), mural_simulate_grid_waves(), mural_simulate_scan_threads()).  Per call:
//   * check kernel (simulate_draw.h), a thread per row: the simulation's status bits;
//   * the plan (row_chunks.h: plan_row_chunks): the segments' rows cut into chunks of at most SIM_CHUNK_ROWS rows;
//   * draw kernel, a grid of at most SIM_GRID_WAVES waves striding over the units (chunk of a segment, group of up to SCQ_UNIT_BLOCKS
//     blocks of 64 replicates).  A wave first walks its chunk 64 rows at a time, a row per lane, and forms each row's three bins ONCE:
//     nine bits (and "nowhere" for a dead lane) kept in LDS, a 16-bit word per (tile, lane) that only its own lane reads back -- the
//     codon lookups are up to 9 dependent global loads a lane, and with a unit per replicate block they were redone for each of the
//     ceil(R / 64) blocks.  Then per replicate block it walks the chunk again: the lane's cum[3] (row_cum), and per Philox call of four
//     replicates the lane's label, its bin lb = bins[label - 1] ("nowhere" for label 0), per bin popc(ballot(lb == b)) added in the lane
//     that owns the replicate (lane 4 j + k); after the chunk ONE wave-instruction per bin adds the 64 counts -- 256 contiguous bytes --
//     with 32-bit INTEGER atomics at table[(tx * 5 + b) * n_rep + rb * 64 + lane], zero counts skipped.
// Draws and bins are recomputed, never stored in memory; no floating-point atomics, no synchronisation, no read-back.
#include "common.h"
#include "conseq_bins.h"
#include "kmer_key.h"
#include "row_chunks.h"
#include "simulate_draw.h"

namespace mural {
namespace {

#ifndef SCQ_UNIT_BLOCKS
#define SCQ_UNIT_BLOCKS 16
#endif
constexpr int SCQ_TILES = (int)(SIM_CHUNK_ROWS / 64);      // tiles of a chunk
constexpr int64_t SCQ_MAX_ROWS = 1ll << 31;                // per call, as mural_summary_conseq_rows
constexpr int64_t SCQ_MAX_SEGMENTS = 1ll << 22;
constexpr uint32_t SCQ_DEAD = SC_NOWHERE | SC_NOWHERE << 3 | SC_NOWHERE << 6;      // the packed bins of a lane without a row

struct SimConseqArgs {
  SimRows rows;
  TxSegments tx;
  int32_t n_rep;
  uint32_t* table;
};

template <typename T>
__global__ __launch_bounds__(SIM_THREADS) void simulate_conseq_draw_kernel(SimConseqArgs A, const int64_t* __restrict__ row0,
                                                                           const int64_t* __restrict__ row1, const int64_t* __restrict__ pre,
                                                                           int64_t n_waves) {
  __shared__ uint32_t aa_words[16];
  __shared__ uint16_t packed_bins[SIM_WAVES][SCQ_TILES][64];
  const uint8_t* aa = stage_aa(A.tx, aa_words);
  const int lane = threadIdx.x & 63;
  uint16_t (&mine)[SCQ_TILES][64] = packed_bins[threadIdx.x >> 6];      // (a lane reads only what it wrote itself: no barrier)
  const int64_t wave = (int64_t)blockIdx.x * SIM_WAVES + (threadIdx.x >> 6);
  const int n_rep = A.n_rep;
  const int n_rb = (n_rep + 63) / 64;
  const int64_t n_rg = (n_rb + SCQ_UNIT_BLOCKS - 1) / SCQ_UNIT_BLOCKS;
  const int64_t units = pre[A.tx.n_seg] * n_rg;
  for (int64_t unit = wave; unit < units; unit += n_waves) {
    const int64_t t = unit / n_rg;
    const int rg = (int)(unit % n_rg);
    const int64_t s = row_chunk_item(pre, A.tx.n_seg, t);
    const int64_t r0 = row0[s] + (t - pre[s]) * SIM_CHUNK_ROWS;
    const int64_t r1 = min(r0 + SIM_CHUNK_ROWS, row1[s]);
    const int64_t b0 = A.tx.seg_b0[s], b1 = A.tx.seg_b1[s], cds0 = A.tx.seg_cds0[s];
    const int32_t tx = A.tx.seg_tx[s];      // (0 <= tx < n_tx: the range kernel gave other segments no chunk)
    const bool minus = A.tx.tx_strand[tx] != 0;
    const int64_t cds_len = A.tx.tx_cds_len[tx];
    int tile = 0;
    for (int64_t row = r0; row < r1; row += 64, ++tile) {      // (at most SCQ_TILES tiles: r1 - r0 <= SIM_CHUNK_ROWS)
      const int64_t i = row + lane;
      uint32_t word = SCQ_DEAD;
      if (i < r1) {
        const int64_t q = A.rows.start[i];
        // (q lies in [b0, b1) unless the rows do not ascend: then the row is skipped here; a bad row draws class 0 below)
        if (q >= b0 && q < b1) {
          int bins[3];
          conseq_row_bins(A.tx, A.rows.strand, aa, s, tx, minus, cds_len, b0, b1, cds0, i, q, bins);
          word = (uint32_t)bins[0] | (uint32_t)bins[1] << 3 | (uint32_t)bins[2] << 6;
        }
      }
      mine[tile][lane] = (uint16_t)word;
    }
    const int rb_end = min(n_rb, (rg + 1) * SCQ_UNIT_BLOCKS);
    for (int rb = rg * SCQ_UNIT_BLOCKS; rb < rb_end; ++rb) {
      const int reps_here = min(64, n_rep - rb * 64);
      const int n_blocks = (reps_here + 3) / 4;
      uint32_t acc[SC_BINS];
#pragma unroll
      for (int b = 0; b < SC_BINS; ++b) acc[b] = 0;
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
            // cum ascends: the label is the first class whose bound is above u; its three bits of `word`, "nowhere" for label 0
            const uint32_t sh = mine_u < cum[0] ? 0u : mine_u < cum[1] ? 3u : mine_u < cum[2] ? 6u : 9u;
            const uint32_t lb = sh < 9u ? (word >> sh) & 7u : (uint32_t)SC_NOWHERE;
#pragma unroll
            for (int b = 0; b < SC_BINS; ++b) {
              const uint32_t hits = (uint32_t)__popcll(__ballot(lb == (uint32_t)b));
              if (lane == j * 4 + k) acc[b] += hits;
            }
          }
        }
      }
      if (lane < reps_here) {
#pragma unroll
        for (int b = 0; b < SC_BINS; ++b)
          if (acc[b]) atomicAdd(&A.table[((int64_t)tx * SC_BINS + b) * n_rep + rb * 64 + lane], acc[b]);
      }
    }
  }
}

}  // namespace
}  // namespace mural

using namespace mural;

extern "C" size_t mural_simulate_conseq_workspace_bytes(int64_t n_segments) {
  return row_chunks_bytes(n_segments);
}

extern "C" int mural_simulate_conseq_rows(const MuralSimulateConseqRows* s, void* ws_ptr, size_t ws_bytes, void* stream) {
  MURAL_REQUIRE(s, "simulate_conseq_rows: NULL argument");
  MURAL_REQUIRE(s->n_class == 4, "simulate_conseq_rows: SNV rows of 4 classes required (n_class = %d)", s->n_class);
  MURAL_REQUIRE(s->n_rep >= 1 && s->n_rep <= SIM_MAX_REP, "simulate_conseq_rows: 1 <= n_rep <= 2^20 required");
  MURAL_REQUIRE(s->n >= 0 && s->n <= SCQ_MAX_ROWS, "simulate_conseq_rows: 0 <= n <= 2^31 required");
  MURAL_REQUIRE(s->n_segments >= 0 && s->n_segments <= SCQ_MAX_SEGMENTS, "simulate_conseq_rows: 0 <= n_segments <= 2^22 required");
  MURAL_REQUIRE(s->n_transcripts >= 0, "simulate_conseq_rows: n_transcripts < 0");
  SimConseqArgs A{};
  if (const int rc = fill_tx_segments("simulate_conseq_rows", s, false, A.tx)) return rc;      // (alt_order alone)
  if (s->n == 0) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->start && s->status, "simulate_conseq_rows: NULL argument");
  MURAL_REQUIRE(s->prob_stride >= 4, "simulate_conseq_rows: prob_stride < n_class");
  A.rows = sim_rows(s->prob, s->prob_stride, s->start, s->strand, 4, s->chrom_key, s->seed, s->status);
  if (s->n_segments > 0) {      // (everything is checked before the first launch)
    if (const int rc = fill_tx_segments("simulate_conseq_rows", s, true, A.tx)) return rc;      // (the genome, and the fill)
    MURAL_REQUIRE(s->seg_b0 && s->seg_b1 && s->seg_cds0 && s->seg_tx && s->seg_prev && s->seg_next && s->tx_strand && s->tx_cds_len &&
                      s->n_transcripts >= 1 && s->table,
                  "simulate_conseq_rows: segments without transcripts or table");
    if (const int rc = check_workspace("simulate_conseq_rows", "mural_simulate_conseq_workspace_bytes", ws_ptr, ws_bytes,
                                       mural_simulate_conseq_workspace_bytes(s->n_segments)))
      return rc;
  }
  const hipStream_t st = (hipStream_t)stream;
  if (const int rc = launch_simulate_check(st, A.rows, s->n, s->prob_f64, 1)) return rc;
  if (s->n_segments == 0) return MURAL_OK;
  A.n_rep = s->n_rep, A.table = s->table;
  WsArena ws(ws_ptr);
  RowChunks w;
  if (const int rc = plan_row_chunks<SIM_THREADS, SIM_SCAN_THREADS>(st, s->start, s->n, s->seg_b0, s->seg_b1, s->seg_tx, s->n_transcripts,
                                                                    s->n_segments, 0, SIM_CHUNK_ROWS, ws, w))
    return rc;
  const int64_t n_rg = ((s->n_rep + 63) / 64 + SCQ_UNIT_BLOCKS - 1) / SCQ_UNIT_BLOCKS;
  const int64_t n_waves = row_chunk_grid_waves(s->n, SIM_CHUNK_ROWS, n_rg, s->n_segments, SIM_GRID_WAVES, SIM_WAVES);
  const dim3 draw_grid((unsigned)(n_waves / SIM_WAVES)), block(SIM_THREADS);
  if (s->prob_f64)
    hipLaunchKernelGGL(simulate_conseq_draw_kernel<double>, draw_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  else
    hipLaunchKernelGGL(simulate_conseq_draw_kernel<float>, draw_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}
