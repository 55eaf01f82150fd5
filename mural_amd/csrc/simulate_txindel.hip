// The simulated null of the INDEL structure table while a prediction shard is on the device (mural_amd/summaries.py:
// SummarySink(simulate=R, indel_transcripts=..., indel_kind=..., simulate_indel_structure=True); tables.simulate_indel_structure_table
// from a written table): per transcript of a BED12 file, INDEL structure bin and replicate, the INDEL rows that the transcript counts
// whose replicate-r draw is a class c >= 1 that falls in that bin.  The draw is csrc/simulate.hip's (simulate_draw.h: Philox key and
// counter, cum, ties), the items, the home base and the bin of a class csrc/summary_txindel.hip's (txindel_bins.h: an insertion's site,
// a deletion's walk); summaries.simulate_txindel_host is the specification; DESIGN.md section 3.26.
//
// The loop bounds are csrc/simulate.hip's: SIM_CHUNK_ROWS rows a chunk, SIM_GRID_WAVES waves a grid, SIM_SCAN_THREADS threads in the
// scan (mural_simulate_chunk_rows(), mural_simulate_grid_waves(), mural_simulate_scan_threads()).  Per call:
//   * check kernel (simulate_draw.h), a thread per row: the simulation's status bits;
//   * the plan (row_chunks.h: plan_row_chunks with a shift): the rows of an item are those whose HOME BASE lies in it, cut into chunks
//     of at most SIM_CHUNK_ROWS rows;
//   * draw kernel, a grid of at most SIM_GRID_WAVES waves striding over the units (chunk of a home item, group of up to SIM_UNIT_BLOCKS
//     blocks of 64 replicates).  The home item and an insertion's second item are wave-uniform and loaded once per unit.  A wave first
//     walks its chunk 64 rows at a time, a row per lane, and forms the bin of every class of the row ONCE through txindel_bins.h -- a
//     deletion's walk is paid here, not per replicate --: 4 bits a class in one 32-bit word, 15 for "not counted", the word kept in LDS
//     per (tile, lane), where only its own lane reads it back.  An OR over the lanes gives the wave-uniform mask of the bins present in
//     the chunk.  Then per replicate block it walks the chunk again: the lane's cum (row_cum, the classes beyond n_class set to 2^32 so
//     that the count of the bounds not above u is the index of the drawn class's 4 bits, and of a 15 where no class is drawn), and
//     per Philox call of four replicates, for each PRESENT bin (a scalar branch, the loop over the ten bins unrolled, the accumulators
//     indexed by constants) popc(ballot(bin == b)) added in the lane that owns the replicate (lane 4 j + k); after the chunk ONE
//     wave-instruction per non-empty bin adds the 64 counts -- 256 contiguous bytes -- with 32-bit INTEGER atomics at
//     table[(tx * 10 + b) * n_rep + rb * 64 + lane], zero counts skipped.
// Draws and bins are recomputed, never stored in memory; no floating-point atomics, no synchronisation, no read-back.
#include "common.h"
#include "kmer_key.h"
#include "row_chunks.h"
#include "simulate_draw.h"
#include "txindel_bins.h"

namespace mural {
namespace {

constexpr uint32_t STI_NOWHERE = 15;                       // the 4 bits of a class that is not counted
constexpr uint32_t STI_DEAD = 0xFFFFFFFFu;                 // the word of a lane without a counted row

struct SimTxindelArgs {      // (the fields txindel_bins.h reads, under its names)
  SimRows rows;
  int64_t n, chrom_len;      // chrom_len < 0: not known, a deletion is clipped to the span alone
  int32_t n_tx, n_rep, kind, off;
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
  uint32_t cls[SIM_MAX_CLASS];      // class c: lo | frame mode << 8 (txindel_class_word)
  uint32_t* table;
};

template <typename T>
__global__ __launch_bounds__(SIM_THREADS) void simulate_txindel_draw_kernel(SimTxindelArgs A, const int64_t* __restrict__ row0,
                                                                            const int64_t* __restrict__ row1,
                                                                            const int64_t* __restrict__ pre, int64_t n_waves) {
  __shared__ uint32_t cls_words[SIM_MAX_CLASS];
  __shared__ uint32_t bin_words[SIM_WAVES][SIM_TILES][64];
#pragma unroll
  for (int j = 0; j < SIM_MAX_CLASS; ++j)      // (constant indices: the words stay scalar arguments)
    if (threadIdx.x == j) cls_words[j] = A.cls[j];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  uint32_t (&mine)[SIM_TILES][64] = bin_words[threadIdx.x >> 6];      // (a lane reads only what it wrote itself: no barrier)
  const int64_t wave = (int64_t)blockIdx.x * SIM_WAVES + (threadIdx.x >> 6);
  const int n_rep = A.n_rep, nc = A.rows.n_class;
  const int n_rb = (n_rep + 63) / 64;
  const int64_t n_rg = (n_rb + SIM_UNIT_BLOCKS - 1) / SIM_UNIT_BLOCKS;
  const int64_t units = pre[A.n_feat] * n_rg;
  const int64_t home_shift = A.off - (A.kind == TI_DELETION_START ? 0 : 1);
  for (int64_t unit = wave; unit < units; unit += n_waves) {
    const int64_t t = unit / n_rg;
    const int rg = (int)(unit % n_rg);
    const int64_t f = row_chunk_item(pre, A.n_feat, t);
    const int64_t r0 = row0[f] + (t - pre[f]) * SIM_CHUNK_ROWS;
    const int64_t r1 = min(r0 + SIM_CHUNK_ROWS, row1[f]);
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
    // the bins of the rows' classes, once per unit
    uint32_t seen = 0;      // bit b: a class of one of this lane's rows falls in bin b
    int tile = 0;
    for (int64_t row = r0; row < r1; row += 64, ++tile) {      // (at most SIM_TILES tiles: r1 - r0 <= SIM_CHUNK_ROWS)
      const int64_t i = row + lane;
      uint32_t word = STI_DEAD;
      if (i < r1) {
        const int64_t q = A.rows.start[i];
        const int64_t j = q + A.off, h = q + home_shift;
        // (h lies in the item unless the rows do not ascend: then the row is skipped here; a bad row draws class 0 below)
        bool live = h >= home.b0 && h < home.b1;
        int site = 5;      // an insertion's bin, or TI_FRAME
        if (A.kind == TI_INSERTION) site = txindel_insertion_site(home, behind, minus, cds_len, j, live);
        if (live) {
          for (int c = 1; c < nc; ++c) {
            const uint32_t bin = (uint32_t)txindel_class_bin(A, f, tx, home, minus, site, j, cls_words[c]);      // 0 .. 9
            word ^= (bin ^ STI_NOWHERE) << (4 * (c - 1));
            seen |= 1u << bin;
          }
        }
      }
      mine[tile][lane] = word;
    }
    uint32_t present = 0;      // wave-uniform: the bins of the chunk
#pragma unroll
    for (int b = 0; b < TI_BINS; ++b)
      if (__ballot((seen >> b) & 1u)) present |= 1u << b;
    if (!present) continue;
    const int rb_end = min(n_rb, (rg + 1) * SIM_UNIT_BLOCKS);
    for (int rb = rg * SIM_UNIT_BLOCKS; rb < rb_end; ++rb) {
      const int reps_here = min(64, n_rep - rb * 64);
      const int n_blocks = (reps_here + 3) / 4;
      uint32_t acc[TI_BINS];
#pragma unroll
      for (int b = 0; b < TI_BINS; ++b) acc[b] = 0;
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
#pragma unroll
        for (int c = 0; c < SIM_MAX_CLASS - 1; ++c)
          if (c >= nc - 1) cum[c] = SIM_ONE;      // (wave-uniform) above every u: the classes that do not exist are never passed
        const uint32_t word = mine[tile][lane];
        for (int j = 0; j < n_blocks; ++j) {
          uint32_t u[4];
          philox4x32_10(s_lo, s_hi, A.rows.chrom_key, last | (uint32_t)(rb * 16 + j), A.rows.seed_lo, A.rows.seed_hi, u);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const u64 mine_u = u[k];
            // cum ascends: the bounds not above u are those of the classes before the drawn one; with no class drawn they are all
            // n_class - 1 of them, and the 4 bits there are STI_NOWHERE (never written: at most 7 classes have bins)
            uint32_t below = 0;
#pragma unroll
            for (int c = 0; c < SIM_MAX_CLASS - 1; ++c) below += mine_u >= cum[c] ? 1u : 0u;
            const uint32_t bin = (word >> (4 * below)) & 15u;
#pragma unroll
            for (int b = 0; b < TI_BINS; ++b) {
              if ((present >> b) & 1u) {      // (scalar)
                const uint32_t hits = (uint32_t)__popcll(__ballot(bin == (uint32_t)b));
                if (lane == j * 4 + k) acc[b] += hits;
              }
            }
          }
        }
      }
      if (lane < reps_here) {
#pragma unroll
        for (int b = 0; b < TI_BINS; ++b)
          if (((present >> b) & 1u) && acc[b])
            atomicAdd(&A.table[((int64_t)tx * TI_BINS + b) * n_rep + rb * 64 + lane], acc[b]);
      }
    }
  }
}

}  // namespace
}  // namespace mural

using namespace mural;

extern "C" size_t mural_simulate_txindel_workspace_bytes(int64_t n_features) {
  return row_chunks_bytes(n_features);
}

extern "C" int mural_simulate_txindel_rows(const MuralSimulateTxindelRows* s, void* ws_ptr, size_t ws_bytes, void* stream) {
  MURAL_REQUIRE(s, "simulate_txindel_rows: NULL argument");
  MURAL_REQUIRE(s->n_class >= 2 && s->n_class <= SIM_MAX_CLASS,
                "simulate_txindel_rows: 2 <= n_class <= 8 required, the bound of the simulation's draw (n_class = %d)", s->n_class);
  if (const int rc = check_sim_tx_bounds("simulate_txindel_rows", s->n_rep, s->n, s->n_features, s->n_segments, s->n_transcripts)) return rc;
  MURAL_REQUIRE(s->kind >= 0 && s->kind <= 2, "simulate_txindel_rows: kind is 0 (insertion), 1 (deletion start) or 2 (deletion end)");
  MURAL_REQUIRE(s->breakpoint_offset == 0 || s->breakpoint_offset == 1, "simulate_txindel_rows: breakpoint_offset is 0 or 1");
  for (int c = 1; c < s->n_class; ++c)
    MURAL_REQUIRE(1 <= s->class_len[c][0] && s->class_len[c][0] <= s->class_len[c][1] && s->class_len[c][1] <= TI_MAX_LEN,
                  "simulate_txindel_rows: class_len[%d] must be 1 <= lo <= hi <= 64", c);
  if (s->n == 0) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->start && s->status, "simulate_txindel_rows: NULL argument");
  MURAL_REQUIRE(s->prob_stride >= s->n_class, "simulate_txindel_rows: prob_stride < n_class");
  SimTxindelArgs A{};
  A.rows = sim_rows(s->prob, s->prob_stride, s->start, s->strand, s->n_class, s->chrom_key, s->seed, s->status);
  if (s->n_features > 0) {      // (everything is checked before the first launch)
    MURAL_REQUIRE(s->feat_b0 && s->feat_b1 && s->feat_tx && s->feat_kind && s->feat_seg && s->feat_prev && s->feat_next && s->tx_strand &&
                      s->tx_cds_len && s->n_transcripts >= 1 && s->table,
                  "simulate_txindel_rows: items without links, transcripts or table");
    MURAL_REQUIRE(s->n_segments == 0 || (s->seg_b0 && s->seg_b1 && s->seg_cds0 && s->seg_tx),
                  "simulate_txindel_rows: n_segments without the segment arrays");
    if (const int rc = check_workspace("simulate_txindel_rows", "mural_simulate_txindel_workspace_bytes", ws_ptr, ws_bytes,
                                       mural_simulate_txindel_workspace_bytes(s->n_features)))
      return rc;
  }
  const hipStream_t st = (hipStream_t)stream;
  if (const int rc = launch_simulate_check(st, A.rows, s->n, s->prob_f64, 1)) return rc;
  if (s->n_features == 0) return MURAL_OK;
  A.n = s->n, A.chrom_len = s->chrom_length, A.n_tx = s->n_transcripts, A.n_rep = s->n_rep, A.kind = s->kind, A.off = s->breakpoint_offset;
  A.seg_b0 = s->seg_b0, A.seg_b1 = s->seg_b1, A.seg_cds0 = s->seg_cds0, A.seg_tx = s->seg_tx, A.n_seg = s->n_segments;
  A.feat_b0 = s->feat_b0, A.feat_b1 = s->feat_b1, A.feat_tx = s->feat_tx, A.feat_kind = s->feat_kind, A.feat_seg = s->feat_seg;
  A.feat_prev = s->feat_prev, A.feat_next = s->feat_next, A.n_feat = s->n_features;
  A.tx_strand = s->tx_strand, A.tx_cds_len = s->tx_cds_len;
  for (int c = 1; c < s->n_class; ++c) A.cls[c] = txindel_class_word(s->class_len[c][0], s->class_len[c][1]);
  A.table = s->table;
  WsArena ws(ws_ptr);
  RowChunks w;
  const int64_t home_shift = A.off - (A.kind == TI_DELETION_START ? 0 : 1);
  if (const int rc = plan_row_chunks<SIM_THREADS, SIM_SCAN_THREADS>(st, s->start, s->n, A.feat_b0, A.feat_b1, A.feat_tx, A.n_tx, A.n_feat,
                                                                    home_shift, SIM_CHUNK_ROWS, ws, w))
    return rc;
  const int64_t n_rg = ((s->n_rep + 63) / 64 + SIM_UNIT_BLOCKS - 1) / SIM_UNIT_BLOCKS;
  const int64_t n_waves = row_chunk_grid_waves(s->n, SIM_CHUNK_ROWS, n_rg, s->n_features, SIM_GRID_WAVES, SIM_WAVES);
  const dim3 draw_grid((unsigned)(n_waves / SIM_WAVES)), block(SIM_THREADS);
  if (s->prob_f64)
    hipLaunchKernelGGL(simulate_txindel_draw_kernel<double>, draw_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  else
    hipLaunchKernelGGL(simulate_txindel_draw_kernel<float>, draw_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}
