// Mutation sets drawn from the predicted rates while a prediction shard is on the device (mural_amd/summaries.py:
// SummarySink(simulate=R, ...); tables.simulate_table from a written table): every row's class is drawn from its probabilities in each of
// R replicates, and either counted per named interval set (mural_simulate_annot_rows: the null distribution of §3.19's observed counts)
// or written out for one replicate as a compacted mutation list (mural_simulate_rows).
//
// The draw is stateless (simulate_rows_host in summaries.py is the specification): Philox4x32-10 with key (seed lo, seed hi) and counter
// (start lo, start hi, chrom_key, (replicate >> 2) | (strand << 31)); replicate r reads output word r & 3 as u.  With
// q_c = floor(double(p_c) * 2^32) (exact; taken as 2^32 from p_c = 1 on) and cum_c = min(q_1 + .. + q_c, 2^32), the class is the smallest
// c >= 1 with u < cum_c and 0 where there is none.  A draw depends on (seed, chromosome, start, strand, replicate) alone, so every table
// is a function of the SET of rows, bit for bit, whatever the parts, chunks or ranks.  All state is integer; draws are recomputed where
// they are needed and never stored.
//
// mural_simulate_annot_rows, per call:
//   * check kernel, a thread per row: the status bits (a bad probability, a negative start, a start below the row before it);
//   * the plan (row_chunks.h: plan_row_chunks): the pieces' rows cut into chunks of at most SIM_CHUNK_ROWS rows;
//   * draw kernel, a fixed grid of SIM_GRID_WAVES waves striding over the units (chunk, block of 64 replicates): the wave finds the
//     chunk's piece, walks the chunk 64 rows at a time (a row per lane, four replicates per Philox call), counts the hits of a (class,
//     replicate) over the 64 rows by ballot + popcount and keeps the count of replicate r0 + l in lane l; after the chunk ONE
//     wave-instruction per class adds the 64 counts -- 256 contiguous bytes -- with 32-bit INTEGER atomics.
// mural_simulate_rows: tile counts of the non-zero labels of one replicate (a wave per 64 rows), their exclusive scan, and a second pass
// that recomputes the labels and writes each hit at prefix + its rank among the tile's hits: stable in row order.
// No floating-point atomics, no synchronisation, no read-back.  The check kernel, the Philox round, a row's cum and the last counter
// word live in simulate_draw.h, with the loop bounds; the per-transcript simulations include it as well.
#include "common.h"
#include "kmer_key.h"
#include "row_chunks.h"
#include "simulate_draw.h"

namespace mural {
namespace {

template <typename T>
__global__ __launch_bounds__(SIM_THREADS) void simulate_draw_kernel(SimRows A, const int32_t* __restrict__ group, int64_t n_pieces,
                                                                    const int64_t* __restrict__ row0, const int64_t* __restrict__ row1,
                                                                    const int64_t* __restrict__ pre, int32_t n_rep, int64_t n_waves,
                                                                    uint32_t* __restrict__ table) {
  const int lane = threadIdx.x & 63, nc = A.n_class;
  const int64_t wave = (int64_t)blockIdx.x * SIM_WAVES + (threadIdx.x >> 6);
  const int64_t n_rb = (n_rep + 63) / 64;
  const int64_t units = pre[n_pieces] * n_rb;
  for (int64_t unit = wave; unit < units; unit += n_waves) {
    const int64_t t = unit / n_rb;
    const int rb = (int)(unit % n_rb);
    const int64_t p = row_chunk_item(pre, n_pieces, t);
    const int64_t r0 = row0[p] + (t - pre[p]) * SIM_CHUNK_ROWS;
    const int64_t r1 = min(r0 + SIM_CHUNK_ROWS, row1[p]);
    const int reps_here = min(64, n_rep - rb * 64);
    const int n_blocks = (reps_here + 3) / 4;
    uint32_t acc[SIM_MAX_CLASS - 1];
#pragma unroll
    for (int c = 0; c < SIM_MAX_CLASS - 1; ++c) acc[c] = 0;
    for (int64_t row = r0; row < r1; row += 64) {
      const int64_t i = row + lane;
      u64 cum[SIM_MAX_CLASS - 1];
#pragma unroll
      for (int c = 0; c < SIM_MAX_CLASS - 1; ++c) cum[c] = 0;
      uint32_t s_lo = 0, s_hi = 0, last = 0;
      if (i < r1) {
        row_cum<T>(A, i, cum);      // (the status is the check kernel's)
        const u64 s = (u64)A.start[i];
        s_lo = (uint32_t)s, s_hi = (uint32_t)(s >> 32);
        last = last_counter_word(A, i, 0);
      }
      for (int j = 0; j < n_blocks; ++j) {
        uint32_t u[4];
        philox4x32_10(s_lo, s_hi, A.chrom_key, last | (uint32_t)(rb * 16 + j), A.seed_lo, A.seed_hi, u);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          uint32_t below = 0;      // rows of the tile whose label is in 1 .. c - 1
#pragma unroll
          for (int c = 1; c < SIM_MAX_CLASS; ++c) {
            if (c < nc) {      // (wave-uniform)
              const uint32_t upto = (uint32_t)__popcll(__ballot((u64)u[k] < cum[c - 1]));      // cum ascends: labels 1 .. c
              if (lane == j * 4 + k) acc[c - 1] += upto - below;
              below = upto;
            }
          }
        }
      }
    }
    const int32_t g = group[p];
    if (lane < reps_here) {
#pragma unroll
      for (int c = 1; c < SIM_MAX_CLASS; ++c)
        if (c < nc && acc[c - 1]) atomicAdd(&table[((int64_t)g * (nc - 1) + (c - 1)) * n_rep + rb * 64 + lane], acc[c - 1]);
    }
  }
}

// the label of row i in replicate `rep`
template <typename T>
__device__ __forceinline__ int row_label(const SimRows& A, int64_t i, int32_t rep) {
  u64 cum[SIM_MAX_CLASS - 1];
  row_cum<T>(A, i, cum);
  const u64 s = (u64)A.start[i];
  uint32_t u[4];
  philox4x32_10((uint32_t)s, (uint32_t)(s >> 32), A.chrom_key, last_counter_word(A, i, (uint32_t)(rep >> 2)), A.seed_lo, A.seed_hi, u);
  const u64 mine = u[rep & 3];
  int lab = 0;
#pragma unroll
  for (int c = SIM_MAX_CLASS - 1; c >= 1; --c)
    if (c < A.n_class && mine < cum[c - 1]) lab = c;
  return lab;
}

// a wave per tile of 64 rows: the number of non-zero labels
template <typename T>
__global__ __launch_bounds__(SIM_THREADS) void simulate_count_kernel(SimRows A, int64_t n, int32_t rep, int64_t n_tiles,
                                                                     int64_t* __restrict__ pre) {
  const int64_t t = (int64_t)blockIdx.x * SIM_WAVES + (threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const int64_t i = t * 64 + (threadIdx.x & 63);
  const int lab = i < n ? row_label<T>(A, i, rep) : 0;
  const int hits = __popcll(__ballot(lab != 0));
  if ((threadIdx.x & 63) == 0) pre[t] = hits;
}

template <typename T>
__global__ __launch_bounds__(SIM_THREADS) void simulate_write_kernel(SimRows A, int64_t n, int32_t rep, int64_t n_tiles,
                                                                     const int64_t* __restrict__ pre, int64_t* __restrict__ out_start,
                                                                     uint8_t* __restrict__ out_strand, uint8_t* __restrict__ out_label) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * SIM_WAVES + (threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const int64_t i = t * 64 + lane;
  const int lab = i < n ? row_label<T>(A, i, rep) : 0;
  const u64 hits = __ballot(lab != 0);
  if (lab != 0) {
    const int64_t at = pre[t] + __popcll(hits & ((1ull << lane) - 1));      // below n: the hits before this one are rows before i
    out_start[at] = A.start[i];
    out_strand[at] = (A.strand != nullptr && A.strand[i] != 0) ? 1 : 0;
    out_label[at] = (uint8_t)lab;
  }
}

int64_t tiles_of(int64_t n) { return (n + 63) / 64; }

}  // namespace
}  // namespace mural

using namespace mural;

extern "C" int64_t mural_simulate_chunk_rows(void) { return SIM_CHUNK_ROWS; }
extern "C" int64_t mural_simulate_grid_waves(void) { return SIM_GRID_WAVES; }
extern "C" int32_t mural_simulate_scan_threads(void) { return SIM_SCAN_THREADS; }
extern "C" int32_t mural_simulate_max_replicates(void) { return SIM_MAX_REP; }

extern "C" size_t mural_simulate_annot_workspace_bytes(int64_t n_pieces) {
  return row_chunks_bytes(n_pieces);
}

extern "C" int mural_simulate_annot_rows(const MuralSimulateAnnotRows* s, void* ws_ptr, size_t ws_bytes, void* stream) {
  MURAL_REQUIRE(s, "simulate_annot_rows: NULL argument");
  MURAL_REQUIRE(s->n >= 0 && s->n_class >= 2 && s->n_class <= SIM_MAX_CLASS, "simulate_annot_rows: n >= 0 and 2 <= n_class <= %d required",
                SIM_MAX_CLASS);
  MURAL_REQUIRE(s->n_pieces >= 0 && s->n_groups >= 0, "simulate_annot_rows: n_pieces < 0 or n_groups < 0");
  MURAL_REQUIRE(s->n_rep >= 1 && s->n_rep <= SIM_MAX_REP, "simulate_annot_rows: 1 <= n_rep <= 2^20 required");
  if (s->n == 0) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->start && s->status, "simulate_annot_rows: NULL argument");
  MURAL_REQUIRE(s->prob_stride >= s->n_class, "simulate_annot_rows: prob_stride < n_class");
  const SimRows A = sim_rows(s->prob, s->prob_stride, s->start, s->strand, s->n_class, s->chrom_key, s->seed, s->status);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(SIM_THREADS);
  if (s->n_pieces > 0) {      // (everything is checked before the first launch)
    MURAL_REQUIRE(s->piece_b0 && s->piece_b1 && s->piece_group && s->n_groups >= 1 && s->table,
                  "simulate_annot_rows: pieces without groups or table");
    if (const int rc = check_workspace("simulate_annot_rows", "mural_simulate_annot_workspace_bytes", ws_ptr, ws_bytes,
                                       mural_simulate_annot_workspace_bytes(s->n_pieces)))
      return rc;
  }
  if (const int rc = launch_simulate_check(st, A, s->n, s->prob_f64, 1)) return rc;
  if (s->n_pieces == 0) return MURAL_OK;
  WsArena ws(ws_ptr);
  RowChunks w;
  if (const int rc = plan_row_chunks<SIM_THREADS, SIM_SCAN_THREADS>(st, s->start, s->n, s->piece_b0, s->piece_b1, s->piece_group, s->n_groups,
                                                                    s->n_pieces, 0, SIM_CHUNK_ROWS, ws, w))
    return rc;
  const int64_t n_waves = row_chunk_grid_waves(s->n, SIM_CHUNK_ROWS, (s->n_rep + 63) / 64, s->n_pieces, SIM_GRID_WAVES, SIM_WAVES);
  const dim3 draw_grid((unsigned)(n_waves / SIM_WAVES));
  if (s->prob_f64)
    hipLaunchKernelGGL(simulate_draw_kernel<double>, draw_grid, block, 0, st, A, s->piece_group, s->n_pieces, w.row0, w.row1, w.pre, s->n_rep,
                       n_waves, s->table);
  else
    hipLaunchKernelGGL(simulate_draw_kernel<float>, draw_grid, block, 0, st, A, s->piece_group, s->n_pieces, w.row0, w.row1, w.pre, s->n_rep,
                       n_waves, s->table);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" size_t mural_simulate_rows_workspace_bytes(int64_t n) {
  if (n <= 0) return 0;
  WsArena ws(nullptr);
  ws.as<int64_t>((size_t)tiles_of(n) + 1);
  return ws.off;
}

extern "C" int mural_simulate_rows(const MuralSimulateRows* s, void* ws_ptr, size_t ws_bytes, void* stream) {
  MURAL_REQUIRE(s, "simulate_rows: NULL argument");
  MURAL_REQUIRE(s->n >= 0 && s->n_class >= 2 && s->n_class <= SIM_MAX_CLASS, "simulate_rows: n >= 0 and 2 <= n_class <= %d required",
                SIM_MAX_CLASS);
  MURAL_REQUIRE(s->replicate >= 0 && s->replicate < SIM_MAX_REP, "simulate_rows: 0 <= replicate < 2^20 required");
  if (s->n == 0) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->start && s->status && s->out_start && s->out_strand && s->out_label && s->count, "simulate_rows: NULL argument");
  MURAL_REQUIRE(s->prob_stride >= s->n_class, "simulate_rows: prob_stride < n_class");
  if (const int rc = check_workspace("simulate_rows", "mural_simulate_rows_workspace_bytes", ws_ptr, ws_bytes,
                                     mural_simulate_rows_workspace_bytes(s->n)))
    return rc;
  const SimRows A = sim_rows(s->prob, s->prob_stride, s->start, s->strand, s->n_class, s->chrom_key, s->seed, s->status);
  const int64_t n_tiles = tiles_of(s->n);
  WsArena ws(ws_ptr);
  int64_t* pre = ws.as<int64_t>((size_t)n_tiles + 1);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(SIM_THREADS);
  const dim3 tile_grid((unsigned)((n_tiles + SIM_WAVES - 1) / SIM_WAVES));
  if (const int rc = launch_simulate_check(st, A, s->n, s->prob_f64, 0)) return rc;      // (a list's rows need not ascend)
  if (s->prob_f64)
    hipLaunchKernelGGL(simulate_count_kernel<double>, tile_grid, block, 0, st, A, s->n, s->replicate, n_tiles, pre);
  else
    hipLaunchKernelGGL(simulate_count_kernel<float>, tile_grid, block, 0, st, A, s->n, s->replicate, n_tiles, pre);
  MURAL_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(excl_scan_kernel<SIM_SCAN_THREADS>, dim3(1), dim3(SIM_SCAN_THREADS), 0, st, pre, n_tiles, s->count);
  MURAL_HIP_CHECK(hipGetLastError());
  if (s->prob_f64)
    hipLaunchKernelGGL(simulate_write_kernel<double>, tile_grid, block, 0, st, A, s->n, s->replicate, n_tiles, pre, s->out_start, s->out_strand,
                       s->out_label);
  else
    hipLaunchKernelGGL(simulate_write_kernel<float>, tile_grid, block, 0, st, A, s->n, s->replicate, n_tiles, pre, s->out_start, s->out_strand,
                       s->out_label);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}
