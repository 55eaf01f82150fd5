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
//   * draw kernel: simulate_draw.h's draw_count_units() (the units, the walk of a chunk, the counts and their atomics) around this
//     file's policy: items = the pieces, owners = their groups, a unit = a chunk and ONE block of 64 replicates; every row has the same
//     word, whose field c holds c, so that the bin is the drawn class minus one; an accumulator per class,
//     table[(g * (n_class - 1) + c - 1) * n_rep + r].
// mural_simulate_rows: tile counts of the non-zero labels of one replicate (a wave per 64 rows), their exclusive scan, and a second pass
// that recomputes the labels and writes each hit at prefix + its rank among the tile's hits: stable in row order.
// No floating-point atomics, no synchronisation, no read-back.  The check kernel, the Philox round, a row's cum, the last counter word
// and the draw-and-count loop live in simulate_draw.h, with the loop bounds; the per-transcript simulations include it as well.
#include "common.h"
#include "kmer_key.h"
#include "row_chunks.h"
#include "simulate_draw.h"

namespace mural {
namespace {

struct AnnotDraw {
  using Word = uint32_t;
  static constexpr int BITS = 4, BOUNDS = SIM_MAX_CLASS - 1, ACCS = SIM_MAX_CLASS - 1, UNIT_BLOCKS = 1;      // (no row words to amortise)
  static constexpr bool ROW_WORDS = false;
  static constexpr Word WORD = 0x76543210u;      // field c: c -- the field beside the last class is a bin that is not present
  const int32_t* group;
  int n_class;
  int32_t g;

  __device__ __forceinline__ bool begin_unit(int64_t p) {
    g = group[p];
    return true;
  }
  __device__ __forceinline__ uint32_t present() const { return (1u << (n_class - 1)) - 1; }
  __device__ __forceinline__ int cell(int b) const { return b; }
  __device__ __forceinline__ int32_t owner() const { return g; }
  __device__ __forceinline__ int bins() const { return n_class - 1; }
};

template <typename T>
__global__ __launch_bounds__(SIM_THREADS) void simulate_draw_kernel(SimDraw D, const int32_t* group) {
  AnnotDraw pol{group, D.rows.n_class};
  draw_count_units<T>(D, pol, nullptr);
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
  if (s->n_pieces > 0) {      // (everything is checked before the first launch)
    MURAL_REQUIRE(s->piece_b0 && s->piece_b1 && s->piece_group && s->n_groups >= 1 && s->table,
                  "simulate_annot_rows: pieces without groups or table");
    if (const int rc = check_workspace("simulate_annot_rows", "mural_simulate_annot_workspace_bytes", ws_ptr, ws_bytes,
                                       mural_simulate_annot_workspace_bytes(s->n_pieces)))
      return rc;
  }
  if (const int rc = launch_simulate_check(st, A, s->n, s->prob_f64, 1)) return rc;
  if (s->n_pieces == 0) return MURAL_OK;
  SimDraw D{};
  D.rows = A, D.n_items = s->n_pieces, D.n_rep = s->n_rep, D.table = s->table;
  return launch_draw_count(st, D, s->prob_f64, s->n, s->piece_b0, s->piece_b1, s->piece_group, s->n_groups, 0, AnnotDraw::UNIT_BLOCKS, ws_ptr,
                           simulate_draw_kernel<float>, simulate_draw_kernel<double>, s->piece_group);
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
