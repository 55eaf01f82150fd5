// The stateless draw of the simulation kernels, shared by csrc/simulate.hip (counts per named interval set, mutation lists),
// csrc/simulate_conseq.hip, csrc/simulate_txstruct.hip and csrc/simulate_txindel.hip (counts per transcript and bin) so that their draws
// cannot drift: the rows' argument block, the check kernel (the status bits of every row), the Philox4x32-10 round, a row's cumulative
// class bounds and the last counter word, with the loop bounds all four files plan their launches on -- and draw_count_units(), the ONE
// loop of the table kernels of simulate.hip, simulate_conseq.hip and simulate_txstruct.hip: which replicate reads which output word of
// which counter, how a draw becomes a bin, where the count of a (bin, replicate) is kept and how it reaches the table.  Such a kernel is
// a policy (its packed row words and its bins) around that loop, and launch_draw_count() is its plan and launch.  simulate_txindel.hip
// keeps a copy of the loop (DESIGN.md section 3.26 says why).
// summaries.simulate_rows_host is the specification; DESIGN.md section 3.20.
#pragma once
#include "common.h"
#include "kmer_key.h"
#include "row_chunks.h"

namespace mural {

constexpr int SIM_MAX_CLASS = 8;
constexpr int SIM_THREADS = 256;
constexpr int SIM_WAVES = SIM_THREADS / 64;
constexpr int SIM_SCAN_THREADS = 1024;
constexpr int64_t SIM_CHUNK_ROWS = 1024;          // rows of one unit of the draw kernels: 16 tiles of 64
constexpr int64_t SIM_GRID_WAVES = 8192;          // waves of the draw kernels' grid; they stride over the units
constexpr int32_t SIM_MAX_REP = 1 << 20;
constexpr u64 SIM_ONE = 1ull << 32;
constexpr int SIM_TILES = (int)(SIM_CHUNK_ROWS / 64);      // tiles of a chunk
constexpr int SIM_UNIT_BLOCKS = 16;               // blocks of 64 replicates of one unit of the per-transcript kernels
constexpr int64_t SIM_TX_MAX_ROWS = 1ll << 31;    // per call of a per-transcript entry, as the mural_summary_*_rows entries
constexpr int64_t SIM_TX_MAX_ITEMS = 1ll << 22;   // items, and CDS segments, of such a call

struct SimRows {
  const void* prob;
  const int64_t* start;
  const uint8_t* strand;      // or nullptr: all '+'
  int64_t prob_stride;
  int32_t n_class;
  uint32_t chrom_key, seed_lo, seed_hi;
  int32_t* status;
};

inline SimRows sim_rows(const void* prob, int64_t prob_stride, const int64_t* start, const uint8_t* strand, int32_t n_class,
                        uint32_t chrom_key, uint64_t seed, int32_t* status) {
  SimRows A{};
  A.prob = prob, A.start = start, A.strand = strand, A.prob_stride = prob_stride, A.n_class = n_class;
  A.chrom_key = chrom_key, A.seed_lo = (uint32_t)seed, A.seed_hi = (uint32_t)(seed >> 32), A.status = status;
  return A;
}

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// cum[c - 1] of row i for c = 1 .. n_class - 1 (0 beyond, and 0 everywhere for a bad row); returns the row's status bits
template <typename T>
__device__ __forceinline__ int32_t row_cum(const SimRows& A, int64_t i, u64 (&cum)[SIM_MAX_CLASS - 1]) {
  const T* __restrict__ p_row = static_cast<const T*>(A.prob) + i * A.prob_stride;
  int32_t bad = A.start[i] < 0 ? (int32_t)SM_BAD_START : 0;
  u64 run = 0;
#pragma unroll
  for (int c = 1; c < SIM_MAX_CLASS; ++c) {
    cum[c - 1] = 0;
    if (c < A.n_class) {
      const double p = (double)p_row[c];      // (float -> double is exact)
      // finite and not negative, on the bit pattern -- non-negative doubles order like their bits --, so that NaN is caught whatever
      // the compiler assumes about comparisons; -0.0 counts as 0
      const u64 bits = (u64)__double_as_longlong(p);
      if (bits >= 0x7FF0000000000000ull && bits != 0x8000000000000000ull) {
        bad |= SM_BAD_PROB;
      } else {
        double s = p * 4294967296.0;          // exact: a power of two
        if (s > 4294967296.0) s = 4294967296.0;
        run += (u64)(long long)floor(s);
        cum[c - 1] = run < SIM_ONE ? run : SIM_ONE;
      }
    }
  }
  if (bad) {
#pragma unroll
    for (int c = 0; c < SIM_MAX_CLASS - 1; ++c) cum[c] = 0;
  }
  return bad;
}

// a thread per row: the status bits (a bad probability, a negative start and, with check_order, a start below the row before it)
template <typename T>
__global__ __launch_bounds__(SIM_THREADS) void simulate_check_kernel(SimRows A, int64_t n, int check_order) {
  const int64_t i = (int64_t)blockIdx.x * SIM_THREADS + threadIdx.x;
  int32_t bad = 0;
  if (i < n) {
    u64 cum[SIM_MAX_CLASS - 1];
    bad = row_cum<T>(A, i, cum);
    if (check_order && i > 0 && A.start[i] < A.start[i - 1]) bad |= SM_BAD_ORDER;
  }
  if (bad) atomicOr(A.status, bad);
}

// the check kernel on `st`; MURAL_OK or the error code of the launch
inline int launch_simulate_check(hipStream_t st, const SimRows& A, int64_t n, bool prob_f64, int check_order) {
  const dim3 grid((unsigned)((n + SIM_THREADS - 1) / SIM_THREADS)), block(SIM_THREADS);
  if (prob_f64)
    hipLaunchKernelGGL(simulate_check_kernel<double>, grid, block, 0, st, A, n, check_order);
  else
    hipLaunchKernelGGL(simulate_check_kernel<float>, grid, block, 0, st, A, n, check_order);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

__device__ __forceinline__ uint32_t last_counter_word(const SimRows& A, int64_t i, uint32_t block) {
  return block | ((A.strand != nullptr && A.strand[i] != 0) ? 0x80000000u : 0u);
}

// ---- the draw-and-count loop of the table kernels ---------------------------------------------------------------------------------------
// What a draw kernel gets beside its policy's arguments: the rows, the plan of their items (row_chunks.h) and the table.
struct SimDraw {
  SimRows rows;
  const int64_t* row0;
  const int64_t* row1;
  const int64_t* pre;
  int64_t n_items, n_waves;
  int32_t n_rep;
  uint32_t* table;      // [owners][bins][n_rep]
};

// the word of a policy whose fields 0 .. BOUNDS all hold "nowhere": a lane without a counted row
template <typename P>
constexpr typename P::Word sim_dead_word() {
  uint32_t w = 0;
  for (int c = 0; c <= P::BOUNDS; ++c) w |= (uint32_t)P::NOWHERE << (P::BITS * c);
  return (typename P::Word)w;
}

// A wave strides over the units (chunk of an item, group of up to UNIT_BLOCKS blocks of 64 replicates).  Every row has a packed WORD of
// BITS-wide fields: field c - 1 is the bin of class c, the field after the last class is "nowhere".  With ROW_WORDS the wave first walks
// its chunk 64 rows at a time, a row per lane, and forms each row's word ONCE per unit (row_word: codon lookups, a deletion's walk) into
// `words`, the wave's own [SIM_TILES][64] of LDS, where only the lane that wrote a word reads it back: no barrier.  Then per replicate
// block it walks the chunk again: the lane's cum (row_cum; the classes that do not exist get the bound 2^32, above every u) and per
// Philox call of four replicates -- counter word `last | (rb * 16 + j)`, replicate rb * 64 + 4 j + k reads output word k -- the number
// of bounds not above u, which for an ascending cum is the index of the drawn class's field and of "nowhere" where no class is drawn;
// per accumulator b of the wave-uniform `present` mask popc(ballot(bin == b)) is added in the lane that owns the replicate (lane
// 4 j + k; the accumulators are indexed by unrolled constants only).  After the chunk ONE wave-instruction per accumulator adds the 64
// counts -- 256 contiguous bytes -- with 32-bit INTEGER atomics at table[(owner * bins + cell(b)) * n_rep + rb * 64 + lane], zero
// counts skipped.  Draws and bins are recomputed, never stored in memory; no floating-point atomics, no synchronisation, no read-back.
//
// The policy P: Word, BITS, BOUNDS (the bounds compared: classes - 1), ACCS (accumulators), NOWHERE, UNIT_BLOCKS, ROW_WORDS (false:
// every row has the word P::WORD and `words` is not read); begin_unit(item): the wave-uniform context of the item, false to skip the
// unit; row_word(i, q): the word of row i at start q, sim_dead_word where it is not counted; present(); cell(b): the table's bin of
// accumulator b, negative where it has none; owner(); bins().
template <typename T, typename P>
__device__ __forceinline__ void draw_count_units(const SimDraw& D, P& pol, typename P::Word (*words)[64]) {
  static_assert(P::BOUNDS < SIM_MAX_CLASS && (P::BOUNDS + 1) * P::BITS <= 8 * (int)sizeof(typename P::Word), "a field per bound, and one");
  static_assert(P::ACCS <= 32 && P::ACCS <= (1 << P::BITS), "an accumulator per value of a field at the most");
  const SimRows& A = D.rows;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * SIM_WAVES + (threadIdx.x >> 6);
  const int n_rep = D.n_rep, nc = A.n_class;
  const int n_rb = (n_rep + 63) / 64;
  const int64_t n_rg = (n_rb + P::UNIT_BLOCKS - 1) / P::UNIT_BLOCKS;
  const int64_t units = D.pre[D.n_items] * n_rg;
  for (int64_t unit = wave; unit < units; unit += D.n_waves) {
    const int64_t t = unit / n_rg;
    const int rg = (int)(unit % n_rg);
    const int64_t item = row_chunk_item(D.pre, D.n_items, t);
    const int64_t r0 = D.row0[item] + (t - D.pre[item]) * SIM_CHUNK_ROWS;
    const int64_t r1 = min(r0 + SIM_CHUNK_ROWS, D.row1[item]);
    if (!pol.begin_unit(item)) continue;
    if constexpr (P::ROW_WORDS) {
      static_assert((int)P::NOWHERE >= P::ACCS && (int)P::NOWHERE < (1 << P::BITS), "nowhere is a field's value and no accumulator");
      int tile = 0;
      for (int64_t row = r0; row < r1; row += 64, ++tile) {      // (at most SIM_TILES tiles: r1 - r0 <= SIM_CHUNK_ROWS)
        const int64_t i = row + lane;
        words[tile][lane] = i < r1 ? pol.row_word(i, A.start[i]) : sim_dead_word<P>();
      }
    }
    const uint32_t present = pol.present();      // wave-uniform
    if (!present) continue;
    const int rb_end = min(n_rb, (rg + 1) * P::UNIT_BLOCKS);
    for (int rb = rg * P::UNIT_BLOCKS; rb < rb_end; ++rb) {
      const int reps_here = min(64, n_rep - rb * 64);
      const int n_blocks = (reps_here + 3) / 4;
      uint32_t acc[P::ACCS];
#pragma unroll
      for (int b = 0; b < P::ACCS; ++b) acc[b] = 0;
      int tile = 0;
      for (int64_t row = r0; row < r1; row += 64, ++tile) {
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
#pragma unroll
        for (int c = 0; c < P::BOUNDS; ++c)
          if (c >= nc - 1) cum[c] = SIM_ONE;      // (wave-uniform) above every u: the classes that do not exist are never passed
        uint32_t word;
        if constexpr (P::ROW_WORDS) word = words[tile][lane];
        else word = P::WORD;
        for (int j = 0; j < n_blocks; ++j) {
          uint32_t u[4];
          philox4x32_10(s_lo, s_hi, A.chrom_key, last | (uint32_t)(rb * 16 + j), A.seed_lo, A.seed_hi, u);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const u64 mine_u = u[k];
            uint32_t below = 0;      // cum ascends: the bounds not above u are those of the classes before the drawn one
#pragma unroll
            for (int c = 0; c < P::BOUNDS; ++c) below += mine_u >= cum[c] ? 1u : 0u;
            const uint32_t bin = (word >> (P::BITS * below)) & ((1u << P::BITS) - 1);
#pragma unroll
            for (int b = 0; b < P::ACCS; ++b) {
              if ((present >> b) & 1u) {      // (scalar)
                const uint32_t hits = (uint32_t)__popcll(__ballot(bin == (uint32_t)b));
                if (lane == j * 4 + k) acc[b] += hits;
              }
            }
          }
        }
      }
      if (lane < reps_here) {
        const int64_t owner = pol.owner();
#pragma unroll
        for (int b = 0; b < P::ACCS; ++b) {
          const int cell = pol.cell(b);
          if (((present >> b) & 1u) && cell >= 0 && acc[b])
            atomicAdd(&D.table[(owner * pol.bins() + cell) * n_rep + rb * 64 + lane], acc[b]);
        }
      }
    }
  }
}

// The plan of the items' rows (plan_row_chunks: an item's rows are those with b0 <= start + shift < b1) and the draw kernel over it on
// `st`, `kernel_f32` or `kernel_f64` by the rows' type.  D holds the rows, n_items > 0, n_rep and the table; the plan and the grid are
// filled in here.  MURAL_OK or the error code of a launch.
template <typename Args>
inline int launch_draw_count(hipStream_t st, SimDraw D, bool prob_f64, int64_t n, const int64_t* b0, const int64_t* b1, const int32_t* owner,
                             int32_t n_owners, int64_t shift, int unit_blocks, void* ws_ptr, void (*kernel_f32)(SimDraw, Args),
                             void (*kernel_f64)(SimDraw, Args), const Args& args) {
  WsArena ws(ws_ptr);
  RowChunks w;
  if (const int rc = plan_row_chunks<SIM_THREADS, SIM_SCAN_THREADS>(st, D.rows.start, n, b0, b1, owner, n_owners, D.n_items, shift,
                                                                    SIM_CHUNK_ROWS, ws, w))
    return rc;
  const int64_t n_rg = ((D.n_rep + 63) / 64 + unit_blocks - 1) / unit_blocks;
  D.row0 = w.row0, D.row1 = w.row1, D.pre = w.pre;
  D.n_waves = row_chunk_grid_waves(n, SIM_CHUNK_ROWS, n_rg, D.n_items, SIM_GRID_WAVES, SIM_WAVES);
  void (*const kernel)(SimDraw, Args) = prob_f64 ? kernel_f64 : kernel_f32;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(D.n_waves / SIM_WAVES)), dim3(SIM_THREADS), 0, st, D, args);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

// the bounds the per-transcript entries share, under the entry's name (an entry without items of its own passes n_features = 0)
inline int check_sim_tx_bounds(const char* entry, int32_t n_rep, int64_t n, int64_t n_features, int64_t n_segments, int32_t n_transcripts) {
  MURAL_REQUIRE(n_rep >= 1 && n_rep <= SIM_MAX_REP, "%s: 1 <= n_rep <= 2^20 required", entry);
  MURAL_REQUIRE(n >= 0 && n <= SIM_TX_MAX_ROWS, "%s: 0 <= n <= 2^31 required", entry);
  MURAL_REQUIRE(n_features >= 0 && n_features <= SIM_TX_MAX_ITEMS, "%s: 0 <= n_features <= 2^22 required", entry);
  MURAL_REQUIRE(n_segments >= 0 && n_segments <= SIM_TX_MAX_ITEMS, "%s: 0 <= n_segments <= 2^22 required", entry);
  MURAL_REQUIRE(n_transcripts >= 0, "%s: n_transcripts < 0", entry);
  return MURAL_OK;
}

}  // namespace mural
