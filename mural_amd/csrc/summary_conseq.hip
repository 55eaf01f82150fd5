// Expected and observed mutations per transcript by consequence while a prediction shard is on the device (mural_amd/summaries.py:
// SummarySink(transcripts=...); tables.consequence_table from a written table): per transcript of a BED12 file the label counts and the
// sums of the probabilities of the SNV rows inside its CDS, split by what each of a row's three substitutions does to the codon it falls
// in -- synonymous, missense, stop gained, stop lost, or unresolved (an incomplete or masked codon).  summaries.summary_conseq_host is
// the specification; DESIGN.md section 3.21.
//
// The host (tables.read_transcripts) turns every transcript into its CDS SEGMENTS [b0, b1) with the CDS offset of the segment's first
// base in transcript orientation and the indices of the transcript's neighbouring segments; transcripts overlap and nest freely, so a
// per-row stabbing query is unbounded, and a row's bin depends on the transcript, so row prefix sums do not apply.  The rows of a part
// ascend in start, so the rows of a segment are ONE range [i0, i1); the work is cut per segment, as csrc/simulate.hip cuts it per piece:
//   * check kernel, a thread per row: the status bits;
//   * range kernel, a wave per segment: [i0, i1) by two 64-ary searches in start, and the number of CHUNKS of at most SC_CHUNK_ROWS rows;
//   * scan kernel, one workgroup: the exclusive prefix of the chunk counts;
//   * reduce kernel, a grid of at most SC_GRID_WAVES waves striding over the chunks: the wave finds the chunk's segment by a 64-ary
//     search in the prefix and walks the chunk 64 rows at a time, a row per lane: the row's CDS offset, its codon's three genomic
//     positions (at most two hops over seg_prev / seg_next each: exons may be 1 bp long), the two amino acids from a 64-byte table in
//     LDS, a bin per class.  The limbs (summary_quant.h: q = rne(p * 2^71) as hi, lo) add up per lane and bin over the chunk, the label
//     counts per bin by ballot + popcount; after the chunk 10 wave butterflies, the fold of lo into hi, and ONE wave-instruction of
//     64-bit INTEGER atomics over the transcript's 15 contiguous cells + its two row counters, zero words skipped;
//   * fold kernel, a thread per (transcript, bin), no atomics: the overflow of the table's lo limbs into hi.
// Bounds.  A lane adds at most 3 limbs below 2^40 per row and SC_CHUNK_ROWS / 64 = 16 rows per chunk: below 2^46 per lane, below 2^52
// per wave before the fold.  A chunk adds lo < 2^40 to a cell; the segments of one transcript are disjoint, so one call adds at most
// n / SC_CHUNK_ROWS + n_segments chunks to a cell; the entry refuses n > 2^31 or n_segments > 2^22, so lo < 2^40 (1 + 2^21 + 2^22) < 2^63
// before the fold that ends every call, and lo < 2^40 on return.
// No per-row bin is stored (the check and the reduce kernel both recompute a row); no floating-point atomics, no synchronisation, no
// read-back.
#include "common.h"
#include "kmer_key.h"
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
constexpr int SC_BINS = 5;                        // synonymous, missense, stop gained, stop lost, unresolved
constexpr int SC_CELL_WORDS = 3 * SC_BINS;        // per transcript: [bin][label count | sum of hi | sum of lo]
constexpr int SC_NOWHERE = SC_BINS;               // the bin of a class that is not counted
constexpr u64 SC_LO_MASK = (1ull << SK_LO_BITS) - 1;

struct ConseqArgs {
  MuralGenome g;
  const void* prob;
  const int64_t* start;
  const uint8_t* strand;      // or nullptr: all '+'
  const void* label;
  int64_t prob_stride, n;
  int32_t label_kind, n_tx;
  const int64_t* seg_b0;
  const int64_t* seg_b1;
  const int64_t* seg_cds0;
  const int32_t* seg_tx;
  const int32_t* seg_prev;
  const int32_t* seg_next;
  int64_t n_seg;
  const uint8_t* tx_strand;
  const int64_t* tx_cds_len;
  uint32_t aa_w[16];          // the 64 amino-acid bytes, four to a word
  uint32_t alt_packed;        // alt_order[r][j] in bits [2 (3 r + j), +2)
  u64* table;
  u64* rows;
  int32_t* status;
};

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// first index of [lo, hi) where pred fails, the whole wave searching; pred holds on a prefix of the range.  A probe per lane splits the
// range 64 ways a round; the range shrinks every round whatever the data hold, and no probe leaves it.
template <typename Pred>
__device__ __forceinline__ int64_t wave_partition_point(int64_t lo, int64_t hi, Pred pred) {
  const int lane = threadIdx.x & 63;
  while (lo < hi) {
    const int64_t step = (hi - lo + 63) / 64;
    const int64_t p = lo + lane * step;
    const int holds = __popcll(__ballot(p < hi && pred(p)));
    if (holds == 0) {
      hi = lo;
    } else {
      hi = min(hi, lo + holds * step);
      lo = lo + (holds - 1) * step + 1;
    }
  }
  return lo;
}

// The checks of row i (status bits, 0 if it counts) and the limbs of its classes 1 .. 3; class 0's probability is not read.
template <typename T>
__device__ __forceinline__ int32_t conseq_row(const ConseqArgs& A, int64_t i, int& lab, u64 (&hi)[3], u64 (&lo)[3]) {
  const T* __restrict__ p_row = static_cast<const T*>(A.prob) + i * A.prob_stride;
  lab = load_label(A.label, A.label_kind, i);
  int32_t bad = 0;
  if (A.start[i] < 0) bad |= SM_BAD_START;
  if (lab < 0 || lab >= 4) bad |= SM_BAD_LABEL;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (!quantise_prob((double)p_row[c + 1], hi[c], lo[c])) bad |= SM_BAD_PROB;      // (float -> double is exact)
  return bad;
}

template <typename T>
__global__ __launch_bounds__(SC_THREADS) void summary_conseq_check_kernel(ConseqArgs A) {
  const int64_t i = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
  int32_t bad = 0;
  if (i < A.n) {
    int lab;
    u64 hi[3], lo[3];
    bad = conseq_row<T>(A, i, lab, hi, lo);
    if (i > 0 && A.start[i] < A.start[i - 1]) bad |= SM_BAD_ORDER;
  }
  if (bad) atomicOr(A.status, bad);
}

// a wave per segment: its rows [i0, i1) and its chunk count; a segment that is empty or names no transcript has none
__global__ __launch_bounds__(SC_THREADS) void summary_conseq_range_kernel(ConseqArgs A, int64_t* __restrict__ row0, int64_t* __restrict__ row1,
                                                                          int64_t* __restrict__ pre) {
  const int64_t s = (int64_t)blockIdx.x * SC_WAVES + (threadIdx.x >> 6);
  if (s >= A.n_seg) return;
  const int32_t tx = A.seg_tx[s];
  const int64_t b0 = A.seg_b0[s], b1 = A.seg_b1[s];
  int64_t i0 = 0, i1 = 0;
  if (tx >= 0 && tx < A.n_tx && b0 < b1) {
    const int64_t* __restrict__ start = A.start;
    i0 = wave_partition_point(0, A.n, [&](int64_t i) { return start[i] < b0; });
    i1 = wave_partition_point(i0, A.n, [&](int64_t i) { return start[i] < b1; });
  }
  if ((threadIdx.x & 63) == 0) {
    row0[s] = i0, row1[s] = i1;
    pre[s] = (i1 - i0 + SC_CHUNK_ROWS - 1) / SC_CHUNK_ROWS;
  }
}

// exclusive prefix of v[0 .. m - 1] in place, v[m] = the total: one workgroup, a thread owns a run
__global__ __launch_bounds__(SC_SCAN_THREADS) void summary_conseq_scan_kernel(int64_t* __restrict__ v, int64_t m) {
  __shared__ int64_t wave_tot[SC_SCAN_THREADS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t run = (m + SC_SCAN_THREADS - 1) / SC_SCAN_THREADS;
  const int64_t t0 = min((int64_t)threadIdx.x * run, m), t1 = min(t0 + run, m);
  int64_t mine = 0;
  for (int64_t t = t0; t < t1; ++t) mine += v[t];
  int64_t incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  if (lane == 63) wave_tot[w] = incl;
  __syncthreads();
  int64_t base = 0, total = 0;
#pragma unroll
  for (int k = 0; k < SC_SCAN_THREADS / 64; ++k) {
    base += k < w ? wave_tot[k] : 0;
    total += wave_tot[k];
  }
  int64_t running = base + incl - mine;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t x = v[t];
    v[t] = running;
    running += x;
  }
  if (threadIdx.x == 0) v[m] = total;
}

// The codon (16 b0 + 4 b1 + b2, read 5' -> 3' on the transcript's strand) that holds CDS offsets cs .. cs + 2 of the transcript of
// segment s, or -1 where a position is not found within two hops, lies outside the record or is masked.  Every index is checked
// before it is used.
__device__ __forceinline__ int conseq_codon(const ConseqArgs& A, int64_t s, int32_t tx, bool minus, int64_t cs) {
  int codon = 0;
  bool found = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int64_t o = cs + j;
    int64_t cur = s;
#pragma unroll
    for (int hop = 0; hop < 2; ++hop) {
      const int64_t c0 = A.seg_cds0[cur], len = A.seg_b1[cur] - A.seg_b0[cur];
      int64_t nx = cur;
      if (o < c0) nx = A.seg_prev[cur];
      else if (o >= c0 + len) nx = A.seg_next[cur];
      if (nx < 0 || nx >= A.n_seg) {
        found = false;
        nx = cur;
      }
      cur = nx;
    }
    const int64_t c0 = A.seg_cds0[cur], sb0 = A.seg_b0[cur], sb1 = A.seg_b1[cur];
    found = found && o >= c0 && o < c0 + (sb1 - sb0) && A.seg_tx[cur] == tx;
    const int64_t pos = minus ? sb1 - 1 - (o - c0) : sb0 + (o - c0);
    int32_t code = 0;
    if (found && pos >= 0 && pos < A.g.length) {
      bool masked = false;
      code = kmer_base(A.g, pos, masked);
      found = !masked;
    } else {
      found = false;
    }
    codon = codon * 4 + (minus ? 3 - code : code);
  }
  return found ? codon : -1;
}

template <typename T>
__global__ __launch_bounds__(SC_THREADS) void summary_conseq_reduce_kernel(ConseqArgs A, const int64_t* __restrict__ row0,
                                                                           const int64_t* __restrict__ row1, const int64_t* __restrict__ pre,
                                                                           int64_t n_waves) {
  __shared__ uint32_t aa_words[16];
#pragma unroll
  for (int j = 0; j < 16; ++j)      // (constant indices: the words stay scalar arguments)
    if (threadIdx.x == j) aa_words[j] = A.aa_w[j];
  __syncthreads();
  const uint8_t* aa = reinterpret_cast<const uint8_t*>(aa_words);
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * SC_WAVES + (threadIdx.x >> 6);
  const int64_t units = pre[A.n_seg];
  for (int64_t unit = wave; unit < units; unit += n_waves) {
    // the segment of chunk `unit`: the last s with pre[s] <= unit (pre[n_seg] = the total > unit, so the point lies in 1 .. n_seg)
    const int64_t s = wave_partition_point(0, A.n_seg + 1, [&](int64_t q) { return pre[q] <= unit; }) - 1;
    const int64_t r0 = row0[s] + (unit - pre[s]) * SC_CHUNK_ROWS;
    const int64_t r1 = min(r0 + SC_CHUNK_ROWS, row1[s]);
    const int64_t b0 = A.seg_b0[s], b1 = A.seg_b1[s], cds0 = A.seg_cds0[s];
    const int32_t tx = A.seg_tx[s];      // (0 <= tx < n_tx: the range kernel gave other segments no chunk)
    const bool minus = A.tx_strand[tx] != 0;
    const int64_t cds_len = A.tx_cds_len[tx];
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
        const int64_t q = A.start[i];
        // (the status is the check kernel's; q lies in [b0, b1) unless the rows do not ascend: then the row is skipped here)
        live = conseq_row<T>(A, i, lab, hi, lo) == 0 && q >= b0 && q < b1;
        if (live) {
          const int64_t x = cds0 + (minus ? b1 - 1 - q : q - b0);
          const int64_t cs = x - x % 3;
          const int codon = (x >= 0 && cs + 2 < cds_len) ? conseq_codon(A, s, tx, minus, cs) : -1;
          if (codon < 0) {
            bins[0] = bins[1] = bins[2] = SC_BINS - 1;
          } else {
            const int sh = 2 * (2 - (int)(x - cs));
            const int own_tx = (codon >> sh) & 3;                       // the base at q, on the transcript's strand
            const bool row_minus = A.strand != nullptr && A.strand[i] != 0;
            const int r = (minus != row_minus) ? 3 - own_tx : own_tx;   // the row's own base
            const uint8_t aa_ref = aa[codon];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const int alt = (int)(A.alt_packed >> (2 * (3 * r + c))) & 3;      // on the row's strand
              const int alt_tx = (minus != row_minus) ? 3 - alt : alt;
              const uint8_t aa_alt = aa[(codon & ~(3 << sh)) | (alt_tx << sh)];
              bins[c] = aa_ref == aa_alt ? 0 : aa_alt == '*' ? 2 : aa_ref == '*' ? 3 : 1;
            }
          }
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
      const u64 l = wave_sum(acc_lo[b]);
      const u64 h = wave_sum(acc_hi[b]) + (l >> SK_LO_BITS);
      if (lane == 3 * b) word = cnt[b];
      if (lane == 3 * b + 1) word = h;
      if (lane == 3 * b + 2) word = l & SC_LO_MASK;
    }
    if (lane == SC_CELL_WORDS) word = n_rows;
    if (lane == SC_CELL_WORDS + 1) word = n_lab0;
    if (word) {      // (0 in the lanes from 17 on)
      if (lane < SC_CELL_WORDS) atomicAdd(&A.table[(int64_t)tx * SC_CELL_WORDS + lane], word);
      else atomicAdd(&A.rows[(int64_t)tx * 2 + (lane - SC_CELL_WORDS)], word);
    }
  }
}

// carry the overflow of the table's lo limbs into its hi limbs: a thread per (transcript, bin), plain loads and stores
__global__ __launch_bounds__(SC_THREADS) void summary_conseq_fold_kernel(u64* __restrict__ table, int64_t n_cells) {
  const int64_t t = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
  if (t >= n_cells) return;
  u64* __restrict__ cell = table + t * 3;
  const u64 lo = cell[2];
  if (lo >> SK_LO_BITS) {
    cell[1] += lo >> SK_LO_BITS;
    cell[2] = lo & SC_LO_MASK;
  }
}

struct ConseqWs { int64_t *row0, *row1, *pre; };
ConseqWs carve(WsArena& ws, int64_t n_seg) {
  ConseqWs w;
  w.row0 = ws.as<int64_t>((size_t)n_seg);
  w.row1 = ws.as<int64_t>((size_t)n_seg);
  w.pre = ws.as<int64_t>((size_t)n_seg + 1);
  return w;
}

}  // namespace
}  // namespace mural

using namespace mural;

extern "C" int64_t mural_summary_conseq_chunk_rows(void) { return SC_CHUNK_ROWS; }
extern "C" int64_t mural_summary_conseq_grid_waves(void) { return SC_GRID_WAVES; }
extern "C" int32_t mural_summary_conseq_scan_threads(void) { return SC_SCAN_THREADS; }

extern "C" size_t mural_summary_conseq_workspace_bytes(int64_t n_segments) {
  if (n_segments <= 0) return 0;
  WsArena ws(nullptr);
  carve(ws, n_segments);
  return ws.off;
}

extern "C" int mural_summary_conseq_rows(const MuralSummaryConseqRows* s, void* ws_ptr, size_t ws_bytes, void* stream) {
  MURAL_REQUIRE(s, "summary_conseq_rows: NULL argument");
  MURAL_REQUIRE(s->n_class == 4, "summary_conseq_rows: SNV rows of 4 classes required (n_class = %d)", s->n_class);
  MURAL_REQUIRE(s->n >= 0 && s->n <= SC_MAX_ROWS, "summary_conseq_rows: 0 <= n <= 2^31 required");
  MURAL_REQUIRE(s->n_segments >= 0 && s->n_segments <= SC_MAX_SEGMENTS, "summary_conseq_rows: 0 <= n_segments <= 2^22 required");
  MURAL_REQUIRE(s->n_transcripts >= 0, "summary_conseq_rows: n_transcripts < 0");
  MURAL_REQUIRE(s->label_kind >= 0 && s->label_kind <= 2, "summary_conseq_rows: label_kind is 0 (float32), 1 (int32) or 2 (int64)");
  uint32_t alt_packed = 0;
  for (int r = 0; r < 4; ++r) {
    unsigned seen = 1u << r;
    for (int j = 0; j < 3; ++j) {
      const unsigned a = s->alt_order[r][j];
      MURAL_REQUIRE(a < 4 && !(seen & (1u << a)), "summary_conseq_rows: alt_order[%d] must name the three other bases once each", r);
      seen |= 1u << a;
      alt_packed |= a << (2 * (3 * r + j));
    }
  }
  if (s->n == 0 || s->n_segments == 0) return MURAL_OK;
  MURAL_REQUIRE(s->genome && s->genome->packed2 && s->genome->nmask && s->genome->length >= 0, "summary_conseq_rows: empty genome");
  MURAL_REQUIRE(s->prob && s->start && s->label && s->status && s->table && s->rows, "summary_conseq_rows: NULL argument");
  MURAL_REQUIRE(s->seg_b0 && s->seg_b1 && s->seg_cds0 && s->seg_tx && s->seg_prev && s->seg_next && s->tx_strand && s->tx_cds_len &&
                    s->n_transcripts >= 1,
                "summary_conseq_rows: segments without transcripts");
  MURAL_REQUIRE(s->prob_stride >= 4, "summary_conseq_rows: prob_stride < n_class");
  const size_t need = mural_summary_conseq_workspace_bytes(s->n_segments);
  if (!ws_ptr || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws_ptr) & 7) != 0) {
    set_error("summary_conseq_rows: the workspace is NULL, misaligned or smaller than mural_summary_conseq_workspace_bytes (%zu)", need);
    return MURAL_E_WORKSPACE;
  }
  ConseqArgs A{};
  A.g = *s->genome;
  A.prob = s->prob, A.start = s->start, A.strand = s->strand, A.label = s->label, A.prob_stride = s->prob_stride, A.n = s->n;
  A.label_kind = s->label_kind, A.n_tx = s->n_transcripts;
  A.seg_b0 = s->seg_b0, A.seg_b1 = s->seg_b1, A.seg_cds0 = s->seg_cds0, A.seg_tx = s->seg_tx, A.seg_prev = s->seg_prev, A.seg_next = s->seg_next;
  A.n_seg = s->n_segments, A.tx_strand = s->tx_strand, A.tx_cds_len = s->tx_cds_len;
  for (int j = 0; j < 64; ++j) A.aa_w[j >> 2] |= (uint32_t)s->aa[j] << (8 * (j & 3));
  A.alt_packed = alt_packed;
  A.table = reinterpret_cast<u64*>(s->table), A.rows = reinterpret_cast<u64*>(s->rows), A.status = s->status;
  WsArena ws(ws_ptr);
  const ConseqWs w = carve(ws, s->n_segments);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(SC_THREADS);
  const dim3 row_grid((unsigned)((s->n + SC_THREADS - 1) / SC_THREADS));
  if (s->prob_f64)
    hipLaunchKernelGGL(summary_conseq_check_kernel<double>, row_grid, block, 0, st, A);
  else
    hipLaunchKernelGGL(summary_conseq_check_kernel<float>, row_grid, block, 0, st, A);
  MURAL_HIP_CHECK(hipGetLastError());
  const dim3 seg_grid((unsigned)((s->n_segments + SC_WAVES - 1) / SC_WAVES));
  hipLaunchKernelGGL(summary_conseq_range_kernel, seg_grid, block, 0, st, A, w.row0, w.row1, w.pre);
  MURAL_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(summary_conseq_scan_kernel, dim3(1), dim3(SC_SCAN_THREADS), 0, st, w.pre, s->n_segments);
  MURAL_HIP_CHECK(hipGetLastError());
  // the chunks are known on the device only; the host knows a bound: every segment has at most ceil(n / chunk) of them
  const int64_t per_seg = (s->n + SC_CHUNK_ROWS - 1) / SC_CHUNK_ROWS;
  int64_t n_waves = SC_GRID_WAVES;
  if (per_seg < SC_GRID_WAVES && s->n_segments < SC_GRID_WAVES / per_seg) n_waves = s->n_segments * per_seg;
  n_waves = (n_waves + SC_WAVES - 1) / SC_WAVES * SC_WAVES;
  const dim3 reduce_grid((unsigned)(n_waves / SC_WAVES));
  if (s->prob_f64)
    hipLaunchKernelGGL(summary_conseq_reduce_kernel<double>, reduce_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  else
    hipLaunchKernelGGL(summary_conseq_reduce_kernel<float>, reduce_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  MURAL_HIP_CHECK(hipGetLastError());
  const int64_t n_cells = (int64_t)s->n_transcripts * SC_BINS;
  hipLaunchKernelGGL(summary_conseq_fold_kernel, dim3((unsigned)((n_cells + SC_THREADS - 1) / SC_THREADS)), block, 0, st, A.table, n_cells);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}
