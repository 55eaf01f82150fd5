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
//   * check kernel, a thread per row: the status bits;
//   * range and scan kernels: the segments' rows cut into chunks of at most SC_CHUNK_ROWS rows (row_chunks.h);
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

// exclusive prefix of v[0 .. m - 1] in place, v[m] = the total: one workgroup
__global__ __launch_bounds__(SC_SCAN_THREADS) void summary_conseq_scan_kernel(int64_t* __restrict__ v, int64_t m) {
  const int64_t total = run_excl_scan<SC_SCAN_THREADS, int64_t>(m, [&](int64_t t) { return v[t]; }, [&](int64_t t, int64_t x) { v[t] = x; });
  if (threadIdx.x == 0) v[m] = total;
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
    const int64_t s = row_chunk_item(pre, A.n_seg, unit);
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
          conseq_row_bins(A, aa, s, tx, minus, cds_len, b0, b1, cds0, i, q, bins);
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
  uint32_t alt_packed = 0;
  int bad_alt = 0;
  MURAL_REQUIRE(conseq_pack_alt_order(s->alt_order, alt_packed, bad_alt),
                "summary_conseq_rows: alt_order[%d] must name the three other bases once each", bad_alt);
  if (s->n == 0 || s->n_segments == 0) return MURAL_OK;
  MURAL_REQUIRE(s->genome && s->genome->packed2 && s->genome->nmask && s->genome->length >= 0, "summary_conseq_rows: empty genome");
  MURAL_REQUIRE(s->prob && s->start && s->label && s->status && s->table && s->rows, "summary_conseq_rows: NULL argument");
  MURAL_REQUIRE(s->seg_b0 && s->seg_b1 && s->seg_cds0 && s->seg_tx && s->seg_prev && s->seg_next && s->tx_strand && s->tx_cds_len &&
                    s->n_transcripts >= 1,
                "summary_conseq_rows: segments without transcripts");
  MURAL_REQUIRE(s->prob_stride >= 4, "summary_conseq_rows: prob_stride < n_class");
  if (const int rc = check_workspace("summary_conseq_rows", "mural_summary_conseq_workspace_bytes", ws_ptr, ws_bytes,
                                     mural_summary_conseq_workspace_bytes(s->n_segments)))
    return rc;
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
  const RowChunks w = carve_row_chunks(ws, s->n_segments);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(SC_THREADS);
  const dim3 row_grid((unsigned)((s->n + SC_THREADS - 1) / SC_THREADS));
  if (s->prob_f64)
    hipLaunchKernelGGL(summary_conseq_check_kernel<double>, row_grid, block, 0, st, A);
  else
    hipLaunchKernelGGL(summary_conseq_check_kernel<float>, row_grid, block, 0, st, A);
  MURAL_HIP_CHECK(hipGetLastError());
  const dim3 seg_grid((unsigned)((s->n_segments + SC_WAVES - 1) / SC_WAVES));
  hipLaunchKernelGGL(row_chunk_range_kernel<SC_THREADS>, seg_grid, block, 0, st, A.start, A.n, A.seg_b0, A.seg_b1, A.seg_tx, A.n_tx, A.n_seg,
                     SC_CHUNK_ROWS, w);
  MURAL_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(summary_conseq_scan_kernel, dim3(1), dim3(SC_SCAN_THREADS), 0, st, w.pre, s->n_segments);
  MURAL_HIP_CHECK(hipGetLastError());
  const int64_t n_waves = row_chunk_grid_waves(s->n, SC_CHUNK_ROWS, 1, s->n_segments, SC_GRID_WAVES, SC_WAVES);
  const dim3 reduce_grid((unsigned)(n_waves / SC_WAVES));
  if (s->prob_f64)
    hipLaunchKernelGGL(summary_conseq_reduce_kernel<double>, reduce_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  else
    hipLaunchKernelGGL(summary_conseq_reduce_kernel<float>, reduce_grid, block, 0, st, A, w.row0, w.row1, w.pre, n_waves);
  MURAL_HIP_CHECK(hipGetLastError());
  const int64_t n_cells = (int64_t)s->n_transcripts * SC_BINS;
  FoldTables F{};
  F.table[0] = A.table, F.n_groups[0] = n_cells, F.nc = 1;      // [transcript][bin][3] = [cell][3][1]
  hipLaunchKernelGGL(summary_fold_kernel<SC_THREADS>, dim3((unsigned)((n_cells + SC_THREADS - 1) / SC_THREADS)), block, 0, st, F);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}
