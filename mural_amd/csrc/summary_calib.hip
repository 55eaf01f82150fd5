// Loss and calibration metrics of a prediction shard while it is on the device (mural_amd/predict.py: SummarySink(calibration=True)):
// the sums behind the NLL / ECE / classwise ECE / Brier block of the reference's validation report (MuRaL/evaluation/evaluation.py:
// 207-295, 339-358), reduced in one pass over the rows of a part from the probabilities and the labels the table would hold.
//
// The per-row definitions are those of calib_metrics_kernel (analytics.hip); this kernel evaluates them in the probabilities' own
// precision P, that one in float64 whatever P is (it rounds each score once to P before binning): q = softmax(log(prob)),
// confidence = max q (the first maximum is the prediction), Brier term = sum_c ([c == label] - q_c)^2, NLL term = -log q_label, bins
// (lower, upper] on the caller's float32 bounds.  What differs is how the rows are ADDED: every cell is an unsigned 64-bit integer and
// every addition an integer one, so the table is a function of the SET of valid rows, bit for bit, whatever the parts, the launch
// geometry or the run.  No floating-point atomic anywhere in this file.
//
// Cells (uint64, H = 6 + n_class header cells, then 4 per bin):
//   [0] rows   [1] inf_rows   [2 + c] rows with label c   [2 + nc] NLL hi  [3 + nc] NLL lo   [4 + nc] Brier hi  [5 + nc] Brier lo
//   [H + 4 (g * n_bins + b) + {0, 1, 2, 3}] = rows, score hi, score lo, hits of bin b of group g: g = 0 the top-label bins (score =
//   the confidence, hit = the prediction is the label), g = 1 + c the bins of class c (score = q_c, hit = the label is c).
// A real-valued sum is two-limb fixed point: a term v >= 0 is quantised ONCE to rne(v * 2^(S + 46)), carried as hi = floor(v * 2^S) and
// lo = rint((v * 2^S - hi) * 2^46) (each step exact in float64: a power-of-two scaling, a difference within one binade or below, one
// rounding to an integer); the value of a pair is (hi * 2^46 + lo) / 2^(S + 46).  S = 16 for the scores (in [0, 1]) and the Brier terms
// (in [0, 2]): a row's error is at most 2^-63; S = 13 for the NLL terms (below 2^10: -log of the smallest positive double is 744.5): at
// most 2^-60.  Bounds: a pair's lo is below 2^46 on return (the fold kernel carries its overflow into hi); hi grows by at most 2^23 per
// row plus the carries (2^40 rows carry at most 2^40 in all): 2^40 rows stay below 2^64.  In between: a lane's registers hold the two
// scalar sums of at most CB_BLOCK_ROWS / CB_THREADS rows, a workgroup's LDS image at most CB_BLOCK_ROWS * 2^46 < 2^59 per lo cell, the
// flush splits each lo cell into its carry (to hi) and a remainder below 2^46, so a launch of CB_SLICE_ROWS rows adds less than
// 2^46 * CB_SLICE_ROWS / CB_BLOCK_ROWS = 2^62 to a global lo cell before the fold.
//
// Same-bin contention: most confidences of a mutation-rate model land in ONE bin, and 64 lanes adding to one LDS address serialise.  The
// lanes of a wave that share a bin are therefore reduced in registers first (ballots for the two counts, shuffles for the two limbs --
// integer sums, so the grouping changes no bit) and the group's first lane makes the LDS adds; two such rounds take the two most frequent
// bins of the wave, whatever is left adds lane by lane.  Label counts and row counts are ballots.
//
// Rows that are skipped everywhere and set the status word: a label outside 0 .. n_class - 1 (bit 1), a probability that is NaN,
// negative or above 1 -- or a row without one positive probability, whose softmax is undefined -- (bit 3).  A valid row with
// q_label == 0 has an infinite NLL term: it is counted in inf_rows, left out of the NLL sum and counted everywhere else.
#include "common.h"
#include "kmer_key.h"      // load_label, the status bits

namespace mural {
namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_MAX_CLASS = 16;
constexpr int CB_LDS_CELLS = 4096;                 // the workgroup's image of the table: 32 KB
constexpr int CB_MAX_BINS = 1024;                  // (bounds[n_bins + 1] sit in LDS as well)
constexpr int64_t CB_BLOCK_ROWS = 1ll << 12;       // rows of a workgroup: one image is zeroed and flushed per that many rows
constexpr int64_t CB_SLICE_ROWS = 1ll << 28;       // rows of a launch (the bound above)
constexpr int CB_LO_BITS = 46;
constexpr u64 CB_LO_MASK = (1ull << CB_LO_BITS) - 1;
constexpr int CB_SCORE_BITS = 16, CB_NLL_BITS = 13;

struct CalibArgs {
  const void* prob;
  const void* label;
  const float* bounds;
  u64* table;
  int32_t* status;
  int64_t prob_stride, n;
  int32_t label_kind, nc, nb, cells;
};

__host__ __device__ __forceinline__ int header_cells(int nc) { return 6 + nc; }
// a lo limb: its carry belongs to the cell in front of it
__device__ __forceinline__ bool is_lo_cell(int idx, int nc) {
  const int h = header_cells(nc);
  return idx < h ? (idx == 3 + nc || idx == 5 + nc) : ((idx - h) & 3) == 2;
}

__device__ __forceinline__ void quantise(double v, int bits, u64& hi, u64& lo) {
  v = v > 0.0 ? v : 0.0;                             // (-0.0 from -log(1))
  const double s = v * (double)(1ull << bits);
  const double h = floor(s);
  hi = (u64)(long long)h;
  lo = (u64)(long long)rint((s - h) * (double)(1ull << CB_LO_BITS));
}

// the bin (lower, upper] of v, -1 if there is none: the guess from v * nb and its neighbours, then every bin
__device__ __forceinline__ int bin_of(double v, const float* __restrict__ bounds, int nb) {
  const int t0 = (int)ceil(v * (double)nb) - 1;
  for (int t = max(t0 - 1, 0); t <= min(t0 + 1, nb - 1); ++t)
    if (v > (double)bounds[t] && v <= (double)bounds[t + 1]) return t;
  for (int t = 0; t < nb; ++t)
    if (v > (double)bounds[t] && v <= (double)bounds[t + 1]) return t;
  return -1;
}

__device__ __forceinline__ void add_cells(u64* __restrict__ cell, u64 rows, u64 hi, u64 lo, u64 hits) {
  atomicAdd(&cell[0], rows);
  if (hi) atomicAdd(&cell[1], hi);
  if (lo) atomicAdd(&cell[2], lo);
  if (hits) atomicAdd(&cell[3], hits);
}

// One score per lane (bin < 0: none) into the bins of one group; called by whole waves.
__device__ __forceinline__ void add_binned(u64* __restrict__ group, int bin, u64 hi, u64 lo, bool hit) {
  const int lane = threadIdx.x & 63;
  u64 todo = __ballot(bin >= 0);
  for (int round = 0; round < 2 && todo; ++round) {
    const int leader = __ffsll((long long)todo) - 1;
    const int b0 = __shfl(bin, leader, 64);
    const bool mine = bin == b0;
    const u64 mask = __ballot(mine);
    const u64 hits = (u64)__popcll(__ballot(mine && hit));
    const u64 h = wave_sum(mine ? hi : 0ull), l = wave_sum(mine ? lo : 0ull);
    if (lane == leader) add_cells(group + 4 * b0, (u64)__popcll(mask), h, l, hits);
    if (mine) bin = -1;
    todo &= ~mask;
  }
  if (bin >= 0) add_cells(group + 4 * bin, 1ull, hi, lo, hit ? 1ull : 0ull);
}

template <typename P>
__global__ __launch_bounds__(CB_THREADS) void summary_calib_rows_kernel(CalibArgs A, int64_t row0, int64_t row1) {
  __shared__ u64 cells[CB_LDS_CELLS];
  __shared__ float bounds[CB_MAX_BINS + 1];
  const int nc = A.nc, nb = A.nb, H = header_cells(nc);
  for (int t = threadIdx.x; t < A.cells; t += CB_THREADS) cells[t] = 0ull;
  for (int t = threadIdx.x; t <= nb; t += CB_THREADS) bounds[t] = A.bounds[t];
  __syncthreads();
  const P* __restrict__ prob = static_cast<const P*>(A.prob);
  const int lane = threadIdx.x & 63;
  const int64_t b0 = row0 + (int64_t)blockIdx.x * CB_BLOCK_ROWS, b1 = min(b0 + CB_BLOCK_ROWS, row1);
  u64 nll_hi = 0, nll_lo = 0, br_hi = 0, br_lo = 0;
  int32_t bad = 0;
  // every lane of the workgroup makes the same number of trips: the ballots and shuffles below see whole waves
  for (int64_t i0 = b0; i0 < b1; i0 += CB_THREADS) {
    const int64_t i = i0 + threadIdx.x;
    bool valid = i < b1;
    int lab = -1, arg = 0;
    P q[CB_MAX_CLASS];
    P conf = (P)-1;
    P m = (P)-INFINITY;
    bool inf_row = false;
    if (valid) {
      lab = load_label(A.label, A.label_kind, i);
      int32_t bad_row = (lab < 0 || lab >= nc) ? SM_BAD_LABEL : 0;
      // the reference's pseudo-logits are log(prob) and its scores softmax(log(prob)), evaluated in prob's own precision
      bool positive = false;
#pragma unroll
      for (int c = 0; c < CB_MAX_CLASS; ++c) {
        if (c < nc) {
          const P p = prob[i * A.prob_stride + c];
          // 0 <= p <= 1 on the bit pattern -- non-negative doubles order like their bits --, so that NaN is caught whatever the
          // compiler assumes about comparisons; -0.0 counts as 0
          const u64 bits = (u64)__double_as_longlong((double)p);
          if (bits > 0x3FF0000000000000ull && bits != 0x8000000000000000ull) bad_row |= SM_BAD_PROB;
          positive |= bits != 0ull && bits != 0x8000000000000000ull;
          q[c] = (P)log(p);
          m = q[c] > m ? q[c] : m;
        }
      }
      if (!positive) bad_row |= SM_BAD_PROB;
      if (bad_row) {
        bad |= bad_row;
        valid = false;
      }
    }
    if (valid) {
      P s = (P)0;
#pragma unroll
      for (int c = 0; c < CB_MAX_CLASS; ++c) {
        if (c < nc) {
          q[c] = (P)exp(q[c] - m);
          s += q[c];
        }
      }
      double brier = 0.0;
      P q_lab = (P)0;
#pragma unroll
      for (int c = 0; c < CB_MAX_CLASS; ++c) {
        if (c < nc) {
          q[c] = q[c] / s;
          if (q[c] > conf) {
            conf = q[c];
            arg = c;
          }
          const P dlt = (c == lab ? (P)1 : (P)0) - q[c];
          brier += (double)(dlt * dlt);
          if (c == lab) q_lab = q[c];
        }
      }
      u64 hi, lo;
      quantise(brier, CB_SCORE_BITS, hi, lo);
      br_hi += hi, br_lo += lo;
      inf_row = !(q_lab > (P)0);
      if (!inf_row) {
        quantise(-(double)(P)log(q_lab), CB_NLL_BITS, hi, lo);
        nll_hi += hi, nll_lo += lo;
      }
    }
    // counts: one ballot each, the wave's first lane adds
    const u64 n_rows = (u64)__popcll(__ballot(valid)), n_inf = (u64)__popcll(__ballot(valid && inf_row));
    if (n_rows) {                                        // (wave-uniform)
      if (lane == 0) {
        atomicAdd(&cells[0], n_rows);
        if (n_inf) atomicAdd(&cells[1], n_inf);
      }
      for (int c = 0; c < nc; ++c) {
        const u64 n_lab = (u64)__popcll(__ballot(valid && lab == c));
        if (n_lab && lane == 0) atomicAdd(&cells[2 + c], n_lab);
      }
      for (int g = 0; g <= nc; ++g) {
        P v = conf;
#pragma unroll
        for (int c = 0; c < CB_MAX_CLASS; ++c)
          if (c + 1 == g) v = q[c];
        int bin = -1;
        u64 hi = 0, lo = 0;
        if (valid) {
          bin = bin_of((double)v, bounds, nb);
          quantise((double)v, CB_SCORE_BITS, hi, lo);
        }
        add_binned(cells + H + 4 * g * nb, bin, hi, lo, g == 0 ? arg == lab : lab == g - 1);
      }
    }
  }
  nll_hi = wave_sum(nll_hi), nll_lo = wave_sum(nll_lo), br_hi = wave_sum(br_hi), br_lo = wave_sum(br_lo);
  if (lane == 0) {
    if (nll_hi) atomicAdd(&cells[2 + nc], nll_hi);
    if (nll_lo) atomicAdd(&cells[3 + nc], nll_lo);
    if (br_hi) atomicAdd(&cells[4 + nc], br_hi);
    if (br_lo) atomicAdd(&cells[5 + nc], br_lo);
  }
  __syncthreads();
  // the non-zero cells once each; a lo limb as its carry (to the hi limb in front of it) and its remainder
  for (int t = threadIdx.x; t < A.cells; t += CB_THREADS) {
    const u64 v = cells[t];
    if (!v) continue;
    if (is_lo_cell(t, nc)) {
      if (v >> CB_LO_BITS) atomicAdd(&A.table[t - 1], v >> CB_LO_BITS);
      if (v & CB_LO_MASK) atomicAdd(&A.table[t], v & CB_LO_MASK);
    } else {
      atomicAdd(&A.table[t], v);
    }
  }
  if (bad) atomicOr(A.status, bad);
}

// carry the overflow of the lo limbs into the hi limbs: a thread per cell, plain loads and stores
__global__ __launch_bounds__(CB_THREADS) void summary_calib_fold_kernel(CalibArgs A) {
  const int t = blockIdx.x * CB_THREADS + threadIdx.x;
  if (t >= A.cells || !is_lo_cell(t, A.nc)) return;
  const u64 lo = A.table[t];
  if (lo >> CB_LO_BITS) {
    A.table[t - 1] += lo >> CB_LO_BITS;
    A.table[t] = lo & CB_LO_MASK;
  }
}

}  // namespace
}  // namespace mural

using namespace mural;

extern "C" int64_t mural_summary_calib_cells(int32_t n_class, int32_t n_bins) {
  if (n_class < 1 || n_class > CB_MAX_CLASS || n_bins < 1 || n_bins > CB_MAX_BINS) return 0;
  const int64_t cells = header_cells(n_class) + 4ll * n_bins * (n_class + 1);
  return cells <= CB_LDS_CELLS ? cells : 0;
}

extern "C" int mural_summary_calib_rows(const MuralSummaryCalibRows* s, void* stream) {
  MURAL_REQUIRE(s, "summary_calib_rows: NULL argument");
  MURAL_REQUIRE(s->n >= 0 && s->n_class >= 1 && s->n_class <= CB_MAX_CLASS && s->n_bins >= 1,
                "summary_calib_rows: n >= 0, 1 <= n_class <= %d and n_bins >= 1 required", CB_MAX_CLASS);
  const int64_t cells = mural_summary_calib_cells(s->n_class, s->n_bins);
  MURAL_REQUIRE(cells > 0, "summary_calib_rows: n_bins * (n_class + 1) = %lld is too large: the table of %lld cells does not fit the %d of a workgroup",
                (long long)s->n_bins * (s->n_class + 1), (long long)header_cells(s->n_class) + 4ll * s->n_bins * (s->n_class + 1),
                CB_LDS_CELLS);
  MURAL_REQUIRE(s->label_kind >= 0 && s->label_kind <= 2, "summary_calib_rows: label_kind is 0 (float32), 1 (int32) or 2 (int64)");
  if (s->n == 0) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->label && s->bounds && s->table && s->status, "summary_calib_rows: NULL argument");
  MURAL_REQUIRE(s->prob_stride >= s->n_class, "summary_calib_rows: prob_stride < n_class");
  CalibArgs A{};
  A.prob = s->prob, A.label = s->label, A.bounds = s->bounds, A.table = reinterpret_cast<u64*>(s->table), A.status = s->status;
  A.prob_stride = s->prob_stride, A.n = s->n, A.label_kind = s->label_kind, A.nc = s->n_class, A.nb = s->n_bins, A.cells = (int32_t)cells;
  const dim3 fold_grid((unsigned)((cells + CB_THREADS - 1) / CB_THREADS));
  for (int64_t r0 = 0; r0 < s->n; r0 += CB_SLICE_ROWS) {
    const int64_t r1 = std::min(r0 + CB_SLICE_ROWS, s->n);
    const dim3 grid((unsigned)((r1 - r0 + CB_BLOCK_ROWS - 1) / CB_BLOCK_ROWS));
    if (s->prob_f64)
      hipLaunchKernelGGL(summary_calib_rows_kernel<double>, grid, dim3(CB_THREADS), 0, (hipStream_t)stream, A, r0, r1);
    else
      hipLaunchKernelGGL(summary_calib_rows_kernel<float>, grid, dim3(CB_THREADS), 0, (hipStream_t)stream, A, r0, r1);
    MURAL_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(summary_calib_fold_kernel, fold_grid, dim3(CB_THREADS), 0, (hipStream_t)stream, A);
    MURAL_HIP_CHECK(hipGetLastError());
  }
  return MURAL_OK;
}
