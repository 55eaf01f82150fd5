// Genome summaries of a prediction shard while it is on the device (mural_amd/predict.py: SummarySink): the window tables of
// `evaluate --window_size` and the totals of `calc_scaling_factor` in one pass over the probabilities, so that neither needs the
// '%.4g' table written and parsed back (csrc/tables.hip stays the tool for tables that exist as files).
//
// The rows of a shard ascend in start, so the rows of one window form ONE contiguous range: the window tables are a segmented reduction.
//   * launch 1, grid (chunks, windows): a workgroup is one wave and takes a fixed chunk of SM_CHUNK rows, 64 per pass.  Per pass a
//     wave64 segmented scan (shuffles, a fixed tree) sums the runs of equal window; a run that goes on into the next pass is carried in
//     registers.  A window that begins and ends inside the chunk is added to the table by the one lane that holds its sum (a plain
//     read-modify-write: nobody else has rows of it); the chunk's first and last window may be shared with the neighbours and are left
//     as two carry records in the workspace.  The blocks of window 0 also reduce the totals of their chunk.
//   * launch 2, one workgroup: a thread per (window size, table column) walks the carry records in chunk order and adds them to the
//     table; one thread adds the chunks' totals in chunk order.
// No floating-point atomics anywhere: the result is a function of the input and of SM_CHUNK alone.  float64 throughout; the row and label
// counts are carried as integers.
#include "common.h"
#include "kmer_key.h"

namespace mural {
namespace {

constexpr int SM_CHUNK = 2048;                 // rows of a workgroup's chunk
constexpr int SM_PASSES = SM_CHUNK / 64;
constexpr int SM_MAX_CLASS = 8;
constexpr int SM_CARRY_THREADS = 256;

struct SummaryArgs {
  const void* prob;
  const int64_t* start;
  const int64_t* end;
  const void* label;
  int64_t prob_stride, n;
  int32_t label_kind, n_windows;
  int64_t window[MURAL_SUMMARY_MAX_WINDOWS], bin0[MURAL_SUMMARY_MAX_WINDOWS], n_bins[MURAL_SUMMARY_MAX_WINDOWS];
  double* table[MURAL_SUMMARY_MAX_WINDOWS];
  const int64_t* reg_b0;
  const int64_t* reg_b1;
  int64_t n_reg;
  int32_t* rec_key;        // [chunks][windows][2]
  double* rec_val;         // [chunks][windows][2][1 + 2 n_class]
  double* part_sum;        // [chunks]
  int64_t* part_cnt;       // [chunks]
  int32_t* status;
};

// #(b[0 .. n) < key) or, with `or_equal`, #(b <= key) of an ascending array
__device__ __forceinline__ int64_t count_below(const int64_t* __restrict__ b, int64_t n, int64_t key, bool or_equal) {
  int64_t a = 0, z = n;
  while (a < z) {
    const int64_t m = (a + z) >> 1;
    if (or_equal ? b[m] <= key : b[m] < key) a = m + 1; else z = m;
  }
  return a;
}

template <typename T, int NC>
__global__ __launch_bounds__(64) void summary_rows_kernel(SummaryArgs A) {
  constexpr int STRIDE = 1 + 2 * NC;
  const int lane = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int j = blockIdx.y;
  const bool windows = j < A.n_windows;
  const bool totals = j == 0;
  const int64_t W = windows ? A.window[j] : 1, bin0 = windows ? A.bin0[j] : 0, n_bins = windows ? A.n_bins[j] : 0;
  double* __restrict__ table = windows ? A.table[j] : nullptr;
  const int64_t rec = (chunk * (A.n_windows > 0 ? A.n_windows : 1) + j) * 2;
  const T* __restrict__ prob = static_cast<const T*>(A.prob);

  int carry_key = -1, carry_cnt = 0, carry_lab[NC];
  double carry_p[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) carry_lab[c] = 0, carry_p[c] = 0.0;
  bool first_open = true;
  int32_t bad = 0;
  double tot_s = 0.0;
  int64_t tot_c = 0;

  for (int pass = 0; pass < SM_PASSES; ++pass) {
    const int64_t i = chunk * SM_CHUNK + (int64_t)pass * 64 + lane;
    if (chunk * SM_CHUNK + (int64_t)pass * 64 >= A.n) break;      // (wave-uniform)
    bool valid = i < A.n;
    int64_t st = 0;
    int lab = 0;
    double p[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = 0.0;
    if (valid) {
      st = A.start[i];
      lab = load_label(A.label, A.label_kind, i);
      if (st < 0) bad |= SM_BAD_START, valid = false;
      if (lab < 0 || lab >= NC) bad |= SM_BAD_LABEL, valid = false;
    }
    if (valid) {
#pragma unroll
      for (int c = 0; c < NC; ++c) p[c] = (double)prob[i * A.prob_stride + c];
    }
    if (totals && valid) {
      int64_t w = 1;
      if (A.reg_b0) w = count_below(A.reg_b0, A.n_reg, A.end[i], false) - count_below(A.reg_b1, A.n_reg, st, true);
      if (w > 0) {
        double r = 0.0;
#pragma unroll
        for (int c = 1; c < NC; ++c) r += p[c];
        tot_s += (double)w * r;
        tot_c += w;
      }
    }
    if (!windows) continue;

    // the row's window; rk: the window of the latest valid row up to this lane (the rows ascend, so it is the running maximum)
    int key = -1;
    if (valid) {
      const int64_t k64 = st / W - bin0;
      if (k64 < 0 || k64 >= n_bins) bad |= SM_BAD_ORDER, valid = false; else key = (int)k64;
    }
    int rk = key;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int u = __shfl_up(rk, off, 64);
      if (lane >= off) rk = max(rk, u);
    }
    rk = max(rk, carry_key);
    int prev = __shfl_up(rk, 1, 64);
    if (lane == 0) prev = carry_key;
    if (valid && key < prev) bad |= SM_BAD_ORDER, valid = false;      // a row that does not ascend is skipped, never misfiled
    const bool head = valid && key != prev;
    // first lane of this lane's run within the pass (0: the run came in with the carry, if no lane before was a head)
    int hpos = head ? lane + 1 : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int u = __shfl_up(hpos, off, 64);
      if (lane >= off) hpos = max(hpos, u);
    }
    const bool cont = hpos == 0;
    const int h = hpos > 0 ? hpos - 1 : 0;

    int cnt = valid ? 1 : 0, labc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) labc[c] = (valid && lab == c) ? 1 : 0;
    if (!valid) {
#pragma unroll
      for (int c = 0; c < NC; ++c) p[c] = 0.0;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const bool take = lane - off >= h;
      const int uc = __shfl_up(cnt, off, 64);
      if (take) cnt += uc;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int ul = __shfl_up(labc[c], off, 64);
        const double up = __shfl_up(p[c], off, 64);
        if (take) labc[c] += ul, p[c] += up;
      }
    }
    if (cont) {
      cnt += carry_cnt;
#pragma unroll
      for (int c = 0; c < NC; ++c) labc[c] += carry_lab[c], p[c] = carry_p[c] + p[c];
    }
    // one lane files a finished run: the chunk's first one as a carry record (it may go on in the chunk before), any other in the table
    auto file = [&](bool as_record, int k, int n_rows, const int* n_lab, const double* sum_p) {
      if (as_record) {
        A.rec_key[rec] = k;
        double* __restrict__ dst = A.rec_val + rec * STRIDE;
        dst[0] = (double)n_rows;
#pragma unroll
        for (int c = 0; c < NC; ++c) dst[1 + c] = (double)n_lab[c], dst[1 + NC + c] = sum_p[c];
      } else {
        double* __restrict__ dst = table + (int64_t)k * STRIDE;
        dst[0] += (double)n_rows;
#pragma unroll
        for (int c = 0; c < NC; ++c) dst[1 + c] += (double)n_lab[c], dst[1 + NC + c] += sum_p[c];
      }
    };
    // the run that came in with the carry ended with the pass before if lane 0 begins a new one: no lane of this pass holds it
    if (__shfl((int)head, 0, 64) != 0 && carry_key >= 0) {
      if (lane == 0) file(first_open, carry_key, carry_cnt, carry_lab, carry_p);
      first_open = false;
    }
    // a run ends in front of the next head; the run of lane 63 goes on as the carry
    const bool next_head = __shfl_down((int)head, 1, 64) != 0;
    const bool tail = lane < 63 && next_head && rk >= 0;
    const unsigned long long tails = __ballot(tail);
    const int first_lane = (first_open && tails) ? (int)__ffsll((long long)tails) - 1 : -1;
    if (tail) file(lane == first_lane, rk, cnt, labc, p);
    if (tails) first_open = false;
    carry_key = __shfl(rk, 63, 64);
    carry_cnt = __shfl(cnt, 63, 64);
#pragma unroll
    for (int c = 0; c < NC; ++c) carry_lab[c] = __shfl(labc[c], 63, 64), carry_p[c] = __shfl(p[c], 63, 64);
  }

  if (windows && lane == 0) {
    // the run that is open at the end of the chunk: the first record if no run ended before (the whole chunk is one window)
    const int64_t r = first_open ? rec : rec + 1;
    A.rec_key[r] = carry_key;
    double* __restrict__ dst = A.rec_val + r * STRIDE;
    dst[0] = (double)carry_cnt;
#pragma unroll
    for (int c = 0; c < NC; ++c) dst[1 + c] = (double)carry_lab[c], dst[1 + NC + c] = carry_p[c];
    if (first_open) A.rec_key[rec + 1] = -1;
  }
  if (totals) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      tot_s += __shfl_xor(tot_s, m, 64);
      tot_c += (int64_t)__shfl_xor((long long)tot_c, m, 64);
    }
    if (lane == 0) A.part_sum[chunk] = tot_s, A.part_cnt[chunk] = tot_c;
  }
  if (bad) atomicOr(A.status, bad);
}

// the carry records into the tables and the chunks' totals into totals[0] / n_sites[0], both in chunk order
__global__ __launch_bounds__(SM_CARRY_THREADS) void summary_carry_kernel(SummaryArgs A, int64_t n_chunks, int stride,
                                                                         double* __restrict__ total, int64_t* __restrict__ n_sites) {
  const int t = threadIdx.x;
  if (t < A.n_windows * stride) {
    const int j = t / stride, col = t % stride;
    double* __restrict__ table = A.table[j];
    const int32_t* __restrict__ keys = A.rec_key;
    const double* __restrict__ vals = A.rec_val;
    int cur = -1;
    double acc = 0.0;
    for (int64_t c = 0; c < n_chunks; ++c) {
      const int64_t r0 = (c * A.n_windows + j) * 2;
      const int k0 = keys[r0], k1 = keys[r0 + 1];
      const double v0 = vals[r0 * stride + col], v1 = vals[(r0 + 1) * stride + col];
      // the records' windows ascend like the rows: otherwise two chunks may have filed rows under one window (col 0 reports it)
      if (col == 0 && ((k0 >= 0 && k0 < cur) || (k1 >= 0 && k1 < (k0 > cur ? k0 : cur)))) atomicOr(A.status, (int32_t)SM_BAD_ORDER);
      if (k0 >= 0) {
        if (k0 != cur) {
          if (cur >= 0) table[(int64_t)cur * stride + col] += acc;
          cur = k0, acc = 0.0;
        }
        acc += v0;
      }
      if (k1 >= 0) {
        if (k1 != cur) {
          if (cur >= 0) table[(int64_t)cur * stride + col] += acc;
          cur = k1, acc = 0.0;
        }
        acc += v1;
      }
    }
    if (cur >= 0) table[(int64_t)cur * stride + col] += acc;
  }
  if (t == SM_CARRY_THREADS - 1) {
    double s = 0.0;
    int64_t k = 0;
    for (int64_t c = 0; c < n_chunks; ++c) s += A.part_sum[c], k += A.part_cnt[c];
    total[0] += s;
    n_sites[0] += k;
  }
}

int64_t chunks_of(int64_t n) { return (n + SM_CHUNK - 1) / SM_CHUNK; }

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

template <typename T>
int launch_rows(const SummaryArgs& A, int nc, dim3 grid, hipStream_t stream) {
  switch (nc) {
#define MURAL_SM_CASE(NC) \
  case NC: hipLaunchKernelGGL((summary_rows_kernel<T, NC>), grid, dim3(64), 0, stream, A); break;
    MURAL_SM_CASE(1) MURAL_SM_CASE(2) MURAL_SM_CASE(3) MURAL_SM_CASE(4) MURAL_SM_CASE(5) MURAL_SM_CASE(6) MURAL_SM_CASE(7) MURAL_SM_CASE(8)
#undef MURAL_SM_CASE
    default: return MURAL_E_INVALID;
  }
  return MURAL_OK;
}

}  // namespace
}  // namespace mural

using namespace mural;

extern "C" int32_t mural_summary_chunk_rows(void) { return SM_CHUNK; }

extern "C" size_t mural_summary_workspace_bytes(int64_t n, int32_t n_class, int32_t n_windows) {
  if (n < 0 || n_class < 1 || n_windows < 0) return 0;
  const size_t chunks = (size_t)chunks_of(n), recs = chunks * (size_t)(n_windows > 0 ? n_windows : 1) * 2;
  return align8(recs * 4) + recs * (size_t)(1 + 2 * n_class) * 8 + chunks * 16;
}

extern "C" int mural_summary_rows(const MuralSummaryRows* s, void* ws, size_t ws_bytes, void* stream) {
  MURAL_REQUIRE(s, "summary_rows: NULL argument");
  MURAL_REQUIRE(s->n >= 0 && s->n_class >= 1 && s->n_class <= SM_MAX_CLASS, "summary_rows: n >= 0 and 1 <= n_class <= %d required",
                SM_MAX_CLASS);
  MURAL_REQUIRE(s->n_windows >= 0 && s->n_windows <= MURAL_SUMMARY_MAX_WINDOWS, "summary_rows: at most %d window sizes per call",
                MURAL_SUMMARY_MAX_WINDOWS);
  MURAL_REQUIRE(s->label_kind >= 0 && s->label_kind <= 2, "summary_rows: label_kind is 0 (float32), 1 (int32) or 2 (int64)");
  for (int j = 0; j < s->n_windows; ++j) {
    MURAL_REQUIRE(s->window[j] > 0 && s->bin0[j] >= 0 && s->n_bins[j] >= 1 && s->table[j], "summary_rows: bad window table %d", j);
    MURAL_REQUIRE(s->n_bins[j] * (1 + 2 * (int64_t)s->n_class) < (1ll << 31), "summary_rows: window table %d too large", j);
  }
  if (s->n == 0) return MURAL_OK;
  MURAL_REQUIRE(s->prob && s->start && s->label && s->status && s->total && s->n_sites, "summary_rows: NULL argument");
  MURAL_REQUIRE(s->prob_stride >= s->n_class, "summary_rows: prob_stride < n_class");
  MURAL_REQUIRE(!s->reg_b0 || (s->reg_b1 && s->end && s->n_reg >= 0), "summary_rows: NULL region argument");
  const size_t need = mural_summary_workspace_bytes(s->n, s->n_class, s->n_windows);
  if (!ws || ws_bytes < need) {
    set_error("summary_rows: workspace of %zu bytes needed, %zu given", need, ws_bytes);
    return MURAL_E_WORKSPACE;
  }
  MURAL_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "summary_rows: the workspace must be 8-byte aligned");
  const int64_t chunks = chunks_of(s->n);
  const int stride = 1 + 2 * s->n_class;
  const size_t recs = (size_t)chunks * (size_t)(s->n_windows > 0 ? s->n_windows : 1) * 2;
  SummaryArgs A{};
  A.prob = s->prob, A.start = s->start, A.end = s->end, A.label = s->label;
  A.prob_stride = s->prob_stride, A.n = s->n, A.label_kind = s->label_kind, A.n_windows = s->n_windows;
  for (int j = 0; j < s->n_windows; ++j)
    A.window[j] = s->window[j], A.bin0[j] = s->bin0[j], A.n_bins[j] = s->n_bins[j], A.table[j] = s->table[j];
  A.reg_b0 = s->reg_b0, A.reg_b1 = s->reg_b1, A.n_reg = s->n_reg;
  char* w = static_cast<char*>(ws);
  A.rec_key = reinterpret_cast<int32_t*>(w);
  w += align8(recs * 4);
  A.rec_val = reinterpret_cast<double*>(w);
  w += recs * (size_t)stride * 8;
  A.part_sum = reinterpret_cast<double*>(w);
  w += (size_t)chunks * 8;
  A.part_cnt = reinterpret_cast<int64_t*>(w);
  A.status = s->status;
  MURAL_REQUIRE(chunks < (1ll << 31), "summary_rows: too many rows for one call");
  const dim3 grid((unsigned)chunks, (unsigned)(s->n_windows > 0 ? s->n_windows : 1));
  const int rc = s->prob_f64 ? launch_rows<double>(A, s->n_class, grid, (hipStream_t)stream)
                             : launch_rows<float>(A, s->n_class, grid, (hipStream_t)stream);
  if (rc) return rc;
  MURAL_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(summary_carry_kernel, dim3(1), dim3(SM_CARRY_THREADS), 0, (hipStream_t)stream, A, chunks, stride, s->total,
                     s->n_sites);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}
