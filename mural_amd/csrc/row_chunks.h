// Row-chunk planning, shared by every reduction that works per ITEM of a part's rows: csrc/simulate.hip (items = the pieces of the
// interval sets, owners = their groups), csrc/summary_conseq.hip and csrc/simulate_conseq.hip (items = CDS segments, owners =
// transcripts), csrc/summary_txstruct.hip, csrc/simulate_txstruct.hip, csrc/summary_txindel.hip and csrc/simulate_txindel.hip (items =
// the parts that tile a transcript's span).  The rows of a part ascend in start, so the rows of an item [b0, b1) are ONE range
// [i0, i1); a long item is cut into CHUNKS of at most chunk_rows rows, so that it becomes many units of work and cannot serialise the
// consumer's launch.  plan_row_chunks() is the whole plan:
//   * row_chunk_range_kernel, a wave per item: [i0, i1) by two 64-ary searches in start + shift (common.h: wave_partition_point), and
//     the item's chunk count in pre[].  shift is 0 except for the INDEL tables, whose rows belong to an item by their home base;
//   * excl_scan_kernel, one workgroup (common.h: run_excl_scan): pre[] becomes the exclusive prefix of the chunk counts, pre[n_items]
//     their total;
// and the consumer, a grid of row_chunk_grid_waves() waves striding over the chunks, finds chunk t's item with row_chunk_item().
#pragma once
#include "common.h"

namespace mural {

struct RowChunks { int64_t *row0, *row1, *pre; };      // [n_items], [n_items], [n_items + 1]

inline RowChunks carve_row_chunks(WsArena& ws, int64_t n_items) {
  RowChunks w;
  w.row0 = ws.as<int64_t>((size_t)n_items);
  w.row1 = ws.as<int64_t>((size_t)n_items);
  w.pre = ws.as<int64_t>((size_t)n_items + 1);
  return w;
}

inline size_t row_chunks_bytes(int64_t n_items) {
  if (n_items <= 0) return 0;
  WsArena ws(nullptr);
  carve_row_chunks(ws, n_items);
  return ws.off;
}

// a wave per item: its rows [i0, i1) -- those with b0 <= start + shift < b1 -- and its chunk count; an item that is empty or whose
// owner lies outside [0, n_owners) has none
template <int THREADS>
__global__ __launch_bounds__(THREADS) void row_chunk_range_kernel(const int64_t* __restrict__ start, int64_t n,
                                                                  const int64_t* __restrict__ b0, const int64_t* __restrict__ b1,
                                                                  const int32_t* __restrict__ owner, int32_t n_owners, int64_t n_items,
                                                                  int64_t shift, int64_t chunk_rows, RowChunks w) {
  const int64_t p = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
  if (p >= n_items) return;
  const int32_t g = owner[p];
  const int64_t lo = b0[p], hi = b1[p];
  int64_t i0 = 0, i1 = 0;
  if (g >= 0 && g < n_owners && lo < hi) {
    i0 = wave_partition_point(0, n, [&](int64_t i) { return start[i] + shift < lo; });
    i1 = wave_partition_point(i0, n, [&](int64_t i) { return start[i] + shift < hi; });
  }
  if ((threadIdx.x & 63) == 0) {
    w.row0[p] = i0, w.row1[p] = i1;
    w.pre[p] = (i1 - i0 + chunk_rows - 1) / chunk_rows;
  }
}

// exclusive prefix of v[0 .. m - 1] in place, v[m] = the total (also to *total_out where given): one workgroup
template <int THREADS>
__global__ __launch_bounds__(THREADS) void excl_scan_kernel(int64_t* __restrict__ v, int64_t m, int64_t* __restrict__ total_out) {
  const int64_t total = run_excl_scan<THREADS, int64_t>(m, [&](int64_t t) { return v[t]; }, [&](int64_t t, int64_t x) { v[t] = x; });
  if (threadIdx.x == 0) {
    v[m] = total;
    if (total_out) *total_out = total;
  }
}

// The plan of n_items > 0 items on `st`: w carved from ws, the range kernel (THREADS threads) and the scan (SCAN_THREADS threads).
// MURAL_OK or the error code of a launch.
template <int THREADS, int SCAN_THREADS>
inline int plan_row_chunks(hipStream_t st, const int64_t* start, int64_t n, const int64_t* b0, const int64_t* b1, const int32_t* owner,
                           int32_t n_owners, int64_t n_items, int64_t shift, int64_t chunk_rows, WsArena& ws, RowChunks& w) {
  w = carve_row_chunks(ws, n_items);
  const dim3 grid((unsigned)((n_items + THREADS / 64 - 1) / (THREADS / 64)));
  hipLaunchKernelGGL(row_chunk_range_kernel<THREADS>, grid, dim3(THREADS), 0, st, start, n, b0, b1, owner, n_owners, n_items, shift,
                     chunk_rows, w);
  MURAL_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(excl_scan_kernel<SCAN_THREADS>, dim3(1), dim3(SCAN_THREADS), 0, st, w.pre, n_items, (int64_t*)nullptr);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

// the item of chunk t: the last p with pre[p] <= t (pre[n_items] = the total > t, so the point lies in 1 .. n_items); the whole wave
__device__ __forceinline__ int64_t row_chunk_item(const int64_t* __restrict__ pre, int64_t n_items, int64_t t) {
  return wave_partition_point(0, n_items + 1, [&](int64_t q) { return pre[q] <= t; }) - 1;
}

// The waves of the consumer's grid.  The units are known on the device only; the host knows a bound: every item has at most
// ceil(n / chunk_rows) chunks of units_per_chunk units each.  At most grid_waves, rounded up to whole workgroups of `waves` waves.
inline int64_t row_chunk_grid_waves(int64_t n, int64_t chunk_rows, int64_t units_per_chunk, int64_t n_items, int64_t grid_waves, int waves) {
  const int64_t per_item = (n + chunk_rows - 1) / chunk_rows * units_per_chunk;
  int64_t n_waves = grid_waves;
  if (per_item < grid_waves && n_items < grid_waves / per_item) n_waves = n_items * per_item;
  return (n_waves + waves - 1) / waves * waves;
}

}  // namespace mural
