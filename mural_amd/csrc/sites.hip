// Site enumeration over a resident packed genome: "which positions of [lo, hi) are A/T sites, C/G sites (all, CpG, non-CpG) or plain
// A/C/G/T positions" answered by a scan over packed2 + nmask (0.28 bytes per base) instead of a BED file with one row per site.  The
// reference has no counterpart: its users write the per-site BED with scripts of their own and `mural_snv predict` parses it back.
//
// One lane owns one 64-bit word of packed2 (32 bases) and the 32 nmask bits of the same bases; a tile is one 256-lane block = 8192
// bases.  Every mask keeps one bit per base at the EVEN bit of its 2-bit lane, so the base classes are three bit operations on the
// word, the nmask word is spread once to the same layout, a neighbour test is a shift by two with one bit from the adjacent word, and
// a popcount counts sites.
//   count: per-tile popcounts -> a one-block prefix sum turns them into offsets (tile_counts[t] = sites before tile t,
//          tile_counts[tiles] = *total = all sites);
//   emit:  the same masks again, a block scan places every lane's sites behind its tile's offset, plain stores write the slice
//          [first, first + n) of the enumeration.  Ascending positions, no atomics: the result does not depend on scheduling.
// A base is a site only when its nmask bit is clear; the packer sets that bit for N and for every IUPAC code of the side table, so
// the table itself is not consulted.
//
// Labels: the regions route has no BED row to take a site's observed mutation from; mural_sites_label joins the enumerated sites to one
// chromosome's list of observed mutations (start strictly ascending, a few MB: it stays in the caches) with one binary search per site.
//
// Model sets: a run that serves one model per site class (A/T, non-CpG C/G, CpG) enumerates the union of the classes (focal SET) and,
// per call of its forward, asks which class every row has (mural_sites_classify: the word arithmetic of the enumeration, one lane per
// row), partitions the row numbers stably by class (mural_rows_split: per-tile counts, the one-block prefix sum, ranks by ballot) and
// puts every model's rows back in place (mural_rows_scatter).  Plain loads and stores throughout.
#include "common.h"

namespace mural {
namespace {

constexpr int ST_THREADS = SCAN_THREADS;
constexpr int ST_WORD_BASES = 32;
constexpr uint64_t EVEN = 0x5555555555555555ull;

// bit i of m -> bit 2i
__device__ __forceinline__ uint64_t spread32(uint32_t m) {
  uint64_t x = m;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & EVEN;
  return x;
}

// the even bits of the first c bases of a word (c <= 0: none, c >= 32: all)
__device__ __forceinline__ uint64_t first_bases(int64_t c) {
  if (c <= 0) return 0ull;
  if (c >= ST_WORD_BASES) return EVEN;
  return ((1ull << (2 * (int)c)) - 1ull) & EVEN;
}

// The site classes of 64-bit word `wi` (0 <= wi < words of nmask; bases [32 wi, 32 wi + 32)), one even bit per base: exactly A / T / C / G
// inside the record and not masked (N, IUPAC), and of the C and G bases those in a CpG.  The ONE CpG rule of this file: the
// neighbours across the word borders come from the adjacent words of the RECORD; a missing, masked or ambiguous neighbour is no G / no C.
struct WordClasses {
  uint64_t valid, a, t, c, g, c_cpg, g_cpg;      // (c_cpg / g_cpg: only with `cpg`)
};

__device__ __forceinline__ WordClasses word_classes(const MuralGenome& g, int64_t wi, bool cpg) {
  const int64_t n16 = (g.length + 15) >> 4, n32 = (g.length + 31) >> 5;      // words of packed2 / nmask
  const int64_t p0 = wi * ST_WORD_BASES;
  const uint64_t w = (uint64_t)g.packed2[2 * wi] | (2 * wi + 1 < n16 ? (uint64_t)g.packed2[2 * wi + 1] << 32 : 0ull);
  WordClasses k;
  // exactly A / C / G / T: inside the record and not masked (N, IUPAC)
  k.valid = ~spread32(g.nmask[wi]) & first_bases(g.length - p0);
  const uint64_t L = w & EVEN, H = (w >> 1) & EVEN;
  k.a = ~H & ~L & k.valid;
  k.t = H & L & k.valid;
  k.c = ~H & L & k.valid;
  k.g = H & ~L & k.valid;
  k.c_cpg = k.g_cpg = 0ull;
  if (cpg) {
    uint64_t g_next = 0ull, c_prev = 0ull;
    if (wi + 1 < n32) g_next = ((g.packed2[2 * wi + 2] & 3u) == 2u && (g.nmask[wi + 1] & 1u) == 0u) ? 1ull : 0ull;
    if (wi > 0) c_prev = ((g.packed2[2 * wi - 1] >> 30) == 1u && (g.nmask[wi - 1] >> 31) == 0u) ? 1ull : 0ull;
    k.c_cpg = k.c & ((k.g >> 2) | (g_next << 62));
    k.g_cpg = k.g & ((k.c << 2) | c_prev);
  }
  return k;
}

// '+' and '-' site masks of 64-bit word `wi` (bases [32 wi, 32 wi + 32)) for the window [lo, hi) of the record; focal SET: `context` is
// the union of MURAL_CLASS_* bits
__device__ __forceinline__ void site_masks(const MuralGenome& g, int64_t lo, int64_t hi, int focal, int context, int64_t wi,
                                           uint64_t* plus, uint64_t* minus) {
  *plus = *minus = 0ull;
  if (wi < 0 || wi >= ((g.length + 31) >> 5)) return;
  const int64_t p0 = wi * ST_WORD_BASES;
  const uint64_t win = first_bases(hi - p0) & ~first_bases(lo - p0);
  if (focal == MURAL_FOCAL_SET) {
    const WordClasses k = word_classes(g, wi, (context & (MURAL_CLASS_NONCPG | MURAL_CLASS_CPG)) != 0);
    uint64_t p = 0ull, m = 0ull;
    if (context & MURAL_CLASS_A) p |= k.a, m |= k.t;
    if (context & MURAL_CLASS_NONCPG) p |= k.c & ~k.c_cpg, m |= k.g & ~k.g_cpg;
    if (context & MURAL_CLASS_CPG) p |= k.c_cpg, m |= k.g_cpg;
    *plus = p & win;
    *minus = m & win;
    return;
  }
  const WordClasses k = word_classes(g, wi, focal == MURAL_FOCAL_C && context != MURAL_CONTEXT_ALL);
  if (focal == MURAL_FOCAL_ANY) {
    *plus = k.valid & win;
  } else if (focal == MURAL_FOCAL_A) {
    *plus = k.a & win;
    *minus = k.t & win;
  } else if (context == MURAL_CONTEXT_ALL) {
    *plus = k.c & win;
    *minus = k.g & win;
  } else if (context == MURAL_CONTEXT_CPG) {
    *plus = k.c_cpg & win;
    *minus = k.g_cpg & win;
  } else {
    *plus = k.c & ~k.c_cpg & win;
    *minus = k.g & ~k.g_cpg & win;
  }
}

__global__ __launch_bounds__(ST_THREADS) void sites_count_kernel(MuralGenome g, int64_t lo, int64_t hi, int focal, int context,
                                                                 int64_t word0, int64_t* __restrict__ tile_counts) {
  uint64_t plus, minus;
  site_masks(g, lo, hi, focal, context, word0 + (int64_t)blockIdx.x * ST_THREADS + threadIdx.x, &plus, &minus);
  int total = 0;
  block_excl_scan(__popcll(plus | minus), &total);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// one block, in place: counts[t] -> sites before tile t; counts[nt] = *total = all sites
__global__ __launch_bounds__(ST_THREADS) void sites_scan_kernel(int64_t* __restrict__ counts, int64_t nt, int64_t* __restrict__ total) {
  const int64_t all = run_excl_scan<ST_THREADS, int64_t>(nt, [&](int64_t b) { return counts[b]; }, [&](int64_t b, int64_t x) { counts[b] = x; });
  if (threadIdx.x == 0) {
    counts[nt] = all;
    *total = all;
  }
}

__global__ __launch_bounds__(ST_THREADS) void sites_emit_kernel(MuralGenome g, int64_t lo, int64_t hi, int focal, int context,
                                                                int64_t word0, const int64_t* __restrict__ tile_off, int64_t first,
                                                                int64_t n, int64_t* __restrict__ pos, uint8_t* __restrict__ strand) {
  const int64_t off0 = tile_off[blockIdx.x];
  if (tile_off[blockIdx.x + 1] <= first || off0 >= first + n) return;      // (block-uniform: the tile holds nothing of the slice)
  const int64_t wi = word0 + (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
  uint64_t plus, minus;
  site_masks(g, lo, hi, focal, context, wi, &plus, &minus);
  uint64_t hits = plus | minus;
  int total = 0;
  int64_t idx = off0 + block_excl_scan(__popcll(hits), &total) - first;
  while (hits) {
    const int b = __ffsll((unsigned long long)hits) - 1;
    hits &= hits - 1;
    if (idx >= 0 && idx < n) {
      pos[idx] = wi * ST_WORD_BASES + (b >> 1);
      strand[idx] = (uint8_t)((minus >> b) & 1ull);
    }
    ++idx;
  }
}

constexpr int64_t SL_MAX_BLOCKS = 1 << 12;      // 2^20 lanes fill the device twice over; longer calls stride

// label[i] = mut_label[j] where mut_start[j] == pos[i], else 0.  A thread walks sites i, i + grid, ..: neighbouring lanes search for
// neighbouring positions and take the same path through the list.  stats[0] += matched rows (one integer atomic per block that found
// any), stats[1] = min(list index of a matched mutation on the other strand): integer atomics only, so both words depend on the set of
// rows alone.
__global__ __launch_bounds__(ST_THREADS) void sites_label_kernel(const int64_t* __restrict__ pos, const uint8_t* __restrict__ strand,
                                                                 int64_t n, const int64_t* __restrict__ mut_start,
                                                                 const uint8_t* __restrict__ mut_strand,
                                                                 const float* __restrict__ mut_label, int64_t m, int check_strand,
                                                                 float* __restrict__ label, unsigned long long* __restrict__ stats) {
  int found = 0;
  const int64_t step = (int64_t)gridDim.x * ST_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x; i < n; i += step) {
    const int64_t p = pos[i];
    int64_t lo = 0, hi = m;                                  // first j with mut_start[j] >= p
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (mut_start[mid] < p) lo = mid + 1;
      else hi = mid;
    }
    float v = 0.0f;
    if (lo < m && mut_start[lo] == p) {
      v = mut_label[lo];
      ++found;
      // (list indices are >= 0 and the caller starts the word at INT64_MAX: the unsigned minimum is the signed one)
      if (check_strand && mut_strand[lo] != strand[i]) atomicMin(&stats[1], (unsigned long long)lo);
    }
    label[i] = v;
  }
  int total = 0;
  block_excl_scan(found, &total);
  if (threadIdx.x == 0 && total) atomicAdd(&stats[0], (unsigned long long)total);
}

// cls[i] = MURAL_ROW_CLASS_A / _NONCPG / _CPG of the site (pos[i], strand[i]), MURAL_ROW_CLASS_NONE for a position outside the record, a
// masked base or a strand that is not the base's.  One lane per row, the word's classes by the helper the enumeration uses.
__global__ __launch_bounds__(ST_THREADS) void sites_classify_kernel(MuralGenome g, const int64_t* __restrict__ pos,
                                                                    const uint8_t* __restrict__ strand, int64_t n,
                                                                    uint8_t* __restrict__ cls) {
  const int64_t i = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t p = pos[i];
  const uint8_t st = strand[i];
  uint8_t c = MURAL_ROW_CLASS_NONE;
  if (p >= 0 && p < g.length && st <= 1) {
    const WordClasses k = word_classes(g, p >> 5, true);
    const uint64_t bit = 1ull << (2 * (int)(p & 31));
    const uint64_t at = st ? k.t : k.a, cg = st ? k.g : k.c, cpg = st ? k.g_cpg : k.c_cpg;
    if (at & bit) c = MURAL_ROW_CLASS_A;
    else if (cg & bit) c = (cpg & bit) ? MURAL_ROW_CLASS_CPG : MURAL_ROW_CLASS_NONCPG;
  }
  cls[i] = c;
}

// Stable partition of rows by class.  A tile is one block = 256 rows; slot `nc` takes every row whose class is >= nc.  The counts are
// kept class-major, counts[c * tiles + t], so that their prefix sum (sites_scan_kernel) is the place in `perm` of the first row of
// class c in tile t: every class < nc is contiguous in perm, the rows of slot nc come last and are not written.
constexpr int RS_MAX_CLASSES = 8;

__device__ __forceinline__ int row_slot(const uint8_t* __restrict__ cls, int64_t i, int64_t n, int nc) {
  if (i >= n) return -1;
  const int c = cls[i];
  return c < nc ? c : nc;
}

// rows of slot `k` in this wave before this lane; wave_cnt[wave][c] = the wave's rows of slot c (all lanes of the block take part)
__device__ __forceinline__ int slot_rank(int k, int nc, int (*wave_cnt)[RS_MAX_CLASSES + 1]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int before = 0;
  for (int c = 0; c <= nc; ++c) {
    const unsigned long long m = __ballot(k == c);
    if (k == c) before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[w][c] = __popcll(m);
  }
  return before;
}

__global__ __launch_bounds__(ST_THREADS) void rows_count_kernel(const uint8_t* __restrict__ cls, int64_t n, int nc, int64_t tiles,
                                                                int64_t* __restrict__ counts) {
  __shared__ int wave_cnt[ST_THREADS / 64][RS_MAX_CLASSES + 1];
  slot_rank(row_slot(cls, (int64_t)blockIdx.x * ST_THREADS + threadIdx.x, n, nc), nc, wave_cnt);
  __syncthreads();
  if ((int)threadIdx.x <= nc) {
    int s = 0;
    for (int w = 0; w < ST_THREADS / 64; ++w) s += wave_cnt[w][threadIdx.x];
    counts[(int64_t)threadIdx.x * tiles + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(ST_THREADS) void rows_emit_kernel(const uint8_t* __restrict__ cls, int64_t n, int nc, int64_t tiles,
                                                               const int64_t* __restrict__ off, int64_t* __restrict__ perm,
                                                               int64_t* __restrict__ class_counts) {
  __shared__ int wave_cnt[ST_THREADS / 64][RS_MAX_CLASSES + 1];
  const int64_t i = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
  const int k = row_slot(cls, i, n, nc);
  int before = slot_rank(k, nc, wave_cnt);
  __syncthreads();
  if (k >= 0 && k < nc) {
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before += wave_cnt[w][k];
    perm[off[(int64_t)k * tiles + blockIdx.x] + before] = i;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x <= nc)      // (off[(nc + 1) * tiles] = n: the scan's total)
    class_counts[threadIdx.x] = off[((int64_t)threadIdx.x + 1) * tiles] - off[(int64_t)threadIdx.x * tiles];
}

constexpr int64_t RSC_MAX_BLOCKS = 1 << 14;

// dst[perm[j]][:] = src[j][:], one lane per element; a perm entry outside [0, dst_rows) is skipped
template <typename T>
__global__ __launch_bounds__(ST_THREADS) void rows_scatter_kernel(const T* __restrict__ src, const int64_t* __restrict__ perm, int64_t m,
                                                                  int cols, int64_t dst_rows, T* __restrict__ dst) {
  const int64_t total = m * cols, step = (int64_t)gridDim.x * ST_THREADS;
  for (int64_t e = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x; e < total; e += step) {
    const int64_t j = e / cols, r = perm[j];
    if (r >= 0 && r < dst_rows) dst[r * cols + (e - j * cols)] = src[e];
  }
}

struct SiteGrid {
  int64_t lo, hi, word0, tiles;
};

SiteGrid site_grid(int64_t length, int64_t lo, int64_t hi) {
  SiteGrid s;
  s.lo = lo < 0 ? 0 : lo;
  s.hi = hi > length ? length : hi;
  if (s.hi < s.lo) s.hi = s.lo;
  s.word0 = s.lo / ST_WORD_BASES;
  const int64_t words = s.hi > s.lo ? (s.hi + ST_WORD_BASES - 1) / ST_WORD_BASES - s.word0 : 0;
  s.tiles = (words + ST_THREADS - 1) / ST_THREADS;
  return s;
}

int check_selection(const char* who, const MuralGenome* g, int32_t focal, int32_t context) {
  MURAL_REQUIRE(g && g->length >= 0 && (g->length == 0 || (g->packed2 && g->nmask)), "%s: bad genome", who);
  if (focal == MURAL_FOCAL_SET) {
    MURAL_REQUIRE(context >= 1 && context <= (MURAL_CLASS_A | MURAL_CLASS_NONCPG | MURAL_CLASS_CPG),
                  "%s: focal SET needs a non-empty union of MURAL_CLASS_* bits, got %d", who, context);
    return MURAL_OK;
  }
  MURAL_REQUIRE(focal == MURAL_FOCAL_A || focal == MURAL_FOCAL_C || focal == MURAL_FOCAL_ANY, "%s: bad focal selector %d", who, focal);
  MURAL_REQUIRE(context == MURAL_CONTEXT_ALL || context == MURAL_CONTEXT_CPG || context == MURAL_CONTEXT_NONCPG,
                "%s: bad context selector %d", who, context);
  MURAL_REQUIRE(context == MURAL_CONTEXT_ALL || focal == MURAL_FOCAL_C, "%s: a CpG context needs focal C", who);
  return MURAL_OK;
}

}  // namespace
}  // namespace mural

using namespace mural;

extern "C" int64_t mural_sites_tiles(int64_t length, int64_t lo, int64_t hi) { return site_grid(length < 0 ? 0 : length, lo, hi).tiles; }

extern "C" int mural_sites_count(const MuralGenome* g, int64_t lo, int64_t hi, int32_t focal, int32_t context, int64_t* tile_counts,
                                 int64_t* total, void* stream) {
  if (int rc = check_selection("sites_count", g, focal, context)) return rc;
  MURAL_REQUIRE(tile_counts && total, "sites_count: NULL argument");
  const SiteGrid s = site_grid(g->length, lo, hi);
  MURAL_REQUIRE(s.tiles < (1ll << 31), "sites_count: window too long");
  if (s.tiles)
    hipLaunchKernelGGL(sites_count_kernel, dim3((unsigned)s.tiles), dim3(ST_THREADS), 0, (hipStream_t)stream, *g, s.lo, s.hi, focal,
                       context, s.word0, tile_counts);
  hipLaunchKernelGGL(sites_scan_kernel, dim3(1), dim3(ST_THREADS), 0, (hipStream_t)stream, tile_counts, s.tiles, total);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" int mural_sites_emit(const MuralGenome* g, int64_t lo, int64_t hi, int32_t focal, int32_t context, const int64_t* tile_counts,
                                int64_t first, int64_t n, int64_t* pos, uint8_t* strand, void* stream) {
  if (int rc = check_selection("sites_emit", g, focal, context)) return rc;
  MURAL_REQUIRE(first >= 0 && n >= 0, "sites_emit: bad slice [%lld, +%lld)", (long long)first, (long long)n);
  const SiteGrid s = site_grid(g->length, lo, hi);
  MURAL_REQUIRE(s.tiles < (1ll << 31), "sites_emit: window too long");
  if (n == 0 || s.tiles == 0) return MURAL_OK;
  MURAL_REQUIRE(tile_counts && pos && strand, "sites_emit: NULL argument");
  hipLaunchKernelGGL(sites_emit_kernel, dim3((unsigned)s.tiles), dim3(ST_THREADS), 0, (hipStream_t)stream, *g, s.lo, s.hi, focal,
                     context, s.word0, tile_counts, first, n, pos, strand);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" int mural_sites_classify(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, int64_t n, uint8_t* cls, void* stream) {
  MURAL_REQUIRE(g && g->length >= 0 && (g->length == 0 || (g->packed2 && g->nmask)), "sites_classify: bad genome");
  MURAL_REQUIRE(n >= 0, "sites_classify: bad size n %lld", (long long)n);
  if (n == 0) return MURAL_OK;
  MURAL_REQUIRE(pos && strand && cls, "sites_classify: NULL argument");
  const int64_t blocks = (n + ST_THREADS - 1) / ST_THREADS;
  MURAL_REQUIRE(blocks < (1ll << 31), "sites_classify: too many rows");
  hipLaunchKernelGGL(sites_classify_kernel, dim3((unsigned)blocks), dim3(ST_THREADS), 0, (hipStream_t)stream, *g, pos, strand, n, cls);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" size_t mural_rows_split_workspace_bytes(int64_t n, int32_t n_classes) {
  if (n < 0 || n_classes < 1 || n_classes > RS_MAX_CLASSES) return 0;
  const int64_t tiles = (n + ST_THREADS - 1) / ST_THREADS;
  return (size_t)((n_classes + 1) * tiles + 1) * sizeof(int64_t);
}

extern "C" int mural_rows_split(const uint8_t* cls, int64_t n, int32_t n_classes, int64_t* perm, int64_t* counts, void* workspace,
                                size_t workspace_bytes, void* stream) {
  MURAL_REQUIRE(n >= 0 && n_classes >= 1 && n_classes <= RS_MAX_CLASSES, "rows_split: bad sizes n %lld, n_classes %d (1..%d)", (long long)n,
                n_classes, RS_MAX_CLASSES);
  MURAL_REQUIRE(counts, "rows_split: NULL counts");
  if (n == 0) {
    MURAL_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)(n_classes + 1) * sizeof(int64_t), (hipStream_t)stream));
    return MURAL_OK;
  }
  MURAL_REQUIRE(cls && perm && workspace, "rows_split: NULL argument");
  if (workspace_bytes < mural_rows_split_workspace_bytes(n, n_classes)) {
    set_error("rows_split: workspace of %zu bytes, %zu needed", workspace_bytes, mural_rows_split_workspace_bytes(n, n_classes));
    return MURAL_E_WORKSPACE;
  }
  const int64_t tiles = (n + ST_THREADS - 1) / ST_THREADS;
  MURAL_REQUIRE(tiles < (1ll << 31), "rows_split: too many rows");
  int64_t* off = (int64_t*)workspace;
  const int64_t entries = (n_classes + 1) * tiles;
  hipLaunchKernelGGL(rows_count_kernel, dim3((unsigned)tiles), dim3(ST_THREADS), 0, (hipStream_t)stream, cls, n, (int)n_classes, tiles, off);
  hipLaunchKernelGGL(sites_scan_kernel, dim3(1), dim3(ST_THREADS), 0, (hipStream_t)stream, off, entries, off + entries);
  hipLaunchKernelGGL(rows_emit_kernel, dim3((unsigned)tiles), dim3(ST_THREADS), 0, (hipStream_t)stream, cls, n, (int)n_classes, tiles,
                     (const int64_t*)off, perm, counts);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" int mural_rows_scatter(const void* src, const int64_t* perm, int64_t m, int32_t cols, int32_t elem_bytes, void* dst,
                                  int64_t dst_rows, void* stream) {
  MURAL_REQUIRE(m >= 0 && cols >= 1 && dst_rows >= 0, "rows_scatter: bad sizes m %lld, cols %d, dst_rows %lld", (long long)m, cols,
                (long long)dst_rows);
  MURAL_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "rows_scatter: elem_bytes %d (4 or 8)", elem_bytes);
  if (m == 0) return MURAL_OK;
  MURAL_REQUIRE(src && perm && dst, "rows_scatter: NULL argument");
  const int64_t blocks = (m * cols + ST_THREADS - 1) / ST_THREADS;
  const dim3 grid((unsigned)(blocks < RSC_MAX_BLOCKS ? blocks : RSC_MAX_BLOCKS));
  if (elem_bytes == 4)
    hipLaunchKernelGGL(rows_scatter_kernel<uint32_t>, grid, dim3(ST_THREADS), 0, (hipStream_t)stream, (const uint32_t*)src, perm, m,
                       (int)cols, dst_rows, (uint32_t*)dst);
  else
    hipLaunchKernelGGL(rows_scatter_kernel<uint64_t>, grid, dim3(ST_THREADS), 0, (hipStream_t)stream, (const uint64_t*)src, perm, m,
                       (int)cols, dst_rows, (uint64_t*)dst);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" int mural_sites_label(const int64_t* pos, const uint8_t* strand, int64_t n, const int64_t* mut_start, const uint8_t* mut_strand,
                                 const float* mut_label, int64_t m, int32_t check_strand, float* label, int64_t* stats, void* stream) {
  MURAL_REQUIRE(n >= 0 && m >= 0, "sites_label: bad sizes n %lld, m %lld", (long long)n, (long long)m);
  if (n == 0) return MURAL_OK;
  MURAL_REQUIRE(pos && strand && label && stats, "sites_label: NULL argument");
  if (m == 0) {                                              // no list for this chromosome: zeros, and no mut_* pointer is read
    MURAL_HIP_CHECK(hipMemsetAsync(label, 0, (size_t)n * sizeof(float), (hipStream_t)stream));
    return MURAL_OK;
  }
  MURAL_REQUIRE(mut_start && mut_strand && mut_label, "sites_label: NULL mutation list");
  const int64_t blocks = (n + ST_THREADS - 1) / ST_THREADS;
  hipLaunchKernelGGL(sites_label_kernel, dim3((unsigned)(blocks < SL_MAX_BLOCKS ? blocks : SL_MAX_BLOCKS)), dim3(ST_THREADS), 0,
                     (hipStream_t)stream, pos, strand, n, mut_start, mut_strand, mut_label, m, (int)check_strand, label,
                     (unsigned long long*)stats);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}
