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

// '+' and '-' site masks of 64-bit word `wi` (bases [32 wi, 32 wi + 32)) for the window [lo, hi) of the record
__device__ __forceinline__ void site_masks(const MuralGenome& g, int64_t lo, int64_t hi, int focal, int context, int64_t wi,
                                           uint64_t* plus, uint64_t* minus) {
  *plus = *minus = 0ull;
  const int64_t n16 = (g.length + 15) >> 4, n32 = (g.length + 31) >> 5;      // words of packed2 / nmask
  if (wi < 0 || wi >= n32) return;
  const int64_t p0 = wi * ST_WORD_BASES;
  const uint64_t w = (uint64_t)g.packed2[2 * wi] | (2 * wi + 1 < n16 ? (uint64_t)g.packed2[2 * wi + 1] << 32 : 0ull);
  // exactly A / C / G / T: inside the record and not masked (N, IUPAC)
  const uint64_t valid = ~spread32(g.nmask[wi]) & first_bases(g.length - p0);
  const uint64_t win = first_bases(hi - p0) & ~first_bases(lo - p0);
  const uint64_t L = w & EVEN, H = (w >> 1) & EVEN;
  if (focal == MURAL_FOCAL_ANY) {
    *plus = valid & win;
  } else if (focal == MURAL_FOCAL_A) {
    *plus = ~H & ~L & valid & win;
    *minus = H & L & valid & win;
  } else {
    const uint64_t c = ~H & L & valid, gg = H & ~L & valid;
    uint64_t p = c, m = gg;
    if (context != MURAL_CONTEXT_ALL) {
      // the neighbours across the word borders come from the adjacent words of the RECORD (the window does not matter); a missing,
      // masked or ambiguous neighbour is no G / no C
      uint64_t g_next = 0ull, c_prev = 0ull;
      if (wi + 1 < n32) g_next = ((g.packed2[2 * wi + 2] & 3u) == 2u && (g.nmask[wi + 1] & 1u) == 0u) ? 1ull : 0ull;
      if (wi > 0) c_prev = ((g.packed2[2 * wi - 1] >> 30) == 1u && (g.nmask[wi - 1] >> 31) == 0u) ? 1ull : 0ull;
      const uint64_t next_is_g = (gg >> 2) | (g_next << 62), prev_is_c = (c << 2) | c_prev;
      if (context == MURAL_CONTEXT_CPG) {
        p = c & next_is_g;
        m = gg & prev_is_c;
      } else {
        p = c & ~next_is_g;
        m = gg & ~prev_is_c;
      }
    }
    *plus = p & win;
    *minus = m & win;
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
  const int64_t per = (nt + ST_THREADS - 1) / ST_THREADS;
  const int64_t b0 = (int64_t)threadIdx.x * per;
  int64_t s = 0;
  for (int64_t b = b0; b < b0 + per && b < nt; ++b) s += counts[b];
  __shared__ int64_t part[ST_THREADS];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t acc = 0;
    for (int t = 0; t < ST_THREADS; ++t) {
      const int64_t v = part[t];
      part[t] = acc;
      acc += v;
    }
    counts[nt] = acc;
    *total = acc;
  }
  __syncthreads();
  int64_t acc = part[threadIdx.x];
  for (int64_t b = b0; b < b0 + per && b < nt; ++b) {      // (every thread reads and writes its own tiles only)
    const int64_t v = counts[b];
    counts[b] = acc;
    acc += v;
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
