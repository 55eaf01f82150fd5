// In-silico saturation mutagenesis around the SNV and INDEL forwards: the window "as if one base were different" (one row per (site, substitution)),
// the enumerator of a window's 3 * W substitutions, and the scatter of the re-predicted log-probabilities into the map; and the window on
// the alternate haplotype of an insertion, deletion or multi-base allele with the enumerator of the sites it reaches (section 3.29).
// Window, strand and k-mer-id rules are encode.hip's, through the same column helpers (encode_window.h; reference:
// MuRaL/data/preprocessing.py:636-723, 756-816; windows :559-567: SNV [pos - R, pos + R], INDEL [pos - R + 1, pos + R]).  The forward in
// between is mural_snv_forward_symbols or mural_indel_forward_symbols; for the latter mural_scores_log_softmax turns its Softplus
// scores into the log-probabilities the map is made of.
#include "common.h"
#include "encode_window.h"

namespace mural {

// The rows' base readers.  A row source is a small struct of table pointers whose operator() builds row i's reader; the window kernel
// below is written once over it.

// one substitution per row: none for sub_base > 3 (255 = "no substitution") or a position outside the record
struct SubstRows {
  const int64_t* __restrict__ sub_pos;
  const uint8_t* __restrict__ sub_base;
  __device__ __forceinline__ OneSubst operator()(const MuralGenome& g, int64_t row) const {
    const int64_t p = sub_pos[row];
    const uint32_t b = sub_base[row];
    return OneSubst{p, b & 3u, b < 4u && p >= 0 && p < g.length};
  }
};

// live: 0 <= p, 0 <= d, p + d <= length, 0 <= k <= 32 (written so that nothing overflows)
__device__ __forceinline__ bool allele_live(int64_t length, int64_t p, int64_t d, int64_t k) {
  return p >= 0 && p <= length && d >= 0 && d <= length - p && k >= 0 && k <= 32;
}

// one index into the allele table per row: -1 or any index outside [0, n_alleles), or an allele that is not live, reads the genome as it is
struct AlleleRows {
  const int64_t* __restrict__ allele;
  const int64_t* __restrict__ a_pos;
  const int64_t* __restrict__ a_ref_len;
  const int64_t* __restrict__ a_alt_len;
  const uint64_t* __restrict__ a_alt;
  int64_t n_alleles;
  __device__ __forceinline__ AlleleEdit operator()(const MuralGenome& g, int64_t row) const {
    const int64_t v = allele[row];
    if (v < 0 || v >= n_alleles) return AlleleEdit{0, 0, 0, 0ull, false};
    const int64_t p = a_pos[v], d = a_ref_len[v], k = a_alt_len[v];
    if (!allele_live(g.length, p, d, k)) return AlleleEdit{0, 0, 0, 0ull, false};
    return AlleleEdit{p, k, k - d, a_alt[v], true};
  }
};

// One launch for both outputs.  Units [0, sym_groups): 4 consecutive bytes of the flattened (row, column) index of `symbols` (one aligned
// 4-byte store where the group lies in one row, as encode_symbols_kernel does); units [sym_groups, sym_groups + n * ncol): one k-mer id.
// pos[] is in the coordinates of the rows' readers: the genome's for SubstRows, the alternate haplotype's for AlleleRows.
template <class Rows>
__global__ __launch_bounds__(256) void reader_windows_kernel(MuralGenome g, const int64_t* __restrict__ pos, const uint8_t* __restrict__ strand,
                                                             Rows rows, int64_t n, int W, int off, int lwidth, int lradius, int order, int ncol,
                                                             int64_t sym_groups, uint8_t* __restrict__ symbols, int64_t* __restrict__ cat_x) {
  const int64_t total_sym = symbols ? n * W : 0;
  const int64_t units = sym_groups + (cat_x ? n * ncol : 0);
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    if (u < sym_groups) {
      const int64_t i0 = u << 2;
      const int64_t row = i0 / W;
      const int j = (int)(i0 - row * W);
      if (j + 3 < W) {
        const int64_t ws = pos[row] + off;
        const bool neg = strand[row] != 0;
        const auto sub = rows(g, row);
        uint32_t packed = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) packed |= window_symbol(g, ws, W, neg, j + e, sub) << (8 * e);
        *reinterpret_cast<uint32_t*>(symbols + i0) = packed;
      } else {
        for (int e = 0; e < 4 && i0 + e < total_sym; ++e) {
          const int64_t i = i0 + e;
          const int64_t r = i / W;
          const int jj = (int)(i - r * W);
          symbols[i] = (uint8_t)window_symbol(g, pos[r] + off, W, strand[r] != 0, jj, rows(g, r));
        }
      }
    } else {
      const int64_t i = u - sym_groups;
      const int64_t row = i / ncol;
      const int col = (int)(i - row * ncol);
      cat_x[i] = window_kmer_id(g, pos[row] - lradius, lwidth, strand[row] != 0, col, order, rows(g, row));
    }
  }
}

// The sites an allele can reach.  Row id = v * (W - 1) + c: slot c of allele v is the site at e = c - (off + W - 1) (SNV: e in [-R, R - 1];
// INDEL: [-R, R - 2]); e < 0 lies left of the allele (ref_pos = alt_pos = p + e), e >= 0 right of the replaced span (ref_pos = p + d + e,
// alt_pos = ref_pos + k - d).  An allele that is not live enumerates as d = k = 0 around its p, with row_allele = -1.  (Sums of table
// values wrap instead of overflowing: such rows are dead anyway.)
__global__ __launch_bounds__(256) void allele_rows_kernel(int64_t length, const int64_t* __restrict__ a_pos, const int64_t* __restrict__ a_ref_len,
                                                          const int64_t* __restrict__ a_alt_len, const uint8_t* __restrict__ strand, int slots,
                                                          int e0, int64_t first, int64_t count, int64_t* __restrict__ ref_pos,
                                                          int64_t* __restrict__ alt_pos, uint8_t* __restrict__ row_strand,
                                                          int64_t* __restrict__ row_allele) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t id = first + i;
    const int64_t v = id / slots;
    const int64_t e = (int64_t)(id - v * slots) - e0;
    const int64_t p = a_pos[v];
    int64_t d = a_ref_len[v], k = a_alt_len[v];
    const bool live = allele_live(length, p, d, k);
    if (!live) d = k = 0;
    const uint64_t rp = (uint64_t)p + (uint64_t)e + (e < 0 ? 0ull : (uint64_t)d);
    ref_pos[i] = (int64_t)rp;
    alt_pos[i] = (int64_t)(e < 0 ? rp : rp + (uint64_t)(k - d));
    row_strand[i] = strand[v] != 0 ? 1 : 0;
    row_allele[i] = live ? v : -1;
  }
}

// variant id v = (site * W + j) * 3 + a  ->  the row (site's pos / strand) and its '+'-strand substitution
__global__ __launch_bounds__(256) void mutagenesis_rows_kernel(MuralGenome g, const int64_t* __restrict__ pos, const uint8_t* __restrict__ strand,
                                                               int W, int off, int64_t first, int64_t count, int64_t* __restrict__ row_pos,
                                                               uint8_t* __restrict__ row_strand, int64_t* __restrict__ sub_pos,
                                                               uint8_t* __restrict__ sub_base) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < count; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = first + k;
    const int64_t cell = v / 3;                  // site * W + j
    const uint32_t a = (uint32_t)(v - cell * 3);
    const int64_t site = cell / W;
    const int j = (int)(cell - site * W);
    const int64_t p = pos[site];
    const bool neg = strand[site] != 0;
    const uint32_t ref = window_symbol(g, p + off, W, neg, j, NoSubst{});      // window orientation
    uint32_t b = 255u;
    if (ref < 4u) {
      const uint32_t alt = a + (a >= ref ? 1u : 0u);                               // a-th of {A, C, G, T} \ {ref}, ascending
      b = neg ? 3u - alt : alt;                                                    // back on the '+' strand
    }
    row_pos[k] = p;
    row_strand[k] = neg ? 1 : 0;
    sub_pos[k] = window_genome_pos(p + off, W, neg, j);
    sub_base[k] = (uint8_t)b;
  }
}

// Every element of the maps has ONE writer among the ids of a run, whatever the chunking: in an A/C/G/T column id a writes its
// alternative's entry and id a = 0 the reference base's as well; in any other column id a writes entry a and id a = 2 entry 3 too.
// The maps are written as bit patterns: the library is built with -fno-honor-nans, a NaN must not pass through float code.
__global__ __launch_bounds__(256) void mutagenesis_reduce_kernel(const float* __restrict__ ref_logp, const float* __restrict__ var_logp,
                                                                 const uint8_t* __restrict__ ref_sym, int W, int C, int64_t first, int64_t count,
                                                                 uint32_t* __restrict__ delta, uint32_t* __restrict__ logp_map) {
  constexpr uint32_t NAN_BITS = 0x7fc00000u;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < count; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = first + k;
    const int64_t cell = v / 3;
    const uint32_t a = (uint32_t)(v - cell * 3);
    const int64_t site = cell / W;
    const uint32_t ref = ref_sym[cell];
    const float* __restrict__ rl = ref_logp + site * C;
    const float* __restrict__ vl = var_logp + k * C;
    const int64_t base = cell * 4 * C;
    if (ref < 4u) {
      const uint32_t alt = a + (a >= ref ? 1u : 0u);
      for (int c = 0; c < C; ++c) {
        const float x = vl[c];
        delta[base + alt * C + c] = __float_as_uint(x - rl[c]);
        if (logp_map) logp_map[base + alt * C + c] = __float_as_uint(x);
      }
      if (a == 0u) {
        for (int c = 0; c < C; ++c) {
          delta[base + ref * C + c] = 0u;                                          // +0.0
          if (logp_map) logp_map[base + ref * C + c] = __float_as_uint(rl[c]);
        }
      }
    } else {
      for (uint32_t b = a; b < (a == 2u ? 4u : a + 1u); ++b) {
        for (int c = 0; c < C; ++c) {
          delta[base + b * C + c] = NAN_BITS;
          if (logp_map) logp_map[base + b * C + c] = NAN_BITS;
        }
      }
    }
  }
}

// The map reduced over sites instead of written (section 3.30).  A term is one (variant id, class); its cell is [group][column][ref][a]
// [class], five words each (PW_*).  Everything added is an integer, so the table does not depend on which adds went through LDS, on the
// order they arrived in or on how the ids were chunked.
enum : int { PW_N = 0, PW_SUM = 1, PW_ABS = 2, PW_SQ_LO = 3, PW_SQ_HI = 4, PW_WORDS = 5 };
enum : int { PF_NONFINITE = 1, PF_RANGE = 2 };     // status[0] bits; status[1], status[2]: how many terms of each kind
constexpr int PROFILE_IDS_GLOBAL = 256;            // ids per block where every add is a global atomic
constexpr int PROFILE_IDS_LDS = 2048;              // ... and where the block sums in LDS first: one flush of the table per 2048 ids
constexpr int PROFILE_LDS_BYTES = 64 * 1024;

template <class Mem>
__device__ __forceinline__ void profile_add(Mem* __restrict__ cell, int64_t q) {
  const u64 mag = (u64)(q < 0 ? -q : q);                                           // < 2^38
  const u64 lo = mag * mag, hi = __umul64hi(mag, mag);                             // q^2 < 2^76
  atomicAdd(cell + PW_N, 1ull);
  if (q == 0) return;
  atomicAdd(cell + PW_SUM, (u64)q);
  atomicAdd(cell + PW_ABS, mag);
  if (lo & ((1ull << 40) - 1)) atomicAdd(cell + PW_SQ_LO, lo & ((1ull << 40) - 1));
  if ((lo >> 40) | hi) atomicAdd(cell + PW_SQ_HI, (lo >> 40) | (hi << 24));
}

// Block b owns the ids [b * ids_per_block, (b + 1) * ids_per_block) of the call, one thread per term.  Groups below lds_groups are summed
// in the block's LDS table (lds_groups * W * 12 * C * 5 words of dynamic shared memory) and flushed once, the others go to `table` directly.
__global__ __launch_bounds__(256) void mutagenesis_profile_kernel(const float* __restrict__ ref_logp, const float* __restrict__ var_logp,
                                                                  const uint8_t* __restrict__ ref_sym, const int32_t* __restrict__ group,
                                                                  int W, int C, int n_groups, int64_t first, int64_t count,
                                                                  int ids_per_block, int lds_groups, u64* __restrict__ table,
                                                                  u64* __restrict__ status) {
  extern __shared__ u64 lds_table[];
  const int64_t group_words = (int64_t)W * 12 * C * PW_WORDS;
  const int lds_words = (int)(lds_groups * group_words);
  for (int i = threadIdx.x; i < lds_words; i += blockDim.x) lds_table[i] = 0;
  if (lds_words) __syncthreads();
  const int64_t k0 = (int64_t)blockIdx.x * ids_per_block;
  const int64_t k1 = k0 + ids_per_block < count ? k0 + ids_per_block : count;
  u64 nonfinite = 0, range = 0;
  for (int64_t t = k0 * C + threadIdx.x; t < k1 * C; t += blockDim.x) {
    const int64_t k = t / C;
    const int c = (int)(t - k * C);
    const int64_t v = first + k;
    const int64_t cell = v / 3;                  // site * W + j
    const int a = (int)(v - cell * 3);
    const int64_t site = cell / W;
    const int j = (int)(cell - site * W);
    const uint32_t ref = ref_sym[cell];
    const int64_t g = group ? (int64_t)group[site] : 0;
    if (ref >= 4u || g < 0 || g >= n_groups) continue;
    // (judged on the bit pattern: the library is built with -fno-honor-nans)
    const float delta = var_logp[t] - ref_logp[site * C + c];
    const uint32_t mag = __float_as_uint(delta) & 0x7fffffffu;
    if (mag >= 0x43800000u) {                    // |delta| >= 256, infinite or NaN
      if (mag >= 0x7f800000u) ++nonfinite; else ++range;
      continue;
    }
    const int64_t q = (int64_t)rintf(delta * 1073741824.0f);                       // exact: a power of two, |q| < 2^38
    const int64_t at = ((((g * W + j) * 4 + ref) * 3 + a) * C + c) * PW_WORDS;
    if (g < lds_groups) profile_add(lds_table + at, q);
    else profile_add(table + at, q);
  }
  if (lds_words) {
    __syncthreads();
    for (int i = threadIdx.x; i < lds_words; i += blockDim.x) {
      const u64 x = lds_table[i];
      if (x) atomicAdd(table + i, x);
    }
  }
  nonfinite = wave_sum(nonfinite), range = wave_sum(range);
  if ((threadIdx.x & 63) == 0 && (nonfinite | range)) {
    atomicOr(status, (u64)((nonfinite ? PF_NONFINITE : 0) | (range ? PF_RANGE : 0)));
    if (nonfinite) atomicAdd(status + 1, nonfinite);
    if (range) atomicAdd(status + 2, range);
  }
}

// out[i][c] = s[c] - (max + log sum exp(s - max)): one thread per row, classes in ascending order, so a row's bits depend on nothing
// but the row
__global__ __launch_bounds__(256) void scores_log_softmax_kernel(const float* __restrict__ scores, int64_t n, int C, float* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float* __restrict__ s = scores + i * C;
    float mx = s[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, s[c]);
    float sum = 0.f;
    for (int c = 0; c < C; ++c) sum += expf(s[c] - mx);
    const float lse = mx + logf(sum);
    for (int c = 0; c < C; ++c) out[i * C + c] = s[c] - lse;
  }
}

static int grid_for(int64_t units, int block, int cap) {
  const int64_t blocks = (units + block - 1) / block;
  return (int)(blocks < cap ? blocks : cap);
}

}  // namespace mural

using namespace mural;

static int require_genome(const MuralGenome* g) {
  MURAL_REQUIRE(g && g->packed2 && g->nmask, "genome pointers must not be NULL");
  MURAL_REQUIRE(g->n_amb == 0 || (g->amb_pos && g->amb_sym), "genome: n_amb > 0 needs amb_pos and amb_sym");
  return MURAL_OK;
}

// symbols (window of `radius` / `indel`) and / or cat_x (the SNV local window) of the rows, read through the rows' readers
template <class Rows>
static int encode_rows(const char* who, const MuralGenome* g, const int64_t* pos, const uint8_t* strand, const Rows& rows, bool rows_ok,
                       int64_t n, int32_t radius, int32_t indel, int32_t local_radius, int32_t local_order, uint8_t* symbols, int64_t* cat_x,
                       void* stream) {
  if (int rc = require_genome(g)) return rc;
  MURAL_REQUIRE(n >= 0, "%s: n must be >= 0", who);
  int off = 0, W = 0, loff = 0, lwidth = 0, ncol = 0;
  if (symbols) {
    if (int rc = window_geometry(radius, indel, &off, &W)) return rc;
    MURAL_REQUIRE((reinterpret_cast<uintptr_t>(symbols) & 3u) == 0, "%s: symbols must be 4-byte aligned", who);
  }
  if (cat_x) {
    MURAL_REQUIRE(local_order >= 1 && local_order <= 12, "local_order must be in [1,12], got %d", local_order);
    if (int rc = window_geometry(local_radius, 0, &loff, &lwidth)) return rc;
    ncol = lwidth - (local_order - 1);
    MURAL_REQUIRE(ncol >= 1, "window too short for order %d", local_order);
  }
  if (n == 0 || (!symbols && !cat_x)) return MURAL_OK;
  MURAL_REQUIRE(pos && strand && rows_ok, "%s: the row arrays must not be NULL", who);
  MURAL_REQUIRE(n <= INT64_MAX / 4 / (W > ncol ? W : ncol), "%s: n out of range", who);
  const int64_t sym_groups = symbols ? (n * W + 3) / 4 : 0;
  const int64_t units = sym_groups + (cat_x ? n * ncol : 0);
  hipLaunchKernelGGL(reader_windows_kernel<Rows>, dim3(grid_for(units, 256, 16384)), dim3(256), 0, (hipStream_t)stream, *g, pos, strand, rows,
                     n, W, off, lwidth, (int)local_radius, (int)local_order, ncol, sym_groups, symbols, cat_x);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

static int encode_subst(const char* who, const MuralGenome* g, const int64_t* pos, const uint8_t* strand, const int64_t* sub_pos,
                        const uint8_t* sub_base, int64_t n, int32_t radius, int32_t indel, int32_t local_radius, int32_t local_order,
                        uint8_t* symbols, int64_t* cat_x, void* stream) {
  return encode_rows(who, g, pos, strand, SubstRows{sub_pos, sub_base}, sub_pos && sub_base, n, radius, indel, local_radius, local_order,
                     symbols, cat_x, stream);
}

extern "C" int mural_encode_subst_windows(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, const int64_t* sub_pos,
                                          const uint8_t* sub_base, int64_t n, int32_t radius, int32_t local_radius, int32_t local_order,
                                          uint8_t* symbols, int64_t* cat_x, void* stream) {
  return encode_subst("encode_subst_windows", g, pos, strand, sub_pos, sub_base, n, radius, 0, local_radius, local_order, symbols, cat_x, stream);
}

extern "C" int mural_encode_subst_symbols(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, const int64_t* sub_pos,
                                          const uint8_t* sub_base, int64_t n, int32_t radius, int32_t indel, uint8_t* symbols, void* stream) {
  MURAL_REQUIRE(n <= 0 || symbols, "encode_subst_symbols: symbols must not be NULL");
  return encode_subst("encode_subst_symbols", g, pos, strand, sub_pos, sub_base, n, radius, indel, 0, 0, symbols, nullptr, stream);
}

extern "C" int mural_mutagenesis_rows_window(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, int64_t n_sites, int32_t radius,
                                             int32_t indel, int64_t first, int64_t count, int64_t* row_pos, uint8_t* row_strand,
                                             int64_t* sub_pos, uint8_t* sub_base, void* stream) {
  if (int rc = require_genome(g)) return rc;
  int off, W;
  if (int rc = window_geometry(radius, indel, &off, &W)) return rc;
  MURAL_REQUIRE(n_sites >= 0 && n_sites <= INT64_MAX / (3 * (int64_t)W), "mutagenesis_rows: n_sites out of range");
  MURAL_REQUIRE(first >= 0 && count >= 0 && first <= n_sites * W * 3 - count,
                "mutagenesis_rows: ids [first, first + count) must lie in [0, n_sites * W * 3)");
  if (count == 0) return MURAL_OK;
  MURAL_REQUIRE(pos && strand && row_pos && row_strand && sub_pos && sub_base, "mutagenesis_rows: pointers must not be NULL");
  hipLaunchKernelGGL(mutagenesis_rows_kernel, dim3(grid_for(count, 256, 16384)), dim3(256), 0, (hipStream_t)stream, *g, pos, strand, W,
                     off, first, count, row_pos, row_strand, sub_pos, sub_base);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" int mural_mutagenesis_rows(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, int64_t n_sites, int32_t radius,
                                      int64_t first, int64_t count, int64_t* row_pos, uint8_t* row_strand, int64_t* sub_pos,
                                      uint8_t* sub_base, void* stream) {
  return mural_mutagenesis_rows_window(g, pos, strand, n_sites, radius, 0, first, count, row_pos, row_strand, sub_pos, sub_base, stream);
}

extern "C" int mural_mutagenesis_reduce_window(const float* ref_logp, const float* var_logp, const uint8_t* ref_symbols, int64_t n_sites,
                                               int32_t W, int32_t n_class, int64_t first, int64_t count, float* delta, float* logp_map,
                                               void* stream) {
  MURAL_REQUIRE(W >= 1, "mutagenesis_reduce: W must be >= 1, got %d", W);
  MURAL_REQUIRE(n_class >= 1, "mutagenesis_reduce: n_class must be >= 1, got %d", n_class);
  MURAL_REQUIRE(n_sites >= 0 && n_sites <= INT64_MAX / (4 * (int64_t)W * n_class), "mutagenesis_reduce: n_sites out of range");
  MURAL_REQUIRE(first >= 0 && count >= 0 && first <= n_sites * W * 3 - count,
                "mutagenesis_reduce: ids [first, first + count) must lie in [0, n_sites * W * 3)");
  if (count == 0) return MURAL_OK;
  MURAL_REQUIRE(ref_logp && var_logp && ref_symbols && delta, "mutagenesis_reduce: pointers must not be NULL");
  hipLaunchKernelGGL(mutagenesis_reduce_kernel, dim3(grid_for(count, 256, 16384)), dim3(256), 0, (hipStream_t)stream, ref_logp, var_logp,
                     ref_symbols, (int)W, (int)n_class, first, count, reinterpret_cast<uint32_t*>(delta), reinterpret_cast<uint32_t*>(logp_map));
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" int mural_mutagenesis_reduce(const float* ref_logp, const float* var_logp, const uint8_t* ref_symbols, int64_t n_sites,
                                        int32_t radius, int32_t n_class, int64_t first, int64_t count, float* delta, float* logp_map,
                                        void* stream) {
  int off, W;
  if (int rc = window_geometry(radius, 0, &off, &W)) return rc;
  return mural_mutagenesis_reduce_window(ref_logp, var_logp, ref_symbols, n_sites, W, n_class, first, count, delta, logp_map, stream);
}

extern "C" int mural_mutagenesis_profile_window(const float* ref_logp, const float* var_logp, const uint8_t* ref_symbols, const int32_t* group,
                                                int64_t n_sites, int32_t W, int32_t n_class, int32_t n_groups, int64_t first, int64_t count,
                                                uint64_t* table, uint64_t* status, void* stream) {
  MURAL_REQUIRE(W >= 1, "mutagenesis_profile: W must be >= 1, got %d", W);
  MURAL_REQUIRE(n_class >= 1, "mutagenesis_profile: n_class must be >= 1, got %d", n_class);
  MURAL_REQUIRE(n_groups >= 1, "mutagenesis_profile: n_groups must be >= 1, got %d", n_groups);
  MURAL_REQUIRE(n_sites >= 0 && n_sites <= (int64_t)1 << 24,
                "mutagenesis_profile: at most 2^24 sites per call (a cell's sums are sized for 2^24 terms of |q| < 2^38), got %lld",
                (long long)n_sites);
  const int64_t group_words = (int64_t)W * 12 * n_class * PW_WORDS;
  MURAL_REQUIRE(group_words <= INT64_MAX / 8 / n_groups && n_sites <= INT64_MAX / (3 * (int64_t)W) / n_class,
                "mutagenesis_profile: sizes out of range");
  MURAL_REQUIRE(first >= 0 && count >= 0 && first <= n_sites * W * 3 - count,
                "mutagenesis_profile: ids [first, first + count) must lie in [0, n_sites * W * 3)");
  if (count == 0) return MURAL_OK;
  MURAL_REQUIRE(ref_logp && var_logp && ref_symbols && table && status, "mutagenesis_profile: pointers must not be NULL");
  // the groups that fit are summed per block in LDS; a call of few ids (no contention to speak of) adds to the table directly
  int64_t lds_groups = PROFILE_LDS_BYTES / 8 / group_words;
  if (lds_groups > n_groups) lds_groups = n_groups;
  if (count < 4 * PROFILE_IDS_LDS) lds_groups = 0;
  const int ids_per_block = lds_groups ? PROFILE_IDS_LDS : PROFILE_IDS_GLOBAL;
  const int64_t blocks = (count + ids_per_block - 1) / ids_per_block;
  MURAL_REQUIRE(blocks <= INT32_MAX, "mutagenesis_profile: count out of range");
  hipLaunchKernelGGL(mutagenesis_profile_kernel, dim3((unsigned)blocks), dim3(256), (size_t)(lds_groups * group_words * 8), (hipStream_t)stream,
                     ref_logp, var_logp, ref_symbols, group, (int)W, (int)n_class, (int)n_groups, first, count, ids_per_block, (int)lds_groups,
                     reinterpret_cast<u64*>(table), reinterpret_cast<u64*>(status));
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" int mural_scores_log_softmax(const float* scores, int64_t n, int32_t n_class, float* out, void* stream) {
  MURAL_REQUIRE(n >= 0 && n_class >= 1 && n <= INT64_MAX / n_class / 4, "scores_log_softmax: bad sizes (n %lld, n_class %d)", (long long)n, n_class);
  if (n == 0) return MURAL_OK;
  MURAL_REQUIRE(scores && out, "scores_log_softmax: pointers must not be NULL");
  hipLaunchKernelGGL(scores_log_softmax_kernel, dim3(grid_for(n, 256, 16384)), dim3(256), 0, (hipStream_t)stream, scores, n, (int)n_class, out);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" int mural_encode_allele_windows(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, const int64_t* allele, int64_t n,
                                           const int64_t* a_pos, const int64_t* a_ref_len, const int64_t* a_alt_len, const uint64_t* a_alt,
                                           int64_t n_alleles, int32_t radius, int32_t indel, int32_t local_radius, int32_t local_order,
                                           uint8_t* symbols, int64_t* cat_x, void* stream) {
  MURAL_REQUIRE(n_alleles >= 0, "encode_allele_windows: n_alleles must be >= 0");
  const bool tables = n_alleles == 0 || (a_pos && a_ref_len && a_alt_len && a_alt);
  return encode_rows("encode_allele_windows", g, pos, strand, AlleleRows{allele, a_pos, a_ref_len, a_alt_len, a_alt, n_alleles},
                     allele && tables, n, radius, indel, local_radius, local_order, symbols, cat_x, stream);
}

extern "C" int mural_allele_rows(const MuralGenome* g, const int64_t* a_pos, const int64_t* a_ref_len, const int64_t* a_alt_len,
                                 int64_t n_alleles, const uint8_t* strand, int32_t radius, int32_t indel, int64_t first, int64_t count,
                                 int64_t* ref_pos, int64_t* alt_pos, uint8_t* row_strand, int64_t* row_allele, void* stream) {
  if (int rc = require_genome(g)) return rc;
  int off, W;
  if (int rc = window_geometry(radius, indel, &off, &W)) return rc;
  const int slots = W - 1;
  MURAL_REQUIRE(n_alleles >= 0 && n_alleles <= INT64_MAX / slots, "allele_rows: n_alleles out of range");
  MURAL_REQUIRE(first >= 0 && count >= 0 && first <= n_alleles * slots - count,
                "allele_rows: ids [first, first + count) must lie in [0, n_alleles * (W - 1))");
  if (count == 0) return MURAL_OK;
  MURAL_REQUIRE(a_pos && a_ref_len && a_alt_len && strand && ref_pos && alt_pos && row_strand && row_allele,
                "allele_rows: pointers must not be NULL");
  hipLaunchKernelGGL(allele_rows_kernel, dim3(grid_for(count, 256, 16384)), dim3(256), 0, (hipStream_t)stream, g->length, a_pos, a_ref_len,
                     a_alt_len, strand, slots, off + W - 1, first, count, ref_pos, alt_pos, row_strand, row_allele);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}
