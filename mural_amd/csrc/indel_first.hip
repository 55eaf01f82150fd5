// The conv of UNet_Small's input unit in training mode, from one symbol byte per window column (reference: the Conv1d of
// MuRaL/model/model_indel.py:29-32 applied at :154-155 with use_reverse, uplblocks[0]'s Conv1d otherwise; run under model.train(),
// MuRaL/training.py:424-436).
//
// An input column takes one of 15 values (MURAL_SYM_*), so a K-tap conv over the 4 channels is a sum of K table entries
//   T[co][k][s] = sum_c W[co][c][k] * dense(s)[c]        (dense = dense_symbol.h: symbol_to_dense)
// and its weight gradient is a histogram of dz keyed by (tap, symbol), contracted with dense(s)[c] at the end.  The dense
// [B][4][L] window (and, with use_reverse, its channel- and length-flipped copy) is never read: flip_CL of a column is the
// complement symbol's column at L - 1 - l (common.h: sym_complement), so both applications of the strand-symmetrising conv come from
// one staged span of bytes.
//
// LDS: the forward table is [K][16] float4 (4 output channels per entry): the 16 entries of a tap span 256 bytes = the 64 banks once,
// so lanes that hold different symbols read different banks and lanes that hold the same symbol read one address (broadcast) -- a
// table indexed by data without bank conflicts.  Symbol 15 (SYM_PAD) is the zero column: the conv's zero padding needs no branch.
// The backward keeps the 16 sums of a (channel, tap) pair in a thread's registers (compare-select per symbol) and meets the other
// slices through private LDS rows (row stride 17 words: a wave's 64 rows start in 64 different banks), so no atomics are needed and
// every sum has a fixed order.  Workgroups of 256 threads = 4 waves of 64.
#include "dense_symbol.h"
#include "indel_train.h"

namespace mural {
namespace {

constexpr int IF_THREADS = 256;
constexpr int IF_TL = 256;          // output positions per tile (one per thread in the forward)
constexpr int IF_COG = 4;           // output channels per workgroup
constexpr int IF_MAX_CHUNKS = 256;  // partial tables per application in the weight gradient (16 K floats each <= the dense route's 1024 rows of 4 K + 1)
constexpr int IF_ROW = 17;          // words per private histogram row (16 symbols + 1: odd stride)
constexpr int IF_DSROW = IF_TL + 2; // words per staged dz row (see the kernel)
typedef float f4 __attribute__((ext_vector_type(4)));

// the span of symbols the tile [l0, l0 + IF_TL) of output positions reads: sp[i] = symbol at input position l0 * stride - pad + i,
// SYM_PAD outside [0, L), N for a byte that is no symbol; complemented for the flipped application
__device__ __forceinline__ void stage_span(const uint8_t* __restrict__ row, int L, int base, int span, bool comp, uint8_t* sp) {
  for (int i = threadIdx.x; i < span; i += IF_THREADS) {
    const int p = base + i;
    uint32_t s = SYM_PAD;
    if (p >= 0 && p < L) {
      s = row[p];
      if (s > 14u) s = SYM_N;
      if (comp) s = sym_complement(s);
    }
    sp[i] = (uint8_t)s;
  }
}

// y[b][co][l] = bias[co] + sum_k T[co][k][sym[b][l * stride + k - pad]];  REV (stride 1, 2 * pad = K - 1, Lout = L): also
// yr[b][co][L - 1 - l] = bias[co] + sum_k T[co][k][complement(sym[b][l - k + pad])] -- the conv of flip_CL(x) at position L - 1 - l reads
// the same span of bytes.  Grid: (tiles, Cout / 4).
template <bool REV>
__global__ __launch_bounds__(IF_THREADS) void indel_first_fwd_kernel(const uint8_t* __restrict__ sym, const float* __restrict__ W,
                                                                     const float* __restrict__ bias, float* __restrict__ y,
                                                                     float* __restrict__ yr, int L, int Lout, int Cout, int K, int stride,
                                                                     int pad, int tiles_per_row, int64_t tiles) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  f4* tab = reinterpret_cast<f4*>(lds);                            // [K][16]
  uint8_t* sp = reinterpret_cast<uint8_t*>(tab + (size_t)K * 16);  // [span]
  const int co0 = blockIdx.y * IF_COG;
  for (int i = threadIdx.x; i < K * 16; i += IF_THREADS) {
    const int k = i >> 4, s = i & 15;
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (s < 15) {
      float d[4];
      symbol_to_dense((uint32_t)s, d, 1);
#pragma unroll
      for (int j = 0; j < IF_COG; ++j) {
        const float* w = W + (size_t)(co0 + j) * 4 * K + k;
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) a = fmaf(w[(size_t)c * K], d[c], a);
        v[j] = a;
      }
    }
    tab[i] = v;
  }
  f4 b4 = {0.f, 0.f, 0.f, 0.f};
  if (bias) b4 = f4{bias[co0], bias[co0 + 1], bias[co0 + 2], bias[co0 + 3]};
  const int span = (IF_TL - 1) * stride + K;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t b = tile / tiles_per_row;
    const int l0 = (int)(tile - b * tiles_per_row) * IF_TL;
    __syncthreads();      // the table is complete / the previous tile's span has been read
    stage_span(sym + (size_t)b * L, L, l0 * stride - pad, span, false, sp);
    __syncthreads();
    const int t = threadIdx.x, l = l0 + t;
    if (l >= Lout) continue;
    f4 acc = b4, accr = b4;
    const uint8_t* mine = sp + t * stride;
    for (int k = 0; k < K; ++k) {
      acc += tab[k * 16 + mine[k]];
      if (REV) accr += tab[k * 16 + sym_complement(mine[K - 1 - k])];
    }
    float* yo = y + ((size_t)b * Cout + co0) * Lout + l;
#pragma unroll
    for (int j = 0; j < IF_COG; ++j) yo[(size_t)j * Lout] = acc[j];
    if (REV) {
      float* ro = yr + ((size_t)b * Cout + co0) * Lout + (Lout - 1 - l);
#pragma unroll
      for (int j = 0; j < IF_COG; ++j) ro[(size_t)j * Lout] = accr[j];
    }
  }
}

// part[app * chunks + chunk][co][k][s] = sum over the chunk's tiles of dz[b][co][l] for the positions whose tap k reads symbol s
// (s = 15: the zero padding, so the 16 sums of a tap add up to sum dz).  Application 1 (the flipped input): dz1[b][co][L - 1 - l]
// with the complemented symbol at l - k + pad -- the same span, taps mirrored.  Grid: (chunks, Cout / 4, applications).
// Thread (slice, channel c, tap k) owns a private row of 16 sums and takes every `slices`-th position of a tile; the slices meet in
// a fixed order at the end.
__global__ __launch_bounds__(IF_THREADS) void indel_first_wgrad_kernel(const uint8_t* __restrict__ sym, const float* __restrict__ dz0,
                                                                       const float* __restrict__ dz1, float* __restrict__ part, int L,
                                                                       int Lout, int Cout, int K, int stride, int pad, int tiles_per_row,
                                                                       int64_t tiles, int chunks) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* ds = lds;                                      // [4][IF_DSROW]: rows 2 words apart in the banks, so the 4 channels x 2 slices
                                                        // (positions t, t + 1) a wave can ask for lie in different banks
  float* priv = ds + IF_COG * IF_DSROW;                 // [IF_THREADS][IF_ROW]
  uint8_t* sp = reinterpret_cast<uint8_t*>(priv + IF_THREADS * IF_ROW);
  const int app = blockIdx.z, co0 = blockIdx.y * IF_COG;
  const float* __restrict__ dz = app ? dz1 : dz0;
  const int np = IF_COG * K, slices = IF_THREADS / np;
  const int sl = threadIdx.x / np, q = threadIdx.x - sl * np, c = q / K, k = q - c * K;
  const bool active = sl < slices;
  const int koff = app ? K - 1 - k : k;
  // the 16 sums of this thread live in registers: a position adds its dz to the one whose index equals its symbol by 16 compare-selects
  // (an LDS read-modify-write per position is a chain of dependent round trips: it made the launch latency-bound)
  float bin[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) bin[s] = 0.f;
  const int span = (IF_TL - 1) * stride + K;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += chunks) {
    const int64_t b = tile / tiles_per_row;
    const int l0 = (int)(tile - b * tiles_per_row) * IF_TL;
    __syncthreads();
    for (int i = threadIdx.x; i < IF_COG * IF_TL; i += IF_THREADS) {
      const int cc = i / IF_TL, t = i - cc * IF_TL, l = l0 + t;
      float v = 0.f;
      if (l < Lout) v = dz[((size_t)b * Cout + co0 + cc) * Lout + (app ? Lout - 1 - l : l)];
      ds[cc * IF_DSROW + t] = v;
    }
    stage_span(sym + (size_t)b * L, L, l0 * stride - pad, span, app != 0, sp);
    __syncthreads();
    if (active) {
      const float* dc = ds + c * IF_DSROW;
      for (int t = sl; t < IF_TL; t += slices) {
        const int sy = sp[t * stride + koff];
        const float v = dc[t];
#pragma unroll
        for (int s = 0; s < 16; ++s) bin[s] += sy == s ? v : 0.f;
      }
    }
  }
  float* mine = priv + threadIdx.x * IF_ROW;
#pragma unroll
  for (int s = 0; s < 16; ++s) mine[s] = bin[s];
  __syncthreads();
  float* out = part + ((size_t)(app * chunks + blockIdx.x) * Cout + co0) * K * 16;
  for (int o = threadIdx.x; o < np * 16; o += IF_THREADS) {
    const int qq = o >> 4, s = o & 15;
    float sm = 0.f;
    for (int j = 0; j < slices; ++j) sm += priv[(j * np + qq) * IF_ROW + s];
    out[o] = sm;
  }
}

// dW[co][c][k] = sum_s dense(s)[c] * sum_chunks part[chunk][co][k][s], db[co] = sum_s sum_chunks part[chunk][co][0][s]; one
// workgroup per output channel, float64, the four waves take every fourth chunk and meet in LDS in a fixed order
__global__ __launch_bounds__(IF_THREADS) void indel_first_wgrad_reduce_kernel(const float* __restrict__ part, int nchunks, int Cout, int K,
                                                                              float* __restrict__ dW, float* __restrict__ db) {
  extern __shared__ __attribute__((aligned(16))) double sm[];      // [4][ne] + [ne]
  const int co = blockIdx.x, ne = K * 16;
  double* tot = sm + 4 * ne;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int e = lane; e < ne; e += 64) {
    double s = 0.0;
    for (int ch = wave; ch < nchunks; ch += 4) s += (double)part[((size_t)ch * Cout + co) * ne + e];
    sm[wave * ne + e] = s;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < ne; e += IF_THREADS) tot[e] = (sm[e] + sm[ne + e]) + (sm[2 * ne + e] + sm[3 * ne + e]);
  __syncthreads();
  for (int o = threadIdx.x; o < 4 * K; o += IF_THREADS) {
    const int c = o / K, k = o - c * K;
    double a = 0.0;
    for (int s = 0; s < 15; ++s) {
      float d[4];
      symbol_to_dense((uint32_t)s, d, 1);
      const float dv = c == 0 ? d[0] : c == 1 ? d[1] : c == 2 ? d[2] : d[3];
      a += tot[k * 16 + s] * (double)dv;
    }
    dW[((size_t)co * 4 + c) * K + k] = (float)a;
  }
  if (threadIdx.x == 0 && db) {
    double a = 0.0;
    for (int s = 0; s < 16; ++s) a += tot[s];
    db[co] = (float)a;
  }
}

// x[b][c][l] = dense(sym[b][l])[c]
__global__ __launch_bounds__(IF_THREADS) void symbols_to_dense_kernel(const uint8_t* __restrict__ sym, int64_t total, int L, float* __restrict__ x) {
  for (int64_t i = (int64_t)blockIdx.x * IF_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * IF_THREADS) {
    const int64_t b = i / L;
    uint32_t s = sym[i];
    if (s > 14u) s = SYM_N;
    symbol_to_dense(s, x + b * 4 * L + (i - b * L), L);
  }
}

int first_geometry(int64_t B, int L, int Cout, int K, int stride, int pad, bool rev, int* Lout) {
  MURAL_REQUIRE(B >= 1 && B <= (1 << 20) && L >= 1 && Cout >= 4 && Cout % IF_COG == 0, "indel_first: bad sizes (B %lld, L %d, Cout %d)", (long long)B,
                L, Cout);
  MURAL_REQUIRE(K >= 1 && K <= 63 && stride >= 1 && pad >= 0 && L + 2 * pad >= K, "indel_first: bad geometry (K %d, stride %d, pad %d)", K, stride,
                pad);
  MURAL_REQUIRE(!rev || (stride == 1 && 2 * pad == K - 1), "indel_first: the flipped application needs stride 1 and pad (K - 1) / 2");
  *Lout = (L + 2 * pad - K) / stride + 1;
  MURAL_REQUIRE((int64_t)B * Cout * *Lout < (int64_t(1) << 40), "indel_first: tensor too large");
  return MURAL_OK;
}

int chunks_of(int64_t tiles) { return (int)(tiles < IF_MAX_CHUNKS ? tiles : IF_MAX_CHUNKS); }

}  // namespace

size_t indel_first_scratch_floats(int64_t B, int Lout, int Cout, int K, int rev) {
  if (B < 1 || Lout < 1 || Cout < 1 || K < 1) return 0;
  const int64_t tiles = B * ((Lout + IF_TL - 1) / IF_TL);
  return (size_t)(rev ? 2 : 1) * chunks_of(tiles) * Cout * K * 16;
}

int indel_first_fwd(const uint8_t* sym, const float* W, const float* bias, int64_t B, int L, int Cout, int K, int stride, int pad, float* y,
                    float* y_rev, hipStream_t st) {
  int Lout = 0;
  if (int rc = first_geometry(B, L, Cout, K, stride, pad, y_rev != nullptr, &Lout)) return rc;
  MURAL_REQUIRE(sym && W && y, "indel_first_fwd: null pointer");
  const int tiles_per_row = (Lout + IF_TL - 1) / IF_TL;
  const int64_t tiles = B * tiles_per_row;
  const size_t lds = (size_t)K * 16 * sizeof(f4) + (size_t)(IF_TL - 1) * stride + K;
  MURAL_REQUIRE(lds <= 64 * 1024, "indel_first_fwd: %zu bytes of LDS (stride %d)", lds, stride);
  const dim3 grid((unsigned)(tiles < 4096 ? tiles : 4096), Cout / IF_COG);
  if (y_rev)
    hipLaunchKernelGGL(indel_first_fwd_kernel<true>, grid, dim3(IF_THREADS), lds, st, sym, W, bias, y, y_rev, L, Lout, Cout, K, stride, pad,
                       tiles_per_row, tiles);
  else
    hipLaunchKernelGGL(indel_first_fwd_kernel<false>, grid, dim3(IF_THREADS), lds, st, sym, W, bias, y, y_rev, L, Lout, Cout, K, stride, pad,
                       tiles_per_row, tiles);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

int indel_first_bwd(const uint8_t* sym, const float* dz, const float* dz_rev, int64_t B, int L, int Cout, int K, int stride, int pad, float* dW,
                    float* db, float* part, size_t part_floats, hipStream_t st) {
  int Lout = 0;
  const bool rev = dz_rev != nullptr;
  if (int rc = first_geometry(B, L, Cout, K, stride, pad, rev, &Lout)) return rc;
  MURAL_REQUIRE(sym && dz && dW && part, "indel_first_bwd: null pointer");
  MURAL_REQUIRE(part_floats >= indel_first_scratch_floats(B, Lout, Cout, K, rev), "indel_first_bwd: scratch too small");
  const int tiles_per_row = (Lout + IF_TL - 1) / IF_TL;
  const int64_t tiles = B * tiles_per_row;
  const int chunks = chunks_of(tiles), apps = rev ? 2 : 1;
  const size_t lds = (size_t)(IF_COG * IF_DSROW + IF_THREADS * IF_ROW) * sizeof(float) + (size_t)(IF_TL - 1) * stride + K;
  MURAL_REQUIRE(lds <= 64 * 1024, "indel_first_bwd: %zu bytes of LDS (stride %d)", lds, stride);
  hipLaunchKernelGGL(indel_first_wgrad_kernel, dim3(chunks, Cout / IF_COG, apps), dim3(IF_THREADS), lds, st, sym, dz, dz_rev, part, L, Lout, Cout,
                     K, stride, pad, tiles_per_row, tiles, chunks);
  MURAL_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(indel_first_wgrad_reduce_kernel, dim3(Cout), dim3(IF_THREADS), (size_t)5 * K * 16 * sizeof(double), st, part, apps * chunks,
                     Cout, K, dW, db);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

}  // namespace mural

using namespace mural;

extern "C" size_t mural_op_indel_first_scratch(int64_t B, int32_t L, int32_t Cout, int32_t K, int32_t stride, int32_t pad, int32_t rev) {
  if (B < 1 || L < 1 || K < 1 || stride < 1 || pad < 0 || L + 2 * pad < K) return 0;
  return indel_first_scratch_floats(B, (L + 2 * pad - K) / stride + 1, Cout, K, rev);
}

extern "C" int mural_op_indel_first_fwd(const uint8_t* sym, const float* W, const float* bias, int64_t B, int32_t L, int32_t Cout, int32_t K,
                                        int32_t stride, int32_t pad, float* y, float* y_rev, void* stream) {
  return indel_first_fwd(sym, W, bias, B, L, Cout, K, stride, pad, y, y_rev, (hipStream_t)stream);
}

extern "C" int mural_op_indel_first_bwd(const uint8_t* sym, const float* dz, const float* dz_rev, int64_t B, int32_t L, int32_t Cout, int32_t K,
                                        int32_t stride, int32_t pad, float* dW, float* db, float* part, size_t part_floats, void* stream) {
  return indel_first_bwd(sym, dz, dz_rev, B, L, Cout, K, stride, pad, dW, db, part, part_floats, (hipStream_t)stream);
}

extern "C" int mural_op_symbols_to_dense(const uint8_t* sym, int64_t n, int32_t L, float* x, void* stream) {
  MURAL_REQUIRE(n >= 0 && L >= 1, "symbols_to_dense: bad sizes");
  if (n == 0) return MURAL_OK;
  MURAL_REQUIRE(sym && x, "symbols_to_dense: null pointer");
  const int64_t total = n * L, g = (total + IF_THREADS - 1) / IF_THREADS;
  hipLaunchKernelGGL(symbols_to_dense_kernel, dim3((unsigned)(g > 16384 ? 16384 : g)), dim3(IF_THREADS), 0, (hipStream_t)stream, sym, total, L, x);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}
