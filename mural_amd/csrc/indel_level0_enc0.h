// The persistent first-level kernel of the INDEL forward (see indel_level0.hip, which instantiates and launches it for the packed genome
// and for the dense entry's classified bytes; indel_level0_symbols.hip does so for the symbols entry).
#pragma once
#include <cstdlib>

#include "conv1d.h"
#include "mfma_tile.h"

namespace mural {
namespace {

constexpr int E0_OUT = 252;         // output positions per tile (= the split form's tile, so tail / tile bookkeeping is shared)
static_assert(E0_OUT == CB_FRONT_OUT, "the level-0 encoder tile is the split form's (convblock_tiles_of)");
constexpr int E0_OUT_DOWN = 248;    // ... of the form that also emits the next level's stride-4 conv (62 columns of it per tile)
constexpr int E0_PITCH = 272;       // = 16 (mod 32) floats
constexpr int E0_C = 8;

__device__ __forceinline__ float silu0(float v) { return v * __builtin_amdgcn_rcpf(1.f + __expf(-v)); }

struct E0Words { uint32_t w[2], m[2]; };   // genome words of a thread's one or two columns of a tile (2-bit bases, not-ACGT mask)

// BYTES: the window's symbols come from one byte per column (ConvBlockArgs::sym_in [B][Lf], the dense entry's one-hot windows
// classified by dense_to_symbols_kernel) instead of the packed genome; a column that is no MuRaL symbol (E0_SYM_DENSE) sends its
// neighbourhood through the exact form, which reads that column's four floats from the dense window itself (f_in [B][4][Lf]).
// SYMS (with BYTES): the bytes are the caller's (symbols entry; instantiated in indel_level0_symbols.hip) and nothing backs them: a
// byte above 14 is staged as N, so the E0_SYM_DENSE branch does not exist in these instances and f_in is never dereferenced.
constexpr uint32_t E0_SYM_DENSE = 16;
template <int TT, bool STAMPS, bool DOWN, bool BYTES = false, bool SYMS = false>
__global__ __launch_bounds__(256, 4) void indel_enc0_kernel(const ConvBlockArgs a, const float* __restrict__ w5, const float* __restrict__ b5,
                                                            const float* __restrict__ w1, const float* __restrict__ b1,
                                                            int tiles_per_row, long long total_tiles, unsigned long long* stamps) {
  constexpr int HW = (TT - 1) / 2;           // half width of the composed conv
  constexpr int ST = TT - 6;                 // taps of the per-symbol layer in front (7 or 1)
  constexpr int NG = (TT - 1) / 3;           // groups of three taps; the last tap goes alone
  constexpr int NSYM = 256 + TT - 1;         // columns a tile decodes: positions l0 + XO - HW .. l0 + XO + 255 + HW
  // DOWN: the tile also emits the next level's strided conv (8 -> 16, k = 7, stride 4, model_indel.py:39-42) of its outputs: 62 columns
  // of it per tile need the block's outputs from three positions in front of the tile's own 248, so the tile's origin moves by four
  constexpr int OUTW = DOWN ? E0_OUT_DOWN : E0_OUT;      // outputs stored per tile
  constexpr int XO = DOWN ? -6 : -2;                     // tile entry p <-> position l0 + XO + p; block output o <-> position l0 + XO + 2 + o
  constexpr int OLO = DOWN ? 4 : 0;                      // block outputs OLO .. OLO + OUTW - 1 are the tile's own
  static_assert(TT == 13 || TT == 7, "composed taps");
  unsigned long long t_prev = STAMPS ? __builtin_amdgcn_s_memrealtime() : 0ull;
  if (STAMPS && threadIdx.x == 0) stamps[8 * blockIdx.x + 6] = t_prev;      // (absolute: when the workgroup started)
#define E0_STAMP(id)                                                           \
  if (STAMPS && threadIdx.x == 0) {                                            \
    const unsigned long long t_now = __builtin_amdgcn_s_memrealtime();         \
    stamps[8 * blockIdx.x + (id)] += t_now - t_prev;                           \
    t_prev = t_now;                                                            \
  }
  __shared__ __attribute__((aligned(16))) float tile[E0_C * E0_PITCH];       // block input x, entry p = position l0 - 2 + p
  // rows of the 3-mer table at a pitch of 12 floats: a lane reads 32 bytes of a random row, and at a pitch of 8 the rows start on
  // 8 distinct bank positions (conflict rate 0.43 of the launch's LDS cycles); 12 gives 16
  constexpr int T3P = 12;
  __shared__ __attribute__((aligned(16))) float t3s[NG * 64 * T3P];
  __shared__ __attribute__((aligned(16))) float t1s[4 * E0_C + E0_C];        // single-tap table | bias of the composed conv
  __shared__ __attribute__((aligned(16))) float stabS[15 * ST * 4 + 4];      // exact form: per-symbol layer | its bias
  __shared__ __attribute__((aligned(16))) float fwS[4 * 7 * E0_C + E0_C];    // exact form: k = 7 conv [ci][k][co] | its bias
  __shared__ __attribute__((aligned(16))) float biasS[16 + E0_C + 16];       // b5 | b1 | bias of the strided conv (read per tile: fewer registers across the loop)
  __shared__ uint32_t planes[3 * 12];                                        // low bit | high bit | not-ACGT, 320 columns each (+ pad)
  __shared__ uint8_t symb[320];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n16 = tid & 15, kk = (tid >> 4) & 3;

  for (int i = tid; i < NG * 64 * E0_C; i += 256) t3s[(i >> 3) * T3P + (i & 7)] = a.e0_t3[i];
  if (tid < 5 * E0_C) t1s[tid] = tid < 4 * E0_C ? a.e0_t1[tid] : a.e0_bias[tid - 4 * E0_C];
  for (int i = tid; i < 15 * ST * 4 + 4; i += 256) stabS[i] = i < 15 * ST * 4 ? a.symtab[i] : a.sym_bias[i - 15 * ST * 4];
  if (tid < 4 * 7 * E0_C + E0_C) fwS[tid] = tid < 4 * 7 * E0_C ? a.f_w[tid] : a.f_b[tid - 4 * 7 * E0_C];
  // the dead lanes behind the last output of a tile (o = 252 .. 255) read entries 256 .. 259: they meet live values in the paired 1x1
  // conv (multiplied by the zero half of A), so they must be finite
  if (tid < 4 * E0_C) tile[(tid >> 2) * E0_PITCH + 256 + (tid & 3)] = 0.f;
  // A fragments, lane (m = n16, kk): k = 5 conv, k-step s = (tap s / 2, ci 4 (s % 2) + kk); 1x1 conv on block PAIRS (b, b + 2)
  // (A = [W1 0] against block b, [0 W1] against block b + 2: one register per k-step, the zero half made by a lane mask at the use)
  float a5[10], a1w[4];
#pragma unroll
  for (int s = 0; s < 10; ++s) a5[s] = w5[((4 * (s & 1) + kk) * 5 + (s >> 1)) * 16 + n16];
#pragma unroll
  for (int q = 0; q < 4; ++q) a1w[q] = w1[(4 * kk + q) * E0_C + (n16 & 7)];
  if (tid < 16 + E0_C) biasS[tid] = tid < 16 ? b5[tid] : b1[tid - 16];
  // DOWN: A fragments of the strided conv, k-step s = (tap s / 2, ci 4 (s % 2) + kk), weights [8][7][16]
  float ad[DOWN ? 14 : 1];
  if constexpr (DOWN) {
#pragma unroll
    for (int s = 0; s < 14; ++s) ad[s] = a.d_w[((4 * (s & 1) + kk) * 7 + (s >> 1)) * 16 + n16];
    if (tid < 16) biasS[16 + E0_C + tid] = a.d_b[tid];
  }

  const long long first = total_tiles * (long long)blockIdx.x / (long long)gridDim.x;
  const long long last = total_tiles * ((long long)blockIdx.x + 1) / (long long)gridDim.x;
  if (first >= last) return;
  int b = (int)(first / tiles_per_row);
  int tile_no = (int)(first - (long long)b * tiles_per_row);
  const int Lf = a.Lf;
  const long long glen = BYTES ? (long long)a.B * a.Lf : a.genome.length;      // BYTES: "genome" = the symbol rows end to end, a row's origin = b Lf

  // a column's place in the genome: window column j of row (ws, neg)
  auto column = [&](int i, int l0, long long ws, bool neg, bool& inwin, bool& ing, long long& g) {
    const int j = l0 + XO - HW + i;
    inwin = (unsigned)j < (unsigned)Lf;
    g = neg ? ws + (long long)(Lf - 1 - j) : ws + (long long)j;
    ing = inwin && g >= 0 && g < glen;
  };
  auto request = [&](int tid, int l0, long long ws, bool neg, E0Words& p) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (r == 1 && wave != 0) break;                       // columns 256 .. : the first wave's second round
      bool inwin, ing;
      long long g;
      column(tid + 256 * r, l0, ws, neg, inwin, ing, g);
      const long long gi = ing ? g : 0;
      if constexpr (BYTES) {
        p.w[r] = a.sym_in[gi];
        p.m[r] = 0u;
      } else {
        p.w[r] = a.genome.packed2[gi >> 4];
        p.m[r] = a.genome.nmask[gi >> 5];
      }
    }
  };

  // (a row's origin and strand are wave-uniform: kept in scalar registers)
  auto uniform64 = [](long long v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
  };
  long long ws = BYTES ? (long long)b * Lf : uniform64(a.g_pos[b] + a.g_off);
  bool neg = BYTES ? false : __builtin_amdgcn_readfirstlane((int)a.g_strand[b]) != 0;
  E0Words cur;
  cur.w[1] = cur.m[1] = 0u;
  request(threadIdx.x, tile_no * OUTW, ws, neg, cur);
  E0_STAMP(0);

#pragma unroll 1
  for (long long tix = first; tix < last; ++tix) {
    const int l0 = tile_no * OUTW;
    // (the lane's address pieces are loop-invariant and the compiler keeps them in ~20 registers: 91 in all, five waves per SIMD --
    // re-deriving them per tile from an opaque thread index fits seven waves per SIMD at 59 registers and is 3 % slower: the
    // launch is bound by instruction issue, not by latency, so registers are cheaper than instructions)
    const int tid = threadIdx.x;
    const int lane = tid & 63, n16 = tid & 15, kk = (tid >> 4) & 3;
    // ---------------------------------------------------------------- symbols of the tile's columns -> bit planes (+ bytes for the exact form)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (r == 1 && wave != 0) break;
      const int i = tid + 256 * r;
      bool inwin, ing;
      long long g;
      column(i, l0, ws, neg, inwin, ing, g);
      uint32_t sy;
      if constexpr (BYTES) {
        sy = cur.w[r];      // (every column of the window has its byte: ing == inwin)
        if constexpr (SYMS) sy = sy > 14u ? (uint32_t)SYM_N : sy;
      } else {
        const bool masked = ((cur.m[r] >> (uint32_t)(g & 31)) & 1u) != 0u;
        sy = (cur.w[r] >> (2u * (uint32_t)(g & 15))) & 3u;
        sy = (ing && !masked) ? sy : (uint32_t)SYM_N;
        if (ing && masked && a.genome.n_amb > 0) sy = genome_sym_iupac(a.genome, g);      // ambiguity codes: the sparse side table
        if (neg) sy = sym_complement(sy);
      }
      sy = (inwin && i < NSYM) ? sy : (uint32_t)SYM_PAD;
      const unsigned long long blo = __ballot((sy & 1u) != 0u), bhi = __ballot((sy & 2u) != 0u), bna = __ballot(sy >= 4u);
      symb[i] = (uint8_t)sy;
      if (lane == 0) {
        const int wq = 2 * (wave + 4 * r);
        planes[wq] = (uint32_t)blo;
        planes[wq + 1] = (uint32_t)(blo >> 32);
        planes[12 + wq] = (uint32_t)bhi;
        planes[12 + wq + 1] = (uint32_t)(bhi >> 32);
        planes[24 + wq] = (uint32_t)bna;
        planes[24 + wq + 1] = (uint32_t)(bna >> 32);
      }
    }
    __syncthreads();                       // (also: the previous tile's block has read the tile)
    E0_STAMP(1);
    // ---------------------------------------------------------------- the next tile's genome words, in flight under this tile's work
    int nb = b, ntile = tile_no + 1;
    if (ntile == tiles_per_row) {
      ntile = 0;
      ++nb;
    }
    long long nws = ws;
    bool nneg = neg;
    E0Words nxt;
    nxt.w[0] = nxt.m[0] = nxt.w[1] = nxt.m[1] = 0u;
    if (tix + 1 < last) {
      if (nb != b) {
        nws = BYTES ? (long long)nb * Lf : uniform64(a.g_pos[nb] + a.g_off);
        nneg = BYTES ? false : __builtin_amdgcn_readfirstlane((int)a.g_strand[nb]) != 0;
      }
      request(tid, ntile * OUTW, nws, nneg, nxt);
    }
    // ---------------------------------------------------------------- front: x[.][l0 - 2 + tid]
    {
      const int l = l0 + XO + tid;
      const int wd = tid >> 5;
      const uint32_t sh = (uint32_t)(tid & 31);
      const uint32_t lo = __builtin_amdgcn_alignbit(planes[wd + 1], planes[wd], sh);
      const uint32_t hi = __builtin_amdgcn_alignbit(planes[12 + wd + 1], planes[12 + wd], sh);
      const uint32_t na = __builtin_amdgcn_alignbit(planes[24 + wd + 1], planes[24 + wd], sh);
      f32x4 x0 = ld4(t1s + 4 * E0_C), x1 = ld4(t1s + 4 * E0_C + 4);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const uint32_t code = ((lo >> (3 * g)) & 7u) | (((hi >> (3 * g)) & 7u) << 3);
        const float* r = t3s + (g * 64 + (int)code) * T3P;
        x0 += ld4(r);
        x1 += ld4(r + 4);
      }
      {
        const uint32_t s = ((lo >> (TT - 1)) & 1u) | (((hi >> (TT - 1)) & 1u) << 1);
        const float* r = t1s + (int)s * E0_C;
        x0 += ld4(r);
        x1 += ld4(r + 4);
      }
      if ((na & ((1u << TT) - 1u)) != 0u) {
        // exact form: S = per-symbol layer on the columns inside the window, x = k = 7 conv of S with S zero outside the window
        f32x4 e0 = ld4(fwS + 4 * 7 * E0_C), e1 = ld4(fwS + 4 * 7 * E0_C + 4);
#pragma unroll 1
        for (int k2 = 0; k2 < 7; ++k2) {
          const int j = l + k2 - 3;
          if ((unsigned)j >= (unsigned)Lf) continue;
          f32x4 S = ld4(stabS + 15 * ST * 4);
          if constexpr (BYTES && !SYMS) {
#pragma unroll 1
            for (int k = 0; k < ST; ++k) {      // (rolled: this instance's slow path also reads the dense window; unrolled it spilled 49 registers)
              const uint32_t sy = symb[tid + k2 + k];
              if (sy == E0_SYM_DENSE) {         // no symbol: the layer is linear in the column's four floats
                const int jc = l0 + XO - HW + tid + k2 + k;
                const float* dv = a.f_in + (size_t)b * 4 * Lf + jc;
#pragma unroll 1
                for (int ci = 0; ci < 4; ++ci) S += splat(dv[(size_t)ci * Lf]) * ld4(stabS + (ci * ST + k) * 4);
              } else if (sy != SYM_PAD) S += ld4(stabS + ((int)sy * ST + k) * 4);
            }
          } else {
#pragma unroll
          for (int k = 0; k < ST; ++k) {
            const uint32_t sy = symb[tid + k2 + k];
            if (sy != SYM_PAD) S += ld4(stabS + ((int)sy * ST + k) * 4);
          }
          }
#pragma unroll
          for (int ci = 0; ci < 4; ++ci) {
            const float* wr = fwS + (ci * 7 + k2) * E0_C;
            e0 += splat(S[ci]) * ld4(wr);
            e1 += splat(S[ci]) * ld4(wr + 4);
          }
        }
        x0 = e0;
        x1 = e1;
      }
      const bool in = l >= 0 && l < a.L;                 // the k = 5 conv zero-pads ITS input
      if (!in) x0 = x1 = splat(0.f);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        tile[c * E0_PITCH + tid] = x0[c];
        tile[(c + 4) * E0_PITCH + tid] = x1[c];
      }
    }
    __syncthreads();
    E0_STAMP(2);
    // ---------------------------------------------------------------- the block: output o = 64 wave + 16 bk + n16 <-> position l0 + o,
    // its five taps at tile entries o .. o + 4
    {
      const int o0 = 64 * wave + n16;
      const float* xb = tile + kk * E0_PITCH + o0;
      int bo = 4 * kk;
      asm volatile("" : "+v"(bo));                     // (the bias reads stay inside the loop)
      const f32x4 bias5 = ld4(biasS + bo);
      f32x4 acc[4] = {bias5, bias5, bias5, bias5};
#pragma unroll
      for (int s = 0; s < 10; ++s)
#pragma unroll
        for (int bk = 0; bk < 4; ++bk)
          acc[bk] = __builtin_amdgcn_mfma_f32_16x16x4f32(a5[s], xb[4 * (s & 1) * E0_PITCH + 16 * bk + (s >> 1)], acc[bk], 0, 0, 0);
      float h[4][4];
#pragma unroll
      for (int bk = 0; bk < 4; ++bk)
#pragma unroll
        for (int q = 0; q < 4; ++q) h[bk][q] = silu0(acc[bk][q]);
      E0_STAMP(3);
      const f32x4 bias1 = ld4(biasS + 16 + (bo & 4));
      f32x4 o[2] = {bias1, bias1};
      uint32_t lowm = n16 < 8 ? 0xffffffffu : 0u;
      asm volatile("" : "+v"(lowm));                   // (not hoisted into eight more live registers)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float wa = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, a1w[q]) & lowm);
#pragma unroll
        for (int p = 0; p < 2; ++p) o[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa, h[p][q], o[p], 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float wb = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, a1w[q]) & ~lowm);
#pragma unroll
        for (int p = 0; p < 2; ++p) o[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb, h[p + 2][q], o[p], 0, 0, 0);
      }
      // lane (n16, kk) holds channels 4 (kk % 2) + q of blocks p + 2 (kk / 2), p = 0, 1: + block input, out
      const int cb = 4 * (kk & 1);
      const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)b * E0_C * a.L, 0, (int)((uint32_t)E0_C * (uint32_t)a.L * 4u), 0x00020000);
      float v[2][4];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int ob = o0 + 16 * (p + 2 * (kk >> 1));
        const int l = l0 + XO + 2 + ob;
        const bool live = ob >= OLO && ob < OLO + OUTW && l < a.L;
        uint32_t off = ((uint32_t)cb * (uint32_t)a.L + (uint32_t)l) * 4u;
        off = live ? off : 0x80000000u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          v[p][q] = o[p][q] + tile[(cb + q) * E0_PITCH + ob + 2];
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v[p][q]), ro, off, (uint32_t)q * (uint32_t)a.L * 4u, 0);
        }
      }
      if constexpr (DOWN) {
        // ------------------------------------------------------------ the next level's strided conv of this tile's outputs: the block
        // outputs go back into the tile (entry = block output index; zero outside the row: the conv pads ITS input), then column
        // c = 16 wave + n16 of the tile's 62 (row column l0 / 4 + c) is D[16 channels] = W[16][(tap, ci)] out[ci][4 c + 1 + tap]
        __syncthreads();                   // every wave has read its block input
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const int ob = o0 + 16 * (p + 2 * (kk >> 1));
          const int l = l0 + XO + 2 + ob;
          const bool in = l >= 0 && l < a.L;
#pragma unroll
          for (int q = 0; q < 4; ++q) tile[(cb + q) * E0_PITCH + ob] = in ? v[p][q] : 0.f;
        }
        __syncthreads();
        const int c = 16 * wave + n16;
        const float* yb = tile + kk * E0_PITCH + 4 * c + 1;
        f32x4 dacc = ld4(biasS + 16 + E0_C + bo);
#pragma unroll
        for (int s = 0; s < 14; ++s) dacc = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[s], yb[4 * (s & 1) * E0_PITCH + (s >> 1)], dacc, 0, 0, 0);
        const int col = l0 / 4 + c;
        const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(a.d_out + (size_t)b * 16 * a.d_L, 0, (int)(16u * (uint32_t)a.d_L * 4u), 0x00020000);
        uint32_t doff = ((uint32_t)(4 * kk) * (uint32_t)a.d_L + (uint32_t)col) * 4u;
        doff = (c < OUTW / 4 && col < a.d_L) ? doff : 0x80000000u;
        // (the four rows as named scalars pinned behind the MFMA chain: without the pin the four stores below came out as four
        // stores of row 0's register, the other three overwritten by the address arithmetic -- caught by the packed-entry tests)
        float d0 = dacc.x, d1 = dacc.y, d2 = dacc.z, d3 = dacc.w;
        asm volatile("" : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3));
        const uint32_t rowb = (uint32_t)a.d_L * 4u;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, d0), rd, doff, 0u, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, d1), rd, doff, rowb, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, d2), rd, doff, 2u * rowb, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, d3), rd, doff, 3u * rowb, 0);
      }
    }
    E0_STAMP(4);
    if (STAMPS && threadIdx.x == 0) stamps[8 * blockIdx.x + 7] += 1;
    cur = nxt;
    ws = nws;
    neg = nneg;
    b = nb;
    tile_no = ntile;
  }
#undef E0_STAMP
}

}  // namespace
}  // namespace mural
