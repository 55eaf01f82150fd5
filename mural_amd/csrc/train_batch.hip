// One training batch gathered and encoded on the device from row indices (mural_train_batch_encode): for batch row b the site
// r = order[first + b] of a row table that spans several chromosomes becomes its k-mer ids, its symbol window and its label in one
// launch -- the values of mural_encode_kmer / mural_encode_symbols / mural_encode_onehot for the same site, bit for bit (the window
// formulas are theirs, the decode helpers are common.h's and dense_symbol.h's).
//
// One workgroup per row.  The packed2 / nmask words under the union of the local and the distal window are read once into LDS, decoded
// once into forward symbols (one byte per genome position, LDS), and both outputs are cut from those bytes.  The kernel is store-bound:
// per row it writes W symbol bytes (+ 8 bytes per k-mer column) against (span / 4 + span / 8) bytes read.  A row of the symbol tensor
// starts at any byte (W is odd for SNV windows), so the stores go by the 4-byte slots of the whole tensor: full slots as one dword, the
// at most two slots shared with the neighbouring rows byte by byte.
#include "common.h"
#include "dense_symbol.h"

namespace mural {

constexpr int TB_THREADS = 256;

struct TrainBatchGeom {
  int off_l, width_l, ncol, order;      // local (k-mer) window
  int off_d, width_d;                   // distal (symbol) window
  int lo, span;                         // union of the two, relative to the site: positions pos + lo .. pos + lo + span - 1
  int n_pw, n_mw;                       // LDS words reserved for packed2 / nmask
};

__global__ __launch_bounds__(TB_THREADS) void train_batch_encode_kernel(
    const MuralGenome* __restrict__ genomes, int n_genomes, const int32_t* __restrict__ row_chrom, const int64_t* __restrict__ row_pos,
    const uint8_t* __restrict__ row_strand, const uint8_t* __restrict__ row_label, int64_t n_rows, const int64_t* __restrict__ order,
    int64_t first, TrainBatchGeom gm, int64_t* __restrict__ cat_out, uint8_t* __restrict__ sym_out, float* __restrict__ onehot_out,
    float* __restrict__ y_out, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) uint32_t tb_lds[];
  uint32_t* s_packed = tb_lds;
  uint32_t* s_mask = tb_lds + gm.n_pw;
  uint8_t* s_fwd = reinterpret_cast<uint8_t*>(tb_lds + gm.n_pw + gm.n_mw);      // forward symbol of genome position g_lo + k

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t r = order[first + b];
  // a row outside the table, or one that names no genome, is an empty record: every position reads as N, the label is 0
  MuralGenome gn{nullptr, nullptr, 0, nullptr, nullptr, 0};
  int64_t pos = 0;
  bool neg = false;
  float label = 0.f;
  bool valid = r >= 0 && r < n_rows;
  if (valid) {
    const int32_t c = row_chrom[r];
    valid = c >= 0 && c < n_genomes;
    if (valid) {
      gn = genomes[c];
      pos = row_pos[r];
      neg = row_strand[r] != 0;
      label = (float)row_label[r];
    }
  }
  if (tid == 0) {
    if (!valid) atomicOr(status, (int)MURAL_E_INVALID);
    y_out[b] = label;
  }

  // ---- the words under the window, once
  const int64_t g_lo = pos + gm.lo;
  const int64_t pw0 = g_lo >> 4, mw0 = g_lo >> 5;                      // (arithmetic shifts: floor for negative positions)
  const int64_t pw_end = (gn.length + 15) >> 4, mw_end = (gn.length + 31) >> 5;
  for (int t = tid; t < gm.n_pw; t += TB_THREADS) {
    const int64_t w = pw0 + t;
    s_packed[t] = (w >= 0 && w < pw_end) ? gn.packed2[w] : 0u;
  }
  for (int t = tid; t < gm.n_mw; t += TB_THREADS) {
    const int64_t w = mw0 + t;
    s_mask[t] = (w >= 0 && w < mw_end) ? gn.nmask[w] : 0u;
  }
  __syncthreads();
  for (int k = tid; k < gm.span; k += TB_THREADS) {
    const int64_t g = g_lo + k;
    uint32_t s = SYM_N;
    if (g >= 0 && g < gn.length) s = sym_from_words(gn, g, s_packed[(int)((g >> 4) - pw0)], s_mask[(int)((g >> 5) - mw0)]);
    s_fwd[k] = (uint8_t)s;
  }
  __syncthreads();

  // ---- k-mer ids (encode_kmer_kernel's loop over the staged symbols: any symbol above T -- N or an IUPAC code -- spoils the k-mer)
  int64_t sentinel = 1;
  for (int d = 0; d < gm.order; ++d) sentinel *= 4;
  for (int col = tid; col < gm.ncol; col += TB_THREADS) {
    int64_t val = 0;
    bool bad = false;
    for (int d = 0; d < gm.order; ++d) {
      const int j = col + d;
      uint32_t s = s_fwd[gm.off_l - gm.lo + (neg ? gm.width_l - 1 - j : j)];
      if (s > 3u) bad = true;
      if (neg) s = 3u - (s & 3u);
      val = val * 4 + (int64_t)(s & 3u);
    }
    cat_out[(int64_t)b * gm.ncol + col] = bad ? sentinel : val;
  }

  // ---- the symbol row, strand-oriented and complemented like encode_symbols_kernel's
  const int W = gm.width_d;
  const int base_d = gm.off_d - gm.lo;
  if (sym_out) {
    const int64_t row0 = (int64_t)b * W;                               // first byte of the row in the tensor
    const int64_t slot_lo = row0 >> 2, slot_hi = (row0 + W - 1) >> 2;
    for (int64_t slot = slot_lo + tid; slot <= slot_hi; slot += TB_THREADS) {
      const int j0 = (int)((slot << 2) - row0);                        // column of the slot's first byte (-3 .. W - 1)
      uint32_t bytes[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + e;
        uint32_t s = 0;
        if (j >= 0 && j < W) {
          s = s_fwd[base_d + (neg ? W - 1 - j : j)];
          if (neg) s = sym_complement(s);
        }
        bytes[e] = s;
      }
      if (j0 >= 0 && j0 + 3 < W) {
        *reinterpret_cast<uint32_t*>(sym_out + (slot << 2)) = bytes[0] | (bytes[1] << 8) | (bytes[2] << 16) | (bytes[3] << 24);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (j0 + e >= 0 && j0 + e < W) sym_out[(slot << 2) + e] = (uint8_t)bytes[e];
      }
    }
  }
  // ---- the same row as dense columns (models whose training path takes the (B, 4, W) tensor)
  if (onehot_out) {
    float* o = onehot_out + (int64_t)b * 4 * W;
    for (int j = tid; j < W; j += TB_THREADS) {
      uint32_t s = s_fwd[base_d + (neg ? W - 1 - j : j)];
      if (neg) s = sym_complement(s);
      symbol_to_dense(s, o + j, W);
    }
  }
}

}  // namespace mural

using namespace mural;

extern "C" int mural_train_batch_encode(const MuralGenome* genomes, int32_t n_genomes, const int32_t* row_chrom, const int64_t* row_pos,
                                        const uint8_t* row_strand, const uint8_t* row_label, int64_t n_rows, const int64_t* order,
                                        int64_t n_order, int64_t first, int32_t B, int32_t local_radius, int32_t local_order,
                                        int32_t distal_radius, int32_t indel, int64_t* cat_out, uint8_t* sym_out, float* onehot_out,
                                        float* y_out, int32_t* status, void* stream) {
  MURAL_REQUIRE(n_genomes >= 0 && n_rows >= 0 && n_order >= 0 && B >= 0, "train_batch_encode: negative count");
  MURAL_REQUIRE(first >= 0 && first <= n_order && (int64_t)B <= n_order - first,
                "train_batch_encode: rows %lld .. %lld of the order lie outside its %lld entries", (long long)first,
                (long long)first + B, (long long)n_order);
  MURAL_REQUIRE(local_order >= 1 && local_order <= 12, "local_order must be in [1,12], got %d", local_order);
  TrainBatchGeom gm;
  if (int rc = window_geometry(local_radius, indel, &gm.off_l, &gm.width_l)) return rc;
  if (int rc = window_geometry(distal_radius, indel, &gm.off_d, &gm.width_d)) return rc;
  gm.order = local_order;
  gm.ncol = gm.width_l - (local_order - 1);
  MURAL_REQUIRE(gm.ncol >= 1, "window too short for order %d", local_order);
  gm.lo = gm.off_l < gm.off_d ? gm.off_l : gm.off_d;
  const int hi_l = gm.off_l + gm.width_l, hi_d = gm.off_d + gm.width_d;
  gm.span = (hi_l > hi_d ? hi_l : hi_d) - gm.lo;
  gm.n_pw = gm.span / 16 + 2;      // span positions starting anywhere in a word touch at most span / 16 + 2 words
  gm.n_mw = gm.span / 32 + 2;
  const size_t lds = (size_t)(gm.n_pw + gm.n_mw) * 4 + (size_t)gm.span;
  MURAL_REQUIRE(lds <= 48 * 1024, "train_batch_encode: a window of %d positions does not fit the kernel's staging buffer", gm.span);
  if (B == 0) return MURAL_OK;
  MURAL_REQUIRE(genomes && row_chrom && row_pos && row_strand && row_label && order, "train_batch_encode: the row table and the order must not be NULL");
  MURAL_REQUIRE(cat_out && y_out && status && (sym_out || onehot_out), "train_batch_encode: cat_out / y_out / status and one of sym_out / onehot_out must not be NULL");
  MURAL_REQUIRE((reinterpret_cast<uintptr_t>(sym_out) & 3u) == 0, "train_batch_encode: the symbol buffer must be 4-byte aligned");
  hipLaunchKernelGGL(train_batch_encode_kernel, dim3(B), dim3(TB_THREADS), lds, (hipStream_t)stream, genomes, n_genomes, row_chrom,
                     row_pos, row_strand, row_label, n_rows, order, first, gm, cat_out, sym_out, onehot_out, y_out, status);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}
