// One column of a site's strand-oriented window, as the window encoders read it (reference: MuRaL/data/preprocessing.py:636-723 k-mer,
// :756-816 one-hot, :559-567 windows).  encode.hip's kernels and the substitution encoder of mutagenesis.hip both go through these, so
// "the window as if one base were different" cannot drift from the window itself: the only difference is the base reader.  The allele
// encoder of mutagenesis.hip (insertions, deletions, multi-base alleles) is the third reader.
#pragma once
#include "common.h"

namespace mural {

// A base reader answers three questions about position q of the sequence the window is cut from: hit(q), "is q one of my own bases";
// base(q), that base (asked only after a hit); ref_pos(q), the genome position q stands for otherwise (the identity unless the reader
// changes the sequence's length).

// the genome as it is
struct NoSubst {
  __device__ __forceinline__ bool hit(int64_t) const { return false; }
  __device__ __forceinline__ uint32_t base(int64_t) const { return 0u; }
  __device__ __forceinline__ int64_t ref_pos(int64_t q) const { return q; }
};

// the genome with the base at '+'-strand position `pos` replaced by the plain base `b` (0..3): an N or IUPAC position becomes that base
// for this reader only (nmask and the amb_pos side table are not consulted there); `live` false reads the genome as it is
struct OneSubst {
  int64_t pos;
  uint32_t b;
  bool live;
  __device__ __forceinline__ bool hit(int64_t g) const { return live && g == pos; }
  __device__ __forceinline__ uint32_t base(int64_t) const { return b; }
  __device__ __forceinline__ int64_t ref_pos(int64_t q) const { return q; }
};

// the alternate haplotype of one allele: the genome with the '+'-strand bases [p, p + d) replaced by the k plain bases of `alt` (base i
// in bits 2i, 2i+1; k <= 32), read in ITS OWN coordinates: q < p is genome[q], p <= q < p + k is alt[q - p], from p + k on genome[q -
// shift] with shift = k - d.  Beyond either end the genome reader answers N, so the end-of-record padding moves by k - d with no rule of
// its own.  The inserted bases are plain bases, as OneSubst's is.  An allele that is not live is built as p = k = shift = 0, live false:
// the genome as it is.
struct AlleleEdit {
  int64_t p;
  int64_t k;
  int64_t shift;
  uint64_t alt;
  bool live;
  __device__ __forceinline__ bool hit(int64_t q) const { return live && q >= p && q < p + k; }
  // (the bit index is below 64 after a hit, and formed in 64 bits)
  __device__ __forceinline__ uint32_t base(int64_t q) const { return (uint32_t)((alt >> (uint64_t)(2 * (q - p))) & 3ull); }
  __device__ __forceinline__ int64_t ref_pos(int64_t q) const { return live && q >= p + k ? q - shift : q; }
};

// position of column j of the strand-oriented window that starts at ws on the '+' strand, in the coordinates of the sequence the base
// reader stands for (the genome's own for NoSubst / OneSubst)
__device__ __forceinline__ int64_t window_genome_pos(int64_t ws, int width, bool neg, int j) {
  return neg ? ws + (width - 1 - j) : ws + j;
}

// column j as a MURAL_SYM_* symbol (IUPAC codes resolved, complemented on '-'; outside the record: N)
template <class Sub>
__device__ __forceinline__ uint32_t window_symbol(const MuralGenome& g, int64_t ws, int width, bool neg, int j, const Sub& sub) {
  const int64_t gp = window_genome_pos(ws, width, neg, j);
  uint32_t s = sub.hit(gp) ? sub.base(gp) : genome_sym_iupac(g, sub.ref_pos(gp));
  if (neg) s = sym_complement(s);
  return s;
}

// order-k index of the k-mer that starts at column `col`; 4^order when one of its bases is not A/C/G/T (IUPAC codes count as N here)
template <class Sub>
__device__ __forceinline__ int64_t window_kmer_id(const MuralGenome& g, int64_t ws, int width, bool neg, int col, int order, const Sub& sub) {
  int64_t val = 0;
  bool bad = false;
  for (int d = 0; d < order; ++d) {
    const int64_t gp = window_genome_pos(ws, width, neg, col + d);
    uint32_t s = sub.hit(gp) ? sub.base(gp) : genome_sym(g.packed2, g.nmask, g.length, sub.ref_pos(gp));
    if (s > 3u) bad = true;
    if (neg) s = 3u - (s & 3u);
    val = val * 4 + (int64_t)(s & 3u);
  }
  int64_t sentinel = 1;
  for (int d = 0; d < order; ++d) sentinel *= 4;
  return bad ? sentinel : val;
}

}  // namespace mural
