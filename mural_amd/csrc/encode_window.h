// One column of a site's strand-oriented window, as the window encoders read it (reference: MuRaL/data/preprocessing.py:636-723 k-mer,
// :756-816 one-hot, :559-567 windows).  encode.hip's kernels and the substitution encoder of mutagenesis.hip both go through these, so
// "the window as if one base were different" cannot drift from the window itself: the only difference is the base reader.
#pragma once
#include "common.h"

namespace mural {

// the genome as it is
struct NoSubst {
  __device__ __forceinline__ bool hit(int64_t) const { return false; }
  __device__ __forceinline__ uint32_t base() const { return 0u; }
};

// the genome with the base at '+'-strand position `pos` replaced by the plain base `b` (0..3): an N or IUPAC position becomes that base
// for this reader only (nmask and the amb_pos side table are not consulted there); `live` false reads the genome as it is
struct OneSubst {
  int64_t pos;
  uint32_t b;
  bool live;
  __device__ __forceinline__ bool hit(int64_t g) const { return live && g == pos; }
  __device__ __forceinline__ uint32_t base() const { return b; }
};

// genome position of column j of the strand-oriented window that starts at ws on the '+' strand
__device__ __forceinline__ int64_t window_genome_pos(int64_t ws, int width, bool neg, int j) {
  return neg ? ws + (width - 1 - j) : ws + j;
}

// column j as a MURAL_SYM_* symbol (IUPAC codes resolved, complemented on '-'; outside the record: N)
template <class Sub>
__device__ __forceinline__ uint32_t window_symbol(const MuralGenome& g, int64_t ws, int width, bool neg, int j, const Sub& sub) {
  const int64_t gp = window_genome_pos(ws, width, neg, j);
  uint32_t s = sub.hit(gp) ? sub.base() : genome_sym_iupac(g, gp);
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
    uint32_t s = sub.hit(gp) ? sub.base() : genome_sym(g.packed2, g.nmask, g.length, gp);
    if (s > 3u) bad = true;
    if (neg) s = 3u - (s & 3u);
    val = val * 4 + (int64_t)(s & 3u);
  }
  int64_t sentinel = 1;
  for (int d = 0; d < order; ++d) sentinel *= 4;
  return bad ? sentinel : val;
}

}  // namespace mural
