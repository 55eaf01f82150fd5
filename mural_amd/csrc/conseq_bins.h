// The consequence bin of a row's three substitutions inside a CDS segment, shared by csrc/summary_conseq.hip and
// csrc/summary_txstruct.hip (expected and observed mutations per transcript) and csrc/simulate_conseq.hip and csrc/simulate_txstruct.hip
// (their simulated nulls) so that the four cannot drift: the transcripts' block of their argument structs (TxSegments, filled and
// checked by fill_tx_segments, its amino-acid table staged into LDS by stage_aa), the codon over seg_prev / seg_next and the
// class-to-bin rule.  summaries.summary_conseq_host is the specification; DESIGN.md section 3.21.
#pragma once
#include "common.h"
#include "kmer_key.h"

namespace mural {

constexpr int SC_BINS = 5;                        // synonymous, missense, stop gained, stop lost, unresolved
constexpr int SC_NOWHERE = SC_BINS;               // the bin of a class that is not counted

// The genome, the CDS segments of a chromosome and the transcripts they belong to, as the kernels read them.
struct TxSegments {
  MuralGenome g;
  const int64_t* seg_b0;
  const int64_t* seg_b1;
  const int64_t* seg_cds0;
  const int32_t* seg_tx;
  const int32_t* seg_prev;
  const int32_t* seg_next;
  int64_t n_seg;
  const uint8_t* tx_strand;
  const int64_t* tx_cds_len;
  uint32_t aa_w[16];          // the 64 amino-acid bytes, four to a word
  uint32_t alt_packed;        // alt_order[r][j] in bits [2 (3 r + j), +2)
};

// The amino-acid table in LDS, for every thread of the workgroup (a barrier); to be read as 64 bytes.
__device__ __forceinline__ const uint8_t* stage_aa(const TxSegments& X, uint32_t (&aa_words)[16]) {
#pragma unroll
  for (int j = 0; j < 16; ++j)      // (constant indices: the words stay scalar arguments)
    if (threadIdx.x == j) aa_words[j] = X.aa_w[j];
  __syncthreads();
  return reinterpret_cast<const uint8_t*>(aa_words);
}

// The codon (16 b0 + 4 b1 + b2, read 5' -> 3' on the transcript's strand) that holds CDS offsets cs .. cs + 2 of the transcript of
// segment s, or -1 where a position is not found within two hops, lies outside the record or is masked.  Every index is checked
// before it is used.
__device__ __forceinline__ int conseq_codon(const TxSegments& A, int64_t s, int32_t tx, bool minus, int64_t cs) {
  int codon = 0;
  bool found = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int64_t o = cs + j;
    int64_t cur = s;
#pragma unroll
    for (int hop = 0; hop < 2; ++hop) {
      const int64_t c0 = A.seg_cds0[cur], len = A.seg_b1[cur] - A.seg_b0[cur];
      int64_t nx = cur;
      if (o < c0) nx = A.seg_prev[cur];
      else if (o >= c0 + len) nx = A.seg_next[cur];
      if (nx < 0 || nx >= A.n_seg) {
        found = false;
        nx = cur;
      }
      cur = nx;
    }
    const int64_t c0 = A.seg_cds0[cur], sb0 = A.seg_b0[cur], sb1 = A.seg_b1[cur];
    found = found && o >= c0 && o < c0 + (sb1 - sb0) && A.seg_tx[cur] == tx;
    const int64_t pos = minus ? sb1 - 1 - (o - c0) : sb0 + (o - c0);
    int32_t code = 0;
    if (found && pos >= 0 && pos < A.g.length) {
      bool masked = false;
      code = kmer_base(A.g, pos, masked);
      found = !masked;
    } else {
      found = false;
    }
    codon = codon * 4 + (minus ? 3 - code : code);
  }
  return found ? codon : -1;
}

// bins[c - 1] of the classes c = 1 .. 3 of row i at q in [b0, b1) of segment s = [b0, b1) (CDS offset cds0, transcript tx on strand
// `minus` with cds_len coding bases); strand: the rows', or nullptr; aa: the 64 amino-acid bytes
__device__ __forceinline__ void conseq_row_bins(const TxSegments& A, const uint8_t* strand, const uint8_t* aa, int64_t s, int32_t tx, bool minus, int64_t cds_len,
                                                int64_t b0, int64_t b1, int64_t cds0, int64_t i, int64_t q, int (&bins)[3]) {
  const int64_t x = cds0 + (minus ? b1 - 1 - q : q - b0);
  const int64_t cs = x - x % 3;
  const int codon = (x >= 0 && cs + 2 < cds_len) ? conseq_codon(A, s, tx, minus, cs) : -1;
  if (codon < 0) {
    bins[0] = bins[1] = bins[2] = SC_BINS - 1;
  } else {
    const int sh = 2 * (2 - (int)(x - cs));
    const int own_tx = (codon >> sh) & 3;                       // the base at q, on the transcript's strand
    const bool row_minus = strand != nullptr && strand[i] != 0;
    const int r = (minus != row_minus) ? 3 - own_tx : own_tx;   // the row's own base
    const uint8_t aa_ref = aa[codon];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int alt = (int)(A.alt_packed >> (2 * (3 * r + c))) & 3;      // on the row's strand
      const int alt_tx = (minus != row_minus) ? 3 - alt : alt;
      const uint8_t aa_alt = aa[(codon & ~(3 << sh)) | (alt_tx << sh)];
      bins[c] = aa_ref == aa_alt ? 0 : aa_alt == '*' ? 2 : aa_ref == '*' ? 3 : 1;
    }
  }
}

// alt_order [4][3] packed for conseq_row_bins; false where a row does not name the three other bases once each (*bad_row: which)
inline bool conseq_pack_alt_order(const uint8_t (&alt_order)[4][3], uint32_t& packed, int& bad_row) {
  packed = 0;
  for (int r = 0; r < 4; ++r) {
    unsigned seen = 1u << r;
    for (int j = 0; j < 3; ++j) {
      const unsigned a = alt_order[r][j];
      if (a >= 4 || (seen & (1u << a))) {
        bad_row = r;
        return false;
      }
      seen |= 1u << a;
      packed |= a << (2 * (3 * r + j));
    }
  }
  return true;
}

// X from the fields of the public argument struct *s of entry `entry`: alt_order is checked always, the genome only where there is
// work (`live`: rows and items); the segment and transcript pointers are the entry's to check.  MURAL_OK or the refusal.
template <typename Pub>
inline int fill_tx_segments(const char* entry, const Pub* s, bool live, TxSegments& X) {
  int bad_alt = 0;
  MURAL_REQUIRE(conseq_pack_alt_order(s->alt_order, X.alt_packed, bad_alt), "%s: alt_order[%d] must name the three other bases once each",
                entry, bad_alt);
  if (!live) return MURAL_OK;
  MURAL_REQUIRE(s->genome && s->genome->packed2 && s->genome->nmask && s->genome->length >= 0, "%s: empty genome", entry);
  X.g = *s->genome;
  X.seg_b0 = s->seg_b0, X.seg_b1 = s->seg_b1, X.seg_cds0 = s->seg_cds0, X.seg_tx = s->seg_tx, X.seg_prev = s->seg_prev, X.seg_next = s->seg_next;
  X.n_seg = s->n_segments, X.tx_strand = s->tx_strand, X.tx_cds_len = s->tx_cds_len;
  for (int j = 0; j < 64; ++j) X.aa_w[j >> 2] |= (uint32_t)s->aa[j] << (8 * (j & 3));
  return MURAL_OK;
}

}  // namespace mural
