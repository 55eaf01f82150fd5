// The bin rule of the INDEL structure tables on the device, shared by csrc/summary_txindel.hip (expected and observed events per transcript)
// and csrc/simulate_txindel.hip (their simulated null) so that the two cannot drift: an item as a transcript sees it, the frame bin, the
// CDS rule, what a deletion meets in an item, an insertion's site and the bin of one class of one row, the deletion's walk included.  It
// stands to these files as conseq_bins.h stands to the codon rule.  summaries.summary_txindel_host (through _txindel_pairs) is the
// specification; DESIGN.md section 3.25.
//
// Every function that reads the structure is a template over the kernel's argument block A, which holds, under these names: feat_b0,
// feat_b1, feat_tx, feat_kind, feat_seg, feat_prev, feat_next, n_feat, seg_b0, seg_b1, seg_cds0, seg_tx, n_seg, kind, chrom_len.
#pragma once
#include "common.h"

namespace mural {

constexpr int TI_MAX_LEN = 64;
constexpr int TI_BINS = 10;      // utr5, utr3, noncoding_exon, splice, splice_utr, intron, start_lost, frameshift, inframe, cds_mixed
constexpr int TI_KIND_CODING_INTRON = 3, TI_KIND_INTRON = 4, TI_KIND_CDS = 5;
constexpr int TI_INSERTION = 0, TI_DELETION_START = 1;      // (2: deletion end)
constexpr int TI_FRAMED = 0, TI_MIXED = 1;                  // (2: a range without a multiple of 3 -- frameshift)
constexpr int TI_FRAME = -1;                                // an insertion whose bin is its class's frame bin
enum : uint32_t { TI_T_START = 1, TI_T_SPLICE = 2, TI_T_SPLICE_UTR = 4, TI_T_NONCODING = 8, TI_T_UTR5 = 16, TI_T_UTR3 = 32 };

// The class word of the lengths lo .. hi: lo | frame mode << 8.  Framed: one length; mixed: the range holds a multiple of 3 and another
// length; otherwise every length shifts the frame.
inline uint32_t txindel_class_word(int lo, int hi) {
  const int mode = lo == hi ? TI_FRAMED : (hi / 3 > (lo - 1) / 3) ? TI_MIXED : 2;
  return (uint32_t)lo | (uint32_t)mode << 8;
}

struct TiItem {
  int64_t b0, b1, cds0;
  int kind;
  bool ok;
};

// Item f as transcript tx sees it; !ok: f is out of range, names another transcript, is empty, has an unknown kind or is a CDS part
// without its segment.  Nothing is read before its index is checked.
template <typename Args>
__device__ __forceinline__ TiItem txindel_item(const Args& A, int64_t f, int32_t tx) {
  TiItem it{0, 0, 0, 0, false};
  if (f < 0 || f >= A.n_feat) return it;
  if (A.feat_tx[f] != tx) return it;
  it.b0 = A.feat_b0[f], it.b1 = A.feat_b1[f], it.kind = A.feat_kind[f];
  if (it.b1 <= it.b0 || it.kind > TI_KIND_CDS) return it;
  if (it.kind == TI_KIND_CDS) {
    const int64_t seg = A.feat_seg[f];
    if (seg < 0 || seg >= A.n_seg) return it;
    if (A.seg_b0[seg] != it.b0 || A.seg_b1[seg] != it.b1 || A.seg_tx[seg] != tx) return it;
    it.cds0 = A.seg_cds0[seg];
  }
  it.ok = true;
  return it;
}

// the frame bin of a class of frame mode `mode`, n CDS bases affected
__device__ __forceinline__ int txindel_frame_bin(int mode, int64_t n) {
  return mode == TI_MIXED ? 9 : (mode != TI_FRAMED || n % 3 != 0) ? 7 : 8;
}

// the CDS rule at a boundary with x CDS bases 5' of it
__device__ __forceinline__ int txindel_cds_rule(int64_t x, int64_t cds_len) {
  return x == 0 ? 0 : x == cds_len ? 1 : x <= 2 ? 6 : TI_FRAME;
}

// what the deleted bases [d0, d1) meet in item `it`: the CDS bases, and the touch flags
__device__ __forceinline__ void txindel_meet(const TiItem& it, bool minus, int64_t d0, int64_t d1, int64_t& n_cds, uint32_t& touch) {
  const int64_t u = max(it.b0, d0), v = min(it.b1, d1);
  if (u >= v) return;
  if (it.kind == TI_KIND_CDS) {
    n_cds += v - u;
    if (it.cds0 < 3) {      // the item holds CDS offsets cds0 .. 2: its 5'-most 3 - cds0 bases
      const bool hit = minus ? v > max(it.b0, it.b1 - (3 - it.cds0)) : u < min(it.b1, it.b0 + (3 - it.cds0));
      if (hit) touch |= TI_T_START;
    }
  } else if (it.kind >= TI_KIND_CODING_INTRON) {
    if (it.b1 - it.b0 >= 4 && (u < it.b0 + 2 || v > it.b1 - 2)) touch |= it.kind == TI_KIND_CODING_INTRON ? TI_T_SPLICE : TI_T_SPLICE_UTR;
  } else {
    touch |= it.kind == 2 ? TI_T_NONCODING : it.kind == 0 ? TI_T_UTR5 : TI_T_UTR3;
  }
}

// The site of an insertion at boundary j whose base j - 1 lies in `home`: its bin, or TI_FRAME where its class's frame bin decides.
// `behind` is the item of base j where j is home's last boundary (ok only where it abuts); `live` is cleared where base j lies in no
// usable item.
__device__ __forceinline__ int txindel_insertion_site(const TiItem& home, const TiItem& behind, bool minus, int64_t cds_len, int64_t j,
                                                      bool& live) {
  const bool gap_a = home.kind == TI_KIND_CODING_INTRON || home.kind == TI_KIND_INTRON;
  if (j < home.b1) {      // bases j - 1 and j in one item
    if (home.kind < TI_KIND_CODING_INTRON) return home.kind;
    if (gap_a) return (home.b1 - home.b0 >= 4 && (j == home.b0 + 1 || j == home.b1 - 1)) ? (home.kind == TI_KIND_CODING_INTRON ? 3 : 4) : 5;
    return txindel_cds_rule(home.cds0 + (minus ? home.b1 - j : j - home.b0), cds_len);
  }
  // on the boundary of two items: base j must lie in the span as well
  live = live && behind.ok;
  const bool gap_b = behind.kind == TI_KIND_CODING_INTRON || behind.kind == TI_KIND_INTRON;
  if (home.kind == TI_KIND_CDS) return txindel_cds_rule(home.cds0 + (minus ? 0 : home.b1 - home.b0), cds_len);
  if (behind.kind == TI_KIND_CDS) return txindel_cds_rule(behind.cds0 + (minus ? behind.b1 - behind.b0 : 0), cds_len);
  if (gap_a && gap_b) return 5;
  return gap_a ? behind.kind : home.kind;      // a gap yields to an exon part
}

// The bin of the class with word w (txindel_class_word) of a counted row at boundary j whose home item is f = `home` of transcript tx.
// An insertion: its site or the class's frame bin.  A deletion removes L = lo bases: the walk goes from the home item over feat_next
// (deletion start) or feat_prev (deletion end) while the items meet the deleted bases, one O(1) overlap per item; a link that is out of
// range, names another transcript or does not abut ends it, so every step moves on by a base or more: at most TI_MAX_LEN steps.
template <typename Args>
__device__ __forceinline__ int txindel_class_bin(const Args& A, int64_t f, int32_t tx, const TiItem& home, bool minus, int site, int64_t j,
                                                 uint32_t w) {
  const int64_t len = w & 0xFF;
  const int mode = (int)(w >> 8);
  if (A.kind == TI_INSERTION) return site == TI_FRAME ? txindel_frame_bin(mode, len) : site;
  const bool fwd = A.kind == TI_DELETION_START;
  int64_t d0 = fwd ? j : max(j - len, (int64_t)0), d1 = fwd ? j + len : j;
  if (fwd && A.chrom_len >= 0) d1 = max(min(d1, A.chrom_len), j + 1);      // (the home base stays)
  int64_t n_cds = 0;
  uint32_t touch = 0;
  txindel_meet(home, minus, d0, d1, n_cds, touch);
  TiItem cur = home;
  int64_t at = f;
  while (fwd ? cur.b1 < d1 : cur.b0 > d0) {      // at most 64 steps: every step moves on by a base or more
    at = fwd ? A.feat_next[at] : A.feat_prev[at];
    const TiItem it = txindel_item(A, at, tx);
    if (!it.ok || (fwd ? it.b0 != cur.b1 : it.b1 != cur.b0)) break;
    txindel_meet(it, minus, d0, d1, n_cds, touch);
    cur = it;
  }
  return (touch & TI_T_START) ? 6 : (touch & TI_T_SPLICE) ? 3 : n_cds > 0 ? txindel_frame_bin(mode, n_cds) : (touch & TI_T_SPLICE_UTR) ? 4
       : (touch & TI_T_NONCODING) ? 2 : (touch & TI_T_UTR5) ? 0 : (touch & TI_T_UTR3) ? 1 : 5;
}

}  // namespace mural
