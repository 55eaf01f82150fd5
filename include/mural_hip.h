/*
 * mural_hip.h -- C ABI of libmural_hip.so, the MI355X (gfx950) hot path for MuRaL models.
 *
 * The reference (CaiLiLab/MuRaL) has no FFI layer: its seam is the Python nn.Module protocol of the
 * classes returned by MuRaL/model/nn_utils.py:186 (model_choice).  Each entry point below names the
 * reference interface it replaces (file:line relative to the reference tree).  The binding that a
 * maintainer would add on the reference side is a ctypes stub; see INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; device pointers are raw HIP device addresses the caller owns ("dev"),
 *     host pointers are marked "host".  The library borrows every pointer for the duration of one call.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises.
 *   - return value: 0 = ok, otherwise a MURAL_E_* code; mural_last_error() gives the message of the
 *     last failure on the calling thread.
 *   - fp32 everywhere; integer outputs are bit-exact w.r.t. the reference.
 */
#ifndef MURAL_HIP_H
#define MURAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  MURAL_OK = 0,
  MURAL_E_INVALID = 1,     /* bad argument / unsupported configuration (maps to ValueError)        */
  MURAL_E_RUNTIME = 2,     /* HIP runtime failure (maps to RuntimeError)                            */
  MURAL_E_WORKSPACE = 3,   /* workspace too small                                                   */
  MURAL_E_ENCODING = 4     /* dense distal input holds a column that is not a MuRaL one-hot/IUPAC
                              column (reported asynchronously through the status word, see below)   */
};

const char* mural_last_error(void);
int mural_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Genome in packed form (product input format):
 *   packed2 : 16 bases per uint32, base i in bits [2*(i%16), +2)  (A0 C1 G2 T3; 0 where masked)
 *   nmask   : 32 bases per uint32, bit (i%32) set when the base is not one of ACGT
 * Bases outside [0, length) read as 'N' (the reference imputes chromosome ends with 'N',
 * MuRaL/data/preprocessing.py:682-695, :791-804).
 * IUPAC ambiguity codes other than N (R Y M S W K B D H V; fractional one-hot columns in the reference,
 * preprocessing.py:762-772) are rare and live in a sparse side table: their bit in nmask is set (the k-mer encoder
 * treats them like N, :655-666) and (amb_pos, amb_sym) lists them in ascending position with their symbol
 * MURAL_SYM_R .. MURAL_SYM_V.  The one-hot encoder and the fused forward resolve them through that table.
 * ---------------------------------------------------------------------------------------------- */
enum { MURAL_SYM_A = 0, MURAL_SYM_C, MURAL_SYM_G, MURAL_SYM_T, MURAL_SYM_N, MURAL_SYM_R, MURAL_SYM_Y, MURAL_SYM_M,
       MURAL_SYM_S, MURAL_SYM_W, MURAL_SYM_K, MURAL_SYM_B, MURAL_SYM_D, MURAL_SYM_H, MURAL_SYM_V };
typedef struct {
  const uint32_t* packed2;   /* dev */
  const uint32_t* nmask;     /* dev */
  int64_t length;            /* bases in this chromosome */
  const int64_t* amb_pos;    /* dev, ascending positions of non-N ambiguity codes (NULL when n_amb == 0) */
  const uint8_t* amb_sym;    /* dev, MURAL_SYM_R .. MURAL_SYM_V per entry */
  int64_t n_amb;
} MuralGenome;

/* Replaces seq_digit_encoder (MuRaL/data/preprocessing.py:636-723) for one site per row.
 * out: dev int64 [n][2*radius + (indel?0:1) - (order-1)], values in [0, 4^order].
 * strand: dev uint8 [n], 0 = '+', 1 = '-'.  indel != 0 selects the indel window (:564-566).      */
int mural_encode_kmer(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, int64_t n,
                      int32_t radius, int32_t order, int32_t indel, int64_t* out, void* stream);

/* Replaces seq_ohe_encoder (MuRaL/data/preprocessing.py:756-816): one-hot columns, 0.25 x 4 for N and the
 * fractional columns of the other IUPAC codes (:762-772, complemented on the '-' strand :774-788).
 * out: dev float [n][4][2*radius + (indel?0:1)].                                                   */
int mural_encode_onehot(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, int64_t n,
                        int32_t radius, int32_t indel, float* out, void* stream);

/* The same windows as one SYMBOL per column (MURAL_SYM_*: A C G T N R Y M S W K B D H V = 0..14, strand-oriented and complemented
 * like the one-hot columns; positions outside the record are N): what mural_op_dense_to_symbols recovers from the one-hot tensor,
 * without the detour -- the `symbols` input of mural_snv_train_forward.  out: dev uint8 [n][2*radius + (indel?0:1)].            */
int mural_encode_symbols(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, int64_t n, int32_t radius,
                         int32_t indel, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * In-silico saturation mutagenesis around the SNV forward (csrc/mutagenesis.hip).  The reference has no such
 * tool; the windows are its encoders' (seq_digit_encoder, MuRaL/data/preprocessing.py:636-723; seq_ohe_encoder, :756-816) on a
 * genome with ONE base replaced, and the forward in between is mural_snv_forward_symbols.
 *
 * mural_encode_subst_windows: one row per (site, substitution), SNV windows (indel = 0).
 *   pos / strand         : dev int64 / uint8 [n], the row's site (strand 1 = '-')
 *   sub_pos / sub_base   : dev int64 / uint8 [n], a '+'-strand genomic position and a '+'-strand base 0..3 (A C G T); a sub_base above 3
 *                          (255 by convention) means "no substitution"
 *   symbols              : dev uint8 [n][2*radius+1], 4-byte aligned, or NULL
 *   cat_x                : dev int64 [n][2*local_radius+1-(local_order-1)], or NULL
 * Row i is, bit for bit, mural_encode_symbols(.., radius, indel=0) / mural_encode_kmer(.., local_radius, local_order, indel=0) of
 * (pos[i], strand[i]) on a genome that is g with the base at sub_pos[i] replaced by sub_base[i]: an N or IUPAC position becomes a plain
 * base (nmask and the amb_pos side table are overridden for that row only).  A sub_pos outside [0, g->length), one outside the row's
 * windows, or "no substitution" gives the unchanged encodings.  The genome buffers are only read.  One launch; n == 0 launches nothing.
 *
 * mural_mutagenesis_rows: the enumerator.  With W = 2*radius+1, variant id v = (site*W + j)*3 + a for site < n_sites, window column j
 * (strand-oriented, as the symbols are) and a in {0,1,2}; the call writes ids [first, first+count) to index v - first of
 *   row_pos / row_strand : dev int64 / uint8 [count], the site's pos / strand
 *   sub_pos              : dev int64 [count], the genomic position of column j: pos + (j - radius) on '+', pos - (j - radius) on '-'
 *   sub_base             : dev uint8 [count]: in WINDOW orientation the alternative is the a-th of {A,C,G,T} without the column's
 *                          reference symbol, ascending; sub_base is that alternative on the '+' strand (complemented for '-' rows).  A
 *                          column whose reference symbol is not A/C/G/T (N, IUPAC, outside the record) has none: its ids get 255.
 *
 * mural_mutagenesis_reduce: ids [first, first+count) scattered into the map.
 *   ref_logp             : dev float [n_sites][n_class], the forward of the unchanged windows
 *   var_logp             : dev float [count][n_class], the forward of the ids' rows
 *   ref_symbols          : dev uint8 [n_sites][W], mural_encode_symbols of the sites
 *   delta                : dev float [n_sites][W][4][n_class], indexed by the alternative base in window orientation:
 *                          var_logp - ref_logp (one float32 subtraction); +0.0 at the reference base; NaN (0x7fc00000) in all four
 *                          entries of a column whose reference symbol is not A/C/G/T
 *   logp_map             : the same shape or NULL: var_logp itself, ref_logp at the reference base, NaN where delta is
 * Every element has one writer among the ids of a run and nothing is accumulated: the maps do not depend on how the ids are chunked.
 * ---------------------------------------------------------------------------------------------- */
int mural_encode_subst_windows(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, const int64_t* sub_pos,
                               const uint8_t* sub_base, int64_t n, int32_t radius, int32_t local_radius, int32_t local_order,
                               uint8_t* symbols, int64_t* cat_x, void* stream);
int mural_mutagenesis_rows(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, int64_t n_sites, int32_t radius,
                           int64_t first, int64_t count, int64_t* row_pos, uint8_t* row_strand, int64_t* sub_pos, uint8_t* sub_base,
                           void* stream);
int mural_mutagenesis_reduce(const float* ref_logp, const float* var_logp, const uint8_t* ref_symbols, int64_t n_sites, int32_t radius,
                             int32_t n_class, int64_t first, int64_t count, float* delta, float* logp_map, void* stream);
/* The same three for either window (the three above are these with indel = 0; same kernels, same bits):
 *   indel = 0: [pos - R, pos + R], W = 2*radius + 1;   indel = 1: [pos - R + 1, pos + R], W = 2*radius (the INDEL model's window).
 * mural_encode_subst_symbols: row i is, bit for bit, mural_encode_symbols(.., radius, indel) on the genome with the base at sub_pos[i]
 *   replaced; symbols dev uint8 [n][W], 4-byte aligned.
 * mural_mutagenesis_rows_window: ids v = (site*W + j)*3 + a with that W; sub_pos is the genomic position of column j of that window
 *   (indel = 1: pos - R + 1 + j on '+', pos + R - j on '-').
 * mural_mutagenesis_reduce_window: takes W itself (any W >= 1; ref_symbols [n_sites][W], maps [n_sites][W][4][n_class]).
 * mural_scores_log_softmax: out[i][c] = s[c] - (max_c s + log sum_c exp(s[c] - max_c s)), float32, one thread per row, classes in
 *   ascending order: a row's bits do not depend on n or on the other rows.  Turns the INDEL forward's Softplus scores into the
 *   log-probabilities of softmax(scores) (what predict writes).  scores / out: dev float [n][n_class], two buffers. */
int mural_encode_subst_symbols(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, const int64_t* sub_pos,
                               const uint8_t* sub_base, int64_t n, int32_t radius, int32_t indel, uint8_t* symbols, void* stream);
int mural_mutagenesis_rows_window(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, int64_t n_sites, int32_t radius,
                                  int32_t indel, int64_t first, int64_t count, int64_t* row_pos, uint8_t* row_strand, int64_t* sub_pos,
                                  uint8_t* sub_base, void* stream);
int mural_mutagenesis_reduce_window(const float* ref_logp, const float* var_logp, const uint8_t* ref_symbols, int64_t n_sites, int32_t W,
                                    int32_t n_class, int64_t first, int64_t count, float* delta, float* logp_map, void* stream);
int mural_scores_log_softmax(const float* scores, int64_t n, int32_t n_class, float* out, void* stream);
/* Mutagenesis profiles: the map reduced over sites in flight instead of written.
 * mural_mutagenesis_profile_window: takes the place of mural_mutagenesis_reduce_window in a chunk; same ids, v = (site*W + j)*3 + a.
 *   ref_logp / var_logp / ref_symbols : as mural_mutagenesis_reduce_window ([n_sites][n_class], [count][n_class], [n_sites][W])
 *   group                : dev int32 [n_sites], or NULL: every site in group 0
 *   table                : dev uint64 [n_groups][W][4][3][n_class][5], cell [group][column j][reference symbol 0..3][a][class]; words
 *                          n (terms added), sum (sum of q, two's complement), abs (sum of |q|), sq_lo (sum of q*q mod 2^40),
 *                          sq_hi (sum of q*q >> 40).  ACCUMULATED into: the caller zeroes it once.
 *   status               : dev uint64 [3], accumulated into likewise: [0] bits (1: a term was infinite or NaN; 2: a finite term had
 *                          |delta| >= 256), [1] / [2] the number of terms of either kind
 * A term is one (id, class): delta = var_logp - ref_logp (the single float32 subtraction of the reduce), q = rne(delta * 2^30), valid when
 * delta is finite and |delta| < 256 (so |q| < 2^38).  An invalid term adds nothing to the table and is counted in status.  A column whose
 * reference symbol is not A/C/G/T and a site whose group lies outside [0, n_groups) add nothing anywhere.  n_sites <= 2^24 (refused
 * otherwise): with at most 2^24 terms per cell no word overflows; the caller who keeps adding to one table watches the n words.  Any
 * [first, first+count) inside [0, n_sites*W*3) may be asked for.  The adds are 64-bit integer atomics (through a per-block LDS table
 * where the groups' cells fit and the call is long enough to be contended): the table is the same integers whatever the chunking and
 * the order of arrival.  One launch; count == 0 launches nothing. */
int mural_mutagenesis_profile_window(const float* ref_logp, const float* var_logp, const uint8_t* ref_symbols, const int32_t* group,
                                     int64_t n_sites, int32_t W, int32_t n_class, int32_t n_groups, int64_t first, int64_t count,
                                     uint64_t* table, uint64_t* status, void* stream);
/* Alleles that change the sequence's length.  Allele v of the table replaces the '+'-strand bases
 * [a_pos[v], a_pos[v] + a_ref_len[v]) by a_alt_len[v] plain bases: base i (0..3 = A C G T) in bits 2i, 2i+1 of a_alt[v].  ref_len = 0 is
 * an insertion before a_pos (a_pos = g->length appends), alt_len = 0 a deletion.  An allele is LIVE iff 0 <= a_pos, 0 <= a_ref_len,
 * a_pos + a_ref_len <= g->length and 0 <= a_alt_len <= 32; any other reads the genome as it is.  Position q of the alternate haplotype
 * (length g->length + alt_len - ref_len) is genome[q] for q < p, alt[q - p] for p <= q < p + alt_len, genome[q - (alt_len - ref_len)]
 * after that and N outside it.  The inserted bases are plain bases (nmask and the amb_pos side table are not consulted for them); every
 * other column keeps the N / IUPAC rules of the plain encoders.
 *
 * mural_encode_allele_windows: one row per (site, allele).
 *   pos / strand         : dev int64 / uint8 [n], the row's site IN ALTERNATE-HAPLOTYPE COORDINATES (strand 1 = '-')
 *   allele               : dev int64 [n], an index into the table; -1 or any value outside [0, n_alleles): no allele
 *   a_pos, a_ref_len, a_alt_len : dev int64 [n_alleles];   a_alt : dev uint64 [n_alleles]
 *   symbols              : dev uint8 [n][W] of window_geometry(radius, indel), 4-byte aligned, or NULL
 *   cat_x                : dev int64 [n][2*local_radius+1-(local_order-1)] (the SNV local window), or NULL
 * Row i is, bit for bit, mural_encode_symbols(.., radius, indel) / mural_encode_kmer(.., local_radius, local_order, indel=0) of (pos[i],
 * strand[i]) on the alternate haplotype.  The kernel of mural_encode_subst_windows with another base reader: one launch, n == 0 launches
 * nothing, the genome buffers are only read.
 *
 * mural_allele_rows: the sites an allele can reach, i.e. all sites outside the replaced span whose window can differ between the two
 * haplotypes.  With (off0, W) the window of (radius, indel), allele v has W - 1 slots; slot c stands for e = c - (off0 + W - 1) (indel =
 * 0: e in [-R, R - 1]; indel = 1: [-R, R - 2]).  e < 0: ref_pos = alt_pos = p + e;  e >= 0: ref_pos = p + ref_len + e, alt_pos = ref_pos +
 * alt_len - ref_len.  Row id = v*(W - 1) + c; the call writes ids [first, first+count) to index id - first of
 *   ref_pos / alt_pos    : dev int64 [count], the site on the genome / on the alternate haplotype (either may lie outside its record)
 *   row_strand           : dev uint8 [count], strand[v] (strand: dev uint8 [n_alleles], one per allele)
 *   row_allele           : dev int64 [count], v, or -1 for an allele that is not live (whose rows are those of ref_len = alt_len = 0) */
int mural_encode_allele_windows(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, const int64_t* allele, int64_t n,
                                const int64_t* a_pos, const int64_t* a_ref_len, const int64_t* a_alt_len, const uint64_t* a_alt,
                                int64_t n_alleles, int32_t radius, int32_t indel, int32_t local_radius, int32_t local_order,
                                uint8_t* symbols, int64_t* cat_x, void* stream);
int mural_allele_rows(const MuralGenome* g, const int64_t* a_pos, const int64_t* a_ref_len, const int64_t* a_alt_len, int64_t n_alleles,
                      const uint8_t* strand, int32_t radius, int32_t indel, int64_t first, int64_t count, int64_t* ref_pos,
                      int64_t* alt_pos, uint8_t* row_strand, int64_t* row_allele, void* stream);

/* One training batch gathered and encoded from ROW INDICES in one launch (csrc/train_batch.hip): the rows of a batch may lie on several
 * chromosomes, which the three encoders above cannot take in one call.
 *   genomes    : dev MuralGenome[n_genomes] (the structs themselves live on the device)
 *   row_chrom / row_pos / row_strand / row_label : dev int32 / int64 / uint8 / uint8 [n_rows], the sites of an epoch (row_chrom
 *                indexes genomes; row_strand 1 = '-'; row_label the class label)
 *   order      : dev int64 [n_order], row numbers in the order the epoch visits them; the batch is order[first .. first + B - 1]
 * For batch row b, r = order[first + b]:
 *   cat_out[b]    (dev int64 [B][cols], cols as mural_encode_kmer's)      = mural_encode_kmer of (row_pos[r], row_strand[r]) on genome row_chrom[r]
 *   sym_out[b]    (dev uint8 [B][W], W as mural_encode_symbols', 4-byte aligned; NULL: not written)   = mural_encode_symbols of the same site
 *   onehot_out[b] (dev float [B][4][W]; NULL: not written)                = mural_encode_onehot of the same site
 *   y_out[b]      (dev float [B])                                         = row_label[r]
 * bit for bit.  At least one of sym_out / onehot_out is given.  An order entry outside [0, n_rows) or a row_chrom outside [0, n_genomes)
 * is never dereferenced: that batch row is encoded as a window of N (k-mer id 4^local_order) with label 0, and MURAL_E_INVALID is OR-ed
 * into *status (dev int32[1], never NULL; nothing is read back).  first / B outside the order fail on the host (MURAL_E_INVALID).    */
int mural_train_batch_encode(const MuralGenome* genomes, int32_t n_genomes, const int32_t* row_chrom, const int64_t* row_pos,
                             const uint8_t* row_strand, const uint8_t* row_label, int64_t n_rows, const int64_t* order, int64_t n_order,
                             int64_t first, int32_t B, int32_t local_radius, int32_t local_order, int32_t distal_radius, int32_t indel,
                             int64_t* cat_out, uint8_t* sym_out, float* onehot_out, float* y_out, int32_t* status, void* stream);

/* Site enumeration (csrc/sites.hip; no reference counterpart -- its users write one BED row per site with scripts of their own):
 * the positions of the window [lo, hi) of the record (0-based half-open like a BED row, clamped to the record) that a prediction run
 * takes as sites, in ascending order, as the (pos, strand) pairs the encoders and the packed forwards take.
 *   focal A:   base exactly A ('+', strand 0) or exactly T ('-', strand 1);
 *   focal C:   base exactly C ('+') or exactly G ('-'); context CPG keeps a '+' site whose NEXT base in the record is exactly G and a
 *              '-' site whose PREVIOUS base is exactly C, NONCPG keeps the others (a neighbour beyond the record's ends, or one that is
 *              N or an IUPAC code, makes the site non-CpG; a neighbour outside [lo, hi) counts like any other);
 *   focal ANY: every base that is exactly A, C, G or T, on '+' (INDEL models).
 * A base whose nmask bit is set (N and every entry of the IUPAC side table) is never a site.  Contexts other than ALL need focal C.
 * mural_sites_count leaves tile_counts[t] = sites before tile t, tile_counts[tiles] = *total = all sites of the window (dev int64
 * [mural_sites_tiles(length, lo, hi) + 1] and dev int64 [1]); mural_sites_emit, given the same window and selection and those
 * offsets, writes the sites number first .. first + n - 1 of the enumeration (the caller keeps first + n <= total) to pos / strand
 * (dev, n entries each).  Deterministic: no atomics.
 *   focal SET: the union of site classes whose MURAL_CLASS_* bits `context` carries (1..7): class A = the sites of focal A, NONCPG /
 *              CPG = those of focal C with that context.  Strand as above (0 for A / C, 1 for T / G), one ascending enumeration --
 *              the rows of a run that serves one model per class (mural_sites_classify).  ANY is NOT the union of all three: it puts
 *              every base on '+'.                                                                                                  */
enum { MURAL_FOCAL_A = 0, MURAL_FOCAL_C = 1, MURAL_FOCAL_ANY = 2, MURAL_FOCAL_SET = 3 };
enum { MURAL_CLASS_A = 1, MURAL_CLASS_NONCPG = 2, MURAL_CLASS_CPG = 4 };
enum { MURAL_CONTEXT_ALL = 0, MURAL_CONTEXT_CPG = 1, MURAL_CONTEXT_NONCPG = 2 };
int64_t mural_sites_tiles(int64_t length, int64_t lo, int64_t hi);
int mural_sites_count(const MuralGenome* g, int64_t lo, int64_t hi, int32_t focal, int32_t context, int64_t* tile_counts,
                      int64_t* total, void* stream);
int mural_sites_emit(const MuralGenome* g, int64_t lo, int64_t hi, int32_t focal, int32_t context, const int64_t* tile_counts,
                     int64_t first, int64_t n, int64_t* pos, uint8_t* strand, void* stream);

/* Rows of several site classes in one call (csrc/sites.hip): which model of a set a row belongs to, the rows of each class, and the
 * members' outputs back in row order.  Plain loads and stores, no atomics: every result is a function of the inputs alone.
 *   mural_sites_classify: cls[i] (dev uint8 [n]) = MURAL_ROW_CLASS_A / _NONCPG / _CPG of the site (pos[i], strand[i]) by the rules of
 *     the enumeration above, MURAL_ROW_CLASS_NONE for a position outside the record, a masked base (N, IUPAC) or a strand that is not
 *     the base's (0 for A / C, 1 for T / G; any other value included).  n == 0 launches nothing.
 *   mural_rows_split: the stable partition of the row indices 0 .. n-1 by a class column (dev uint8 [n]).  perm (dev int64 [n]) lists
 *     every row of class 0 in ascending row order, then class 1, .. class n_classes - 1 (1 <= n_classes <= 8); counts (dev int64
 *     [n_classes + 1]): counts[c] = rows of class c, counts[n_classes] = rows of a class >= n_classes, which are left out of perm (its
 *     last counts[n_classes] entries are not written).  workspace: dev, mural_rows_split_workspace_bytes(n, n_classes) bytes (0 for
 *     bad arguments), MURAL_E_WORKSPACE when smaller.  n == 0 zeroes counts and reads no other pointer.
 *   mural_rows_scatter: dst[perm[j]][:] = src[j][:] for j < m; rows of `cols` elements of elem_bytes 4 or 8 (float / double), dst of
 *     dst_rows rows; a perm entry outside [0, dst_rows) is skipped.  perm entries are distinct (a slice of mural_rows_split's).      */
enum { MURAL_ROW_CLASS_A = 0, MURAL_ROW_CLASS_NONCPG = 1, MURAL_ROW_CLASS_CPG = 2, MURAL_ROW_CLASS_NONE = 255 };
int mural_sites_classify(const MuralGenome* g, const int64_t* pos, const uint8_t* strand, int64_t n, uint8_t* cls, void* stream);
size_t mural_rows_split_workspace_bytes(int64_t n, int32_t n_classes);
int mural_rows_split(const uint8_t* cls, int64_t n, int32_t n_classes, int64_t* perm, int64_t* counts, void* workspace,
                     size_t workspace_bytes, void* stream);
int mural_rows_scatter(const void* src, const int64_t* perm, int64_t m, int32_t cols, int32_t elem_bytes, void* dst, int64_t dst_rows,
                       void* stream);

/* Observed mutations joined to enumerated sites (csrc/sites.hip): the label column of a regions run.  pos / strand: what
 * mural_sites_emit wrote (dev, n entries, pos ascending).  mut_start / mut_strand / mut_label: ONE chromosome's list of observed
 * mutations (dev, m entries, mut_start STRICTLY ascending; strand 0 '+', 1 '-'; label = the class, mut_type).  One binary search per
 * site: label[i] = mut_label[j] where mut_start[j] == pos[i], 0 where no entry matches (dev float [n]).
 *   stats: dev int64 [2], set to {0, INT64_MAX} by the caller before the first call; it accumulates over calls:
 *     stats[0] += the rows that found an entry (an entry whose label is 0 counts);
 *     stats[1]  = min(stats[1], j) over matched entries j with mut_strand[j] != strand[i], only when check_strand != 0 (the SNV
 *                 selections; focal ANY puts every site on '+' and passes 0).
 *   Integer atomics only: both words depend on the set of rows alone, however they are split into calls, parts or ranks.
 * n == 0 launches nothing; m == 0 writes zeros and reads no mut_* pointer (they may be NULL).  64-bit indices throughout.          */
int mural_sites_label(const int64_t* pos, const uint8_t* strand, int64_t n, const int64_t* mut_start, const uint8_t* mut_strand,
                      const float* mut_label, int64_t m, int32_t check_strand, float* label, int64_t* stats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SNV model family (Network0 / Network1 / Network2, MuRaL/model/model_snv.py:19-525), eval mode.
 * Raw parameters are handed over as HOST pointers in the reference's state_dict naming; the library
 * folds BatchNorm running statistics, builds the first-layer 3-mer lookup tables and the MFMA weight
 * fragments, and keeps device copies inside the opaque handle.
 * ---------------------------------------------------------------------------------------------- */
typedef struct { const float *weight, *bias, *running_mean, *running_var; } MuralBN;   /* host, [C] each */
typedef struct { const float *weight, *bias; } MuralAffine;                             /* host */

typedef struct {            /* ResBlock, model_snv.py:794-812 */
  MuralBN bn1; MuralAffine conv1;   /* conv weight [C][C][3] */
  MuralBN bn2; MuralAffine conv2;
} MuralResBlock;

typedef struct {            /* one conv tower, model_snv.py:350-388 (mid) / :392-430 (large) */
  MuralBN bn_in;  MuralAffine conv_in;     /* conv1.0 / conv1.1   weight [C][4][K] */
  MuralResBlock rbs1[2];                    /* RBs1.{0,1} */
  MuralBN bn_mid; MuralAffine conv_mid;    /* conv2.0 / conv2.1   weight [C][C][K] */
  MuralResBlock rbs2[2];                    /* RBs2.{0,1} */
  MuralBN bn_out; MuralAffine conv_out;    /* conv3.0 / conv3.1 (+ReLU) */
  MuralBN fc_bn;  MuralAffine fc;          /* distal_fc.0 / distal_fc.2  weight [n_class][C] */
} MuralTower;

typedef struct {            /* local branch, model_snv.py:322-339 */
  const float* emb;                         /* emb_layer.weight [emb_rows][5] */
  MuralAffine lin[2];                       /* lin_layers.{0,1}: [h1][5*cols], [h2][h1] */
  MuralBN bn[2];                            /* bn_layers.{0,1} */
  MuralAffine out;                          /* local_fc.0 (Network2) / model.output_layer (Network0) */
} MuralLocal;

typedef struct {
  int32_t model_no;        /* 0 local-only, 1 towers only, 2 both (nn_utils.py:213-216)            */
  int32_t n_class;
  int32_t local_cols;      /* number of k-mer columns = len(emb_dims)                              */
  int32_t emb_rows;        /* 4^local_order + 1                                                    */
  int32_t hidden1, hidden2;
  int32_t channels;        /* CNN_out_channels (this build: 32)                                    */
  int32_t ksize;           /* CNN_kernel_size  (this build: 3)                                     */
  int32_t distal_len;      /* 2*distal_radius + 1                                                  */
  float bn_eps;            /* 1e-5 */
} MuralSnvShape;

typedef struct { MuralLocal local; MuralTower mid, large; } MuralSnvParams;

typedef struct MuralSnvModel MuralSnvModel;

int  mural_snv_model_create(const MuralSnvShape* shape, const MuralSnvParams* host_params, MuralSnvModel** out);
void mural_snv_model_destroy(MuralSnvModel* m);

/* scratch the forward calls need for a batch of n rows (bytes; allocate once, reuse).
 * dense != 0: for mural_snv_forward_dense (adds n*distal_len symbol bytes); 0: for mural_snv_forward_packed */
size_t mural_snv_workspace_bytes(const MuralSnvModel* m, int64_t n, int32_t dense);
/* The smallest workspace the forward calls accept.  mural_snv_workspace_bytes keeps the pooled stage-3 inputs of up to four
 * 131072-site chunks (5.5 KB per site at the default geometry: + 2.2 GB on calls of >= 524288 sites) so that the short stages run as
 * one launch per tower (~1 % faster); with a workspace between the two sizes they run per chunk -- same results bit for bit.       */
size_t mural_snv_workspace_bytes_min(const MuralSnvModel* m, int64_t n, int32_t dense);

/* Replaces Network{0,1,2}.forward((cont_x, cat_x), distal_x) (model_snv.py:104-108, :226-287, :439-525)
 * for already-encoded tensors.  cat_x: dev int64 [n][local_cols] (ignored for model_no 1);
 * distal_x: dev float [n][4][distal_len] contiguous (ignored for model_no 0).
 * out: dev float [n][n_class] -- log-probabilities (Network1/2) or raw logits (Network0).
 * status: dev int32[1], set to MURAL_E_ENCODING by the kernels if a distal column is not a MuRaL
 * encoding; while it is set the call's output is overwritten with NaN, so the failure is visible
 * without a host round trip (the caller reads and clears the word whenever it synchronises); may be NULL. */
int mural_snv_forward_dense(const MuralSnvModel* m, const int64_t* cat_x, const float* distal_x, int64_t n,
                            float* out, void* workspace, size_t workspace_bytes, int32_t* status, void* stream);
/* The same forward for windows handed over as ONE SYMBOL BYTE per column (dev uint8 [n][distal_len], MURAL_SYM_* codes 0..14 as
 * mural_op_dense_to_symbols / mural_host_dense_to_symbols / mural_encode_symbols write them; the bytes are not checked).  Workspace:
 * mural_snv_workspace_bytes(m, n, 0).                                                                                            */
int mural_snv_forward_symbols(const MuralSnvModel* m, const int64_t* cat_x, const uint8_t* symbols, int64_t n, float* out,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Fused encode + forward straight from the packed genome: the path `mural_snv predict` takes
 * (replaces preprocessing.py:636-723 + :756-816 + model_snv.py:439-525 for n sites).
 * local_radius / local_order describe the k-mer window of the local branch.                        */
int mural_snv_forward_packed(const MuralSnvModel* m, const MuralGenome* g, const int64_t* pos,
                             const uint8_t* strand, int64_t n, int32_t local_radius, int32_t local_order,
                             float* out, void* workspace, size_t workspace_bytes, void* stream);

/* Cross-position reuse for dense same-strand site lists (no reference counterpart beyond the window
 * sharing of its encoders, MuRaL/data/preprocessing.py:602-610, :808-814).  Same result as mural_snv_forward_packed (within
 * rounding of identical operation sequences; parity tests: 1e-5 on probabilities) for n sites of one chromosome that lie inside
 * [pos_min, pos_max] (host-known bounds, at most mural_snv_reuse_chunk_span() bases apart) on the strands named by `strands`
 * (bit 0: '+' sites occur, bit 1: '-' sites occur; a site outside the bounds or on an unnamed strand comes back as NaN): the
 * first conv stage of both towers is evaluated once per base of the span and strand as dilated convs over pooled rows, and per
 * site only the pooled columns next to the window edges are recomputed.  Pays off from a site density of a few percent of the
 * bases.  Needs mural_snv_reuse_supported(m) (model_no 1 / 2, fused shape,
 * at least 18 pooled columns per tower: distal_radius >= 135).                                                       */
int     mural_snv_reuse_supported(const MuralSnvModel* m);
int64_t mural_snv_reuse_chunk_span(void);
size_t  mural_snv_reuse_workspace_bytes(const MuralSnvModel* m, int64_t n, int64_t span, int32_t strands);
int mural_snv_forward_packed_reuse(const MuralSnvModel* m, const MuralGenome* g, const int64_t* pos, const uint8_t* strand,
                                   int64_t n, int32_t strands, int64_t pos_min, int64_t pos_max, int32_t local_radius,
                                   int32_t local_order, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* Debug/validation hook used by the parity tests: same as forward_dense for the first tile, and dumps
 * the LDS-resident stage outputs of that tile to `taps` (dev float, see mural_snv_tap_layout).      */
int mural_snv_debug_taps(const MuralSnvModel* m, const int64_t* cat_x, const float* distal_x, int64_t n,
                         float* out, void* workspace, size_t workspace_bytes, float* taps, size_t taps_floats,
                         void* stream);
/* geometry of the fused kernel for this model: fills out[0..15] =
 * {P, NBUF_floats, L2_large, L3_large, L4_large, L2_mid, L3_mid, L4_mid, n_tap_slots, ...}          */
int mural_snv_tap_layout(const MuralSnvModel* m, int32_t* out16);

/* ------------------------------------------------------------------------------------------------
 * INDEL model (UNet_Small, MuRaL/model/model_indel.py:21-176), eval mode.  Parameters are HOST pointers in the
 * reference's state_dict naming; conv weights are [Cout][Cin][K].
 * ---------------------------------------------------------------------------------------------- */
typedef struct { MuralAffine conv; MuralBN bn; } MuralConvBN;            /* Sequential(Conv1d, BatchNorm1d) */
typedef struct { const float* conv5_w; MuralBN bn1; const float* conv1_w; MuralBN bn2; } MuralConvBlock;   /* :6-19 */

typedef struct {
  int32_t n_class;
  int32_t channels;        /* CNN_out_channels (8 in every shipped model)                          */
  int32_t ksize;           /* CNN_kernel_size (7)                                                  */
  int32_t down[6];         /* down_list                                                            */
  int32_t use_reverse;     /* strand-symmetrising input conv present (insertion models)            */
  int32_t length;          /* input length 2*distal_radius                                         */
  float bn_eps;
} MuralIndelShape;

typedef struct {
  MuralConvBN sym;                 /* conv.{0,1} (only when use_reverse)                           */
  MuralConvBN up_l[6];             /* uplblocks.i.{0,1}                                            */
  MuralConvBlock up_b[6];          /* upblocks.i.0.conv.{0,1,3,4}                                  */
  MuralConvBN down_l[5];           /* downlblocks.j.{1,2}                                          */
  MuralConvBlock down_b[5];        /* downblocks.j.0.conv.{0,1,3,4}                                */
  MuralAffine out1; MuralBN out_bn; MuralAffine out2;   /* out_conv.{0,1,3}                        */
  MuralBN fc_bn; MuralAffine fc;   /* out_fc.{0,2}                                                 */
} MuralIndelParams;

typedef struct MuralIndelModel MuralIndelModel;
int  mural_indel_model_create(const MuralIndelShape* shape, const MuralIndelParams* host_params, MuralIndelModel** out);
void mural_indel_model_destroy(MuralIndelModel* m);
size_t mural_indel_workspace_bytes(const MuralIndelModel* m, int64_t n);
/* Replaces UNet_Small.forward(distal_input) (model_indel.py:151-176).  distal_x: dev float [n][4][length];
 * out: dev float [n][n_class] positive Softplus scores (callers apply softmax, run_predict.py:214).  Any float tensor is accepted;
 * columns that are one-hot / IUPAC-fraction columns of the reference's encoder (preprocessing.py:756-816) travel as one symbol byte
 * each through the table-driven first level of the packed entry (same scores bit for bit), the others are evaluated from their floats. */
int mural_indel_forward_dense(const MuralIndelModel* m, const float* distal_x, int64_t n, float* out,
                              void* workspace, size_t workspace_bytes, void* stream);
/* The same for sites of a packed genome: replaces seq_ohe_encoder (MuRaL/data/preprocessing.py:756-816; indel window
 * [pos - R + 1, pos + R], :564-566) + UNet_Small.forward.  The window is decoded inside the first level's kernel and the
 * strand-symmetrising input conv (model_indel.py:29-32, :154-155) is evaluated there per symbol, so the one-hot window never
 * exists in HBM.  pos: dev int64 [n], strand: dev uint8 [n] (1 = '-'); the model's length must be 2 * R.                    */
int mural_indel_forward_packed(const MuralIndelModel* m, const MuralGenome* genome, const int64_t* pos, const uint8_t* strand,
                               int64_t n, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* The same from one symbol byte per window column: symbols dev uint8 [n][length], MURAL_SYM_* codes 0..14 (what mural_encode_symbols /
 * mural_encode_subst_symbols write).  The scores equal, bit for bit, mural_indel_forward_dense on the one-hot windows the bytes stand
 * for (and so mural_indel_forward_packed when the bytes are mural_encode_symbols(.., indel = 1) of the sites).  Where the first level is
 * the fused kernel (down_list[0] == 1, 8 channels, k = 7, length a multiple of 4) the bytes are its input as they are: no dense window
 * exists in HBM and nothing is classified back; any other geometry expands each chunk into the workspace first.  A byte above 14 is
 * outside the contract: it reads as N in both geometries and never causes an access outside the caller's buffers.
 * mural_indel_workspace_bytes(m, n) suffices; n == 0 launches nothing.                                                         */
int mural_indel_forward_symbols(const MuralIndelModel* m, const uint8_t* symbols, int64_t n, float* out, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training-mode building blocks (MuRaL/training.py:404-450 over model_snv.py:439-525): forward with
 * batch-statistics BatchNorm and every backward, on [B][C][L] fp32 device tensors.  Composed by the
 * autograd glue in mural_amd/model/train_ops.py.  "zeroed by the caller" marks accumulation targets.
 * ---------------------------------------------------------------------------------------------- */
int mural_op_relayout(const float* W, float* wt, int32_t Cout, int32_t Cin, int32_t K, int32_t dgrad, void* stream);
int mural_op_conv1d(const float* in, const float* wt, const float* bias, float* out, int64_t B, int32_t Cin,
                    int32_t Cout, int32_t L, int32_t K, const float* pre_s, const float* pre_t, int32_t pre_relu,
                    int32_t post_relu, const float* res1, const float* res2, void* stream);
/* Batch sums of the training-mode BatchNorms live in accumulator blocks double[MURAL_BN_SLOTS][2][C], zeroed by the
 * caller: producers add into the copy picked by their workgroup index (same-address atomics serialise), readers sum. */
#define MURAL_BN_SLOTS 32
int mural_op_bn_stats(const float* x, int64_t B, int32_t C, int32_t L, int32_t relu, double* acc, void* stream);
int mural_op_bn_finalize(const double* acc, double n, int32_t C, const float* gamma,
                         const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                         float* scale, float* shift, float* mean, float* invstd, void* stream);
int mural_op_bn_apply(const float* x, int64_t B, int32_t C, int32_t L, int32_t relu, const float* scale,
                      const float* shift, float* y, void* stream);
int mural_op_bn_backward(const float* dz, const float* x, int64_t B, int32_t C, int32_t L, int32_t relu,
                         const float* mean, const float* invstd, const float* gamma, double* acc,
                         int32_t have_sums, const float* add1, const float* add2, float* dx, float* dgamma, float* dbeta,
                         void* stream);
int mural_op_conv_wgrad(const float* dy, const float* x, int64_t B, int32_t C, int32_t L, int32_t K,
                        const float* scale, const float* shift, int32_t pre_relu, float* dW, float* db,
                        float* part, size_t part_floats, void* stream);
/* MaxPool1d(k, s, p) in floor mode with -inf padding; arg holds the position of the FIRST maximum of each window, like torch.
 * A NaN input is skipped, not propagated (torch propagates it): the maximum of the window's other values is returned. */
int mural_op_maxpool_fwd(const float* x, int64_t rows, int32_t L, int32_t k, int32_t s, int32_t p, float* y,
                         int32_t* arg /* argmax positions for the backward; may be NULL (inference) */, void* stream);
int mural_op_maxpool_bwd_needs_zero(int32_t k, int32_t s);   /* 1: dx must be zeroed by the caller (overlapping windows) */
int mural_op_maxpool_bwd(const float* dy, const int32_t* arg, int64_t rows, int32_t L, int32_t Lout, int32_t k, int32_t s,
                         int32_t p, float* dx, void* stream);
/* First layer of a tower in training mode: maxpool1(Conv1d(BN(one-hot))) from window symbols (model_snv.py:473-475,
 * 496-497 under training.py:424), BN(4) batch statistics from the symbol histogram.  mural_op_first_plan gives the sizes of
 * the caller-allocated buffers: tab (floats), arg (bytes per pooled output) and the backward scratch (floats).       */
int mural_op_first_plan(int32_t C, int32_t pk, int64_t* tab_floats, int64_t* arg_bytes, int64_t* scratch_floats);
int mural_op_first_fwd(const uint8_t* sym, int64_t B, int32_t Lwin, int32_t col0, int32_t L1, int32_t C, int32_t pk,
                       int32_t ps, int32_t pp, const float* gamma, const float* beta, const float* W,
                       const float* bias, float eps, float momentum, float* running_mean, float* running_var,
                       unsigned long long* counts, float* tab, float* y, void* arg, void* stream);
int mural_op_first_bwd(const float* dy, const void* arg, const uint8_t* sym, int64_t B, int32_t Lwin,
                       int32_t col0, int32_t L1, int32_t C, int32_t pk, int32_t ps, int32_t pp, const float* tab,
                       const float* W, float* scratch, float* dW, float* dbias, float* dgamma, float* dbeta, void* stream);
int mural_op_linear_fwd(const float* x, const float* W, const float* b, int64_t B, int32_t I, int32_t O, float* y,
                        void* stream);
/* dx (optional), dW [O][I] and db [O] are fully written */
int mural_op_linear_bwd(const float* dy, const float* x, const float* W, int64_t B, int32_t I, int32_t O, float* dx,
                        float* dW, float* db, void* stream);
int mural_op_embedding_fwd(const int64_t* cat, const float* E, int64_t B, int32_t cols, int32_t rows, float* y,
                           void* stream);
/* dE [rows][5] zeroed by the caller; any table size (a table of up to 150 KB is summed in LDS first, a larger one directly);
 * indices outside [0, rows) count as row 0 / the last row, as in the forward */
int mural_op_embedding_bwd(const int64_t* cat, const float* dy, int64_t B, int32_t cols, int32_t rows, float* dE,
                           void* stream);
int mural_op_dropout(const float* x, int64_t total, float p, uint64_t seed, const uint64_t* seed_dev, float* y,
                     void* stream);
int mural_op_relu_mask(const float* g, const float* ref, int64_t total, float* y, void* stream);
int mural_op_head_fwd(const float* loc, const float* mid, const float* lar, int64_t B, int32_t nc, float* out,
                      void* stream);
int mural_op_head_bwd(const float* loc, const float* mid, const float* lar, const float* dout, int64_t B, int32_t nc,
                      float* dloc, float* dmid, float* dlar, void* stream);
int mural_op_dense_to_symbols(const float* x, int64_t n, int32_t L, uint8_t* sym, int32_t* status, void* stream);
/* Its HOST twin for loaders that yield host tensors (the reference's predict loop copies every fp32 window to the device batch by
 * batch, MuRaL/model/nn_utils.py:52-56): xs[b] = HOST float [rows[b]][4][L]; sym = HOST uint8 [sum rows][L], 255 for a column that is
 * no MuRaL encoding (*n_bad counts them).  Host threads; no device work.                                                          */
int mural_host_dense_to_symbols(const float* const* xs, const int64_t* rows, int64_t n_batches, int32_t L, uint8_t* sym,
                                int64_t* n_bad);
/* the small fields (y, cat_x) of the same host batches copied side by side into one (pinned) buffer: bytes[b] bytes from srcs[b]     */
int mural_host_concat(const void* const* srcs, const int64_t* bytes, int64_t n, void* dst);

/* ---------------------------------------------------------------------------------------------------------------
 * Post-head calibration of the prediction path in one pass over the (n, n_class) rows (run_predict.py:214-225):
 * F.softmax of the model output (skipped when in_is_prob) -> full-Dirichlet map softmax(W . [log clip(p); 1]) when
 * dirichlet_w != NULL (dev double [n_class][n_class + 1]; dirichletcal/calib/fulldirichlet.py:78-80, multinomial.py:60-64) ->
 * poisson_calibrate (MuRaL/model/calibration.py:10-23) when poisson != 0 -> apply_scaling (MuRaL/scripts/scaling.py:10-28)
 * when scale != 0.  out: dev double or float [n][n_class].  n_class <= 16.
 * ------------------------------------------------------------------------------------------------------------- */
int mural_calibrate_rows(const float* in, int64_t n, int32_t n_class, int32_t in_is_prob, const double* dirichlet_w,
                         int32_t poisson, double scale, void* out, int32_t out_f64, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The SNV training step in one call per direction (MuRaL/training.py:424-427: preds = model.forward(...) under model.train(),
 * loss.backward()), Network0 / 1 / 2 with CNN_out_channels = 32, CNN_kernel_size = 3.  `params`: DEVICE pointers in the
 * state_dict naming of MuralSnvParams (running_mean / running_var are updated in place like nn.BatchNorm1d with `momentum`;
 * num_batches_tracked is the caller's).  dropout_p[5] / seeds[5]: emb_dropout, the two local_dropout layers, distal_fc_dropout
 * of the mid and of the large tower, with the seed of each mask (seed_dev: optional device-resident counter added to every
 * seed).  Input: cat_x (dev int64 [B][local_cols]) and either distal_x (dev float [B][4][distal_len]; `status` as in
 * mural_snv_forward_dense) or `symbols` (dev uint8 [B][distal_len] from mural_op_dense_to_symbols).  out: dev float [B][n_class]
 * (log-probabilities; raw logits for Network0).  The workspace (mural_snv_train_workspace_bytes) carries every saved tensor
 * from the forward to the backward of the same batch and must not be touched in between.
 * mural_snv_train_backward: `grads` has the layout of `params`; every weight / bias / emb pointer receives the gradient of
 * that tensor for d(loss)/d(out) = dout (fully written, no accumulation); running_* pointers are ignored.
 * ------------------------------------------------------------------------------------------------------------- */
size_t mural_snv_train_workspace_bytes(const MuralSnvShape* shape, int64_t B);
int mural_snv_train_forward(const MuralSnvShape* shape, const MuralSnvParams* params, const int64_t* cat_x, const float* distal_x,
                            const uint8_t* symbols, int64_t B, const float* dropout_p, const uint64_t* seeds,
                            const uint64_t* seed_dev, float momentum, float* out, void* workspace, size_t workspace_bytes,
                            int32_t* status, void* stream);
int mural_snv_train_backward(const MuralSnvShape* shape, const MuralSnvParams* params, const MuralSnvParams* grads,
                             const int64_t* cat_x, const float* dout, int64_t B, const float* dropout_p, const uint64_t* seeds,
                             const uint64_t* seed_dev, void* workspace, size_t workspace_bytes, void* stream);

/* The criterion of the reference's training loops, nn.CrossEntropyLoss(reduction='sum') on the model output x [B][nc] with labels y
 * (MuRaL/training.py:327, :425), in one launch per direction: loss[0] = -sum_i (x[i][y_i] - logsumexp(x[i])) summed in a fixed order
 * (reproducible), prob = softmax(x) kept for the backward; dx = g[0] (prob - onehot(y)).  A label outside [0, nc) makes the loss NaN. */
int mural_op_ce_sum_fwd(const float* x, const int64_t* y, int64_t B, int32_t nc, float* prob, float* loss, void* stream);
int mural_op_ce_sum_bwd(const float* prob, const int64_t* y, const float* g, int64_t B, int32_t nc, float* dx, void* stream);
/* torch.nn.utils.clip_grad_norm_(parameters, max_norm) of training.py:430 over one flat float32 gradient buffer of n elements (16-byte
 * aligned; zero in the padding between the parameters' slots): total[0] = 2-norm, flat *= min(max_norm / (norm + 1e-6), 1).  scratch64:
 * 64 doubles of device scratch.  Two launches, fixed summation order (bitwise reproducible).                                        */
int mural_op_clip_grad_norm(float* flat, int64_t n, float max_norm, double* scratch64, float* total, void* stream);

/* torch.optim.Adam.step() of the reference's training loops (MuRaL/training.py:346-350, :432; amsgrad and maximize off) over flat float32
 * buffers that share ONE slot layout -- parameters, gradients, exp_avg, exp_avg_sq of every parameter at the same offsets, zero in the
 * padding (it stays zero) -- as one elementwise launch; n = elements (a multiple of 4, buffers 16-byte aligned), step = the 1-based
 * count of this update (bias corrections 1 - beta^step are formed on the host in double).                                             */
int mural_op_adam_flat(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
                       double beta2, double eps, double weight_decay, int64_t step, void* stream);

/* The state of a training loop that the HOST keeps in the reference (Adam's step count and bias corrections, the scheduled learning rate,
 * the epoch's loss sum: MuRaL/training.py:432-450) as one 128-byte block in DEVICE memory (8-byte aligned, zeroed by the caller, lr set),
 * so that a step captured into a HIP graph reads this step's values at every replay.  Only the tick kernel writes it; the caller writes
 * fields between steps with ordinary stream-ordered copies and reads the block back when it wants the figures.                         */
typedef struct MuralTrainState {
  double lr;            /*   0: the learning rate of the NEXT update                                                    */
  int64_t step;         /*   8: Adam updates done (the `step` of torch's optimizer state)                                */
  int64_t ticks;        /*  16: scheduler ticks done (`last_epoch` of torch's StepLR)                                    */
  double loss_sum;      /*  24: sum of the losses handed to the ticks, in double, in tick order                          */
  int64_t rows;         /*  32: sum of the ticks' `rows`                                                                 */
  int64_t steps_done;   /*  40: ticks since the caller last zeroed loss_sum / rows / steps_done                          */
  float step_size;      /*  48: (float)(lr / (1 - beta1^step))   } what the latest tick left for                         */
  float bc2_sqrt;       /*  52: (float)sqrt(1 - beta2^step)      } mural_op_adam_flat_state                              */
  int64_t reserved[9];  /*  56: zero                                                                                     */
} MuralTrainState;

/* One step of that state, one single-workgroup launch, in this order: step += 1; step_size / bc2_sqrt from the current lr (the host
 * expressions of mural_op_adam_flat, in double, rounded once); if loss (device float*, may be NULL): loss_sum += *loss, rows += rows;
 * steps_done += 1; then the scheduler tick -- torch's chainable StepLR plus the reference's restart rule (training.py:444-450), IEEE double
 * operations in the host's order: ticks += 1; if sched_step_size > 0 and ticks % sched_step_size == 0: lr *= gamma; if lr < min_lr: lr =
 * restart_lr.  sched_step_size == 0: no per-step scheduler (min_lr = 0 then switches the restart rule off as well).                    */
int mural_op_train_state_tick(MuralTrainState* state, const float* loss, int64_t rows, double beta1, double beta2,
                              int64_t sched_step_size, double gamma, double min_lr, double restart_lr, void* stream);
/* mural_op_adam_flat with step_size / bc2_sqrt read from *state (left there by the tick enqueued before it): same update, vector width,
 * grid and argument checks.  Reads the block, never writes it.                                                                        */
int mural_op_adam_flat_state(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const MuralTrainState* state,
                             double beta1, double beta2, double eps, double weight_decay, void* stream);

/* torch.optim.AdamW(amsgrad=True).step() (the reference's 'AdamW' / 'AdamW2', training.py:351-356; maximize off) over flat float32 buffers
 * of ONE slot layout -- parameters, gradients, exp_avg, exp_avg_sq, max_exp_avg_sq; zero padding stays zero -- as one elementwise launch:
 * p *= 1 - lr weight_decay (formed in double, rounded once); m += (1 - beta1)(g - m); v = beta2 v + (1 - beta2) g^2; vmax = max(vmax, v);
 * p -= step_size m / (sqrt(vmax) / bc2_sqrt + eps), step_size and bc2_sqrt as in mural_op_adam_flat.  n, alignment, step: as there.   */
int mural_op_adamw_amsgrad_flat(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, int64_t n,
                                double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, void* stream);
/* ... with lr, step_size and bc2_sqrt read from *state as a tick left them (lr: the rate the tick's scheduler left for the next update).
 * Same update, vector width, grid and argument checks.  Reads the block, never writes it.                                              */
int mural_op_adamw_amsgrad_flat_state(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, int64_t n,
                                      const MuralTrainState* state, double beta1, double beta2, double eps, double weight_decay,
                                      void* stream);
/* torch.optim.SGD(momentum, nesterov=True, dampening=0).step() with L2 weight decay (the reference's 'SGD', training.py:357-360) over flat
 * float32 buffers of ONE slot layout (parameters, gradients, momentum buffer), one elementwise launch: g' = g + weight_decay p;
 * buf = momentum buf + g'; p -= lr (g' + momentum buf).  A zero buf reproduces torch's first step (buf = g').                         */
int mural_op_sgd_flat(float* param, const float* grad, float* buf, int64_t n, double lr, double momentum, double weight_decay, void* stream);
/* ... with lr read from *state.  Reads the block, never writes it.                                                                    */
int mural_op_sgd_flat_state(float* param, const float* grad, float* buf, int64_t n, const MuralTrainState* state, double momentum,
                            double weight_decay, void* stream);

/* Long windows (distal_radius from ~15000 up to the first-stage kernel's LDS limit) whose second conv stage fits no fused kernel: the
 * handle is FRONT-ONLY (mural_snv_tap_layout()[10] == 1; the forward entries above refuse it) and this entry runs what still is fused --
 * window decode + first layer + pool (model_snv.py:473-476 of the large tower) and its first ResBlock stage on halo'd segments of the
 * pooled row, 86 % of the model's arithmetic.  s3_out: dev float [n][L3][32] = the large tower's pooled second-stage input (channel-
 * last), L3 = mural_snv_tap_layout()[3]; the caller finishes per layer (mural_amd/model/generic_eval.py).  Serves every long-window
 * model (distal_radius >= 2000).                                                                                                    */
int mural_snv_forward_front(const MuralSnvModel* m, const MuralGenome* genome, const int64_t* pos, const uint8_t* strand, int64_t n,
                            int32_t local_radius, int32_t local_order, float* s3_out, void* workspace, size_t workspace_bytes, void* stream);
/* ... and its second half where the mid tower and the head still run fused (mural_snv_tap_layout()[12] == 1; then at most
 * mural_snv_tap_layout()[11] sites per front / finish pair, both on THE SAME workspace: the front call leaves the local branch's logits
 * (hence its local_radius / local_order) and the mid tower's pooled row there): large_logits dev float [n][n_class] = the large
 * tower's fc output computed by the caller from s3_out (model_snv.py:482-495) -> out dev float [n][n_class] log-probabilities.      */
int mural_snv_forward_finish(const MuralSnvModel* m, const float* large_logits, int64_t n, float* out, void* workspace,
                             size_t workspace_bytes, void* stream);

/* name of the dominant kernel (the fused tower kernel), for bench.py's roofline report */
const char* mural_snv_kernel_name(void);

/* Live timing of the dominant kernel: between begin and end every launch of it is bracketed by HIP events
 * on the launch stream; end() synchronises those events and returns the summed duration and the count.  */
int mural_profile_begin(void);
int mural_profile_end(double* total_ms, int64_t* launches);

/* ---------------------------------------------------------------------------------------------------------------
 * Host-side ingest (no device work): FASTA -> packed genome, BED -> site arrays, bed_reader row order.
 * Replaces SeqIO.to_dict(SeqIO.parse(...)) (MuRaL/data/preprocessing.py:836), bed_reader (:39-106) and the base maps of
 * the per-character encoders (:655-666, :762-772) for the packed-genome path.
 * ------------------------------------------------------------------------------------------------------------- */
/* names: n_cap x name_cap chars (record id = text after '>' up to the first whitespace); lengths / offsets per record
 * (offset = byte offset of the first sequence line).  n_records = records in the file (may exceed n_cap).           */
int mural_fasta_scan(const char* path, int64_t n_cap, int32_t name_cap, char* names, int64_t* lengths,
                     int64_t* offsets, int64_t* n_records);
/* Pack one record into the MuralGenome format; amb_pos / amb_sym receive the positions and MURAL_SYM_* symbols of IUPAC
 * codes other than N (up to amb_cap; n_amb counts all of them); any non-nucleotide character is MURAL_E_INVALID (the
 * reference raises KeyError).                                                                                        */
int mural_fasta_pack(const char* path, int64_t offset, int64_t length, uint32_t* packed2, uint32_t* nmask,
                     int64_t* amb_pos, uint8_t* amb_sym, int64_t amb_cap, int64_t* n_amb);
/* Six-column BED (chrom start end name score strand); chrom_id indexes chrom_names (order of first appearance);
 * strand: 0 '+', 1 '-'; score = class label.  cap = 0 counts rows / chromosomes.                                    */
int mural_bed_read(const char* path, int64_t cap, int32_t* chrom_id, int64_t* start, int64_t* end, float* score,
                   uint8_t* strand, int32_t n_chrom_cap, int32_t name_cap, char* chrom_names, int64_t* n_rows,
                   int32_t* n_chroms);
/* Rank-local streaming ingest for N-rank prediction -- replaces the reference's "one BedTool per process, split big inputs by hand"
 * (MuRaL/scripts/run_predict.py:107, MuRaL/commands/predict.py:134-137).  mural_bed_index_scan lists the PIECES (<= piece_rows
 * consecutive rows of one chromosome: name, byte range, rows, start of the first row) among the lines that start in
 * [byte_lo, byte_hi); byte_lo = byte_hi = 0 only reports file_bytes (the inflated size of a gzip file).  n_pieces may exceed cap.
 * piece_order (may be NULL): four values per piece -- 1 if every row's (start, strand) is >= its predecessor's ('+' < '-'), i.e. the
 * piece already is in the order of the reference's output table (run_predict.py:227) | start of its last row | strand of its first
 * row | strand of its last row (0 '+', 1 '-', -1 no strand field).
 * mural_bed_parse_range parses rows skip_rows .. skip_rows + n_rows - 1 of the rows in [byte_lo, byte_hi) (all on `chrom`).
 * Every ingest entry point reads gzip files too (inflated once per process; pybedtools / gzip.open in the reference).            */
int mural_bed_index_scan(const char* path, int64_t byte_lo, int64_t byte_hi, int64_t piece_rows, int32_t name_cap, int64_t cap,
                         char* names, int64_t* piece_lo, int64_t* piece_hi, int64_t* piece_rows_out, int64_t* piece_first_start,
                         int64_t* piece_order, int64_t* n_pieces, int64_t* file_bytes);
int mural_bed_parse_range(const char* path, int64_t byte_lo, int64_t byte_hi, int64_t skip_rows, int64_t n_rows, const char* chrom,
                          int64_t* start, int64_t* end, float* score, uint8_t* strand);
/* order[k] = input row of output row k in bed_reader order (+ rows, then - rows of every central_bp-wide segment)    */
int mural_bed_segment_order(const int32_t* chrom_id, const int64_t* start, const uint8_t* strand, int64_t n,
                            int64_t central_bp, int64_t* order, int64_t* group, int64_t* n_groups);

/* ---------------------------------------------------------------------------------------------------------------
 * The prediction table (MuRaL/scripts/run_predict.py:230-238: sort_values(['chrom', 'start']) + to_csv(sep='\t',
 * float_format='%.4g', index=False)) formatted at kernel speed.  One text row per site:
 *     chrom \t start \t end \t strand \t mut_type \t prob0 ... \t prob{k-1} \n
 * integers as decimals, mut_type = int64(label) like numpy's astype, probabilities as Python's '%.4g' (byte-identical:
 * exact round-half-even on the binary value; NaN -> empty field = pandas' na_rep).  Rows are emitted in the order
 * perm[0..n) (NULL = input order): the caller sorts, the formatter writes.  The header line is the caller's.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
  const char* chrom_names;   /* HOST: n_chroms x name_stride chars, NUL-terminated (also for the device call)      */
  int32_t n_chroms, name_stride;
  const int32_t* chrom_id;   /* [n] index into chrom_names, NULL = every row is chromosome 0                        */
  const int64_t* start;      /* [n] */
  const int64_t* end;        /* [n] */
  const uint8_t* strand;     /* [n] 0 '+', 1 '-' */
  const float* label;        /* [n] BED score column (class label) */
  const void* prob;          /* [n][prob_stride] float or double, the first n_class entries of a row are written    */
  int32_t prob_f64, n_class;
  int64_t prob_stride;
  const int64_t* perm;       /* [n] output row i = input row perm[i]; NULL = identity                               */
  int64_t n;
  int32_t layout;            /* 0: the prediction table row above; 1: the six-column BED row bed_reader consumes
                                (chrom start end . label strand; prob is not read) -- synthetic inputs are written with it */
  int32_t reserved;
} MuralTsvRows;
/* upper bound of one formatted row in bytes (text buffers hold n * bound), -1 on a bad table                        */
int64_t mural_tsv_row_bound(const MuralTsvRows* t);
size_t mural_tsv_format_workspace_bytes(int64_t n);
/* column pointers, out, n_bytes (int64) and ws are DEVICE addresses; three launches on `stream`, no synchronisation:
 * the text lands in out[0 .. *n_bytes)                                                                             */
int mural_tsv_format_device(const MuralTsvRows* t, char* out, int64_t cap, int64_t* n_bytes, void* ws, size_t ws_bytes,
                            void* stream);
/* the same formatter on `threads` host threads (0 = up to 16) for tables in host memory                            */
int mural_tsv_format_host(const MuralTsvRows* t, char* out, int64_t cap, int64_t* n_bytes, int32_t threads);
/* '%.4g' of one value into out12 (NUL-terminated); returns the length                                              */
int mural_tsv_format_g4(double v, char* out12);
/* The reference's "different bases" check (MuRaL/data/preprocessing.py:479-484) on a gathered shard: rows is a device
 * (n, row_stride) float / double matrix whose column `col` holds the strand-complemented focal base, group the
 * non-decreasing bed_reader group id per row; bit 0 of *status (device int32) is set when two rows of one group differ. */
int mural_focal_group_check(const void* rows, int32_t rows_f64, int64_t row_stride, int64_t col, const int64_t* group,
                            int64_t n, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Validation-epoch analytics (device-side segmented reductions into float64 tables; the correlation / Newton algebra
 * on the tables is host work).  Replaces the pandas group-bys and per-row loops of MuRaL/evaluation/evaluation.py:
 * freq_kmer_comp_multi (:48-67), corr_calc_sub (:124-193), Evaluator.evaluate_regional_score (:544-587), ECELoss /
 * ClasswiseECELoss / BrierScore / mean CE (:209-290, :340-358) and the loss / gradient / Hessian sums of the full-Dirichlet
 * fit (dirichlet_python/dirichletcal/calib/multinomial.py:153-172).  status: device int32, bit 0 = bad code / chrom /
 * start, bit 1 = label or key out of range (such rows are skipped).  Tables must be zeroed by the caller.
 * ------------------------------------------------------------------------------------------------------------- */
/* keys[i] = base-5 number of codes[i][left0 .. left0+d) ++ codes[i][right0 .. right0+d) (order-1 codes 0..4);
 * with region_size > 0: + (i / region_size) * 5^(2d), rows of regions >= n_regions get key -1                      */
int mural_eval_kmer_keys(const int64_t* codes, int64_t n, int32_t ncols, int32_t left0, int32_t right0, int32_t d,
                         int64_t region_size, int64_t n_regions, int32_t* keys, int32_t* status, void* stream);
/* keys[i] = chrom_base[chrom_id[i]] + start[i] / window                                                           */
int mural_eval_window_keys(const int32_t* chrom_id, const int64_t* start, int64_t n, int64_t window,
                           const int64_t* chrom_base, int32_t n_chrom, int32_t* keys, int32_t* status, void* stream);
/* table [n_groups][1 + 2 n_class] += { rows, rows with label c, sum of prob[:, c] } of the rows with key g >= 0     */
int mural_eval_group_obs_pred(const int32_t* keys, const int32_t* label, const void* prob, int32_t prob_f64, int64_t n,
                              int32_t n_class, int32_t n_groups, double* table, int32_t* status, void* stream);
/* out [2 + 3 n_bins (1 + n_class)] += { NLL sum, Brier sum, top-label bins [n_bins][3], class bins [n_class][n_bins][3] }
 * with bin b = (bounds[b], bounds[b+1]] and cells (rows, score sum, hits)                                           */
int mural_eval_calib_metrics(const void* prob, int32_t prob_f64, const int32_t* label, int64_t n, int32_t n_class,
                             int32_t n_bins, const float* bounds, double* out, int32_t* status, void* stream);
/* out [1 + km + (km)^2] (km = n_class (n_class + 1)) += { loss sum, gradient, Hessian (if need_hessian) } of the
 * multinomial regression on [log clip(prob); 1] at weights [n_class][n_class + 1] (float64, device); n_class <= 8    */
int mural_eval_dirichlet_fit_terms(const void* prob, int32_t prob_f64, const int32_t* label, int64_t n, int32_t n_class,
                                   const double* weights, int32_t need_hessian, double* out, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The prediction table read back (mural_amd/tables.py: evaluate, calc_scaling_factor, scale).  Replaces the per-line parsing
 * loops of MuRaL/scripts/calc_kmer_corr.py:200-270 and calc_regional_corr.py:168-212 and the whole-table pd.read_csv of
 * MuRaL/scripts/scaling.py:22, :67.  A reader streams the table (plain or gzip, the header line skipped: the caller validates
 * it) in chunks cut after a newline (chunk_bytes is the target size; a chunk holds one row at least) and parses each chunk on
 * the device.  mural_table_next fills *chunk with the device columns of the next chunk (owned by the reader, valid until the
 * next call; n_rows = 0 at the end) and returns after the parse has completed (the next chunk is read meanwhile).  A malformed
 * row is MURAL_E_INVALID with its line number.  Chromosome ids are global over the table (order of first appearance),
 * mural_table_chrom_name names them.  Everything on `stream`.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct MuralTableReader MuralTableReader;
typedef struct {
  int64_t n_rows, row0;      /* rows of this chunk; rows of the table before it                                    */
  int64_t* start;            /* dev [n_rows] */
  int64_t* end;              /* dev [n_rows] */
  int32_t* mut_type;         /* dev [n_rows] */
  float* label;              /* dev [n_rows] mut_type as float (the formatter's label column)                      */
  uint8_t* strand;           /* dev [n_rows] 0 '+', 1 '-' */
  double* prob;              /* dev [n_rows][n_class] */
  int32_t* chrom_id;         /* dev [n_rows] */
  int32_t n_runs, n_chroms;  /* chromosome runs of this chunk; chromosomes named so far                            */
  const int64_t* run_row;    /* host [n_runs] first row of each run */
  const int32_t* run_chrom;  /* host [n_runs] its chromosome id */
  int64_t text_bytes;        /* bytes of text in the chunk */
} MuralTableChunk;
int mural_table_open(const char* path, int32_t n_class, int64_t chunk_bytes, MuralTableReader** reader);
int mural_table_next(MuralTableReader* reader, MuralTableChunk* chunk, void* stream);
const char* mural_table_chrom_name(const MuralTableReader* reader, int32_t id);
/* seconds reading / inflating (worker thread), seconds waiting for it, seconds of the device parse, text bytes so far */
int mural_table_stats(const MuralTableReader* reader, double* out4);
void mural_table_close(MuralTableReader* reader);
/* scaling.py:24-27 on the rows: prob[:, 1:] *= factor; prob[:, 0] = 1 - sum(prob[:, 1:]) (float64, left to right)          */
int mural_table_scale_rows(double* prob, int64_t n, int32_t n_class, double factor, void* stream);
/* scaling.py:67-90 (calc_mu_scaling_factor): per-block partials [mural_table_prob_sum_blocks()] of sum_rows w * sum_{c>=1}
 * prob and of sum_rows w, in an order fixed by n.  w = 1 without regions (reg_off NULL); otherwise the number of regions of
 * the row's chromosome that overlap [start, end) (pybedtools intersect without -u): reg_b0 / reg_b1 hold each chromosome's
 * region starts / ends, each sorted, in [reg_off[c], reg_off[c+1])                                                          */
int32_t mural_table_prob_sum_blocks(void);
int mural_table_prob_sum(const double* prob, const int32_t* chrom_id, const int64_t* start, const int64_t* end, int64_t n,
                         int32_t n_class, const int64_t* reg_off, const int64_t* reg_b0, const int64_t* reg_b1,
                         int32_t n_reg_chrom, double* part_sum, int64_t* part_cnt, void* stream);
/* calc_kmer_corr.py:246-262 with get_expanded_region (MuRaL/data/preprocessing.py:524-567): key = base-4 k-mer of
 * chrom[start - k/2 (+1 indel) : end + k/2] (Python slice), reverse-complemented on '-'; -1 if it is not k bases of A/C/G/T.
 * mode 0: the row's strand, 1 '+', 2 '-', 3 both (key_a forward, key_b reverse complement).  All rows on genome g.          */
int mural_table_kmer_keys(const MuralGenome* g, const int64_t* start, const int64_t* end, const uint8_t* strand, int64_t n,
                          int32_t k, int32_t indel, int32_t mode, int32_t* key_a, int32_t* key_b, void* stream);
/* first[key] = min(first[key], 2 * (row0 + i) + sub) over the rows with a key in [0, n_groups): the dict insertion order of
 * the reference's per-key tables                                                                                          */
int mural_table_first_row(const int32_t* keys, int64_t n, int64_t row0, int32_t sub, int32_t n_groups, uint64_t* first,
                          void* stream);
/* mn[c] = min(mn[c], start), mx[c] = max(mx[c], start) over the rows of chromosome c (the windows a chunk touches)        */
int mural_table_start_range(const int32_t* chrom_id, const int64_t* start, int64_t n, int32_t n_chrom, int64_t* mn,
                            int64_t* mx, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Genome summaries of a shard while it is on the device (mural_amd/predict.py: SummarySink; csrc/summary.hip): what
 * mural_eval_window_keys + mural_eval_group_obs_pred and mural_table_prob_sum compute from the written table, in one pass
 * over the rows of ONE chromosome that ascend in start.  No floating-point atomics: the result depends on the input (and the
 * fixed chunk of mural_summary_chunk_rows() rows per workgroup) alone, bit for bit.  float64 sums, exact counts.
 *   window tables: table[j] [n_bins[j]][1 + 2 n_class] += { rows, rows with label c, sum of prob[:, c] } of the rows with
 *     start / window[j] - bin0[j] == bin (the row layout of mural_eval_group_obs_pred); zeroed by the caller before the
 *     first part of a chromosome;
 *   totals: total[0] += sum_rows w * sum_{c>=1} prob[c], n_sites[0] += sum_rows w; w = 1 (reg_b0 NULL) or the number of
 *     regions overlapping [start, end), reg_b0 / reg_b1 [n_reg] the chromosome's region starts / ends, each sorted
 *     (mural_table_prob_sum's rule);
 *   status (device int32): bit 0 a negative start, bit 1 a label outside 0 .. n_class - 1 (or no whole number), bit 2 a
 *     start outside a table's windows or below an earlier row's; such rows are skipped.
 * Two launches on `stream`, no synchronisation.  n_class <= 8.
 * ------------------------------------------------------------------------------------------------------------- */
#define MURAL_SUMMARY_MAX_WINDOWS 4
typedef struct {
  const void* prob;          /* dev [n][prob_stride], float (prob_f64 = 0) or double; columns 0 .. n_class-1 are read          */
  int32_t prob_f64, label_kind;                     /* label: 0 float32, 1 int32, 2 int64                                       */
  int64_t prob_stride;       /* elements */
  const int64_t* start;      /* dev [n] */
  const int64_t* end;        /* dev [n] (read with regions only) */
  const void* label;         /* dev [n] */
  int64_t n;
  int32_t n_class, n_windows;
  int64_t window[MURAL_SUMMARY_MAX_WINDOWS], bin0[MURAL_SUMMARY_MAX_WINDOWS], n_bins[MURAL_SUMMARY_MAX_WINDOWS];
  double* table[MURAL_SUMMARY_MAX_WINDOWS];         /* dev */
  const int64_t* reg_b0;     /* dev [n_reg] or NULL */
  const int64_t* reg_b1;
  int64_t n_reg;
  double* total;             /* dev [1] */
  int64_t* n_sites;          /* dev [1] */
  int32_t* status;           /* dev [1] */
} MuralSummaryRows;
int32_t mural_summary_chunk_rows(void);
size_t mural_summary_workspace_bytes(int64_t n, int32_t n_class, int32_t n_windows);
/* ws: device scratch of mural_summary_workspace_bytes(n, n_class, n_windows) bytes, 8-byte aligned                          */
int mural_summary_rows(const MuralSummaryRows* s, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * k-mer rate tables of a shard while it is on the device (SummarySink(kmers=...); csrc/summary_kmer.hip): what
 * mural_table_kmer_keys + mural_eval_group_obs_pred + mural_table_first_row compute from the written table, in one pass
 * over the rows (any order) of a part of ONE chromosome, for up to MURAL_SUMMARY_MAX_KMERS k-mer lengths at once.  The
 * key of a row is mural_table_kmer_keys' (csrc/kmer_key.h holds the one decode both use); a row without a key for one k
 * still counts for the others.  Exact integer sums, integer atomics only: each probability is quantised once to
 * q = rne(p * 2^71), carried as hi = floor(p * 2^31) and lo = rint((p * 2^31 - hi) * 2^40), so the tables are a function
 * of the SET of rows alone -- bit-identical across runs and splits into parts.
 *   table[j] [4^k[j]][3][n_class] of unsigned 64-bit cells += { rows with label c, sum of hi of prob[:, c], sum of lo };
 *     on return lo < 2^40 (its overflow is carried into hi after at most 2^21 rows); the value of a class's cell is
 *     (hi * 2^40 + lo) / 2^71; zeroed by the caller before the first part;
 *   first[j] [4^k[j]] = min(first, order_base + 2 * start + sub), sub = 1 for mode 3's reverse-complement key: the dict
 *     insertion order of the reference's per-key tables when order_base is the chromosome's ordinal shifted above any
 *     2 * start + 1; set to all ones by the caller before the first part;
 *   status (device int32): bit 0 a negative start, bit 1 a label outside 0 .. n_class - 1 (or no whole number), bit 3 a
 *     probability that is NaN, negative or above 1; such rows are skipped in every table.
 * indel / mode: as mural_table_kmer_keys (mode 3 adds the row under both keys).  mural_summary_kmer_in_lds: 1 when the
 * table of (k, n_class) is accumulated in a workgroup's LDS and flushed, 0 when the rows add to global memory.
 * Launches on `stream`, no synchronisation.  n_class <= 8, 1 <= k <= 15.
 * ------------------------------------------------------------------------------------------------------------- */
#define MURAL_SUMMARY_MAX_KMERS 4
typedef struct {
  const MuralGenome* genome; /* the chromosome of the rows */
  const void* prob;          /* dev [n][prob_stride], float (prob_f64 = 0) or double; columns 0 .. n_class-1 are read          */
  int32_t prob_f64, label_kind;                     /* label: 0 float32, 1 int32, 2 int64                                       */
  int64_t prob_stride;       /* elements */
  const int64_t* start;      /* dev [n] */
  const int64_t* end;        /* dev [n] */
  const uint8_t* strand;     /* dev [n], 1 = '-' (read in mode 0 only) */
  const void* label;         /* dev [n] */
  int64_t n;
  int32_t n_class, n_k, indel, mode;
  int32_t k[MURAL_SUMMARY_MAX_KMERS];
  uint64_t* table[MURAL_SUMMARY_MAX_KMERS];         /* dev */
  uint64_t* first[MURAL_SUMMARY_MAX_KMERS];         /* dev */
  int64_t order_base;
  int32_t* status;           /* dev [1] */
} MuralSummaryKmerRows;
int32_t mural_summary_kmer_in_lds(int32_t k, int32_t n_class);
int mural_summary_kmer_rows(const MuralSummaryKmerRows* s, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Motif rate tables (`evaluate --motif_only`, MuRaL/scripts/calc_motif_corr.py:191-261; SummarySink(motifs=...) in flight,
 * tables.motif_table from a written table; csrc/summary_kmer.hip): one pass over the rows (any order) of a part of ONE
 * chromosome, for up to MURAL_SUMMARY_MAX_KMERS motif lengths m (odd, 3 .. 15) at once.  A row adds to every window of m
 * bases that contains its site, on the reference strand (no strand is read): window i is the Python slice
 * chrom[start - i : end + m-1 - i], i = 0 .. m-1, of an SNV row and chrom[start - i + 1 : end + m - i], i = 1 .. m-1, of an
 * INDEL row (`indel`); a window that is not m bases long after Python's clipping, or holds a base other than A/C/G/T, is
 * skipped, the row's other windows still count.  A motif and its reverse complement share the cell of
 * min(key, revcomp(key)), key = the base-4 number of the window (A0 C1 G2 T3, first base most significant): the tables
 * are indexed by all 4^m keys and the half of them that is the larger of its pair stays zero.  The cells, their
 * quantisation and the integer atomics are mural_summary_kmer_rows'.
 *   table[j] [4^m[j]][3][n_class] += per window { 1 for the row's label, hi of prob[:, c], lo of prob[:, c] }; on return
 *     lo < 2^40 (carried into hi after at most 2^18 rows: a row adds up to m <= 15 times to one cell, so lo stays below
 *     2^40 + 15 * 2^18 * 2^40 < 2^63; hi is exact for floor((2^32 - 2) / m) rows in one cell); zeroed by the caller;
 *   first[j] [4^m[j]] = min(first, (order_base + pos) << 5 | i << 1 | o), pos = the row's start, or with order_by_row
 *     its index in this call; o = 1 where the window's own key is the larger of the pair.  The minimum is the window
 *     the reference sees first (rows in table order, i ascending), which fixes the dict order of the entries and, by o,
 *     the orientation an entry is named after; set to all ones by the caller; 0 <= order_base + pos < 2^58;
 *   status: as mural_summary_kmer_rows; such rows are skipped in every table.
 * mural_summary_motif_in_lds: mural_summary_kmer_in_lds' rule, 4^m * (3 n_class + 1) * 8 bytes <= 160 KiB (0 for an m
 * that is refused).  One launch per m.  Launches on `stream`, no synchronisation.  n_class <= 8.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
  const MuralGenome* genome; /* the chromosome of the rows */
  const void* prob;          /* dev [n][prob_stride], float (prob_f64 = 0) or double; columns 0 .. n_class-1 are read          */
  int32_t prob_f64, label_kind;                     /* label: 0 float32, 1 int32, 2 int64                                       */
  int64_t prob_stride;       /* elements */
  const int64_t* start;      /* dev [n] */
  const int64_t* end;        /* dev [n] */
  const void* label;         /* dev [n] */
  int64_t n;
  int32_t n_class, n_m, indel, order_by_row;
  int32_t m[MURAL_SUMMARY_MAX_KMERS];
  uint64_t* table[MURAL_SUMMARY_MAX_KMERS];         /* dev */
  uint64_t* first[MURAL_SUMMARY_MAX_KMERS];         /* dev */
  int64_t order_base;
  int32_t* status;           /* dev [1] */
} MuralSummaryMotifRows;
int32_t mural_summary_motif_in_lds(int32_t m, int32_t n_class);
int mural_summary_motif_rows(const MuralSummaryMotifRows* s, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Loss and calibration metrics of a shard while it is on the device (SummarySink(calibration=True);
 * csrc/summary_calib.hip): the sums behind NLL / ECE / classwise ECE / Brier as calibrate_prob reports them
 * (MuRaL/evaluation/evaluation.py:207-295, 339-358), in one pass over the rows (any order) of a part.  Per row, in the
 * probabilities' own precision: q = softmax(log(prob)), confidence = max q (the first maximum is the prediction), Brier
 * term = sum_c ([c == label] - q_c)^2, NLL term = -log q_label, bins (lower, upper] on bounds [n_bins + 1] (the float32
 * linspace(0, 1, n_bins + 1) of the reference).  Integer cells and integer atomics only: the table is a function of the SET
 * of valid rows, bit for bit.
 *   table [mural_summary_calib_cells(n_class, n_bins)] of unsigned 64-bit cells, H = 6 + n_class, zeroed by the caller
 *     before the first part:
 *       [0] rows  [1] inf_rows  [2 + c] rows with label c  [2 + nc], [3 + nc] NLL hi, lo  [4 + nc], [5 + nc] Brier hi, lo
 *       [H + 4 (g n_bins + b) + 0 .. 3] rows, score hi, score lo, hits of bin b of group g: g = 0 the top-label bins
 *       (score = the confidence, hit = the prediction is the label), g = 1 + c class c (score = q_c, hit = label is c);
 *     a sum's term v is quantised once to rne(v * 2^(S + 46)): hi = floor(v * 2^S), lo = rint((v * 2^S - hi) * 2^46), value
 *     of a pair (hi * 2^46 + lo) / 2^(S + 46); S = 16 for scores and Brier terms, 13 for NLL terms (a row's error is at
 *     most 2^-60); on return lo < 2^46; 2^40 rows do not overflow a cell;
 *   a valid row with q_label == 0 (an infinite NLL term) counts in inf_rows and everywhere but the NLL sum;
 *   status (device int32): bit 1 a label outside 0 .. n_class - 1 (or no whole number), bit 3 a probability that is NaN,
 *     negative or above 1 (or a row with no positive probability); such rows are skipped everywhere.
 * mural_summary_calib_cells: 6 + n_class + 4 n_bins (n_class + 1), or 0 where that is more than the 4096 cells a
 * workgroup holds (or a size is out of range): mural_summary_calib_rows refuses such a table with MURAL_E_INVALID.
 * Two launches on `stream` per 2^28 rows, no synchronisation.  n_class <= 16.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
  const void* prob;          /* dev [n][prob_stride], float (prob_f64 = 0) or double; columns 0 .. n_class-1 are read          */
  int32_t prob_f64, label_kind;                     /* label: 0 float32, 1 int32, 2 int64                                       */
  int64_t prob_stride;       /* elements */
  const void* label;         /* dev [n] */
  int64_t n;
  int32_t n_class, n_bins;
  const float* bounds;       /* dev [n_bins + 1], ascending */
  uint64_t* table;           /* dev */
  int32_t* status;           /* dev [1] */
} MuralSummaryCalibRows;
int64_t mural_summary_calib_cells(int32_t n_class, int32_t n_bins);
int mural_summary_calib_rows(const MuralSummaryCalibRows* s, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Expected and observed mutations per annotated interval set of a shard while it is on the device
 * (SummarySink(annotations=...) in flight, tables.annotation_table from a written table; csrc/summary_annot.hip): per
 * group -- a name of the annotation file, e.g. the exons of a gene -- the label counts and probability sums of the rows
 * whose start lies in one of the group's pieces.  One call takes the rows of a part of ONE chromosome, ascending in start
 * (equal starts are legal), and that chromosome's pieces: piece p is [piece_b0[p], piece_b1[p]) of group piece_group[p];
 * row i belongs to it when piece_b0[p] <= start[i] < piece_b1[p] (`end` is not read).  The pieces of one group are
 * disjoint (tables.read_annotations merges them), those of different groups overlap freely, in any order.  Both ends of a
 * piece are lower bounds in start (the first row with start >= b), so a piece's rows are one range and its sums the
 * difference of two row prefix sums: tile sums of mural_summary_annot_tile_rows() rows, their exclusive scan, one lookup
 * per piece -- no per-row search of the pieces.  The cells, their quantisation (q = rne(p * 2^71) as two limbs) and the
 * integer atomics are mural_summary_kmer_rows': the table is a function of the SET of rows alone, bit for bit.
 *   table [n_groups][3][n_class] of unsigned 64-bit cells += per row of a piece { 1 for the row's label, hi of prob[:, c],
 *     lo of prob[:, c] }; on return lo < 2^40; the value of a class's cell is (hi * 2^40 + lo) / 2^71; zeroed by the
 *     caller once -- the groups are global, one table serves every chromosome and part;
 *   status (device int32): bit 0 a negative start, bit 1 a label outside 0 .. n_class - 1 (or no whole number), bit 3 a
 *     probability that is NaN, negative or above 1 -- such rows are skipped; bit 2 a start below the row before it inside
 *     the call: the table's content is then unspecified (nothing is read or written out of bounds).  A piece whose group
 *     is outside 0 .. n_groups - 1 is skipped.
 * The call works through slices of mural_summary_annot_slice_rows() = 2^23 rows (the unfolded lo prefixes stay below
 * 2^63) and mural_summary_annot_fold_pieces() = 2^20 pieces between two folds of the table; both are additive and invisible
 * to the caller.  ws: device scratch of mural_summary_annot_workspace_bytes(n, n_class) bytes -- (tiles of a slice + 1) *
 * 3 n_class * 8: 7.5 MB for a part of 5 M rows of 4 classes --, 8-byte aligned.  n == 0 or n_pieces == 0 launches nothing.
 * Launches on `stream`, no synchronisation, no read-back, no floating-point atomics.  n_class <= 8.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
  const void* prob;          /* dev [n][prob_stride], float (prob_f64 = 0) or double; columns 0 .. n_class-1 are read          */
  int32_t prob_f64, label_kind;                     /* label: 0 float32, 1 int32, 2 int64                                       */
  int64_t prob_stride;       /* elements */
  const int64_t* start;      /* dev [n], ascending */
  const void* label;         /* dev [n] */
  int64_t n;
  int32_t n_class, n_groups;
  const int64_t* piece_b0;   /* dev [n_pieces] */
  const int64_t* piece_b1;   /* dev [n_pieces] */
  const int32_t* piece_group; /* dev [n_pieces] */
  int64_t n_pieces;
  uint64_t* table;           /* dev [n_groups][3][n_class] */
  int32_t* status;           /* dev [1] */
} MuralSummaryAnnotRows;
int32_t mural_summary_annot_tile_rows(void);
int64_t mural_summary_annot_slice_rows(void);
int64_t mural_summary_annot_fold_pieces(void);
size_t mural_summary_annot_workspace_bytes(int64_t n, int32_t n_class);
int mural_summary_annot_rows(const MuralSummaryAnnotRows* s, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Expected and observed mutations per transcript by consequence of a shard while it is on the device
 * (SummarySink(transcripts=...) in flight, tables.consequence_table from a written table; csrc/summary_conseq.hip;
 * mural_amd.summaries.summary_conseq_host is the specification).  One call takes the SNV rows (n_class == 4) of a part of ONE
 * chromosome, ascending in start (equal starts are legal), and that chromosome's CDS segments as tables.read_transcripts
 * lists them: segment s is [seg_b0[s], seg_b1[s]) of transcript seg_tx[s], seg_cds0[s] the CDS offset of its first base in
 * transcript orientation (its last genomic base on a '-' transcript), seg_prev / seg_next the indices of the transcript's
 * neighbouring segments in that orientation (-1 at the ends); tx_strand [n_transcripts] (non-zero: '-') and tx_cds_len
 * [n_transcripts] are global.  For row i at q = start[i] and every segment with seg_b0 <= q < seg_b1:
 *   g = the reference base at q, r = the row's own base (complemented where strand[i] != 0); class c = 1 .. 3 is the
 *   substitution r > alt_order[r][c - 1] on the row's strand; x = the CDS offset of q; the codon is offsets 3 floor(x / 3) ..
 *   + 2, mapped to genomic positions over seg_prev / seg_next (at most two hops each) and read 5' -> 3' on the
 *   transcript's strand; aa [64] is indexed by 16 b0 + 4 b1 + b2 (A0 C1 G2 T3), '*' a stop.  All three classes go to bin 4
 *   (unresolved) where 3 floor(x / 3) + 2 >= tx_cds_len, a codon base is masked or lies outside the record, or a position is
 *   not found; otherwise class c goes to bin 0 (aa_ref == aa_alt), 2 (aa_alt == '*'), 3 (aa_ref == '*') or 1.
 *   table [n_transcripts][5][3] of unsigned 64-bit cells: cell [t][b] += { 1 where label[i] == c, hi of prob[i][c], lo of
 *     prob[i][c] } per (row, c) routed to bin b, the limbs of mural_summary_kmer_rows (q = rne(p * 2^71)); on return
 *     lo < 2^40; zeroed by the caller once -- the transcript ids are global, one table serves every chromosome and part;
 *   rows [n_transcripts][2] += { rows inside the CDS, rows of label 0 among them };
 *   class 0's probability is never read; a row counts once per transcript that covers it; both tables are a function of
 *   the SET of rows alone, bit for bit;
 *   status (device int32): bit 0 a negative start, bit 1 a label outside 0 .. 3 (or no whole number), bit 3 a probability
 *     of a class >= 1 that is NaN, negative or above 1 -- such rows are skipped; bit 2 a start below the row before it
 *     inside the call: the tables' content is then unspecified (nothing is read or written out of bounds).  A segment
 *     whose transcript is outside 0 .. n_transcripts - 1 is skipped.
 * strand: dev uint8 [n] or NULL for all '+'.  alt_order: each row names the three other bases once (MURAL_E_INVALID
 * otherwise).  The segments' row ranges are cut into chunks of at most mural_summary_conseq_chunk_rows() rows, listed by an
 * exclusive scan of the chunk counts (one workgroup of mural_summary_conseq_scan_threads() threads, a run of segments
 * each), and a grid of at most mural_summary_conseq_grid_waves() waves strides over the chunks.  n <= 2^31 and n_segments <=
 * 2^22 per call (MURAL_E_INVALID above: the bound that keeps a cell's lo limb below 2^63 until the fold that ends the call).
 * ws: mural_summary_conseq_workspace_bytes(n_segments) bytes (24 per segment), 8-byte aligned; MURAL_E_WORKSPACE when
 * smaller.  n == 0 or n_segments == 0 launches nothing.  Launches on `stream`, no synchronisation, no read-back, no
 * floating-point atomics.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
  const MuralGenome* genome; /* the chromosome of the rows */
  const void* prob;          /* dev [n][prob_stride], float (prob_f64 = 0) or double; columns 1 .. 3 are read                  */
  int32_t prob_f64, label_kind;                     /* label: 0 float32, 1 int32, 2 int64                                       */
  int64_t prob_stride;       /* elements */
  const int64_t* start;      /* dev [n], ascending */
  const uint8_t* strand;     /* dev [n], 1 = '-', or NULL */
  const void* label;         /* dev [n] */
  int64_t n;
  int32_t n_class, n_transcripts;                   /* n_class == 4 */
  const int64_t* seg_b0;     /* dev [n_segments] */
  const int64_t* seg_b1;     /* dev [n_segments] */
  const int64_t* seg_cds0;   /* dev [n_segments] */
  const int32_t* seg_tx;     /* dev [n_segments] */
  const int32_t* seg_prev;   /* dev [n_segments] */
  const int32_t* seg_next;   /* dev [n_segments] */
  int64_t n_segments;
  const uint8_t* tx_strand;  /* dev [n_transcripts] */
  const int64_t* tx_cds_len; /* dev [n_transcripts] */
  uint8_t aa[64];
  uint8_t alt_order[4][3];
  uint8_t reserved[4];
  uint64_t* table;           /* dev [n_transcripts][5][3] */
  uint64_t* rows;            /* dev [n_transcripts][2] */
  int32_t* status;           /* dev [1] */
} MuralSummaryConseqRows;
int64_t mural_summary_conseq_chunk_rows(void);
int64_t mural_summary_conseq_grid_waves(void);
int32_t mural_summary_conseq_scan_threads(void);
size_t mural_summary_conseq_workspace_bytes(int64_t n_segments);
int mural_summary_conseq_rows(const MuralSummaryConseqRows* s, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Expected and observed mutations per transcript by where a row lies in the transcript's structure
 * (SummarySink(transcripts=..., transcript_structure=True) in flight, tables.structure_table from a written table;
 * csrc/summary_txstruct.hip; mural_amd.summaries.summary_txstruct_host is the specification).  The rows, the genome, the
 * segments, the transcripts, aa, alt_order, the status bits and the limbs are those of mural_summary_conseq_rows.  The
 * chromosome's ITEMS are those of tables.read_transcript_structure: item f is [feat_b0[f], feat_b1[f]) of transcript
 * feat_tx[f]; a transcript's items tile its span without overlap.  feat_kind[f] is 0 a 5'UTR exon part, 1 a 3'UTR exon part, 2
 * an exon of a transcript without CDS, 3 a coding intron (a CDS base on both sides), 4 any other gap, 5 a CDS part, which is
 * CDS segment feat_seg[f] (-1 for the other kinds).  For row i at q = start[i] and every item with feat_b0 <= q < feat_b1, its
 * classes c = 1 .. 3 go to one of 9 bins:
 *   kinds 0, 1, 2: bin 0 (utr5), 1 (utr3), 2 (noncoding_exon);
 *   kinds 3, 4: an item shorter than 4 bases has no splice sites (bin 6, intron); otherwise its 5' two bases in transcript
 *     orientation are the donor, the other end's two the acceptor: bin 3 (splice_donor) / 4 (splice_acceptor) in a coding
 *     intron, bin 5 (splice_utr) in any other, and bin 6 for the bases between;
 *   kind 5: x = the CDS offset of q, the codon and the amino acids as mural_summary_conseq_rows; class c goes to bin 7
 *     (start_lost) where x < 3, the codon resolves and aa_alt != aa_ref, to bin 8 (cds) otherwise.  BED12 carries no
 *     frame and ATG is not demanded: start lost is "changes the amino acid of CDS codon 0".
 *   table [n_transcripts][9][3] += { 1 where label[i] == c, hi of prob[i][c], lo of prob[i][c] }; on return lo < 2^40;
 *   rows [n_transcripts][2] += { rows inside the span, rows of label 0 among them }; a row counts once per transcript whose
 *   span covers it.  Bins 7 + 8 of a transcript add up to the five bins of mural_summary_conseq_rows.
 * A CDS item whose feat_seg is outside 0 .. n_segments - 1 or names another segment, an item of an unknown kind and an item
 * whose transcript is outside 0 .. n_transcripts - 1 are skipped.  Chunks of at most mural_summary_txstruct_chunk_rows()
 * rows, a scan workgroup of mural_summary_txstruct_scan_threads() threads, a grid of at most
 * mural_summary_txstruct_grid_waves() waves.  n <= 2^31 and n_features <= 2^22 per call (MURAL_E_INVALID above: a
 * transcript's items are disjoint, so a cell takes at most n / chunk_rows + n_features folded terms in a call, which keeps its
 * lo limb below 2^63 until the fold that ends the call).  ws: mural_summary_txstruct_workspace_bytes(n_features) bytes (24
 * per item), 8-byte aligned; MURAL_E_WORKSPACE when smaller.  n == 0 or n_features == 0 launches nothing; n_segments == 0
 * is legal (no CDS on the chromosome).  Launches on `stream`, no synchronisation, no read-back, no floating-point atomics.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
  const MuralGenome* genome; /* the chromosome of the rows */
  const void* prob;          /* dev [n][prob_stride], float (prob_f64 = 0) or double; columns 1 .. 3 are read                  */
  int32_t prob_f64, label_kind;                     /* label: 0 float32, 1 int32, 2 int64                                       */
  int64_t prob_stride;       /* elements */
  const int64_t* start;      /* dev [n], ascending */
  const uint8_t* strand;     /* dev [n], 1 = '-', or NULL */
  const void* label;         /* dev [n] */
  int64_t n;
  int32_t n_class, n_transcripts;                   /* n_class == 4 */
  const int64_t* seg_b0;     /* dev [n_segments] */
  const int64_t* seg_b1;     /* dev [n_segments] */
  const int64_t* seg_cds0;   /* dev [n_segments] */
  const int32_t* seg_tx;     /* dev [n_segments] */
  const int32_t* seg_prev;   /* dev [n_segments] */
  const int32_t* seg_next;   /* dev [n_segments] */
  int64_t n_segments;
  const uint8_t* tx_strand;  /* dev [n_transcripts] */
  const int64_t* tx_cds_len; /* dev [n_transcripts] */
  uint8_t aa[64];
  uint8_t alt_order[4][3];
  uint8_t reserved[4];
  uint64_t* table;           /* dev [n_transcripts][9][3] */
  uint64_t* rows;            /* dev [n_transcripts][2] */
  int32_t* status;           /* dev [1] */
  const int64_t* feat_b0;    /* dev [n_features] */
  const int64_t* feat_b1;    /* dev [n_features] */
  const int32_t* feat_tx;    /* dev [n_features] */
  const uint8_t* feat_kind;  /* dev [n_features] */
  const int32_t* feat_seg;   /* dev [n_features] */
  int64_t n_features;
} MuralSummaryTxstructRows;
int64_t mural_summary_txstruct_chunk_rows(void);
int64_t mural_summary_txstruct_grid_waves(void);
int32_t mural_summary_txstruct_scan_threads(void);
size_t mural_summary_txstruct_workspace_bytes(int64_t n_features);
int mural_summary_txstruct_rows(const MuralSummaryTxstructRows* s, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Expected and observed INDEL events per transcript by what they do to the transcript's structure
 * (SummarySink(indel_transcripts=...) in flight, tables.indel_structure_table from a written table;
 * csrc/summary_txindel.hip; mural_amd.summaries.summary_txindel_host is the specification).  One call takes the INDEL rows
 * (2 <= n_class <= 16) of a part of ONE chromosome, ascending in start (equal starts are legal); the limbs, the tables'
 * layout and the status bits are those of mural_summary_conseq_rows, bit 1 a label outside 0 .. n_class - 1.  Class 0's
 * probability, the rows' strand and the genome are never read: an INDEL event is a reference-strand fact.  The items, the
 * segments and the transcripts are those of mural_summary_txstruct_rows (seg_prev / seg_next are not needed); feat_prev /
 * feat_next [n_features] are the same transcript's neighbouring items in genomic order, -1 at the span's ends
 * (tables.structure_links).
 *   kind: 0 insertion, 1 deletion start, 2 deletion end -- of the whole call, as there is one model per kind.
 *   breakpoint_offset: 0 or 1; the event's boundary is j = start + breakpoint_offset, between 0-based bases j - 1 and j.
 *   class_len[c] = { lo, hi } for c >= 1, 1 <= lo <= hi <= 64 (MURAL_E_INVALID otherwise): the lengths class c stands for.
 *     A class is FRAMED when lo == hi, MIXED when its range holds a multiple of 3 and another length; any other range
 *     (1-2, 4-5) shifts the frame whatever its length.  A deletion of class c is located by its L = lo bases.
 *   The home base h is j - 1 for an insertion and a deletion end, j for a deletion start.  A row counts for every
 *   transcript whose span holds h (an insertion: and j), once, through the item that holds h.  The 10 bins: 0 utr5, 1 utr3,
 *   2 noncoding_exon, 3 splice, 4 splice_utr, 5 intron, 6 start_lost, 7 frameshift, 8 inframe, 9 cds_mixed.
 *   x(j) is the number of CDS bases 5' of boundary j in transcript orientation: seg_cds0 + (j - seg_b0) on '+', seg_cds0 +
 *   (seg_b1 - j) on '-'.  The FRAME BIN of class c with n CDS bases affected: 9 for a mixed class, 7 for a range that always
 *   shifts, and for a framed class 7 where n % 3 != 0, else 8.  The CDS RULE at boundary j: x == 0 gives bin 0, x ==
 *   tx_cds_len bin 1, x <= 2 bin 6 for every class, otherwise the frame bin with n = lo.
 *   Insertion, A the item of base j - 1 and B that of base j.  A == B: kinds 0, 1, 2 give bins 0, 1, 2; in a gap of 4 or more
 *   bases j == a + 1 or j == b - 1 splits a splice dinucleotide -- bin 3 in a coding intron (kind 3), bin 4 in any other gap
 *   (kind 4) --, every other gap position is bin 5; a CDS part follows the CDS rule.  A != B: a gap yields to an exon part
 *   (the inserted bases extend the exon); where one of the two is a CDS part it decides by the CDS rule (A first); two other
 *   exon parts have one kind.
 *   Deletion: the deleted bases are D = [j, j + L) (deletion start) or [j - L, j) (deletion end), clipped to the
 *   transcript's span and, where chrom_length >= 0, to [0, chrom_length) (the home base stays).  Over the items that meet D,
 *   reached from the home item over feat_next / feat_prev: n_cds = the CDS bases in D; touch_start = a CDS base of offset < 3
 *   is in D; touch_splice = one of the first two or last two bases of a coding intron of 4 or more bases is in D;
 *   touch_splice_utr = the same for a kind-4 gap.  The first that holds decides: touch_start bin 6; touch_splice bin 3; n_cds
 *   > 0 the frame bin with n = n_cds; touch_splice_utr bin 4; a kind-2 base bin 2; a kind-0 base bin 0; a kind-1 base bin 1;
 *   otherwise bin 5.  A link that is out of range, names another transcript, an item that is empty, of an unknown kind, a
 *   CDS part without its segment or that does not abut the item before it ends the walk (a home item of that sort is
 *   skipped, and so is an insertion whose B is one): nothing is read out of bounds and a walk has at most 64 steps.
 *   table [n_transcripts][10][3] += { 1 where label[i] == c, hi of prob[i][c], lo of prob[i][c] } per (row, c >= 1) routed to
 *     bin b; on return lo < 2^40;  rows [n_transcripts][2] += { rows counted, rows of label 0 among them }.  Both are a
 *     function of the SET of rows alone, bit for bit.
 * Chunks of at most mural_summary_txindel_chunk_rows() rows of one home item, a scan workgroup of
 * mural_summary_txindel_scan_threads() threads, a grid of at most mural_summary_txindel_grid_waves() waves.  n <= 2^31 and
 * n_features <= 2^22 per call (MURAL_E_INVALID above: a row adds at most n_class - 1 <= 15 limbs to a cell, a wave folds
 * its chunk's sum before it adds, and a cell takes at most n / chunk_rows + n_features folded terms in a call, which keeps
 * its lo limb below 2^63 until the fold that ends the call).  ws: mural_summary_txindel_workspace_bytes(n_features) bytes (24
 * per item), 8-byte aligned; MURAL_E_WORKSPACE when smaller.  n == 0 or n_features == 0 launches nothing.  Launches on
 * `stream`, no synchronisation, no read-back, no floating-point atomics.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
  const void* prob;          /* dev [n][prob_stride], float (prob_f64 = 0) or double; columns 1 .. n_class - 1 are read        */
  int32_t prob_f64, label_kind;                     /* label: 0 float32, 1 int32, 2 int64                                       */
  int64_t prob_stride;       /* elements */
  const int64_t* start;      /* dev [n], ascending */
  const void* label;         /* dev [n] */
  int64_t n;
  int32_t n_class, n_transcripts;
  int32_t kind, breakpoint_offset;
  int64_t chrom_length;      /* or -1: not known */
  int32_t class_len[16][2];  /* [c] = { lo, hi }, c >= 1 */
  const int64_t* seg_b0;     /* dev [n_segments] */
  const int64_t* seg_b1;     /* dev [n_segments] */
  const int64_t* seg_cds0;   /* dev [n_segments] */
  const int32_t* seg_tx;     /* dev [n_segments] */
  int64_t n_segments;
  const uint8_t* tx_strand;  /* dev [n_transcripts] */
  const int64_t* tx_cds_len; /* dev [n_transcripts] */
  uint64_t* table;           /* dev [n_transcripts][10][3] */
  uint64_t* rows;            /* dev [n_transcripts][2] */
  int32_t* status;           /* dev [1] */
  const int64_t* feat_b0;    /* dev [n_features] */
  const int64_t* feat_b1;    /* dev [n_features] */
  const int32_t* feat_tx;    /* dev [n_features] */
  const uint8_t* feat_kind;  /* dev [n_features] */
  const int32_t* feat_seg;   /* dev [n_features] */
  const int32_t* feat_prev;  /* dev [n_features] */
  const int32_t* feat_next;  /* dev [n_features] */
  int64_t n_features;
} MuralSummaryTxindelRows;
int64_t mural_summary_txindel_chunk_rows(void);
int64_t mural_summary_txindel_grid_waves(void);
int32_t mural_summary_txindel_scan_threads(void);
size_t mural_summary_txindel_workspace_bytes(int64_t n_features);
int mural_summary_txindel_rows(const MuralSummaryTxindelRows* s, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Mutation sets drawn from the rates of a shard while it is on the device (SummarySink(simulate=R, ...) in flight,
 * tables.simulate_table from a written table; csrc/simulate.hip).  The draw is stateless and integer
 * (mural_amd.summaries.simulate_rows_host is its specification): Philox4x32-10 with key (seed lo, seed hi) and counter
 * (start lo, start hi, chrom_key, (replicate >> 2) | (strand << 31)), replicate r reading output word r & 3 as u;
 * q_c = floor(double(p_c) * 2^32) (2^32 from p_c = 1 on) for c = 1 .. n_class - 1, cum_c = min(q_1 + .. + q_c, 2^32); the
 * class of the row is the smallest c >= 1 with u < cum_c, 0 where there is none (class 0's probability is never read).
 * A draw depends on (seed, chrom_key, start, strand, replicate) alone -- not on the row's index --, so every output is a
 * function of the SET of rows, bit for bit, for any split into calls; two rows with equal chrom_key, start and strand
 * draw the same value.  chrom_key: crc32 of the chromosome's name (the caller forms it).  strand: dev uint8 [n], non-zero
 * for '-', or NULL for all '+'.  status (device int32, bits as mural_summary_kmer_rows): bit 3 a probability of a class
 * >= 1 that is NaN, negative or infinite, bit 0 a negative start -- such rows draw class 0 in every replicate --, bit 2
 * (mural_simulate_annot_rows only) a start below the row before it inside the call.  2 <= n_class <= 8.
 *
 * mural_simulate_annot_rows: rows and pieces as mural_summary_annot_rows (one chromosome, start ascending; no label).
 *   table [n_groups][n_class - 1][n_rep] of unsigned 32-bit cells: cell [g][c - 1][r] += the rows inside the pieces of
 *   group g whose replicate-r draw is class c (a row counts once per group that covers it); zeroed by the caller once,
 *   it accumulates over calls, parts and chromosomes.  1 <= n_rep <= mural_simulate_max_replicates() = 2^20.
 *   A piece's rows are one range of start (two lower bounds); the ranges are cut into chunks of at most
 *   mural_simulate_chunk_rows() rows, listed by an exclusive scan of the chunk counts (one workgroup of
 *   mural_simulate_scan_threads() threads, a run of pieces each), and a grid of at most mural_simulate_grid_waves() waves
 *   strides over the (chunk, block of 64 replicates) units: a row per lane, four replicates per Philox call, hits counted
 *   by ballot and popcount, one 32-bit INTEGER atomic wave-instruction of 64 contiguous replicates per class and chunk.
 *   ws: mural_simulate_annot_workspace_bytes(n_pieces) bytes (24 per piece), 8-byte aligned; MURAL_E_WORKSPACE when
 *   smaller.  n == 0 launches nothing; n_pieces == 0 only checks the rows.
 * mural_simulate_rows: replicate `replicate` of the rows as a mutation list -- the rows whose draw is not 0, compacted
 *   in row order (stable): out_start / out_strand / out_label [n] hold *count entries (count: dev int64, SET, not added
 *   to).  ws: mural_simulate_rows_workspace_bytes(n) bytes (8 per 64 rows); MURAL_E_WORKSPACE when smaller.  n == 0
 *   launches nothing and leaves *count as it is.
 * Both launch on `stream`: no synchronisation, no read-back, no floating-point atomics; draws are recomputed, never
 * stored.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
  const void* prob;          /* dev [n][prob_stride], float (prob_f64 = 0) or double; columns 1 .. n_class-1 are read          */
  int32_t prob_f64, n_class;
  int64_t prob_stride;       /* elements */
  const int64_t* start;      /* dev [n], ascending */
  const uint8_t* strand;     /* dev [n] or NULL */
  int64_t n;
  uint32_t chrom_key;
  int32_t n_rep;
  uint64_t seed;
  const int64_t* piece_b0;   /* dev [n_pieces] */
  const int64_t* piece_b1;   /* dev [n_pieces] */
  const int32_t* piece_group; /* dev [n_pieces] */
  int64_t n_pieces;
  int32_t n_groups, reserved;
  uint32_t* table;           /* dev [n_groups][n_class - 1][n_rep] */
  int32_t* status;           /* dev [1] */
} MuralSimulateAnnotRows;
typedef struct {
  const void* prob;
  int32_t prob_f64, n_class;
  int64_t prob_stride;
  const int64_t* start;      /* dev [n] */
  const uint8_t* strand;     /* dev [n] or NULL */
  int64_t n;
  uint32_t chrom_key;
  int32_t replicate;
  uint64_t seed;
  int64_t* out_start;        /* dev [n] */
  uint8_t* out_strand;       /* dev [n] */
  uint8_t* out_label;        /* dev [n] */
  int64_t* count;            /* dev [1] */
  int32_t* status;           /* dev [1] */
} MuralSimulateRows;
int64_t mural_simulate_chunk_rows(void);
int64_t mural_simulate_grid_waves(void);
int32_t mural_simulate_scan_threads(void);
int32_t mural_simulate_max_replicates(void);
size_t mural_simulate_annot_workspace_bytes(int64_t n_pieces);
int mural_simulate_annot_rows(const MuralSimulateAnnotRows* s, void* ws, size_t ws_bytes, void* stream);
size_t mural_simulate_rows_workspace_bytes(int64_t n);
int mural_simulate_rows(const MuralSimulateRows* s, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The simulated null of the consequence table of a shard while it is on the device (SummarySink(simulate=R,
 * transcripts=..., simulate_transcripts=True) in flight, tables.simulate_consequence_table from a written table;
 * csrc/simulate_conseq.hip; mural_amd.summaries.simulate_conseq_host is the specification).  Rows as
 * mural_simulate_annot_rows (SNV rows, n_class == 4, of a part of ONE chromosome, ascending in start; no label is read),
 * genome, segments, transcripts, aa and alt_order as mural_summary_conseq_rows.
 *   table [n_transcripts][5][n_rep] of unsigned 32-bit cells: cell [t][b][r] += the rows inside the CDS of transcript t
 *   whose replicate-r draw (the draw of mural_simulate_annot_rows, unchanged) is a class c >= 1 whose substitution falls in
 *   bin b of t (the bin of mural_summary_conseq_rows: 0 syn, 1 mis, 2 stop gained, 3 stop lost, 4 unresolved).  A row
 *   counts once per transcript that covers it; class 0 counts nowhere.  Zeroed by the caller once, it accumulates over
 *   calls, parts and chromosomes, and is a function of the SET of rows and the seed alone, bit for bit.
 *   status: the simulation's bits -- bit 3 a probability of a class >= 1 that is NaN, negative or infinite, bit 0 a
 *   negative start (such rows draw class 0 in every replicate), bit 2 a start below the row before it inside the call;
 *   a probability of 1 or more is taken as 1.  A segment whose transcript is outside 0 .. n_transcripts - 1 is skipped.
 * MURAL_E_INVALID, before the first launch: n_class != 4, n_rep outside 1 .. 2^20, n > 2^31, n_segments > 2^22, an
 * alt_order row that does not name the three other bases once each.  The loop bounds are mural_simulate_chunk_rows(),
 * mural_simulate_grid_waves() and mural_simulate_scan_threads(): the grid strides over units of (chunk of a segment,
 * group of up to 16 blocks of 64 replicates); a row's bins are formed once per unit.
 * ws: mural_simulate_conseq_workspace_bytes(n_segments) bytes (24 per segment), 8-byte aligned; MURAL_E_WORKSPACE when
 * smaller.  n == 0 launches nothing; n_segments == 0 only checks the rows.  Launches on `stream`: no synchronisation, no
 * read-back, no floating-point atomics; draws and bins are recomputed, never stored.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
  const MuralGenome* genome; /* the chromosome of the rows */
  const void* prob;          /* dev [n][prob_stride], float (prob_f64 = 0) or double; columns 1 .. 3 are read                  */
  int32_t prob_f64, n_class; /* n_class == 4 */
  int64_t prob_stride;       /* elements */
  const int64_t* start;      /* dev [n], ascending */
  const uint8_t* strand;     /* dev [n], 1 = '-', or NULL */
  int64_t n;
  uint32_t chrom_key;
  int32_t n_rep;
  uint64_t seed;
  const int64_t* seg_b0;     /* dev [n_segments] */
  const int64_t* seg_b1;     /* dev [n_segments] */
  const int64_t* seg_cds0;   /* dev [n_segments] */
  const int32_t* seg_tx;     /* dev [n_segments] */
  const int32_t* seg_prev;   /* dev [n_segments] */
  const int32_t* seg_next;   /* dev [n_segments] */
  int64_t n_segments;
  const uint8_t* tx_strand;  /* dev [n_transcripts] */
  const int64_t* tx_cds_len; /* dev [n_transcripts] */
  int32_t n_transcripts, reserved;
  uint8_t aa[64];
  uint8_t alt_order[4][3];
  uint8_t reserved2[4];
  uint32_t* table;           /* dev [n_transcripts][5][n_rep] */
  int32_t* status;           /* dev [1] */
} MuralSimulateConseqRows;
size_t mural_simulate_conseq_workspace_bytes(int64_t n_segments);
int mural_simulate_conseq_rows(const MuralSimulateConseqRows* s, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The simulated null of the structure table of a shard while it is on the device (SummarySink(simulate=R,
 * transcripts=..., transcript_structure=True, simulate_transcripts=True, simulate_structure=True) in flight,
 * tables.simulate_structure_table from a written table; csrc/simulate_txstruct.hip;
 * mural_amd.summaries.simulate_txstruct_host is the specification).  Rows, chrom_key, n_rep, seed, genome, segments,
 * transcripts, aa and alt_order as mural_simulate_conseq_rows; the chromosome's items (feat_*) as
 * mural_summary_txstruct_rows.
 *   table [n_transcripts][9][n_rep] of unsigned 32-bit cells: cell [t][b][r] += the rows inside [chromStart, chromEnd) of
 *   transcript t whose replicate-r draw (the draw of mural_simulate_annot_rows, unchanged) is a class c >= 1 that falls in
 *   bin b of t (the bin of mural_summary_txstruct_rows: 0 utr5 .. 8 cds).  A row counts once per transcript whose span
 *   covers it; class 0 counts nowhere; no label is read.  Zeroed by the caller once, it accumulates over calls, parts and
 *   chromosomes, and is a function of the SET of rows and the seed alone, bit for bit.  Bins 7 + 8 of a transcript and
 *   replicate add up to the five bins of mural_simulate_conseq_rows at the same chrom_key and seed.
 *   status: the simulation's bits -- bit 3 a probability of a class >= 1 that is NaN, negative or infinite, bit 0 a
 *   negative start (such rows draw class 0 in every replicate), bit 2 a start below the row before it inside the call;
 *   a probability of 1 or more is taken as 1.  A CDS item whose feat_seg is outside 0 .. n_segments - 1 or names another
 *   segment, an item of an unknown kind and an item whose transcript is outside 0 .. n_transcripts - 1 are skipped.
 * MURAL_E_INVALID, before the first launch: n_class != 4, n_rep outside 1 .. 2^20, n > 2^31, n_features > 2^22,
 * n_segments > 2^22, an alt_order row that does not name the three other bases once each.  The loop bounds are
 * mural_simulate_chunk_rows(), mural_simulate_grid_waves() and mural_simulate_scan_threads(): the grid strides over units
 * of (chunk of an item, group of up to 16 blocks of 64 replicates); a row's three slots are formed once per unit.
 * ws: mural_simulate_txstruct_workspace_bytes(n_features) bytes (24 per item), 8-byte aligned; MURAL_E_WORKSPACE when
 * smaller.  n == 0 launches nothing; n_features == 0 only checks the rows; n_segments == 0 is legal (no CDS on the
 * chromosome).  Launches on `stream`: no synchronisation, no read-back, no floating-point atomics; draws and bins are
 * recomputed, never stored.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
  const MuralGenome* genome; /* the chromosome of the rows */
  const void* prob;          /* dev [n][prob_stride], float (prob_f64 = 0) or double; columns 1 .. 3 are read                  */
  int32_t prob_f64, n_class; /* n_class == 4 */
  int64_t prob_stride;       /* elements */
  const int64_t* start;      /* dev [n], ascending */
  const uint8_t* strand;     /* dev [n], 1 = '-', or NULL */
  int64_t n;
  uint32_t chrom_key;
  int32_t n_rep;
  uint64_t seed;
  const int64_t* seg_b0;     /* dev [n_segments] */
  const int64_t* seg_b1;     /* dev [n_segments] */
  const int64_t* seg_cds0;   /* dev [n_segments] */
  const int32_t* seg_tx;     /* dev [n_segments] */
  const int32_t* seg_prev;   /* dev [n_segments] */
  const int32_t* seg_next;   /* dev [n_segments] */
  int64_t n_segments;
  const uint8_t* tx_strand;  /* dev [n_transcripts] */
  const int64_t* tx_cds_len; /* dev [n_transcripts] */
  int32_t n_transcripts, reserved;
  uint8_t aa[64];
  uint8_t alt_order[4][3];
  uint8_t reserved2[4];
  uint32_t* table;           /* dev [n_transcripts][9][n_rep] */
  int32_t* status;           /* dev [1] */
  const int64_t* feat_b0;    /* dev [n_features] */
  const int64_t* feat_b1;    /* dev [n_features] */
  const int32_t* feat_tx;    /* dev [n_features] */
  const uint8_t* feat_kind;  /* dev [n_features] */
  const int32_t* feat_seg;   /* dev [n_features] */
  int64_t n_features;
} MuralSimulateTxstructRows;
size_t mural_simulate_txstruct_workspace_bytes(int64_t n_features);
int mural_simulate_txstruct_rows(const MuralSimulateTxstructRows* s, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The simulated null of the INDEL structure table of a shard while it is on the device (SummarySink(simulate=R,
 * indel_transcripts=..., indel_kind=..., simulate_indel_structure=True) in flight,
 * tables.simulate_indel_structure_table from a written table; csrc/simulate_txindel.hip;
 * mural_amd.summaries.simulate_txindel_host is the specification).  Rows, strand, chrom_key, n_rep and seed as
 * mural_simulate_annot_rows, 2 <= n_class <= 8 (the bound of the simulation's draw); kind, breakpoint_offset,
 * chrom_length, class_len, the items with their links, the segments and the transcripts as mural_summary_txindel_rows.
 *   DRAW.  That of mural_simulate_annot_rows, unchanged: Philox4x32-10 with key (seed lo, seed hi) and counter (start lo,
 *   start hi, chrom_key, (replicate >> 2) | strand << 31), replicate r reading word r & 3 as u; q_c = floor(p_c 2^32) with
 *   p_c >= 1 taken as 1, cum_c = min(q_1 + .. + q_c, 2^32); the class is the smallest c >= 1 with u < cum_c, 0 where there is
 *   none.  A row with a NaN, negative or infinite p_c (status bit 3) or a negative start (bit 0) draws class 0 in every
 *   replicate; a start below the row before it inside the call sets bit 2.  Two rows of equal chromosome, start and strand
 *   draw the same value.
 *   BIN.  That of mural_summary_txindel_rows, unchanged (txindel_bins.h): the home base h = start + breakpoint_offset - 1
 *   for an insertion and a deletion end, start + breakpoint_offset for a deletion start; a row counts for every transcript
 *   whose span holds h (an insertion: and base j = start + breakpoint_offset), once, through the item that holds h; the bin
 *   of class c is the insertion's site or frame bin, or what the L = lo(c) deleted bases meet on the walk over feat_next /
 *   feat_prev, clipped to the span and to chrom_length.  Broken links end a walk; a home item that is empty, of an unknown
 *   kind or a CDS part without its segment is skipped, and so is an insertion whose second item is one.
 *   table [n_transcripts][10][n_rep] of unsigned 32-bit cells: cell [t][b][r] += the rows that transcript t counts whose
 *   replicate-r draw is a class c >= 1 with bin(row, t, c) == b.  Class 0 counts nowhere; no label is read.  Zeroed by the
 *   caller once, it accumulates over calls, parts and chromosomes, and is a function of the SET of rows and the seed alone,
 *   bit for bit.  A cell takes at most one count per row per call: with n <= 2^31 it cannot wrap in a call; across calls
 *   the caller keeps the rows a transcript counts below 2^32.
 * MURAL_E_INVALID, before the first launch: n_class outside 2 .. 8, n_rep outside 1 .. 2^20, n > 2^31, n_features > 2^22,
 * n_segments > 2^22, kind outside 0 .. 2, breakpoint_offset outside 0 .. 1, a class_len pair outside 1 <= lo <= hi <= 64.
 * The loop bounds are mural_simulate_chunk_rows(), mural_simulate_grid_waves() and mural_simulate_scan_threads(): the grid
 * strides over units of (chunk of a home item, group of up to 16 blocks of 64 replicates); a row's bins are formed once per
 * unit.  ws: mural_simulate_txindel_workspace_bytes(n_features) bytes (24 per item), 8-byte aligned; MURAL_E_WORKSPACE when
 * smaller.  n == 0 launches nothing; n_features == 0 only checks the rows; n_segments == 0 is legal.  Launches on `stream`:
 * no synchronisation, no read-back, no floating-point atomics; draws and bins are recomputed, never stored.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
  const void* prob;          /* dev [n][prob_stride], float (prob_f64 = 0) or double; columns 1 .. n_class - 1 are read        */
  int32_t prob_f64, n_class; /* 2 <= n_class <= 8 */
  int64_t prob_stride;       /* elements */
  const int64_t* start;      /* dev [n], ascending */
  const uint8_t* strand;     /* dev [n], 1 = '-', or NULL */
  int64_t n;
  uint32_t chrom_key;
  int32_t n_rep;
  uint64_t seed;
  int32_t kind, breakpoint_offset;
  int64_t chrom_length;      /* or -1: not known */
  int32_t class_len[16][2];  /* [c] = { lo, hi }, c >= 1 */
  const int64_t* seg_b0;     /* dev [n_segments] */
  const int64_t* seg_b1;     /* dev [n_segments] */
  const int64_t* seg_cds0;   /* dev [n_segments] */
  const int32_t* seg_tx;     /* dev [n_segments] */
  int64_t n_segments;
  const uint8_t* tx_strand;  /* dev [n_transcripts] */
  const int64_t* tx_cds_len; /* dev [n_transcripts] */
  int32_t n_transcripts, reserved;
  uint32_t* table;           /* dev [n_transcripts][10][n_rep] */
  int32_t* status;           /* dev [1] */
  const int64_t* feat_b0;    /* dev [n_features] */
  const int64_t* feat_b1;    /* dev [n_features] */
  const int32_t* feat_tx;    /* dev [n_features] */
  const uint8_t* feat_kind;  /* dev [n_features] */
  const int32_t* feat_seg;   /* dev [n_features] */
  const int32_t* feat_prev;  /* dev [n_features] */
  const int32_t* feat_next;  /* dev [n_features] */
  int64_t n_features;
} MuralSimulateTxindelRows;
size_t mural_simulate_txindel_workspace_bytes(int64_t n_features);
int mural_simulate_txindel_rows(const MuralSimulateTxindelRows* s, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Training-mode ops of the INDEL U-Net (MuRaL/model/model_indel.py:6-19, :151-176 under model.train()): a general
 * Conv1d (stride, zero padding, input upsampled by `up` = nn.Upsample(scale_factor) in front of the conv) with its
 * backward, and the element-wise activations.  x [B][Cin][Lin], W [Cout][Cin][K] (torch layout), y [B][Cout][Lout].
 * ------------------------------------------------------------------------------------------------------------- */
int mural_op_convg_out_length(int32_t Lin, int32_t K, int32_t stride, int32_t pad, int32_t up);   /* -1: bad geometry */
/* wt: scratch of Cout*Cin*K floats */
int mural_op_convg_fwd(const float* x, const float* W, const float* bias, float* wt, float* y, int64_t B, int32_t Cin,
                       int32_t Lin, int32_t Cout, int32_t K, int32_t stride, int32_t pad, int32_t up, void* stream);
size_t mural_op_convg_bwd_scratch(int32_t Cin, int32_t Cout, int32_t K);                          /* floats */
/* dx (optional), dW and db (optional) are fully written */
int mural_op_convg_bwd(const float* dy, const float* x, const float* W, int64_t B, int32_t Cin, int32_t Lin, int32_t Cout,
                       int32_t K, int32_t stride, int32_t pad, int32_t up, float* dx, float* dW, float* db, float* part,
                       size_t part_floats, void* stream);
/* The U-Net's unit in one call per direction: z = act(BatchNorm1d(Conv1d(upsample_up(x)))) [+ res1] [+ res2] in training mode
 * (reference MuRaL/model/model_indel.py:6-19, :117-123 under model.train(): nn.Conv1d -> nn.BatchNorm1d [-> nn.SiLU / nn.ReLU] and the
 * residual adds around them).  act: 0 none, 1 ReLU, 2 SiLU, 3 Softplus.  y0 [B][Cout][Lout] receives the conv output and state
 * [4][Cout] = scale | shift | mean | invstd (both saved for the backward); acc: zeroed [MURAL_BN_SLOTS][2][Cout] doubles; running
 * statistics updated in place like nn.BatchNorm1d (momentum, unbiased variance).  The backward takes dz (the residuals' gradients are
 * dz itself), a fresh zeroed acc, a scratch dy0 [B][Cout][Lout] and the part scratch of mural_op_convg_bwd. */
int mural_op_convg_bn_fwd(const float* x, const float* W, const float* bias, float* wt, float* y0, int64_t B, int32_t Cin,
                          int32_t Lin, int32_t Cout, int32_t K, int32_t stride, int32_t pad, int32_t up, const float* gamma,
                          const float* beta, float eps, float momentum, float* running_mean, float* running_var, double* acc,
                          float* state, int32_t act, const float* res1, const float* res2, float* z, void* stream);
int mural_op_convg_bn_bwd(const float* dz, const float* x, const float* W, const float* y0, const float* state, const float* gamma,
                          int64_t B, int32_t Cin, int32_t Lin, int32_t Cout, int32_t K, int32_t stride, int32_t pad, int32_t up,
                          int32_t act, double* acc, float* dy0, float* dx, float* dW, float* db, float* dgamma, float* dbeta,
                          float* part, size_t part_floats, const float* wt_dgrad, void* stream);
/* The weight layouts the conv kernels read -- forward [Cin][K][Cout], input gradient [Cout][K flipped][Cin] (stride-1 layers) -- for
 * every conv of a model in ONE launch per training step.  jobs: DEVICE array sorted by start (running sum of Cout * Cin * K).
 * mural_op_convg_fwd / _bn_fwd take W == NULL when wt already holds the forward layout; mural_op_convg_bn_bwd takes the prepared
 * input-gradient layout as wt_dgrad (NULL: derived from W inside the call). */
typedef struct MuralRelayoutJob {
  const float* W;        /* [Cout][Cin][K] (torch layout) */
  float* wt_fwd;         /* [Cin][K][Cout] */
  float* wt_dgrad;       /* [Cout][K][Cin], taps flipped; NULL: not needed */
  int32_t Cout, Cin, K, reserved;
  int64_t start;
} MuralRelayoutJob;
int mural_op_relayout_multi(const MuralRelayoutJob* jobs, int32_t n_jobs, int64_t total, void* stream);
/* The INDEL training step as one call per direction (reference: UNet_Small.forward under model.train(),
 * MuRaL/model/model_indel.py:151-176, inside the step of MuRaL/training.py:424-436).  params / grads: DEVICE pointers in the
 * state_dict naming (MuralIndelParams); the forward updates the BatchNorms' running statistics in place (the strand-symmetrising
 * layer's twice, in the reference's order) and leaves everything the backward needs in the workspace; the backward writes every
 * parameter gradient (fully, no accumulation).  x: dev float [B][4][length]; out / dout: dev float [B][n_class].  dropout_p, seed,
 * seed_dev: out_fc's Dropout (see mural_op_dropout).  mural_indel_train_workspace_bytes: 0 on a bad shape.                      */
size_t mural_indel_train_workspace_bytes(const MuralIndelShape* shape, int64_t B);
int mural_indel_train_forward(const MuralIndelShape* shape, const MuralIndelParams* params, const float* x, int64_t B,
                              float dropout_p, uint64_t seed, const uint64_t* seed_dev, float momentum, float* out,
                              void* workspace, size_t workspace_bytes, void* stream);
int mural_indel_train_backward(const MuralIndelShape* shape, const MuralIndelParams* params, const MuralIndelParams* grads,
                               const float* x, const float* dout, int64_t B, float dropout_p, uint64_t seed,
                               const uint64_t* seed_dev, void* workspace, size_t workspace_bytes, void* stream);
/* The same step from SYMBOL WINDOWS: symbols = dev uint8 [B][length], one MURAL_SYM_* code per window column (what
 * mural_train_batch_encode / mural_encode_symbols / mural_op_dense_to_symbols write; a byte above 14 counts as N, the bytes are not
 * checked otherwise).  Same semantics as the dense pair -- running statistics (the strand-symmetrising BatchNorm's twice), every
 * gradient fully written -- but the unit that consumes the window (the strand-symmetrising conv with use_reverse, up_l[0] otherwise)
 * is evaluated per symbol (mural_op_indel_first_fwd / _bwd): neither the dense window nor its flipped copy exists, and the workspace is
 * smaller by at least that copy (B * 4 * length floats) with use_reverse.  The backward takes the forward's symbols and workspace. */
size_t mural_indel_train_symbols_workspace_bytes(const MuralIndelShape* shape, int64_t B);
int mural_indel_train_forward_symbols(const MuralIndelShape* shape, const MuralIndelParams* params, const uint8_t* symbols, int64_t B,
                                      float dropout_p, uint64_t seed, const uint64_t* seed_dev, float momentum, float* out,
                                      void* workspace, size_t workspace_bytes, void* stream);
int mural_indel_train_backward_symbols(const MuralIndelShape* shape, const MuralIndelParams* params, const MuralIndelParams* grads,
                                       const uint8_t* symbols, const float* dout, int64_t B, float dropout_p, uint64_t seed,
                                       const uint64_t* seed_dev, void* workspace, size_t workspace_bytes, void* stream);
/* The conv of that unit alone, Conv1d(4 -> Cout, K, stride, pad) over the one-hot / IUPAC-fraction columns of the symbols (sym: dev uint8
 * [B][L]; Cout a multiple of 4, K <= 63; W [Cout][4][K], bias [Cout] or NULL).  y [B][Cout][Lout], Lout = (L + 2 pad - K) / stride + 1.
 * y_rev (optional; needs stride 1, pad (K - 1) / 2): the same conv of the channel- and length-flipped window, from the same bytes.
 * Backward: dW [Cout][4][K] and db [Cout] (optional) = the weight gradient of dz, plus that of dz_rev (optional) through the flipped
 * window; fully written, summed in a fixed order.  part: scratch of mural_op_indel_first_scratch floats (rev: dz_rev will be given). */
size_t mural_op_indel_first_scratch(int64_t B, int32_t L, int32_t Cout, int32_t K, int32_t stride, int32_t pad, int32_t rev);
int mural_op_indel_first_fwd(const uint8_t* sym, const float* W, const float* bias, int64_t B, int32_t L, int32_t Cout, int32_t K,
                             int32_t stride, int32_t pad, float* y, float* y_rev, void* stream);
int mural_op_indel_first_bwd(const uint8_t* sym, const float* dz, const float* dz_rev, int64_t B, int32_t L, int32_t Cout, int32_t K,
                             int32_t stride, int32_t pad, float* dW, float* db, float* part, size_t part_floats, void* stream);
/* symbols -> the dense columns they stand for: x [n][4][L] float (the inverse of mural_op_dense_to_symbols; a byte above 14 gives N) */
int mural_op_symbols_to_dense(const uint8_t* sym, int64_t n, int32_t L, float* x, void* stream);
/* kind: 1 ReLU, 2 SiLU, 3 Softplus (beta 1, threshold 20); backward takes the forward INPUT x */
int mural_op_act_fwd(const float* x, int64_t n, int32_t kind, float* y, void* stream);
int mural_op_act_bwd(const float* dy, const float* x, int64_t n, int32_t kind, float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MURAL_HIP_H */
