// The prediction table read back on the device: a streaming reader and the kernels of the four file-level tools built on it
// (mural_amd/tables.py).  Counterparts in the reference, which parse the table row by row in Python or load it whole in pandas:
//   the per-line loops of MuRaL/scripts/calc_kmer_corr.py:200-270 and calc_regional_corr.py:168-212
//   pd.read_csv / sum / to_csv of MuRaL/scripts/scaling.py:10-28, :45-107 (and pybedtools' intersect for the benchmark regions)
//
// The table is never held whole.  The host cuts the text into chunks after a newline (plain files are read, gzip files inflated as a
// stream, every member of a multi-member file), fills a ring of two pinned buffers on a worker thread -- reading / inflating chunk i+1
// overlaps with the device work on chunk i -- and copies each chunk to the device asynchronously.  Per chunk on the device:
//   (a) newline flags -> per-block counts -> one-block prefix sum -> row end offsets,
//   (b) one thread per row parses start / end / mut_type as integers, strand as 0/1 and prob0.. as float64,
//   (c) a row whose chrom bytes differ from the previous row's starts a chromosome run; the host names the runs from their first rows.
// Floats: the exact fast path (decimal mantissa <= 2^53, |power of ten| <= 22 -> one correctly rounded multiply or divide by an exact
// power of ten) gives what float() / pandas give; every other field is listed and re-parsed on the host with strtod.
#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <future>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "kmer_key.h"

namespace mural {
namespace {

constexpr int TB_THREADS = 256;
constexpr int TB_BYTES_PER_THREAD = 16;
constexpr int TB_TILE = TB_THREADS * TB_BYTES_PER_THREAD;
constexpr int64_t TB_MAX_ROW = 64 * 1024;      // a row may run this far past the chunk's target size

// error codes of the per-chunk status word: key = (row << 8) | (field << 3) | code, the smallest key wins
enum : int { ST_NUMBER = 1, ST_FIELDS = 2, ST_STRAND = 3, ST_EMPTY = 4 };

__constant__ double c_p10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

struct ChunkMeta {
  int64_t n_rows;
  unsigned long long status;
  unsigned long long n_slow;
  unsigned long long n_runs;
};

static_assert(TB_THREADS == SCAN_THREADS, "block_excl_scan (common.h) is written for 256-thread blocks");

__device__ __forceinline__ int count_newlines(const char* __restrict__ buf, int64_t len, int64_t p0) {
  int c = 0;
#pragma unroll
  for (int j = 0; j < TB_BYTES_PER_THREAD; ++j) c += (p0 + j < len && buf[p0 + j] == '\n') ? 1 : 0;
  return c;
}

__global__ __launch_bounds__(TB_THREADS) void nl_count_kernel(const char* __restrict__ buf, int64_t len, int32_t* __restrict__ block_cnt) {
  const int64_t p0 = (int64_t)blockIdx.x * TB_TILE + (int64_t)threadIdx.x * TB_BYTES_PER_THREAD;
  int total = 0;
  block_excl_scan(count_newlines(buf, len, p0), &total);
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = total;
}

// one block: block_off[b] = rows before tile b, meta->n_rows = all rows
__global__ __launch_bounds__(TB_THREADS) void nl_scan_kernel(const int32_t* __restrict__ block_cnt, int64_t nb,
                                                             int64_t* __restrict__ block_off, ChunkMeta* __restrict__ meta) {
  const int64_t rows = run_excl_scan<TB_THREADS, int64_t>(nb, [&](int64_t b) { return (int64_t)block_cnt[b]; },
                                                          [&](int64_t b, int64_t x) { block_off[b] = x; });
  if (threadIdx.x == 0) meta->n_rows = rows;
}

__global__ __launch_bounds__(TB_THREADS) void nl_emit_kernel(const char* __restrict__ buf, int64_t len,
                                                             const int64_t* __restrict__ block_off, int64_t rows_cap,
                                                             int32_t* __restrict__ row_end) {
  const int64_t p0 = (int64_t)blockIdx.x * TB_TILE + (int64_t)threadIdx.x * TB_BYTES_PER_THREAD;
  int total = 0;
  int64_t idx = block_off[blockIdx.x] + block_excl_scan(count_newlines(buf, len, p0), &total);
  for (int j = 0; j < TB_BYTES_PER_THREAD; ++j)
    if (p0 + j < len && buf[p0 + j] == '\n') {
      if (idx < rows_cap) row_end[idx] = (int32_t)(p0 + j);
      ++idx;
    }
}

// field [p, e) as a decimal integer (optional sign, 1..18 digits)
__device__ __forceinline__ bool parse_int(const char* p, const char* e, int64_t* out) {
  bool neg = false;
  if (p < e && (*p == '-' || *p == '+')) neg = *p++ == '-';
  if (p == e || e - p > 18) return false;
  int64_t v = 0;
  for (; p < e; ++p) {
    const unsigned d = (unsigned)(*p - '0');
    if (d > 9) return false;
    v = v * 10 + d;
  }
  *out = neg ? -v : v;
  return true;
}

// 0 = parsed exactly, 1 = valid decimal outside the exact fast path (the host re-parses it), 2 = malformed
__device__ __forceinline__ int parse_f64(const char* p, const char* e, double* out) {
  bool neg = false;
  if (p < e && (*p == '-' || *p == '+')) neg = *p++ == '-';
  uint64_t m = 0;
  int nd = 0, exp10 = 0;
  bool any = false, dot = false, slow = false;
  for (; p < e; ++p) {
    const char ch = *p;
    if (ch == '.') {
      if (dot) return 2;
      dot = true;
      continue;
    }
    const unsigned d = (unsigned)(ch - '0');
    if (d > 9) break;
    any = true;
    if (m == 0 && d == 0) {
      if (dot) --exp10;
    } else if (nd < 19) {
      m = m * 10 + d;
      ++nd;
      if (dot) --exp10;
    } else {
      slow = true;
    }
  }
  if (!any) return 2;
  if (p < e) {
    if (*p != 'e' && *p != 'E') return 2;
    ++p;
    bool eneg = false;
    if (p < e && (*p == '-' || *p == '+')) eneg = *p++ == '-';
    if (p == e) return 2;
    int x = 0;
    for (; p < e; ++p) {
      const unsigned d = (unsigned)(*p - '0');
      if (d > 9) return 2;
      if (x < 100000) x = x * 10 + (int)d;
    }
    exp10 += eneg ? -x : x;
  }
  if (m == 0) {
    *out = neg ? -0.0 : 0.0;
    return 0;
  }
  if (slow || m > (1ull << 53) || exp10 < -22 || exp10 > 22) return 1;
  const double v = exp10 >= 0 ? (double)m * c_p10[exp10] : (double)m / c_p10[-exp10];
  *out = neg ? -v : v;
  return 0;
}

__device__ __forceinline__ const char* next_tab(const char* p, const char* e) {
  while (p < e && *p != '\t') ++p;
  return p;
}

__device__ __forceinline__ void report(ChunkMeta* meta, int64_t row, int field, int code) {
  atomicMin(&meta->status, ((unsigned long long)row << 8) | ((unsigned long long)field << 3) | (unsigned long long)code);
}

__global__ __launch_bounds__(TB_THREADS) void parse_rows_kernel(const char* __restrict__ buf, const int32_t* __restrict__ row_end,
                                                                ChunkMeta* __restrict__ meta, int64_t rows_cap, int nc,
                                                                int64_t* __restrict__ start, int64_t* __restrict__ end,
                                                                int32_t* __restrict__ mut, float* __restrict__ label,
                                                                uint8_t* __restrict__ strand, double* __restrict__ prob,
                                                                uint64_t* __restrict__ slow, uint64_t slow_cap,
                                                                uint64_t* __restrict__ runs) {
  const int64_t n = min(meta->n_rows, rows_cap);
  const int64_t i = (int64_t)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t b = i == 0 ? 0 : (int64_t)row_end[i - 1] + 1;
  const char* p = buf + b;
  const char* e = buf + row_end[i];
  double* pr = prob + i * nc;
  if (p == e) {
    report(meta, i, 0, ST_EMPTY);
    return;
  }
  // chrom: a run starts where the bytes differ from the previous row's
  const char* t = next_tab(p, e);
  bool first = i == 0;
  if (!first) {
    const char* q = buf + (i == 1 ? 0 : (int64_t)row_end[i - 2] + 1);
    const char* qe = buf + row_end[i - 1];
    const int64_t len = t - p;
    first = (qe - q) <= len || q[len] != '\t';
    for (int64_t k = 0; !first && k < len; ++k) first = q[k] != p[k];
  }
  if (first) {
    const unsigned long long r = atomicAdd(&meta->n_runs, 1ull);
    if (r < (unsigned long long)rows_cap) runs[r] = ((uint64_t)i << 32) | (uint64_t)b;
  }
  int64_t iv[3];
  for (int f = 1; f < 5; ++f) {
    if (t == e) {
      report(meta, i, f, ST_FIELDS);
      return;
    }
    p = t + 1;
    t = next_tab(p, e);
    if (f == 3) {
      if (t - p != 1 || (*p != '+' && *p != '-')) {
        report(meta, i, f, ST_STRAND);
        return;
      }
      strand[i] = *p == '-' ? 1 : 0;
    } else if (!parse_int(p, t, &iv[f == 4 ? 2 : f - 1])) {
      report(meta, i, f, ST_NUMBER);
      return;
    }
  }
  start[i] = iv[0];
  end[i] = iv[1];
  mut[i] = (int32_t)iv[2];
  label[i] = (float)iv[2];
  for (int c = 0; c < nc; ++c) {
    if (t == e) {
      report(meta, i, 5 + c, ST_FIELDS);
      return;
    }
    p = t + 1;
    t = next_tab(p, e);
    double v = 0.0;
    const int rc = parse_f64(p, t, &v);
    if (rc == 2) {
      report(meta, i, 5 + c, ST_NUMBER);
      return;
    }
    if (rc == 1) {
      const unsigned long long s = atomicAdd(&meta->n_slow, 1ull);
      if (s < slow_cap) slow[s] = ((uint64_t)(i * nc + c) << 32) | (uint64_t)(p - buf);
    }
    pr[c] = v;
  }
  if (t != e) report(meta, i, 5 + nc, ST_FIELDS);
}

// chrom_id[i] = run_chrom[the run holding row i]; run_row ascending, run_row[0] = 0
__global__ __launch_bounds__(TB_THREADS) void chrom_fill_kernel(const int64_t* __restrict__ run_row, const int32_t* __restrict__ run_chrom,
                                                                int32_t n_runs, int64_t n, int32_t* __restrict__ chrom_id) {
  const int64_t i = (int64_t)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = n_runs;      // last run with run_row <= i
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (run_row[mid] <= i) lo = mid; else hi = mid;
  }
  chrom_id[i] = run_chrom[lo];
}

__global__ __launch_bounds__(TB_THREADS) void scatter_f64_kernel(const int64_t* __restrict__ idx, const double* __restrict__ val, int64_t n,
                                                                 double* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i < n) dst[idx[i]] = val[i];
}

// scaling.py:24-27: prob[1:] *= f, prob0 = 1 - sum(prob[1:]) summed left to right in float64
__global__ __launch_bounds__(TB_THREADS) void scale_rows_kernel(double* __restrict__ prob, int64_t n, int nc, double f) {
  const int64_t i = (int64_t)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i >= n) return;
  double* r = prob + i * nc;
  double s = 0.0;
  for (int c = 1; c < nc; ++c) {
    const double v = r[c] * f;
    r[c] = v;
    s += v;
  }
  r[0] = 1.0 - s;
}

constexpr int PS_BLOCKS = 512;

// per-block partial of sum_rows w_i * sum_{c >= 1} prob[i][c] and sum_rows w_i in a fixed order (grid-stride rows per thread, a fixed
// tree per block): the result depends on n only.  w_i = 1, or with regions the number of regions of the row's chromosome that overlap
// [start, end): #(b0 < end) - #(b1 <= start) over the sorted region starts / ends (bedtools intersect without -u).
__global__ __launch_bounds__(TB_THREADS) void prob_sum_kernel(const double* __restrict__ prob, const int32_t* __restrict__ chrom_id,
                                                              const int64_t* __restrict__ start, const int64_t* __restrict__ end,
                                                              int64_t n, int nc, const int64_t* __restrict__ reg_off,
                                                              const int64_t* __restrict__ reg_b0, const int64_t* __restrict__ reg_b1,
                                                              int32_t n_reg_chrom, double* __restrict__ part_sum,
                                                              int64_t* __restrict__ part_cnt) {
  double s = 0.0;
  int64_t cnt = 0;
  for (int64_t i = (int64_t)blockIdx.x * TB_THREADS + threadIdx.x; i < n; i += (int64_t)PS_BLOCKS * TB_THREADS) {
    int64_t w = 1;
    if (reg_off) {
      const int32_t c = chrom_id[i];
      w = 0;
      if (c >= 0 && c < n_reg_chrom) {
        const int64_t lo = reg_off[c], hi = reg_off[c + 1];
        int64_t a = lo, z = hi;      // #(b0 < end)
        const int64_t e = end[i], st = start[i];
        while (a < z) {
          const int64_t m = (a + z) >> 1;
          if (reg_b0[m] < e) a = m + 1; else z = m;
        }
        const int64_t n_before_end = a - lo;
        a = lo, z = hi;              // #(b1 <= start)
        while (a < z) {
          const int64_t m = (a + z) >> 1;
          if (reg_b1[m] <= st) a = m + 1; else z = m;
        }
        w = n_before_end - (a - lo);
      }
    }
    if (w > 0) {
      double r = 0.0;
      for (int c = 1; c < nc; ++c) r += prob[i * nc + c];
      s += (double)w * r;
      cnt += w;
    }
  }
  __shared__ double ls[TB_THREADS];
  __shared__ int64_t lc[TB_THREADS];
  ls[threadIdx.x] = s;
  lc[threadIdx.x] = cnt;
  __syncthreads();
  for (int off = TB_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      ls[threadIdx.x] += ls[threadIdx.x + off];
      lc[threadIdx.x] += lc[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part_sum[blockIdx.x] = ls[0];
    part_cnt[blockIdx.x] = lc[0];
  }
}

// k-mer of each row (get_expanded_region, MuRaL/data/preprocessing.py:524-567, and the slice of calc_kmer_corr.py:246-251 with
// Python's slice semantics): key = base-4 number of the k bases (A0 C1 G2 T3), of their reverse complement on '-'; -1 when the slice
// is not k bases long or holds a base other than A/C/G/T (either case).  mode 0: the row's strand; 1 '+'; 2 '-'; 3 both (key_fwd and
// key_rev).
__global__ __launch_bounds__(TB_THREADS) void kmer_keys_kernel(MuralGenome g, const int64_t* __restrict__ start, const int64_t* __restrict__ end,
                                                               const uint8_t* __restrict__ strand, int64_t n, int k, int indel, int mode,
                                                               int32_t* __restrict__ key_a, int32_t* __restrict__ key_b) {
  const int64_t i = (int64_t)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i >= n) return;
  int32_t fwd, rev;
  kmer_key_decode(g, start[i], end[i], k, indel, fwd, rev);
  if (mode == 3) {
    key_a[i] = fwd;
    key_b[i] = rev;
  } else {
    key_a[i] = kmer_key_minus(mode, strand, i) ? rev : fwd;
  }
}

// first[key] = min over the rows with that key of 2 * (row0 + i) + sub: the reference's dict insertion order
__global__ __launch_bounds__(TB_THREADS) void first_row_kernel(const int32_t* __restrict__ keys, int64_t n, int64_t row0, int sub,
                                                               int32_t n_groups, unsigned long long* __restrict__ first) {
  const int64_t i = (int64_t)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i >= n) return;
  const int32_t key = keys[i];
  if (key >= 0 && key < n_groups) atomicMin(&first[key], (unsigned long long)(2 * (row0 + i) + sub));
}

// per-chromosome min / max of start (the window range a chunk's rows touch)
__global__ __launch_bounds__(TB_THREADS) void start_range_kernel(const int32_t* __restrict__ chrom_id, const int64_t* __restrict__ start,
                                                                 int64_t n, int32_t n_chrom, long long* __restrict__ mn,
                                                                 long long* __restrict__ mx) {
  const int64_t i = (int64_t)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i >= n) return;
  const int32_t c = chrom_id[i];
  if (c < 0 || c >= n_chrom) return;
  atomicMin(&mn[c], (long long)start[i]);
  atomicMax(&mx[c], (long long)start[i]);
}

unsigned grid_of(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + TB_THREADS - 1) / TB_THREADS); }

// ---------------------------------------------------------------------------------------------------------------------------------
// host side: the byte source (plain or gzip) and the chunker
// ---------------------------------------------------------------------------------------------------------------------------------
struct Source {
  int fd = -1;
  bool gz = false, eof = false, in_eof = false;
  z_stream zs{};
  std::vector<unsigned char> in;
  ~Source() {
    if (gz) inflateEnd(&zs);
    if (fd >= 0) close(fd);
  }
  int open_file(const char* path, std::string* err) {
    fd = ::open(path, O_RDONLY);
    if (fd < 0) {
      *err = std::string("cannot open ") + path;
      return -1;
    }
    unsigned char magic[2] = {0, 0};
    const ssize_t got = pread(fd, magic, 2, 0);
    gz = got == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
    if (gz) {
      in.resize(1 << 20);
      if (inflateInit2(&zs, 15 + 16) != Z_OK) {
        *err = "zlib: inflateInit2 failed";
        return -1;
      }
    }
    return 0;
  }
  // up to `cap` bytes of the (inflated) text; 0 = end of file, -1 = error
  int64_t pull(char* dst, int64_t cap, std::string* err) {
    if (eof || cap <= 0) return 0;
    if (!gz) {
      const ssize_t n = ::read(fd, dst, (size_t)std::min<int64_t>(cap, 1 << 30));
      if (n < 0) {
        *err = "read failed";
        return -1;
      }
      if (n == 0) eof = true;
      return n;
    }
    zs.next_out = reinterpret_cast<Bytef*>(dst);
    zs.avail_out = (uInt)std::min<int64_t>(cap, 1 << 30);
    while (zs.avail_out > 0) {
      if (zs.avail_in == 0 && !in_eof) {
        const ssize_t n = ::read(fd, in.data(), in.size());
        if (n < 0) {
          *err = "read failed";
          return -1;
        }
        if (n == 0) in_eof = true;
        zs.next_in = in.data();
        zs.avail_in = (uInt)n;
      }
      if (zs.avail_in == 0 && in_eof) {
        if (zs.total_in > 0) {      // inside a member that never ended
          *err = "zlib: truncated gzip stream";
          return -1;
        }
        eof = true;
        break;
      }
      const int rc = inflate(&zs, Z_NO_FLUSH);
      if (rc == Z_STREAM_END) {
        inflateReset(&zs);      // the next member (multi-member / bgzip); total_in is 0 again
      } else if (rc != Z_OK && rc != Z_BUF_ERROR) {
        *err = std::string("zlib: ") + (zs.msg ? zs.msg : "corrupt gzip stream");
        return -1;
      }
    }
    return (int64_t)(std::min<int64_t>(cap, 1 << 30) - zs.avail_out);
  }
};

struct Buf {
  char* host = nullptr;      // pinned
  int64_t len = 0;
  bool last = false;
  std::string err;
};

}  // namespace
}  // namespace mural

using namespace mural;

struct MuralTableReader {
  Source src;
  int32_t nc = 0;
  int64_t target = 0, cap = 0, rows_cap = 0, nb_cap = 0, row0 = 0, chunks = 0;
  std::string carry;
  bool finished = false;
  Buf buf[2];
  int cur = 0;
  std::future<void> pending;
  // device
  char* d_text = nullptr;
  int32_t* d_block_cnt = nullptr;
  int64_t* d_block_off = nullptr;
  int32_t* d_row_end = nullptr;
  ChunkMeta* d_meta = nullptr;
  int64_t *d_start = nullptr, *d_end = nullptr;
  int32_t *d_mut = nullptr, *d_chrom = nullptr;
  float* d_label = nullptr;
  uint8_t* d_strand = nullptr;
  double* d_prob = nullptr;
  uint64_t *d_slow = nullptr, *d_runs = nullptr;
  int64_t* d_run_row = nullptr;
  int32_t* d_run_chrom = nullptr;
  int64_t* d_fix_idx = nullptr;
  double* d_fix_val = nullptr;
  int64_t fix_cap = 0;
  // host
  std::vector<std::string> names;
  std::unordered_map<std::string, int32_t> ids;
  std::vector<int64_t> run_row;
  std::vector<int32_t> run_chrom;
  double fill_s = 0.0, wait_s = 0.0, device_s = 0.0;
  int64_t text_bytes = 0;

  // fill b with the next chunk: the carry of the previous one + pulled bytes, cut after the last newline at or before the target
  // size (or the first one past it: a chunk holds one row at least)
  void fill(Buf& b) {
    const auto t0 = std::chrono::steady_clock::now();
    b.err.clear();
    b.last = false;
    int64_t len = (int64_t)carry.size();
    std::memcpy(b.host, carry.data(), carry.size());
    carry.clear();
    while (len < target) {
      const int64_t n = src.pull(b.host + len, target - len, &b.err);
      if (n < 0) return;
      if (n == 0) break;
      len += n;
    }
    const int64_t head = std::min(len, target);
    const char* nl = head ? static_cast<const char*>(memrchr(b.host, '\n', (size_t)head)) : nullptr;
    int64_t scanned = head;
    while (!nl) {
      if (scanned < len) nl = static_cast<const char*>(std::memchr(b.host + scanned, '\n', (size_t)(len - scanned)));
      scanned = len;
      if (nl || src.eof || len >= cap) break;
      const int64_t n = src.pull(b.host + len, std::min<int64_t>(cap - len, 4096), &b.err);
      if (n < 0) return;
      len += n;
    }
    if (!nl && !src.eof) {
      b.err = "a row of the prediction table is longer than " + std::to_string((long long)TB_MAX_ROW) + " bytes";
      return;
    }
    if (!nl) {      // the end of the text without a final newline
      if (len > 0) b.host[len++] = '\n';
      b.len = len;
    } else {
      const int64_t cut = nl - b.host + 1;
      carry.assign(b.host + cut, (size_t)(len - cut));
      b.len = cut;
    }
    b.last = src.eof && carry.empty();
    fill_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }

  void free_all() {
    if (pending.valid()) pending.wait();
    for (Buf& b : buf)
      if (b.host) (void)hipHostFree(b.host);
    void* dev[] = {d_text, d_block_cnt, d_block_off, d_row_end, d_meta, d_start, d_end, d_mut, d_chrom, d_label, d_strand,
                   d_prob, d_slow, d_runs, d_run_row, d_run_chrom, d_fix_idx, d_fix_val};
    for (void* p : dev)
      if (p) (void)hipFree(p);
  }
};

namespace {
template <typename T>
int dev_alloc(T** p, int64_t count) {
  MURAL_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(p), (size_t)std::max<int64_t>(count, 1) * sizeof(T)));
  return MURAL_OK;
}
}  // namespace

extern "C" int mural_table_open(const char* path, int32_t n_class, int64_t chunk_bytes, MuralTableReader** out) {
  MURAL_REQUIRE(path && out, "table_open: NULL argument");
  MURAL_REQUIRE(n_class >= 1 && n_class <= 16, "table_open: 1 <= n_class <= 16 required (got %d)", n_class);
  MURAL_REQUIRE(chunk_bytes >= 1 && chunk_bytes <= (1ll << 30), "table_open: chunk_bytes must be in [1, 2^30] (got %lld)",
                (long long)chunk_bytes);
  *out = nullptr;
  std::unique_ptr<MuralTableReader> r(new MuralTableReader());
  std::string err;
  if (r->src.open_file(path, &err)) {
    set_error("%s", err.c_str());
    return MURAL_E_INVALID;
  }
  r->nc = n_class;
  r->target = chunk_bytes;
  r->cap = chunk_bytes + TB_MAX_ROW;
  r->rows_cap = r->cap / (2 * (n_class + 5)) + 2;      // a row holds n_class + 5 fields of >= 1 byte and their separators
  r->nb_cap = (r->cap + 1 + TB_TILE - 1) / TB_TILE;
  // the header line (validated by the caller) is skipped here; what follows it is the first chunk's carry
  {
    std::vector<char> tmp(TB_MAX_ROW);
    int64_t len = 0;
    const char* nl = nullptr;
    while (!nl && len < TB_MAX_ROW) {
      const int64_t n = r->src.pull(tmp.data() + len, TB_MAX_ROW - len, &err);
      if (n < 0) {
        set_error("%s: %s", path, err.c_str());
        return MURAL_E_INVALID;
      }
      if (n == 0) break;
      nl = static_cast<const char*>(std::memchr(tmp.data() + len, '\n', (size_t)n));
      len += n;
    }
    if (nl) r->carry.assign(nl + 1, (size_t)(tmp.data() + len - (nl + 1)));
    else if (len >= TB_MAX_ROW) {
      set_error("%s: the header line is longer than %lld bytes", path, (long long)TB_MAX_ROW);
      return MURAL_E_INVALID;
    }
  }
  MuralTableReader* t = r.get();
  for (Buf& b : t->buf)
    if (hipHostMalloc(reinterpret_cast<void**>(&b.host), (size_t)t->cap + 16, hipHostMallocDefault) != hipSuccess) {
      set_error("table_open: hipHostMalloc of %lld bytes failed", (long long)t->cap);
      t->free_all();
      return MURAL_E_RUNTIME;
    }
  const int64_t rc_ = t->rows_cap, nc = n_class;
  int rc = dev_alloc(&t->d_text, t->cap + 16);
  if (!rc) rc = dev_alloc(&t->d_block_cnt, t->nb_cap);
  if (!rc) rc = dev_alloc(&t->d_block_off, t->nb_cap + 1);
  if (!rc) rc = dev_alloc(&t->d_row_end, rc_);
  if (!rc) rc = dev_alloc(&t->d_meta, 1);
  if (!rc) rc = dev_alloc(&t->d_start, rc_);
  if (!rc) rc = dev_alloc(&t->d_end, rc_);
  if (!rc) rc = dev_alloc(&t->d_mut, rc_);
  if (!rc) rc = dev_alloc(&t->d_chrom, rc_);
  if (!rc) rc = dev_alloc(&t->d_label, rc_);
  if (!rc) rc = dev_alloc(&t->d_strand, rc_);
  if (!rc) rc = dev_alloc(&t->d_prob, rc_ * nc);
  if (!rc) rc = dev_alloc(&t->d_slow, rc_ * nc);
  if (!rc) rc = dev_alloc(&t->d_runs, rc_);
  if (!rc) rc = dev_alloc(&t->d_run_row, rc_);
  if (!rc) rc = dev_alloc(&t->d_run_chrom, rc_);
  if (rc) {
    t->free_all();
    return rc;
  }
  MuralTableReader* raw = r.release();
  raw->pending = std::async(std::launch::async, [raw] { raw->fill(raw->buf[0]); });
  *out = raw;
  return MURAL_OK;
}

extern "C" void mural_table_close(MuralTableReader* r) {
  if (!r) return;
  r->free_all();
  delete r;
}

extern "C" const char* mural_table_chrom_name(const MuralTableReader* r, int32_t id) {
  if (!r || id < 0 || id >= (int32_t)r->names.size()) return nullptr;
  return r->names[(size_t)id].c_str();
}

extern "C" int mural_table_stats(const MuralTableReader* r, double* out4) {
  MURAL_REQUIRE(r && out4, "table_stats: NULL argument");
  out4[0] = r->fill_s;
  out4[1] = r->wait_s;
  out4[2] = r->device_s;
  out4[3] = (double)r->text_bytes;
  return MURAL_OK;
}

extern "C" int mural_table_next(MuralTableReader* r, MuralTableChunk* c, void* stream_) {
  MURAL_REQUIRE(r && c, "table_next: NULL argument");
  hipStream_t stream = (hipStream_t)stream_;
  std::memset(c, 0, sizeof(*c));
  c->row0 = r->row0;
  c->n_chroms = (int32_t)r->names.size();
  if (r->finished) return MURAL_OK;
  const auto t0 = std::chrono::steady_clock::now();
  r->pending.wait();
  r->pending = std::future<void>();
  Buf& b = r->buf[r->cur];
  const auto t1 = std::chrono::steady_clock::now();
  r->wait_s += std::chrono::duration<double>(t1 - t0).count();
  if (!b.err.empty()) {
    r->finished = true;
    set_error("%s", b.err.c_str());
    return MURAL_E_INVALID;
  }
  const int64_t len = b.len;
  r->text_bytes += len;
  if (len == 0) {
    r->finished = true;
    return MURAL_OK;
  }
  const int64_t nb = (len + TB_TILE - 1) / TB_TILE;
  const int nc = r->nc;
  MURAL_HIP_CHECK(hipMemcpyAsync(r->d_text, b.host, (size_t)len, hipMemcpyHostToDevice, stream));
  MURAL_HIP_CHECK(hipMemsetAsync(r->d_meta, 0, sizeof(ChunkMeta), stream));
  MURAL_HIP_CHECK(hipMemsetAsync(&r->d_meta->status, 0xff, 8, stream));
  hipLaunchKernelGGL(nl_count_kernel, dim3((unsigned)nb), dim3(TB_THREADS), 0, stream, r->d_text, len, r->d_block_cnt);
  hipLaunchKernelGGL(nl_scan_kernel, dim3(1), dim3(TB_THREADS), 0, stream, r->d_block_cnt, nb, r->d_block_off, r->d_meta);
  hipLaunchKernelGGL(nl_emit_kernel, dim3((unsigned)nb), dim3(TB_THREADS), 0, stream, r->d_text, len, r->d_block_off, r->rows_cap,
                     r->d_row_end);
  // (rows beyond rows_cap are malformed rows; the parse launch covers rows_cap at most and the check below reports them)
  const int64_t max_rows = std::min<int64_t>(r->rows_cap, len);
  hipLaunchKernelGGL(parse_rows_kernel, dim3(grid_of(max_rows)), dim3(TB_THREADS), 0, stream, r->d_text, r->d_row_end, r->d_meta,
                     r->rows_cap, nc, r->d_start, r->d_end, r->d_mut, r->d_label, r->d_strand, r->d_prob, r->d_slow,
                     (uint64_t)(r->rows_cap * nc), r->d_runs);
  MURAL_HIP_CHECK(hipGetLastError());
  // the next chunk is read / inflated while the device works on this one (its buffer's last copy has completed: the previous call
  // synchronised the stream after it)
  if (!b.last) {
    Buf* nb_ = &r->buf[r->cur ^ 1];
    r->pending = std::async(std::launch::async, [r, nb_] { r->fill(*nb_); });
  } else {
    r->finished = true;
  }
  ChunkMeta meta;
  MURAL_HIP_CHECK(hipMemcpyAsync(&meta, r->d_meta, sizeof(meta), hipMemcpyDeviceToHost, stream));
  MURAL_HIP_CHECK(hipStreamSynchronize(stream));
  r->device_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
  const int64_t n = meta.n_rows;
  if (n > r->rows_cap && meta.status == ~0ull) {
    set_error("prediction table: rows near line %lld are shorter than %d columns", (long long)(r->row0 + r->rows_cap + 2), nc + 5);
    r->finished = true;
    return MURAL_E_INVALID;
  }
  if (meta.status != ~0ull) {
    static const char* what[] = {"", "malformed number", "wrong number of columns", "strand is not '+' or '-'", "empty row"};
    const int64_t row = (int64_t)(meta.status >> 8);
    const int field = (int)((meta.status >> 3) & 31), code = (int)(meta.status & 7);
    static const char* cols[] = {"chrom", "start", "end", "strand", "mut_type"};
    std::string col = field < 5 ? cols[field] : ("prob" + std::to_string(field - 5));
    if (code == ST_FIELDS) col = "expected " + std::to_string(nc + 5) + " columns";
    set_error("prediction table row %lld (line %lld): %s (%s)", (long long)(r->row0 + row), (long long)(r->row0 + row + 2),
              what[code], col.c_str());
    r->finished = true;
    return MURAL_E_INVALID;
  }
  // chromosome runs: sort by row, name from the first row's bytes, merge with the names seen so far
  std::vector<uint64_t> runs((size_t)meta.n_runs);
  MURAL_HIP_CHECK(hipMemcpy(runs.data(), r->d_runs, runs.size() * 8, hipMemcpyDeviceToHost));
  std::sort(runs.begin(), runs.end());
  r->run_row.resize(runs.size());
  r->run_chrom.resize(runs.size());
  for (size_t k = 0; k < runs.size(); ++k) {
    const char* p = b.host + (runs[k] & 0xffffffffull);
    const char* e = static_cast<const char*>(std::memchr(p, '\t', (size_t)(b.host + len - p)));
    std::string name(p, (size_t)(e - p));
    auto it = r->ids.find(name);
    int32_t id;
    if (it == r->ids.end()) {
      id = (int32_t)r->names.size();
      r->ids.emplace(name, id);
      r->names.push_back(std::move(name));
    } else {
      id = it->second;
    }
    r->run_row[k] = (int64_t)(runs[k] >> 32);
    r->run_chrom[k] = id;
  }
  MURAL_HIP_CHECK(hipMemcpyAsync(r->d_run_row, r->run_row.data(), runs.size() * 8, hipMemcpyHostToDevice, stream));
  MURAL_HIP_CHECK(hipMemcpyAsync(r->d_run_chrom, r->run_chrom.data(), runs.size() * 4, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(chrom_fill_kernel, dim3(grid_of(n)), dim3(TB_THREADS), 0, stream, r->d_run_row, r->d_run_chrom,
                     (int32_t)runs.size(), n, r->d_chrom);
  // fields outside the exact fast path: strtod on the host copy, patched into the device rows
  if (meta.n_slow > 0) {
    std::vector<uint64_t> slow((size_t)meta.n_slow);
    MURAL_HIP_CHECK(hipMemcpy(slow.data(), r->d_slow, slow.size() * 8, hipMemcpyDeviceToHost));
    std::vector<int64_t> idx(slow.size());
    std::vector<double> val(slow.size());
    for (size_t k = 0; k < slow.size(); ++k) {
      idx[k] = (int64_t)(slow[k] >> 32);
      val[k] = std::strtod(b.host + (slow[k] & 0xffffffffull), nullptr);
    }
    if ((int64_t)slow.size() > r->fix_cap) {
      if (r->d_fix_idx) MURAL_HIP_CHECK(hipFree(r->d_fix_idx));
      if (r->d_fix_val) MURAL_HIP_CHECK(hipFree(r->d_fix_val));
      r->d_fix_idx = nullptr;
      r->d_fix_val = nullptr;
      r->fix_cap = 0;
      if (int rc = dev_alloc(&r->d_fix_idx, (int64_t)slow.size())) return rc;
      if (int rc = dev_alloc(&r->d_fix_val, (int64_t)slow.size())) return rc;
      r->fix_cap = (int64_t)slow.size();
    }
    MURAL_HIP_CHECK(hipMemcpy(r->d_fix_idx, idx.data(), idx.size() * 8, hipMemcpyHostToDevice));
    MURAL_HIP_CHECK(hipMemcpy(r->d_fix_val, val.data(), val.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(scatter_f64_kernel, dim3(grid_of((int64_t)idx.size())), dim3(TB_THREADS), 0, stream, r->d_fix_idx, r->d_fix_val,
                       (int64_t)idx.size(), r->d_prob);
  }
  // the run tables are read by chrom_fill_kernel: keep them until it has run (the next call overwrites them)
  MURAL_HIP_CHECK(hipStreamSynchronize(stream));
  MURAL_HIP_CHECK(hipGetLastError());
  c->n_rows = n;
  c->start = r->d_start;
  c->end = r->d_end;
  c->mut_type = r->d_mut;
  c->label = r->d_label;
  c->strand = r->d_strand;
  c->prob = r->d_prob;
  c->chrom_id = r->d_chrom;
  c->n_runs = (int32_t)runs.size();
  c->n_chroms = (int32_t)r->names.size();
  c->run_row = r->run_row.data();
  c->run_chrom = r->run_chrom.data();
  c->text_bytes = len;
  r->row0 += n;
  r->cur ^= 1;
  ++r->chunks;
  return MURAL_OK;
}

extern "C" int mural_table_scale_rows(double* prob, int64_t n, int32_t n_class, double factor, void* stream) {
  MURAL_REQUIRE(n >= 0 && n_class >= 1, "table_scale_rows: bad sizes");
  if (n == 0) return MURAL_OK;
  MURAL_REQUIRE(prob, "table_scale_rows: NULL argument");
  hipLaunchKernelGGL(scale_rows_kernel, dim3(grid_of(n)), dim3(TB_THREADS), 0, (hipStream_t)stream, prob, n, n_class, factor);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" int32_t mural_table_prob_sum_blocks(void) { return PS_BLOCKS; }

extern "C" int mural_table_prob_sum(const double* prob, const int32_t* chrom_id, const int64_t* start, const int64_t* end, int64_t n,
                                    int32_t n_class, const int64_t* reg_off, const int64_t* reg_b0, const int64_t* reg_b1,
                                    int32_t n_reg_chrom, double* part_sum, int64_t* part_cnt, void* stream) {
  MURAL_REQUIRE(n >= 0 && n_class >= 1, "table_prob_sum: bad sizes");
  MURAL_REQUIRE(prob && part_sum && part_cnt, "table_prob_sum: NULL argument");
  MURAL_REQUIRE(!reg_off || (chrom_id && start && end && reg_b0 && reg_b1 && n_reg_chrom >= 0), "table_prob_sum: NULL region argument");
  hipLaunchKernelGGL(prob_sum_kernel, dim3(PS_BLOCKS), dim3(TB_THREADS), 0, (hipStream_t)stream, prob, chrom_id, start, end, n, n_class,
                     reg_off, reg_b0, reg_b1, n_reg_chrom, part_sum, part_cnt);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" int mural_table_kmer_keys(const MuralGenome* g, const int64_t* start, const int64_t* end, const uint8_t* strand, int64_t n,
                                     int32_t k, int32_t indel, int32_t mode, int32_t* key_a, int32_t* key_b, void* stream) {
  MURAL_REQUIRE(g && start && end && key_a, "table_kmer_keys: NULL argument");
  MURAL_REQUIRE(k >= 1 && k <= 15, "table_kmer_keys: 1 <= k <= 15 required (got %d)", k);
  MURAL_REQUIRE(mode >= 0 && mode <= 3 && (mode != 0 || strand) && (mode != 3 || key_b), "table_kmer_keys: bad strand mode");
  if (n == 0) return MURAL_OK;
  hipLaunchKernelGGL(kmer_keys_kernel, dim3(grid_of(n)), dim3(TB_THREADS), 0, (hipStream_t)stream, *g, start, end, strand, n, k, indel,
                     mode, key_a, key_b);
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" int mural_table_first_row(const int32_t* keys, int64_t n, int64_t row0, int32_t sub, int32_t n_groups, uint64_t* first,
                                     void* stream) {
  MURAL_REQUIRE(n >= 0 && n_groups >= 1 && (sub == 0 || sub == 1), "table_first_row: bad arguments");
  if (n == 0) return MURAL_OK;
  MURAL_REQUIRE(keys && first, "table_first_row: NULL argument");
  hipLaunchKernelGGL(first_row_kernel, dim3(grid_of(n)), dim3(TB_THREADS), 0, (hipStream_t)stream, keys, n, row0, sub, n_groups,
                     reinterpret_cast<unsigned long long*>(first));
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

extern "C" int mural_table_start_range(const int32_t* chrom_id, const int64_t* start, int64_t n, int32_t n_chrom, int64_t* mn,
                                       int64_t* mx, void* stream) {
  MURAL_REQUIRE(n >= 0 && n_chrom >= 1, "table_start_range: bad sizes");
  if (n == 0) return MURAL_OK;
  MURAL_REQUIRE(chrom_id && start && mn && mx, "table_start_range: NULL argument");
  hipLaunchKernelGGL(start_range_kernel, dim3(grid_of(n)), dim3(TB_THREADS), 0, (hipStream_t)stream, chrom_id, start, n, n_chrom,
                     reinterpret_cast<long long*>(mn), reinterpret_cast<long long*>(mx));
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}
