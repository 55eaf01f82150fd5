// Internal helpers shared by the translation units of libmural_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mural_hip.h"

namespace mural {

// ---- environment switches --------------------------------------------------------------------------------------------------------
// The PRODUCT library (libmural_hip.so) reads two variables: MURAL_HOST_THREADS (host threads of the ingest passes, csrc/ingest.hip)
// and TMPDIR (inflated copies of gzip inputs).  Every other switch is a development switch -- an A/B of two kernels, a validation
// path, a diagnostic, or a timing experiment that produces WRONG results -- listed in ONE table (encode.hip: dev_switch_table) and
// read through dev_env(), which answers "not set" unless the debug flavour is loaded (libmural_hip_debug.so: csrc/debug_hooks.hip sets
// g_dev_switches).  A stray MURAL_* variable cannot change what the product library computes.
struct DevSwitch { const char* name; const char* what; };
const DevSwitch* dev_switch_table();      // terminated by {nullptr, nullptr}
extern bool g_dev_switches;
const char* dev_env(const char* name);    // getenv(name) in the debug flavour (the name must be in the table), nullptr otherwise
int dev_int(const char* name, int dflt);  // atoi of dev_env(name), dflt where that is nullptr

void set_error(const char* fmt, ...);
// Validation of the workspace carvers (tests only): MURAL_DEBUG_WS_GUARD=<bytes> in the environment puts that many unused bytes behind
// every region a carver hands out, and the regions of the calling thread's latest carve are kept for mural_debug_last_ws_layout, so
// that a test can poison a workspace, run a call and see that nothing was written outside the regions.
size_t ws_guard_bytes();
void ws_layout_reset();
void ws_layout_add(size_t off, size_t bytes);
extern thread_local std::vector<size_t> g_ws_layout;      // (offset, bytes) pairs, read by mural_debug_last_ws_layout

// THE workspace carver: a bump pointer over the caller's workspace, regions at 256-byte offsets.  base == nullptr: a sizing run
// (every region comes back nullptr, `off` ends at the bytes needed).  An empty region takes no space, no guard and no layout entry.
struct WsArena {
  char* base;
  size_t off = 0;
  size_t guard;           // validation only (MURAL_DEBUG_WS_GUARD above): unused bytes behind every region
  explicit WsArena(void* b) : base(static_cast<char*>(b)), guard(ws_guard_bytes()) { ws_layout_reset(); }
  void* take(size_t bytes) {
    const size_t o = off;
    if (bytes) ws_layout_add(o, bytes);
    off = (off + bytes + (bytes ? guard : 0) + 255) & ~size_t(255);
    return base ? base + o : nullptr;
  }
  template <typename T>
  T* as(size_t n) { return static_cast<T*>(take(n * sizeof(T))); }
  float* f(size_t n) { return as<float>(n); }
  double* d(size_t n) { return as<double>(n); }
  int32_t* i(size_t n) { return as<int32_t>(n); }
  uint8_t* b(size_t n) { return as<uint8_t>(n); }
};

// dense (n, 4, L) one-hot / IUPAC-fraction windows -> one symbol byte per column (encode.hip).  A column that is no valid encoding
// becomes N and sets MURAL_E_ENCODING in *status (bad_code < 0), or becomes bad_code without a report
int launch_dense_to_symbols(const float* x, int64_t n, int L, uint8_t* sym, int32_t* status, hipStream_t stream, int bad_code = -1);

#define MURAL_HIP_CHECK(expr)                                                                      \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      ::mural::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return MURAL_E_RUNTIME;                                                                      \
    }                                                                                              \
  } while (0)

#define MURAL_REQUIRE(cond, ...)            \
  do {                                      \
    if (!(cond)) {                          \
      ::mural::set_error(__VA_ARGS__);      \
      return MURAL_E_INVALID;               \
    }                                       \
  } while (0)

// MURAL_OK, or the refusal of a workspace that is NULL, not 8-byte aligned or smaller than the `need` bytes that `bytes_fn` names
inline int check_workspace(const char* entry, const char* bytes_fn, const void* ws, size_t ws_bytes, size_t need) {
  if (ws && ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 7) == 0) return MURAL_OK;
  set_error("%s: the workspace is NULL, misaligned or smaller than %s (%zu)", entry, bytes_fn, need);
  return MURAL_E_WORKSPACE;
}

// the window of a site at `pos` (reference: MuRaL/data/preprocessing.py:559-567): genome positions pos + off .. pos + off + width - 1; the
// indel window is the even one (:564-566)
inline int window_geometry(int radius, int indel, int* off, int* width) {
  MURAL_REQUIRE(radius >= 1, "radius must be >= 1, got %d", radius);
  *off = indel ? -radius + 1 : -radius;
  *width = indel ? 2 * radius : 2 * radius + 1;
  return MURAL_OK;
}

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to (kernel, device): a launch site raises it once per device ordinal
// (never inside a stream capture after the first call on that device).  Thread-safe; setting it twice is harmless.
struct DynLdsOnce {
  std::atomic<uint64_t> done{0};
  template <typename... Fn>
  int ensure(Fn... fns) {
    int dev = 0;
    MURAL_HIP_CHECK(hipGetDevice(&dev));
    const uint64_t bit = dev < 64 ? (1ull << dev) : 0ull;
    if (bit && (done.load(std::memory_order_acquire) & bit)) return MURAL_OK;
    const void* list[] = {reinterpret_cast<const void*>(fns)...};
    for (const void* f : list)
      MURAL_HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    done.fetch_or(bit, std::memory_order_release);
    return MURAL_OK;
  }
};

// symbols of the in-LDS base alphabet
enum : uint8_t { SYM_A = 0, SYM_C = 1, SYM_G = 2, SYM_T = 3, SYM_N = 4, SYM_PAD = 15, SYM_BAD = 255 };
constexpr int N_SYM = 16;

// exact unsigned division by a runtime constant: valid while n * d < 2^32
struct FastDiv {
  uint32_t d, m;
  __host__ __device__ static constexpr FastDiv make(uint32_t d) {
    FastDiv f{};
    f.d = d;
    f.m = (uint32_t)((0x100000000ull / d) + 1ull);
    return f;
  }
  __device__ __forceinline__ uint32_t div(uint32_t n) const { return d == 1 ? n : __umulhi(n, m); }
  // the same without the branch on d == 1 (there m == 1 and the high product is 0): for code that divides per element in long
  // unrolled sequences, where a wave-uniform branch per division costs more instruction fetch than two scalar-masked ALU ops
  __device__ __forceinline__ uint32_t divnb(uint32_t n) const { return __umulhi(n, m) + (n & (0u - (uint32_t)(d == 1))); }
};

// exact n / d for n <= the bound the host built it for: q = (n * M) >> S with 2^S > bound * d (FastDiv's single multiply stops at
// n * d < 2^32: a flattened (row, column) index of a long batch needs the wider product)
struct DivWide {
  uint32_t M, S;
  static DivWide make(uint32_t d, uint64_t bound) {      // bound * d < 2^62, bound < 2^31
    uint32_t S = 0;
    while ((1ull << S) <= bound * d) ++S;
    DivWide r;
    r.S = S;
    r.M = (uint32_t)(((1ull << S) + d - 1) / d);
    return r;
  }
  __device__ __forceinline__ uint32_t div(uint32_t n) const { return (uint32_t)(((uint64_t)n * M) >> S); }
};

// ---------------------------------------------------------------------------------------------
// A per-device side stream for independent work inside one library call.  Fork: the side stream waits for everything queued on
// the caller's stream; join: the caller's stream waits for the side stream.  Both are legal inside a stream capture (the side
// stream joins the capture and leaves it at the join).
// ---------------------------------------------------------------------------------------------
struct SideStream {
  hipStream_t side = nullptr, side2 = nullptr;
  hipEvent_t fork_ev = nullptr, join_ev = nullptr, join2_ev = nullptr;
  // One set of streams / events per device: a caller holds `mu` from its fork to its join (SideStreamHold), so two host threads that
  // drive the same device cannot cross-wire each other's fork / join events.  (The enqueue between fork and join is host work of a
  // few hundred microseconds; the device side stays concurrent.)
  std::mutex mu;
  bool ready = false;
  int init() {          // called with `mu` held
    if (ready) return MURAL_OK;
    // (default priority: serving the mid tower's chain first gained 2 % on the training leg run alone and halved it after other legs)
    MURAL_HIP_CHECK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    MURAL_HIP_CHECK(hipStreamCreateWithFlags(&side2, hipStreamNonBlocking));
    MURAL_HIP_CHECK(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming));
    MURAL_HIP_CHECK(hipEventCreateWithFlags(&join_ev, hipEventDisableTiming));
    MURAL_HIP_CHECK(hipEventCreateWithFlags(&join2_ev, hipEventDisableTiming));
    ready = true;
    return MURAL_OK;
  }
  int fork(hipStream_t main, bool both = false) {
    MURAL_HIP_CHECK(hipEventRecord(fork_ev, main));
    MURAL_HIP_CHECK(hipStreamWaitEvent(side, fork_ev, 0));
    if (both) MURAL_HIP_CHECK(hipStreamWaitEvent(side2, fork_ev, 0));
    return MURAL_OK;
  }
  int fork2(hipStream_t main) {      // the second side stream alone (an earlier point of the caller's stream than fork())
    MURAL_HIP_CHECK(hipEventRecord(fork_ev, main));
    MURAL_HIP_CHECK(hipStreamWaitEvent(side2, fork_ev, 0));
    return MURAL_OK;
  }
  int join(hipStream_t main, bool both = false) {
    MURAL_HIP_CHECK(hipEventRecord(join_ev, side));
    MURAL_HIP_CHECK(hipStreamWaitEvent(main, join_ev, 0));
    if (both) {
      MURAL_HIP_CHECK(hipEventRecord(join2_ev, side2));
      MURAL_HIP_CHECK(hipStreamWaitEvent(main, join2_ev, 0));
    }
    return MURAL_OK;
  }
};

SideStream* side_stream_slot(int dev);      // encode.hip: ONE table for the whole library (not one per translation unit)

// Exclusive use of the current device's side streams for the lifetime of the object (fork .. join of one library call).
struct SideStreamHold {
  SideStream* ss = nullptr;
  std::unique_lock<std::mutex> lock;
  int acquire() {
    int dev = 0;
    MURAL_HIP_CHECK(hipGetDevice(&dev));
    MURAL_REQUIRE(dev >= 0 && dev < 64, "device index %d out of range", dev);
    SideStream* s = side_stream_slot(dev);
    lock = std::unique_lock<std::mutex>(s->mu);
    if (int rc = s->init()) return rc;
    ss = s;
    return MURAL_OK;
  }
  SideStream* operator->() const { return ss; }
};

// ---------------------------------------------------------------------------------------------
// prefix sums of per-thread counts (tables.hip: rows of a text chunk; sites.hip: sites of a genome tile)
// ---------------------------------------------------------------------------------------------
constexpr int SCAN_THREADS = 256;

__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  return v;
}

// exclusive prefix of `v` over the block (256 threads = 4 waves); *total = the block's sum
__device__ __forceinline__ int block_excl_scan(int v, int* total) {
  __shared__ int wave_tot[SCAN_THREADS / 64];
  const int incl = wave_incl_scan(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) wave_tot[w] = incl;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int k = 0; k < SCAN_THREADS / 64; ++k) {
    base += k < w ? wave_tot[k] : 0;
    sum += wave_tot[k];
  }
  __syncthreads();
  *total = sum;
  return base + incl - v;
}

typedef unsigned long long u64;      // the integer cells of the table reductions (summary_*.hip, simulate.hip)

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// first index of [lo, hi) where pred fails, the whole wave searching; pred holds on a prefix of the range.  A probe per lane splits the
// range 64 ways a round; the range shrinks every round whatever the data hold, and no probe leaves it.  (amb_lower_bound_wave below is
// the same search with its predicate written in: it is inlined into the encode and stage-1 kernels, whose code is left as it is.)
template <typename Pred>
__device__ __forceinline__ int64_t wave_partition_point(int64_t lo, int64_t hi, Pred pred) {
  const int lane = threadIdx.x & 63;
  while (lo < hi) {
    const int64_t step = (hi - lo + 63) / 64;
    const int64_t p = lo + lane * step;
    const int holds = __popcll(__ballot(p < hi && pred(p)));
    if (holds == 0) {
      hi = lo;
    } else {
      hi = min(hi, lo + holds * step);
      lo = lo + (holds - 1) * step + 1;
    }
  }
  return lo;
}

// The exclusive prefix of m elements by ONE workgroup of THREADS threads, every thread of which calls: store(t, load(0) + .. +
// load(t - 1)) for t = 0 .. m - 1, the total comes back in every thread.  A thread owns a run of ceil(m / THREADS) consecutive elements
// (the last runs may be short or empty): it sums its run, the run sums are scanned by shuffles and the wave totals through LDS, and it
// walks its run again.  load(t) is called before store(t) and by the same thread, so the prefix may replace the elements in place.
template <int THREADS, typename T, typename Load, typename Store>
__device__ __forceinline__ T run_excl_scan(int64_t m, Load load, Store store) {
  __shared__ T wave_tot[THREADS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t run = (m + THREADS - 1) / THREADS;
  const int64_t t0 = min((int64_t)threadIdx.x * run, m), t1 = min(t0 + run, m);
  T mine = 0;
  for (int64_t t = t0; t < t1; ++t) mine += load(t);
  T incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  if (lane == 63) wave_tot[w] = incl;
  __syncthreads();
  T base = 0, total = 0;
#pragma unroll
  for (int k = 0; k < THREADS / 64; ++k) {
    base += k < w ? wave_tot[k] : 0;
    total += wave_tot[k];
  }
  T running = base + incl - mine;
  for (int64_t t = t0; t < t1; ++t) {
    const T x = load(t);
    store(t, running);
    running += x;
  }
  return total;
}

// ---------------------------------------------------------------------------------------------
// packed genome access
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t genome_sym(const uint32_t* __restrict__ packed2,
                                               const uint32_t* __restrict__ nmask, int64_t length, int64_t g) {
  if (g < 0 || g >= length) return SYM_N;
  uint32_t w = packed2[g >> 4];
  uint32_t m = nmask[g >> 5];
  uint32_t two = (w >> (2u * (uint32_t)(g & 15))) & 3u;
  return ((m >> (uint32_t)(g & 31)) & 1u) ? (uint32_t)SYM_N : two;
}

// first index of the ascending side table with amb_pos[i] >= key (plain binary search, one thread)
__device__ __forceinline__ int64_t amb_lower_bound(const int64_t* __restrict__ amb_pos, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (amb_pos[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the same bound found by a whole wave: 64 probes per round, wave-uniform result
__device__ __forceinline__ int64_t amb_lower_bound_wave(const int64_t* __restrict__ amb_pos, int64_t n, int64_t key, int lane) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t step = (hi - lo + 63) >> 6;
    const int64_t idx = lo + (int64_t)lane * step;
    const bool less = idx < hi && amb_pos[idx] < key;
    const int cnt = __popcll(__ballot(less));          // the table ascends: `less` lanes form a prefix
    if (cnt == 0) {
      hi = lo;
    } else {
      const int64_t nhi = lo + (int64_t)cnt * step;
      lo = lo + (int64_t)(cnt - 1) * step + 1;
      hi = nhi < hi ? nhi : hi;
    }
  }
  return lo;
}

// symbol of position g inside the record, given its packed2 word `w` and nmask word `m` (from memory or from a staged copy): the IUPAC
// codes are resolved through the side table (strand-agnostic, forward symbol)
__device__ __forceinline__ uint32_t sym_from_words(const MuralGenome& gn, int64_t g, uint32_t w, uint32_t m) {
  if (((m >> (uint32_t)(g & 31)) & 1u) == 0u) return (w >> (2u * (uint32_t)(g & 15))) & 3u;
  if (gn.n_amb > 0) {
    const int64_t i = amb_lower_bound(gn.amb_pos, gn.n_amb, g);
    if (i < gn.n_amb && gn.amb_pos[i] == g) return gn.amb_sym[i];
  }
  return SYM_N;
}

// symbol of genome position g with IUPAC codes resolved through the side table (strand-agnostic, forward symbol)
__device__ __forceinline__ uint32_t genome_sym_iupac(const MuralGenome& gn, int64_t g) {
  if (g < 0 || g >= gn.length) return SYM_N;
  return sym_from_words(gn, g, gn.packed2[g >> 4], gn.nmask[g >> 5]);
}

// complement within the 16-symbol alphabet (A<->T, C<->G, N, R<->Y, M<->K, S, W, B<->V, D<->H, PAD)
__device__ __forceinline__ uint32_t sym_complement(uint32_t s) {
  // table packed 4 bits per symbol: index 0..15 -> 3,2,1,0,4,6,5,10,8,9,7,14,13,12,11,15
  const uint64_t tbl = 0xFBCDE798A5640123ull;
  return (uint32_t)((tbl >> (4u * s)) & 0xFull);
}

}  // namespace mural
