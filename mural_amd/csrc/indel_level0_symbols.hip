// The symbols entry's instances of the persistent first-level kernel (indel_level0_enc0.h; mural_indel_forward_symbols): one symbol byte
// per column from the caller (ConvBlockArgs::sym_in) and no dense window behind them (f_in == nullptr) -- a byte above 14 is staged as N.
#include "indel_level0_enc0.h"

namespace mural {

int launch_indel_enc0_symbols(const ConvBlockArgs& a, int tiles_per_row, long long total, hipStream_t stream) {
  MURAL_REQUIRE(a.sym_in && !a.f_in, "level-0 launch: the symbols instances take bytes without a dense window");
  const bool down = a.d_out != nullptr;
  const int v = (a.sym_taps == 7 ? 0 : 1) + (down ? 2 : 0);      // the instance that is launched
  static int wg_per_cu[4] = {0, 0, 0, 0}, cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    MURAL_HIP_CHECK(hipGetDevice(&dev));
    MURAL_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    cus = prop.multiProcessorCount;
  }
#define MURAL_E0S_CASES(X)                         \
  switch (v) {                                     \
    case 0: X(13, false, false, true, true); break; \
    case 1: X(7, false, false, true, true); break;  \
    case 2: X(13, false, true, true, true); break;  \
    default: X(7, false, true, true, true); break;  \
  }
  if (wg_per_cu[v] == 0) {
    int n = 0;
#define MURAL_E0S_OCC(...) MURAL_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, indel_enc0_kernel<__VA_ARGS__>, 256, 0))
    MURAL_E0S_CASES(MURAL_E0S_OCC)
#undef MURAL_E0S_OCC
    wg_per_cu[v] = n > 7 ? 7 : (n > 0 ? n : 1);
  }
  const long long want = (long long)cus * wg_per_cu[v];
  const dim3 grid((unsigned)(total < want ? total : want));
  unsigned long long* const stamps = nullptr;      // (the byte-source instances carry no phase stamps)
#define MURAL_E0S(...) hipLaunchKernelGGL((indel_enc0_kernel<__VA_ARGS__>), grid, dim3(256), 0, stream, a, a.w5, a.b5, a.w1, a.b1, tiles_per_row, total, stamps)
  MURAL_E0S_CASES(MURAL_E0S)
#undef MURAL_E0S
#undef MURAL_E0S_CASES
  MURAL_HIP_CHECK(hipGetLastError());
  return MURAL_OK;
}

}  // namespace mural
