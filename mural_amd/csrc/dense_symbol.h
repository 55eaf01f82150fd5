// Classification of one column of a dense (n, 4, L) one-hot / IUPAC-fraction window into its symbol (reference encoding:
// MuRaL/data/preprocessing.py:756-816): shared by the dense -> symbol pass (encode.hip) and the small-batch first-stage kernel, which
// reads the dense window itself (snv_stage1.hip).
#pragma once
#include "common.h"

namespace mural {

__device__ __forceinline__ int frac_digit(float v) {
  if (v == 0.0f) return 0;
  if (v == 1.0f) return 1;
  if (v == 0.5f) return 2;
  if (v == 0.25f) return 3;
  if (v == (float)(1.0 / 3.0)) return 4;
  return -1;
}

// symbol -> its dense column: o[ch * stride] for the 4 channels.  Channel set of the symbol (bit ch = base ch is possible): one-hot,
// pairs 0.5, triples 1/3, N 0.25 (preprocessing.py:758-772)
__device__ __forceinline__ void symbol_to_dense(uint32_t s, float* __restrict__ o, int64_t stride) {
  const uint32_t set = (0xF7BDEC963A5F8421ull >> (4u * s)) & 0xFu;
  const int members = __popc(set);
  const float v = members == 1 ? 1.0f : members == 2 ? 0.5f : members == 3 ? (float)(1.0 / 3.0) : 0.25f;
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) o[(int64_t)ch * stride] = ((set >> ch) & 1u) ? v : 0.0f;
}

// dense (n,4,L) one-hot / IUPAC-fraction tensor -> 1 symbol per column (what the fused kernel consumes)
__device__ __forceinline__ int dense_symbol(float v0, float v1, float v2, float v3) {
  const int d0 = frac_digit(v0), d1 = frac_digit(v1), d2 = frac_digit(v2), d3 = frac_digit(v3);
  int s = -1;
  if ((d0 | d1 | d2 | d3) >= 0) {
    switch (d0 + 5 * d1 + 25 * d2 + 125 * d3) {
      case 1: s = 0; break;      // A
      case 5: s = 1; break;      // C
      case 25: s = 2; break;     // G
      case 125: s = 3; break;    // T
      case 468: s = 4; break;    // N
      case 52: s = 5; break;     // R
      case 260: s = 6; break;    // Y
      case 12: s = 7; break;     // M
      case 60: s = 8; break;     // S
      case 252: s = 9; break;    // W
      case 300: s = 10; break;   // K
      case 620: s = 11; break;   // B
      case 604: s = 12; break;   // D
      case 524: s = 13; break;   // H
      case 124: s = 14; break;   // V
      default: break;
    }
  }
  return s;
}

}  // namespace mural
