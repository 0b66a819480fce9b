// trik_hsv_wave.h -- the plain 64-lane sum and the packed 16-bit vector types,
// for every kernel file (no other project header needed).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

namespace trik_hsv {

// Two 16-bit lanes in the halves of one register (packed VOP3P arithmetic; the
// compiler schedules the packed ops and inserts their wait states)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

// The sum of v over the wave, in every lane (wave_sum<uint64_t>(n) sums a 32-bit n in 64 bits)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  static_assert(std::is_same<T, uint32_t>::value || std::is_same<T, uint64_t>::value, "uint32_t or uint64_t");
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

}  // namespace trik_hsv
