#pragma once
// XCD-aware block numbering shared by the stencil kernels.
#include <cstdint>

#include <hip/hip_runtime.h>

namespace igg {

__device__ __forceinline__ int64_t xcd_remap(int64_t b, int64_t nb) {
  // Bijective round-robin inversion (cdna_hip_programming.md §5 'XCD swizzle
  // must be bijective'): blocks dealt to XCD k get the contiguous id range k*q..
  const int64_t q = nb / 8, r = nb % 8, xcd = b % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + b / 8;
}

}  // namespace igg
