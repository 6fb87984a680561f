// spread kernels for gfx950 (igg/spread.hpp): the two plan passes, one lane
// per point, and the apply pass, one lane per touched cell.
//
// Plan. A point's coordinates give, per dimension, its two corners, their
// factors and how many local cells each reaches (spread_axis); the count pass
// stores the product, the fill pass writes the point's (cell, point, weight)
// entries at its offset in the running sum of the counts. The run table and
// the segments sit in the kernel arguments and are indexed by unrolled loops
// with selects, so nothing is spilled.
//
// Apply. The addresses come from data: lane i reads cell i's linear index,
// splits it into the field's strides (64-bit element offsets), walks its CSR
// segment in order - gathering V[point] - and does the one read-modify-write
// per field. The trip count of the walk is data dependent and a lane folds a
// long segment alone: that is the price of a fixed order of additions
// (profiles/spread_g/NOTES.md). No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include "igg/common.hpp"
#include "igg/spread.hpp"

namespace igg {
namespace {

constexpr int BLOCK = SPREAD_BLOCK;

__global__ void __launch_bounds__(BLOCK) spread_count_kernel(const SpreadPlanArgs A) {
  const int64_t lanes = static_cast<int64_t>(gridDim.x) * BLOCK;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x; p < A.npts; p += lanes) {
    SpreadAxis ax[3];
    A.count[p] = spread_point(A, p, ax);
  }
}

__global__ void __launch_bounds__(BLOCK) spread_fill_kernel(const SpreadPlanArgs A) {
  const int64_t lanes = static_cast<int64_t>(gridDim.x) * BLOCK;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x; p < A.npts; p += lanes)
    spread_fill_point(A, p, p > 0 ? A.cum[p - 1] : 0);
}

template <typename T>
__global__ void __launch_bounds__(BLOCK) spread_apply_kernel(const SpreadArgs A) {
  const double* __restrict__ V = A.V;
  if (A.row) {  // a source's row counter, read on the device (wave-uniform)
    const int64_t r = *A.row;
    if (r < 0 || r >= A.nrows) return;
    V += r * A.row_stride;
  }
  const int64_t lanes = static_cast<int64_t>(gridDim.x) * BLOCK;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x; i < A.ncells; i += lanes)
    spread_cell<T>(A, V, i);
}

}  // namespace

void launch_spread_count(const SpreadPlanArgs& a, int blocks, hipStream_t stream) {
  if (blocks < 1 || a.nd < 1 || a.nd > 3) fail("spread_count: ", blocks, " blocks, ", a.nd, " dimensions");
  hipLaunchKernelGGL(spread_count_kernel, dim3(blocks), dim3(BLOCK), 0, stream, a);
  IGG_HIP_CHECK(hipGetLastError());
}

void launch_spread_fill(const SpreadPlanArgs& a, int blocks, hipStream_t stream) {
  if (blocks < 1 || a.nd < 1 || a.nd > 3) fail("spread_fill: ", blocks, " blocks, ", a.nd, " dimensions");
  hipLaunchKernelGGL(spread_fill_kernel, dim3(blocks), dim3(BLOCK), 0, stream, a);
  IGG_HIP_CHECK(hipGetLastError());
}

void launch_spread_apply(const SpreadArgs& a, int elem_size, int blocks, hipStream_t stream) {
  if (blocks < 1 || a.nd < 1 || a.nd > 3 || a.nf < 1 || a.nf > SPREAD_MAX_FIELDS)
    fail("spread_apply: ", blocks, " blocks, ", a.nd, " dimensions, ", a.nf, " fields in one launch");
  if (elem_size == 4)
    hipLaunchKernelGGL(spread_apply_kernel<float>, dim3(blocks), dim3(BLOCK), 0, stream, a);
  else
    hipLaunchKernelGGL(spread_apply_kernel<double>, dim3(blocks), dim3(BLOCK), 0, stream, a);
  IGG_HIP_CHECK(hipGetLastError());
}

}  // namespace igg
