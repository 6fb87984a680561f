// sample_kernel for gfx950 (igg/sample.hpp): gather and interpolate, one point
// per lane and SAMPLE_POINTS points per lane in flight.
//
// The addresses come from data: a point's coordinates give, per dimension, the
// two corner indices, the weight and whether this rank owns the cell
// (sample_axis), once per point and shared by every field of the launch. A
// field adds its strides: one 64-bit element offset per corner. All 2^nd corner
// loads of a field for both points of a lane are issued before the first is
// used, so a lane has 2 * 2^nd independent loads outstanding against the
// latency of an uncoalesced gather. A point this rank does not own reads
// element 0 (one hot line) and stores 0. Nothing branches on a point's value:
// selects only, and every lane that has a point stores. No LDS, no atomics,
// no scratch.
//
// The two corners along the memory-innermost axis are two loads, not one wider
// load: which axis is innermost depends on the layout, a pair is aligned to
// its own size at even indices only, and the clamped upper corner of the last
// cell is not the lower one's neighbour (profiles/sample_g/NOTES.md).
#include <hip/hip_runtime.h>

#include "igg/common.hpp"
#include "igg/sample.hpp"

namespace igg {
namespace {

constexpr int BLOCK = SAMPLE_BLOCK;
constexpr int NP = SAMPLE_POINTS;

template <typename T, int ND>
__global__ void __launch_bounds__(BLOCK) sample_kernel(const SampleArgs A) {
  constexpr int NC = 1 << ND;
  uint64_t* __restrict__ out = A.out;
  if (A.row) {  // a recorder's row counter, read on the device (wave-uniform)
    const int64_t r = *A.row;
    if (r < 0 || r >= A.nrows) return;
    out += r * A.row_stride;
  }
  const int64_t lanes = static_cast<int64_t>(gridDim.x) * BLOCK;
  for (int64_t p0 = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x; p0 < A.npts; p0 += NP * lanes) {
    int64_t lo[NP][ND], hi[NP][ND];
    double t[NP][ND];
    bool valid[NP], owned[NP], live[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int64_t p = p0 + k * lanes;
      live[k] = p < A.npts;
      const int64_t q = live[k] ? p : p0;  // a lane without a second point rereads its first
      valid[k] = true, owned[k] = true;
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const SampleAxis a = sample_axis(A.dim[d], A.P[q * A.ps0 + d * A.ps1]);
        valid[k] = valid[k] && a.valid, owned[k] = owned[k] && a.owned;
        lo[k][d] = a.lo, hi[k][d] = a.hi, t[k][d] = a.t;
      }
      if (!(valid[k] && owned[k])) {
#pragma unroll
        for (int d = 0; d < ND; ++d) lo[k][d] = 0, hi[k][d] = 0;
      }
    }
    for (int f = 0; f < A.nf; ++f) {
      const T* __restrict__ base = static_cast<const T*>(A.field[f].base);
      T v[NP][NC];
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        // corner c takes the upper index of axis d where bit (ND - 1 - d) of c is set
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          int64_t off = 0;
#pragma unroll
          for (int d = 0; d < ND; ++d) off += (((c >> (ND - 1 - d)) & 1) ? hi[k][d] : lo[k][d]) * A.field[f].stride[d];
          v[k][c] = base[off];
        }
      }
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        double w[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) w[c] = static_cast<double>(v[k][c]);
        // collapse in index order, the last axis first
#pragma unroll
        for (int d = ND - 1; d >= 0; --d) {
#pragma unroll
          for (int c = 0; c < (1 << d); ++c) w[c] = sample_lerp(w[2 * c], w[2 * c + 1], t[k][d]);
        }
        if (live[k])
          out[f * A.out_fs + p0 + k * lanes] = sample_bits(w[0], valid[k], owned[k], A.me0 != 0);
      }
    }
  }
}

template <typename T>
void launch_t(const SampleArgs& a, int blocks, hipStream_t stream) {
  if (a.nd == 1)
    hipLaunchKernelGGL((sample_kernel<T, 1>), dim3(blocks), dim3(BLOCK), 0, stream, a);
  else if (a.nd == 2)
    hipLaunchKernelGGL((sample_kernel<T, 2>), dim3(blocks), dim3(BLOCK), 0, stream, a);
  else
    hipLaunchKernelGGL((sample_kernel<T, 3>), dim3(blocks), dim3(BLOCK), 0, stream, a);
}

}  // namespace

void launch_sample(const SampleArgs& a, int elem_size, int blocks, hipStream_t stream) {
  if (blocks < 1 || a.nd < 1 || a.nd > 3 || a.nf < 1 || a.nf > SAMPLE_MAX_FIELDS)
    fail("sample: ", blocks, " blocks, ", a.nd, " dimensions, ", a.nf, " fields in one launch");
  if (elem_size == 4)
    launch_t<float>(a, blocks, stream);
  else
    launch_t<double>(a, blocks, stream);
  IGG_HIP_CHECK(hipGetLastError());
}

}  // namespace igg
