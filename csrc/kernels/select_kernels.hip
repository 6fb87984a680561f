// Converting lattice copies for gfx950 (igg/select.hpp): select_convert_kernel,
// f64 in, f32 out, described here, and its mirror select_widen_kernel, f32 in,
// f64 out, described where it stands.
//
// rows path: a wave takes one row of the lattice (unit stride on both sides);
// the row's (i0, i1) decode and both row pointers are wave-uniform scalar
// arithmetic, once per row. The destination row is split at its 16-B
// boundaries: up to three head elements and up to three tail elements are
// stored singly by predicated lanes, the body as aligned f32x4 stores, one per
// lane and pass. The four doubles behind a store start at any element of the
// source (the row of an owned box usually starts at an odd one), so they are
// read as two 16-B loads that promise only 8-B alignment. A lane issues
// SELECT_UNROLL such units before it converts and stores any; a unit past the
// end of the row reloads the row's last unit (in bounds) and is not stored.
//
// element path: one output per lane over the flattened lattice, any strides.
//
// Both paths mask by predication only: what lies between and around the
// selected elements is never loaded on the rows path beyond the row itself,
// never at all on the element path, and never enters arithmetic. No LDS.
#include <hip/hip_runtime.h>

#include "igg/common.hpp"
#include "igg/select.hpp"

namespace igg {
namespace {

constexpr int BLOCK = SELECT_BLOCK;
constexpr int WAVES = BLOCK / 64;
constexpr int U = SELECT_UNROLL;

typedef double D2 __attribute__((ext_vector_type(2)));
typedef D2 D2e __attribute__((aligned(8)));  // element-aligned pair
typedef float F4 __attribute__((ext_vector_type(4)));

template <typename IDX>
__global__ void __launch_bounds__(BLOCK) select_convert_kernel(const SelectBatch batch) {
  const uint32_t b = blockIdx.x;
  int c = 0;
  while (c + 1 < batch.n && b >= batch.block_start[c + 1]) ++c;
  const SelectJob& J = batch.job[c];
  const uint32_t local = b - batch.block_start[c];
  const uint32_t nb = batch.block_start[c + 1] - batch.block_start[c];
  const double* __restrict__ src = J.src;
  float* __restrict__ dst = J.dst;
  const IDX c1 = static_cast<IDX>(J.c[1]), c2 = static_cast<IDX>(J.c[2]);
  if (J.rows) {
    const uint32_t lane = threadIdx.x & 63;
    const IDX nrows = static_cast<IDX>(J.c[0]) * c1;
    const IDX nw = static_cast<IDX>(nb) * WAVES;
    const IDX S0 = static_cast<IDX>(J.S[0]), S1 = static_cast<IDX>(J.S[1]);
    const IDX T0 = static_cast<IDX>(J.T[0]), T1 = static_cast<IDX>(J.T[1]);
    for (IDX row = static_cast<IDX>(local) * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); row < nrows;
         row += nw) {
      const IDX i0 = row / c1, i1 = row - i0 * c1;
      const double* s = src + (i0 * S0 + i1 * S1);
      float* d = dst + (i0 * T0 + i1 * T1);
      // elements before the destination row's first 16-B boundary
      IDX h = (4u - (static_cast<uint32_t>(reinterpret_cast<uintptr_t>(d) >> 2) & 3u)) & 3u;
      if (h > c2) h = c2;
      const IDX nvec = (c2 - h) >> 2, tail = (c2 - h) & 3;
      const IDX t0 = h + (nvec << 2);
      if (lane < h) d[lane] = static_cast<float>(s[lane]);
      if (lane >= 32 && lane - 32 < tail) d[t0 + (lane - 32)] = static_cast<float>(s[t0 + (lane - 32)]);
      const double* sb = s + h;
      F4* db = reinterpret_cast<F4*>(d + h);
      for (IDX u0 = lane; u0 < nvec; u0 += 64 * U) {
        D2 lo[U], hi[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const IDX u = u0 + 64 * k;
          const double* p = sb + ((u < nvec ? u : nvec - 1) << 2);
          lo[k] = *reinterpret_cast<const D2e*>(p);
          hi[k] = *reinterpret_cast<const D2e*>(p + 2);
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const IDX u = u0 + 64 * k;
          if (u < nvec)
            db[u] = F4{static_cast<float>(lo[k].x), static_cast<float>(lo[k].y), static_cast<float>(hi[k].x),
                       static_cast<float>(hi[k].y)};
        }
      }
    }
  } else {
    const IDX total = static_cast<IDX>(J.c[0]) * c1 * c2;
    const IDX stride = static_cast<IDX>(nb) * BLOCK;
    const IDX S0 = static_cast<IDX>(J.S[0]), S1 = static_cast<IDX>(J.S[1]), S2 = static_cast<IDX>(J.S[2]);
    const IDX T0 = static_cast<IDX>(J.T[0]), T1 = static_cast<IDX>(J.T[1]), T2 = static_cast<IDX>(J.T[2]);
    for (IDX e = static_cast<IDX>(local) * BLOCK + threadIdx.x; e < total; e += stride) {
      const IDX q = e / c2, i2 = e - q * c2;
      const IDX i0 = q / c1, i1 = q - i0 * c1;
      dst[i0 * T0 + i1 * T1 + i2 * T2] = static_cast<float>(src[i0 * S0 + i1 * S1 + i2 * S2]);
    }
  }
}

typedef F4 F4e __attribute__((aligned(4)));  // element-aligned quad

// The widening mirror: f32 in, f64 out (scatter_g's receiver). Same batch, same
// paths. rows path: the destination row is split at its 16-B boundary - at
// most one head element and at most three tail elements are stored singly by
// predicated lanes - and the body goes in units of four doubles, two aligned
// 16-B stores fed by one 16-B load of four floats that promises only 4-B
// alignment (the rows of a compact staging buffer, or of a box inside a global
// array, start at any element). A lane issues SELECT_UNROLL such loads before
// it converts and stores any; a unit past the end of the row reloads the row's
// last unit (in bounds) and is not stored. The two stores of a unit are not
// issued by the lane that loaded it: 64 lanes storing 16 B at a pitch of 32 B
// fill half of every line an instruction touches, and the kernel then ran at
// 0.88 of copy3d's time instead of the 0.75 its bytes predict. So the lanes
// exchange floats in registers (ds_bpermute; no LDS is allocated) and every
// store instruction writes 64 contiguous pairs of doubles, 1 KiB: 0.78
// (profiles/scatter_g/NOTES.md). The body loop is therefore wave-uniform.
template <typename IDX>
__global__ void __launch_bounds__(BLOCK) select_widen_kernel(const WidenBatch batch) {
  const uint32_t b = blockIdx.x;
  int c = 0;
  while (c + 1 < batch.n && b >= batch.block_start[c + 1]) ++c;
  const WidenJob& J = batch.job[c];
  const uint32_t local = b - batch.block_start[c];
  const uint32_t nb = batch.block_start[c + 1] - batch.block_start[c];
  const float* __restrict__ src = J.src;
  double* __restrict__ dst = J.dst;
  const IDX c1 = static_cast<IDX>(J.c[1]), c2 = static_cast<IDX>(J.c[2]);
  if (J.rows) {
    const uint32_t lane = threadIdx.x & 63;
    const IDX nrows = static_cast<IDX>(J.c[0]) * c1;
    const IDX nw = static_cast<IDX>(nb) * WAVES;
    const IDX S0 = static_cast<IDX>(J.S[0]), S1 = static_cast<IDX>(J.S[1]);
    const IDX T0 = static_cast<IDX>(J.T[0]), T1 = static_cast<IDX>(J.T[1]);
    for (IDX row = static_cast<IDX>(local) * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); row < nrows;
         row += nw) {
      const IDX i0 = row / c1, i1 = row - i0 * c1;
      const float* s = src + (i0 * S0 + i1 * S1);
      double* d = dst + (i0 * T0 + i1 * T1);
      // the element before the destination row's first 16-B boundary, if any
      IDX h = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(d) >> 3) & 1u;
      if (h > c2) h = c2;
      const IDX nvec = (c2 - h) >> 2, tail = (c2 - h) & 3;
      const IDX t0 = h + (nvec << 2);
      if (lane < h) d[lane] = static_cast<double>(s[lane]);
      if (lane >= 32 && lane - 32 < tail) d[t0 + (lane - 32)] = static_cast<double>(s[t0 + (lane - 32)]);
      const float* sb = s + h;
      D2* db = reinterpret_cast<D2*>(d + h);
      const int half = lane >> 1;
      const bool odd = lane & 1;
      for (IDX ub = 0; ub < nvec; ub += 64 * U) {  // (wave-uniform: every lane takes part in the exchanges)
        F4 v[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const IDX u = ub + 64 * k + lane;
          v[k] = *reinterpret_cast<const F4e*>(sb + ((u < nvec ? u : nvec - 1) << 2));
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const IDX base = ub + 64 * k;  // the wave's 64 units: 128 pairs of doubles, stored 64 contiguous pairs at a time
#pragma unroll
          for (int hb = 0; hb < 2; ++hb) {
            const int from = 32 * hb + half;  // the lane that loaded this pair's unit
            const float x = __shfl(v[k].x, from, 64), y = __shfl(v[k].y, from, 64);
            const float z = __shfl(v[k].z, from, 64), w = __shfl(v[k].w, from, 64);
            if (base + from < nvec)
              db[2 * base + 64 * hb + lane] = D2{static_cast<double>(odd ? z : x), static_cast<double>(odd ? w : y)};
          }
        }
      }
    }
  } else {
    const IDX total = static_cast<IDX>(J.c[0]) * c1 * c2;
    const IDX stride = static_cast<IDX>(nb) * BLOCK;
    const IDX S0 = static_cast<IDX>(J.S[0]), S1 = static_cast<IDX>(J.S[1]), S2 = static_cast<IDX>(J.S[2]);
    const IDX T0 = static_cast<IDX>(J.T[0]), T1 = static_cast<IDX>(J.T[1]), T2 = static_cast<IDX>(J.T[2]);
    for (IDX e = static_cast<IDX>(local) * BLOCK + threadIdx.x; e < total; e += stride) {
      const IDX q = e / c2, i2 = e - q * c2;
      const IDX i0 = q / c1, i1 = q - i0 * c1;
      dst[i0 * T0 + i1 * T1 + i2 * T2] = static_cast<double>(src[i0 * S0 + i1 * S1 + i2 * S2]);
    }
  }
}

}  // namespace

void launch_select_widen(const WidenBatch& batch, bool wide, hipStream_t stream) {
  if (batch.n < 1 || batch.n > SELECT_MAX_JOBS) fail("select_widen: ", batch.n, " jobs in one launch");
  const uint32_t blocks = batch.block_start[batch.n];
  if (blocks == 0) return;
  if (wide)
    hipLaunchKernelGGL(select_widen_kernel<uint64_t>, dim3(blocks), dim3(BLOCK), 0, stream, batch);
  else
    hipLaunchKernelGGL(select_widen_kernel<uint32_t>, dim3(blocks), dim3(BLOCK), 0, stream, batch);
  IGG_HIP_CHECK(hipGetLastError());
}

void launch_select_convert(const SelectBatch& batch, bool wide, hipStream_t stream) {
  if (batch.n < 1 || batch.n > SELECT_MAX_JOBS) fail("select_convert: ", batch.n, " jobs in one launch");
  const uint32_t blocks = batch.block_start[batch.n];
  if (blocks == 0) return;
  if (wide)
    hipLaunchKernelGGL(select_convert_kernel<uint64_t>, dim3(blocks), dim3(BLOCK), 0, stream, batch);
  else
    hipLaunchKernelGGL(select_convert_kernel<uint32_t>, dim3(blocks), dim3(BLOCK), 0, stream, batch);
  IGG_HIP_CHECK(hipGetLastError());
}

}  // namespace igg
