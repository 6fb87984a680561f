// Reduction kernels for gfx950 (igg/reduce.hpp): sums, squares, products and
// maxima over boxes of f32 / f64 fields, accumulated in f64.
//
// Stage 1 reads every element of a box once: a tile is one load per lane
// (16 B on the flat and rows paths, one element on the element path), a
// workgroup issues REDUCE_UNROLL tiles per input before it consumes any, and
// walks its tiles grid-stride in a fixed order. Lanes outside the box load a
// safe address of the same job and are masked by SELECTS, never by arithmetic
// (what lies outside the box may be NaN). A wave combines by cross-lane moves,
// the four waves through LDS behind one barrier, and lane 0 stores the
// workgroup's partial (value, NaN flag) with one 16-B store. Stage 2 combines
// a job's partials in index order. fmax drops NaN, so the MAX-type ops carry
// the flag; sums propagate NaN on their own.
#include <hip/hip_runtime.h>

#include "igg/common.hpp"
#include "igg/reduce.hpp"
#include "igg/reduce_device.hpp"

namespace igg {
namespace {

constexpr int BLOCK = REDUCE_BLOCK;
constexpr int U = REDUCE_UNROLL;
constexpr int CAP = REDUCE_MAX_BLOCKS;
constexpr int WAVES = BLOCK / 64;

// Workgroup result in thread 0: lanes by cross-lane moves, waves through LDS.
template <bool MAXT>
__device__ inline void block_combine(double& r, bool& nan, double* sv, int* sf) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) r = combine<MAXT>(r, __shfl_down(r, off));
  nan = __any(nan) != 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sv[wave] = r;
    sf[wave] = nan ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    r = sv[0];
    nan = sf[0] != 0;
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
      r = combine<MAXT>(r, sv[w]);
      nan = nan || sf[w] != 0;
    }
  }
}

template <typename T, int VEC, int OP>
__global__ void __launch_bounds__(BLOCK) reduce_stage1_kernel(const ReduceBatch batch, D2* __restrict__ partials) {
  constexpr bool TWO = OP == R_DOT || OP == R_SUMSQ_DIFF || OP == R_MAXABS_DIFF;
  constexpr bool MAXT = OP == R_MAX || OP == R_MIN || OP == R_MAXABS || OP == R_MAXABS_DIFF;
  const double ident = MAXT ? -__builtin_inf() : 0.0;
  __shared__ double sv[WAVES];
  __shared__ int sf[WAVES];
  const uint32_t b = blockIdx.x;
  int c = 0;
  while (c + 1 < batch.n && b >= batch.block_start[c + 1]) ++c;
  const ReduceJob& J = batch.job[c];
  const uint32_t local = b - batch.block_start[c];
  const uint32_t lxl = J.lx_log2;
  const uint32_t tx = threadIdx.x & ((1u << lxl) - 1u), ty = threadIdx.x >> lxl;
  const uint32_t ly = static_cast<uint32_t>(BLOCK) >> lxl;
  const T* pa = static_cast<const T*>(J.a);
  const T* pb = static_cast<const T*>(J.b);
  const int64_t head = J.head;
  const uint32_t tiles = J.tiles, ncx = J.cx, ng1 = J.g1, n1 = J.n1, nv = J.nv;
  const int64_t n2 = J.n2;
  double acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = ident;
  bool nan = false;
  const uint32_t step = J.nblocks * U;
  for (uint32_t t0 = local * U; t0 < tiles; t0 += step) {
    uint32_t cx = t0 % ncx;
    const uint32_t q = t0 / ncx;
    uint32_t g1 = q % ng1, i0 = q / ng1;
    Pack<T, VEC> va[U], vb[U];
    uint32_t mask[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i1 = g1 * ly + ty;
      const uint32_t j = (cx << lxl) + tx;
      const int64_t pos0 = static_cast<int64_t>(j) * VEC - head;  // of the load's first element in its row
      uint32_t m = 0;
      if (t0 + u < tiles && i1 < n1 && j < nv) {
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (pos0 + e >= 0 && pos0 + e < n2) m |= 1u << e;
      }
      mask[u] = m;
      // (a lane without an element loads the job's first vector: in bounds, masked below)
      const int64_t oa = m ? static_cast<int64_t>(i0) * J.s[0] + static_cast<int64_t>(i1) * J.s[1] + pos0 * J.s[2]
                           : -head;
      va[u].load(pa + oa);
      if (TWO) {
        const int64_t ob = m ? static_cast<int64_t>(i0) * J.sb[0] + static_cast<int64_t>(i1) * J.sb[1] + pos0 * J.sb[2]
                             : -head;
        vb[u].load(pb + ob);
      }
      if (++cx == ncx) {
        cx = 0;
        if (++g1 == ng1) g1 = 0, ++i0;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const bool on = (mask[u] >> e) & 1u;
        const double t = term<OP>(va[u].get(e), TWO ? vb[u].get(e) : 0.0);
        if (MAXT) nan = nan || (on && t != t);
        acc[e] = combine<MAXT>(acc[e], on ? t : ident);
      }
    }
  }
  double r = acc[0];
#pragma unroll
  for (int e = 1; e < VEC; ++e) r = combine<MAXT>(r, acc[e]);
  block_combine<MAXT>(r, nan, sv, sf);
  if (threadIdx.x == 0) partials[static_cast<int64_t>(c) * CAP + local] = D2{r, nan ? 1.0 : 0.0};
}

__global__ void __launch_bounds__(BLOCK) reduce_stage2_kernel(const ReduceStage2 args, const D2* __restrict__ partials) {
  __shared__ double sv[WAVES];
  __shared__ int sf[WAVES];
  const int job = blockIdx.x;
  const uint32_t nb = args.nblocks[job];
  const D2* p = partials + static_cast<int64_t>(job) * CAP;
  const bool maxt = args.max_type != 0;
  double r = maxt ? -__builtin_inf() : 0.0;
  bool nan = false;
  for (uint32_t i = threadIdx.x; i < nb; i += BLOCK) {
    const D2 v = p[i];
    r = maxt ? __builtin_fmax(r, v.x) : r + v.x;
    nan = nan || v.y != 0.0;
  }
  if (maxt) block_combine<true>(r, nan, sv, sf);
  else block_combine<false>(r, nan, sv, sf);
  if (threadIdx.x == 0) {
    if (!maxt) {
      args.out[job] = r;
    } else if (args.flags) {
      args.out[job] = r;  // fmax dropped every NaN: a finite value or -inf
      args.flags[job] = nan ? 1.0 : 0.0;
    } else {
      const double v = nan ? __builtin_nan("") : r;
      args.out[job] = args.negate ? -v : v;
    }
  }
}

template <typename T, int VEC, int OP>
void launch1(const ReduceBatch& batch, void* partials, hipStream_t stream) {
  const uint32_t blocks = batch.block_start[batch.n];
  hipLaunchKernelGGL((reduce_stage1_kernel<T, VEC, OP>), dim3(blocks), dim3(BLOCK), 0, stream, batch,
                     static_cast<D2*>(partials));
}

template <typename T, int VEC>
void launch_op(int op, const ReduceBatch& batch, void* partials, hipStream_t stream) {
  switch (op) {
    case R_SUM: launch1<T, VEC, R_SUM>(batch, partials, stream); break;
    case R_SUMSQ: launch1<T, VEC, R_SUMSQ>(batch, partials, stream); break;
    case R_MAX: launch1<T, VEC, R_MAX>(batch, partials, stream); break;
    case R_MIN: launch1<T, VEC, R_MIN>(batch, partials, stream); break;
    case R_MAXABS: launch1<T, VEC, R_MAXABS>(batch, partials, stream); break;
    case R_DOT: launch1<T, VEC, R_DOT>(batch, partials, stream); break;
    case R_SUMSQ_DIFF: launch1<T, VEC, R_SUMSQ_DIFF>(batch, partials, stream); break;
    case R_MAXABS_DIFF: launch1<T, VEC, R_MAXABS_DIFF>(batch, partials, stream); break;
    default: fail("reduce: unknown op ", op);
  }
}

}  // namespace

void launch_reduce_stage1(int op, int elem_size, bool vector_loads, const ReduceBatch& batch, void* partials,
                          hipStream_t stream) {
  if (batch.n < 1 || batch.n > REDUCE_MAX_JOBS) fail("reduce: ", batch.n, " jobs in one launch");
  for (int k = 0; k < batch.n; ++k)
    if (batch.job[k].nblocks > static_cast<uint32_t>(CAP)) fail("reduce: job over the block cap");
  if (elem_size == 4) {
    if (vector_loads) launch_op<float, 4>(op, batch, partials, stream);
    else launch_op<float, 1>(op, batch, partials, stream);
  } else if (elem_size == 8) {
    if (vector_loads) launch_op<double, 2>(op, batch, partials, stream);
    else launch_op<double, 1>(op, batch, partials, stream);
  } else {
    fail("reduce: 4- or 8-byte elements (got ", elem_size, ")");
  }
  IGG_HIP_CHECK(hipGetLastError());
}

void launch_reduce_stage2(const ReduceStage2& args, const void* partials, hipStream_t stream) {
  if (args.n < 1 || args.n > REDUCE_MAX_JOBS) fail("reduce: ", args.n, " jobs in one launch");
  hipLaunchKernelGGL(reduce_stage2_kernel, dim3(static_cast<unsigned>(args.n)), dim3(BLOCK), 0, stream, args,
                     static_cast<const D2*>(partials));
  IGG_HIP_CHECK(hipGetLastError());
}

}  // namespace igg
