// Projection kernels for gfx950 (igg/project.hpp): reduce a box of an f32 /
// f64 field over some of its axes and keep the others, accumulated in f64.
//
// Stage 1 reads every element of the box once, in one of two families
// (igg/project_plan.hpp). Inner axis kept: a lane owns the outputs of its
// load, walks its slice of the reduced range with PROJECT_UNROLL1 loads per
// input in flight (twice as many for a one-input op) and never meets another
// lane; elements of the head and tail loads that lie outside the row are
// accumulated like the others and NOT stored (what lies outside the box may be
// NaN: it reaches no output). Inner axis reduced: a group of lanes lies along
// a row and walks the tiles of one (slice, output) pair; lanes outside the row
// load the first load of the same output and are masked by SELECTS, never by
// arithmetic; the group combines by cross-lane moves, and through LDS where it
// spans waves. Both walk in batches of U independent loads and finish with
// batches of U/2, U/4 .. 1, so a short range is still one round of loads.
// Each (slice, output) pair stores one partial (value, NaN flag) with one 16-B
// store: fmax drops NaN, so the MAX-type ops carry the flag; sums propagate
// NaN on their own. Stage 2 writes every cell of the global-shaped
// destination: the slices of a cell of this box combined in index order, the
// identity elsewhere. Offsets inside the loops are 32-bit where the plan
// proved that they fit, 64-bit otherwise.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "igg/common.hpp"
#include "igg/project.hpp"
#include "igg/reduce_device.hpp"

namespace igg {
namespace {

constexpr int BLOCK = PROJECT_BLOCK;
constexpr int WAVES = BLOCK / 64;

template <int OP>
struct OpKind {
  static constexpr bool two = OP == R_DOT || OP == R_SUMSQ_DIFF || OP == R_MAXABS_DIFF;
  static constexpr bool maxt = OP == R_MAX || OP == R_MIN || OP == R_MAXABS || OP == R_MAXABS_DIFF;
};

// Family 1: slots [KO, R0, R1, KI], lanes along KI.
template <typename T, int VEC, int OP, typename I>
__global__ void __launch_bounds__(BLOCK) project_keep_inner_kernel(const ProjectJob J, D2* __restrict__ partials) {
  constexpr bool TWO = OpKind<OP>::two, MAXT = OpKind<OP>::maxt;
  constexpr int U = TWO ? PROJECT_UNROLL1 : 2 * PROJECT_UNROLL1;  // loads in flight per lane: the same bytes
  const double ident = MAXT ? -__builtin_inf() : 0.0;
  const uint32_t lxl = J.lanes_log2;
  const uint32_t tx = threadIdx.x & ((1u << lxl) - 1u), ty = threadIdx.x >> lxl;
  const uint32_t ly = static_cast<uint32_t>(BLOCK) >> lxl;
  const T* pa = static_cast<const T*>(J.a);
  const T* pb = static_cast<const T*>(J.b);
  const int64_t head = J.head, nki = J.n[3], nr1 = J.n[2];
  const I sr1 = static_cast<I>(J.s[2]), sr1b = static_cast<I>(J.sb[2]);
  const I wrap = static_cast<I>(J.s[1] - nr1 * J.s[2]), wrapb = static_cast<I>(J.sb[1] - nr1 * J.sb[2]);
  for (uint32_t bu = blockIdx.x; bu < J.block_units; bu += gridDim.x) {
    const uint32_t cx = bu % J.cx, gy = bu / J.cx;
    const uint32_t j = (cx << lxl) + tx, unit = gy * ly + ty;
    if (j >= J.nv || unit >= J.units) continue;  // (no lane waits for another in this kernel)
    const uint32_t ko = unit / J.slices, sl = unit % J.slices;
    // (one slice: no 64-bit division per unit)
    const int64_t rb = J.slices == 1 ? 0 : static_cast<int64_t>(sl) * J.reduced / J.slices;
    const int64_t re = J.slices == 1 ? J.reduced : static_cast<int64_t>(sl + 1) * J.reduced / J.slices;
    const int64_t pos0 = static_cast<int64_t>(j) * VEC - head;  // of the load's first element in its row
    const T* la = pa + static_cast<int64_t>(ko) * J.s[0] + pos0 * J.s[3];
    const T* lb = pb + static_cast<int64_t>(ko) * J.sb[0] + pos0 * J.sb[3];
    I r1 = 0, off = 0, offb = 0;
    if (rb != 0) {
      r1 = static_cast<I>(rb % nr1);
      off = static_cast<I>((rb / nr1) * J.s[1] + (rb % nr1) * J.s[2]);
      offb = static_cast<I>((rb / nr1) * J.sb[1] + (rb % nr1) * J.sb[2]);
    }
    double acc[VEC];
    bool nan[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = ident, nan[e] = false;
    // N independent loads, then their terms
    auto batch = [&](auto width) {
      constexpr int N = decltype(width)::value;
      Pack<T, VEC> va[N], vb[N];
#pragma unroll
      for (int u = 0; u < N; ++u) {
        va[u].load(la + off);
        if (TWO) vb[u].load(lb + offb);
        off += sr1, offb += sr1b;
        if (++r1 == static_cast<I>(nr1)) r1 = 0, off += wrap, offb += wrapb;
      }
#pragma unroll
      for (int u = 0; u < N; ++u) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const double t = term<OP>(va[u].get(e), TWO ? vb[u].get(e) : 0.0);
          if (MAXT) nan[e] = nan[e] || t != t;
          acc[e] = combine<MAXT>(acc[e], t);
        }
      }
    };
    I left = static_cast<I>(re - rb);
    for (; left >= U; left -= U) batch(std::integral_constant<int, U>{});
    if (U > 8 && (left & 8)) batch(std::integral_constant<int, 8>{});
    if (U > 4 && (left & 4)) batch(std::integral_constant<int, 4>{});
    if (left & 2) batch(std::integral_constant<int, 2>{});
    if (left & 1) batch(std::integral_constant<int, 1>{});
    D2* out = partials + static_cast<int64_t>(sl) * J.nout + static_cast<int64_t>(ko) * nki;
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      if (pos0 + e >= 0 && pos0 + e < nki) out[pos0 + e] = D2{acc[e], nan[e] ? 1.0 : 0.0};
  }
}

// Family 2: slots [K0, K1, RO, RI], a group of lanes along RI.
template <typename T, int VEC, int OP, typename I>
__global__ void __launch_bounds__(BLOCK) project_reduce_inner_kernel(const ProjectJob J, D2* __restrict__ partials) {
  constexpr bool TWO = OpKind<OP>::two, MAXT = OpKind<OP>::maxt;
  constexpr int U = TWO ? PROJECT_UNROLL2 : 2 * PROJECT_UNROLL2;  // loads in flight per lane: the same bytes
  const double ident = MAXT ? -__builtin_inf() : 0.0;
  __shared__ double sv[WAVES];
  __shared__ int sf[WAVES];
  const uint32_t gl = J.lanes_log2;
  const uint32_t lane = threadIdx.x & ((1u << gl) - 1u), grp = threadIdx.x >> gl;
  const uint32_t gpb = static_cast<uint32_t>(BLOCK) >> gl;
  const T* pa = static_cast<const T*>(J.a);
  const T* pb = static_cast<const T*>(J.b);
  const I head = static_cast<I>(J.head), nri = static_cast<I>(J.n[3]);
  const I sro = static_cast<I>(J.s[2]), srob = static_cast<I>(J.sb[2]);
  const I sri = static_cast<I>(J.s[3]), srib = static_cast<I>(J.sb[3]);
  const uint32_t ncx = J.cx, nv = J.nv, nout = static_cast<uint32_t>(J.nout), nk1 = static_cast<uint32_t>(J.n[1]);
  for (uint32_t bu = blockIdx.x; bu < J.block_units; bu += gridDim.x) {
    const uint32_t unit = bu * gpb + grp;
    const bool live = unit < J.units;  // (a group without a unit walks no tile and stores nothing)
    const uint32_t sl = live ? unit / nout : 0u, o = live ? unit % nout : 0u;
    const uint32_t k0 = o / nk1, k1 = o % nk1;
    // (one slice: no 64-bit division per unit - an output of K.K.R is one short row)
    int64_t tb = 0, te = live ? J.reduced : 0;
    if (J.slices != 1 && live) {
      tb = static_cast<int64_t>(sl) * J.reduced / J.slices;
      te = static_cast<int64_t>(sl + 1) * J.reduced / J.slices;
    }
    const T* la = pa + static_cast<int64_t>(k0) * J.s[0] + static_cast<int64_t>(k1) * J.s[1];
    const T* lb = pb + static_cast<int64_t>(k0) * J.sb[0] + static_cast<int64_t>(k1) * J.sb[1];
    I ro = 0;
    uint32_t c = 0;
    if (tb != 0) ro = static_cast<I>(tb / ncx), c = static_cast<uint32_t>(tb % ncx);
    double acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = ident;
    bool nan = false;
    // one tile: the lane's load of row `ro`, chunk `c` (a lane past the row's end loads the output's first
    // load - in bounds - and is masked), then on to the next tile
    auto load_tile = [&](Pack<T, VEC>& va, Pack<T, VEC>& vb, uint32_t& mask) {
      const uint32_t j = (c << gl) + lane;
      const I pos0 = static_cast<I>(j) * VEC - head;  // of the load's first element in its row
      uint32_t m = 0;
      if (j < nv) {
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (pos0 + e >= 0 && pos0 + e < nri) m |= 1u << e;
      }
      mask = m;
      va.load(la + (m ? ro * sro + pos0 * sri : -head));
      if (TWO) vb.load(lb + (m ? ro * srob + pos0 * srib : -head));
      if (++c == ncx) c = 0, ++ro;
    };
    auto consume = [&](const Pack<T, VEC>& va, const Pack<T, VEC>& vb, uint32_t mask) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const bool on = (mask >> e) & 1u;
        const double t = term<OP>(va.get(e), TWO ? vb.get(e) : 0.0);
        if (MAXT) nan = nan || (on && t != t);
        acc[e] = combine<MAXT>(acc[e], on ? t : ident);  // a select: what lies outside the row may be NaN
      }
    };
    auto batch = [&](auto width) {
      constexpr int N = decltype(width)::value;
      Pack<T, VEC> va[N], vb[N];
      uint32_t mask[N];
#pragma unroll
      for (int u = 0; u < N; ++u) load_tile(va[u], vb[u], mask[u]);
#pragma unroll
      for (int u = 0; u < N; ++u) consume(va[u], vb[u], mask[u]);
    };
    int64_t left = te - tb;
    for (; left >= U; left -= U) batch(std::integral_constant<int, U>{});
    if (U > 4 && (left & 4)) batch(std::integral_constant<int, 4>{});
    if (left & 2) batch(std::integral_constant<int, 2>{});
    if (left & 1) batch(std::integral_constant<int, 1>{});
    double r = acc[0];
#pragma unroll
    for (int e = 1; e < VEC; ++e) r = combine<MAXT>(r, acc[e]);
    int nf = nan ? 1 : 0;
    // the group: cross-lane moves inside a wave (a group of at most 64 lanes is aligned in its wave) ...
    for (uint32_t w = (gl > 6 ? 64u : (1u << gl)) >> 1; w > 0; w >>= 1) {
      r = combine<MAXT>(r, __shfl_xor(r, static_cast<int>(w)));
      nf |= __shfl_xor(nf, static_cast<int>(w));
    }
    if (gl > 6) {  // ... and its waves through LDS, in wave order (the same branch in every lane of the workgroup)
      const uint32_t wave = threadIdx.x >> 6, wpg = 1u << (gl - 6);
      if ((threadIdx.x & 63u) == 0) sv[wave] = r, sf[wave] = nf;
      __syncthreads();
      if (lane == 0) {
        r = sv[grp * wpg];
        nf = sf[grp * wpg];
        for (uint32_t w = 1; w < wpg; ++w) {
          r = combine<MAXT>(r, sv[grp * wpg + w]);
          nf |= sf[grp * wpg + w];
        }
      }
      __syncthreads();  // before the next unit's waves store
    }
    if (live && lane == 0) partials[static_cast<int64_t>(sl) * nout + o] = D2{r, nf ? 1.0 : 0.0};
  }
}

__global__ void __launch_bounds__(BLOCK) project_stage2_kernel(const ProjectStage2 A, const D2* __restrict__ partials) {
  const int64_t c = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (c >= A.extent[0] * A.extent[1]) return;
  const int64_t g0 = c / A.extent[1], g1 = c % A.extent[1];
  int64_t i0 = g0 - A.start[0], i1 = g1 - A.start[1];
  if (i0 < 0) i0 += A.extent[0];  // the box wraps past the periodic extent
  if (i1 < 0) i1 += A.extent[1];
  const bool maxt = A.max_type != 0;
  double r = maxt ? -__builtin_inf() : 0.0;
  bool nan = false;
  if (i0 < A.own[0] && i1 < A.own[1]) {
    const D2* p = partials + i0 * A.pstride[0] + i1 * A.pstride[1];
    for (uint32_t s = 0; s < A.slices; ++s) {
      const D2 v = p[static_cast<int64_t>(s) * A.nout];
      r = maxt ? __builtin_fmax(r, v.x) : r + v.x;
      nan = nan || v.y != 0.0;
    }
  }
  const int64_t at = g0 * A.stride[0] + g1 * A.stride[1];
  if (!maxt) {
    A.dst[at] = r;
  } else if (A.flags) {
    A.dst[at] = r;  // fmax dropped every NaN: a finite value or -inf
    A.flags[at] = nan ? 1.0 : 0.0;
  } else {
    const double v = nan ? __builtin_nan("") : r;
    A.dst[at] = A.negate ? -v : v;
  }
}

template <typename T, int VEC, typename I, int OP>
void launch1(const ProjectPlan& plan, const ProjectJob& job, void* partials, hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(plan.blocks)), block(BLOCK);
  if (plan.family == 1)
    hipLaunchKernelGGL((project_keep_inner_kernel<T, VEC, OP, I>), grid, block, 0, stream, job,
                       static_cast<D2*>(partials));
  else
    hipLaunchKernelGGL((project_reduce_inner_kernel<T, VEC, OP, I>), grid, block, 0, stream, job,
                       static_cast<D2*>(partials));
}

template <typename T, int VEC, typename I>
void launch_op(int op, const ProjectPlan& plan, const ProjectJob& job, void* partials, hipStream_t stream) {
  switch (op) {
    case R_SUM: launch1<T, VEC, I, R_SUM>(plan, job, partials, stream); break;
    case R_SUMSQ: launch1<T, VEC, I, R_SUMSQ>(plan, job, partials, stream); break;
    case R_MAX: launch1<T, VEC, I, R_MAX>(plan, job, partials, stream); break;
    case R_MIN: launch1<T, VEC, I, R_MIN>(plan, job, partials, stream); break;
    case R_MAXABS: launch1<T, VEC, I, R_MAXABS>(plan, job, partials, stream); break;
    case R_DOT: launch1<T, VEC, I, R_DOT>(plan, job, partials, stream); break;
    case R_SUMSQ_DIFF: launch1<T, VEC, I, R_SUMSQ_DIFF>(plan, job, partials, stream); break;
    case R_MAXABS_DIFF: launch1<T, VEC, I, R_MAXABS_DIFF>(plan, job, partials, stream); break;
    default: fail("project: unknown op ", op);
  }
}

template <typename T, int VEC>
void launch_width(int op, const ProjectPlan& plan, const ProjectJob& job, void* partials, hipStream_t stream) {
  if (plan.vector && plan.index_bits == 32) launch_op<T, VEC, int32_t>(op, plan, job, partials, stream);
  else if (plan.vector) launch_op<T, VEC, int64_t>(op, plan, job, partials, stream);
  else launch_op<T, 1, int64_t>(op, plan, job, partials, stream);
}

}  // namespace

void launch_project_stage1(int op, int elem_size, const ProjectPlan& plan, const ProjectJob& job, void* partials,
                           hipStream_t stream) {
  if (plan.blocks < 1 || plan.blocks > PROJECT_MAX_BLOCKS) fail("project: ", plan.blocks, " workgroups");
  if (elem_size == 4) launch_width<float, 4>(op, plan, job, partials, stream);
  else if (elem_size == 8) launch_width<double, 2>(op, plan, job, partials, stream);
  else fail("project: 4- or 8-byte elements (got ", elem_size, ")");
  IGG_HIP_CHECK(hipGetLastError());
}

void launch_project_stage2(const ProjectStage2& args, const void* partials, hipStream_t stream) {
  const int64_t cells = args.extent[0] * args.extent[1];
  if (cells < 1) return;
  const int64_t blocks = (cells + BLOCK - 1) / BLOCK;
  if (blocks > 0x7fffffffLL) fail("project: destination too large (", cells, " cells)");
  hipLaunchKernelGGL(project_stage2_kernel, dim3(static_cast<unsigned>(blocks)), dim3(BLOCK), 0, stream, args,
                     static_cast<const D2*>(partials));
  IGG_HIP_CHECK(hipGetLastError());
}

}  // namespace igg
