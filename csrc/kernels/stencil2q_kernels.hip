// Specialisations of the two-step diffusion pass (body: igg/stencil2_impl.hpp;
// scheme: stencil2_kernels.hip, which holds the general kernels and sends
// these cases here):
//   NOZ  the tile spans the row (n2 <= tile width, one tile along z): no z
//        ring, so the edge threads and the tile index along z are compiled out;
//   QIN  the pass reads Q = dtlam/Cp (launch_quotient, below) where the general
//        kernel reads Cp and divides: the same bytes, no division, and the
//        quotient of a plane is its loaded registers.
// All of them leave bitwise the values of the general kernel.
#include <hip/hip_runtime.h>

#include "igg/stencil2_impl.hpp"

namespace igg {
namespace {

using twostep::K2Args;

template <typename T, int BY, int RY, int VZ, int BZ, bool NOZ, bool QIN>
__global__ void __launch_bounds__(64 * BY * BZ)
diffusion3d_twostep_x_kernel(const K2Args<T> a) {
  twostep::body<T, BY, RY, VZ, BZ, NOZ, QIN>(a);
}

template <typename T, int BY, int RY, int BZ>
void launch_special(const DiffusionArgs& a, hipStream_t stream) {
  constexpr int VZ = 16 / static_cast<int>(sizeof(T));
  const bool noz = a.n[2] <= twostep::tile_width<T, BZ>(), qin = a.q != 0;
  if (noz && qin)
    twostep::launch_form<T, BY, RY, BZ>(&diffusion3d_twostep_x_kernel<T, BY, RY, VZ, BZ, true, true>, a, true, stream);
  else if (noz)
    twostep::launch_form<T, BY, RY, BZ>(&diffusion3d_twostep_x_kernel<T, BY, RY, VZ, BZ, true, false>, a, false, stream);
  else if (qin)
    twostep::launch_form<T, BY, RY, BZ>(&diffusion3d_twostep_x_kernel<T, BY, RY, VZ, BZ, false, true>, a, true, stream);
  else
    fail("diffusion3d_twostep: the general kernel runs this case");
}

template <typename T>
void dispatch_special(const DiffusionArgs& a, hipStream_t s) {
  switch (a.form) {  // the forms of stencil2_kernels.hip
    case 0: launch_special<T, 2, 4, 4>(a, s); break;
    case 1: launch_special<T, 4, 4, 2>(a, s); break;
    case 2: launch_special<T, 4, 4, 1>(a, s); break;
    default: fail("diffusion3d_twostep: no form ", a.form);
  }
}

// q = dtlam / cp: the expression of the pass, one 16-byte vector per thread
// and a scalar tail.
template <typename T, int VZ>
__global__ void __launch_bounds__(256) quotient_kernel(T* __restrict__ q, const T* __restrict__ cp, int64_t n, T dtlam) {
  using V = typename twostep::Vec2<T, VZ>::type;
  const int64_t nv = n / VZ;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < nv) {
    const V c = reinterpret_cast<const V*>(cp)[i];
    V r;
#pragma unroll
    for (int e = 0; e < VZ; ++e) r[e] = dtlam / c[e];
    reinterpret_cast<V*>(q)[i] = r;
  } else if (i - nv < n - nv * VZ) {
    const int64_t j = nv * VZ + (i - nv);
    q[j] = dtlam / cp[j];
  }
}

template <typename T>
void launch_quotient_t(uintptr_t q, uintptr_t cp, int64_t n, double dt_lam, hipStream_t stream) {
  constexpr int VZ = 16 / static_cast<int>(sizeof(T));
  const int64_t threads = n / VZ + n % VZ;
  const int64_t blocks = (threads + 255) / 256;
  if (blocks > 0x7fffffffLL) fail("quotient: grid too large");
  hipLaunchKernelGGL((quotient_kernel<T, VZ>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream,
                     reinterpret_cast<T*>(q), reinterpret_cast<const T*>(cp), n, static_cast<T>(dt_lam));
  IGG_HIP_CHECK(hipGetLastError());
}

}  // namespace

void launch_diffusion3d_twostep_special(const DiffusionArgs& a, hipStream_t stream) {
  if (a.elem_bytes == 8) dispatch_special<double>(a, stream);
  else dispatch_special<float>(a, stream);
}

void launch_quotient(uintptr_t q, uintptr_t cp, int64_t n, double dt_lam, int elem_bytes, hipStream_t stream) {
  if (elem_bytes != 4 && elem_bytes != 8) fail("quotient: ", elem_bytes, " bytes per element");
  if (n <= 0) return;
  if ((q | cp) % 16 != 0) fail("quotient: arrays must be 16-byte aligned");
  if (elem_bytes == 8) launch_quotient_t<double>(q, cp, n, dt_lam, stream);
  else launch_quotient_t<float>(q, cp, n, dt_lam, stream);
}

}  // namespace igg
