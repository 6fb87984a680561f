// Adjoint of the 2-D staggered acoustic step for gfx950 (igg/acoustic_adj.hpp):
//   (gP2, gVx2, gVy2) -> (gP, gVx, gVy) = S^T (gP2, gVx2, gVy2)
// The transpose is again a staggered leapfrog with the forward step's data
// flow (r in the part of P2), so it takes the forward vector-march layout
// (acoustic_kernels.hip acoustic2d_vmarch_kernel): 64 lanes of one 16-byte
// vector (VJ = 4 float32, 2 float64), 62 owned vectors plus one halo vector on
// each side, a wave marches CH rows of x. Row i loads gP2(i), gVx2(i+1) and
// gVy2(i); gVx2(i) and r(i-1) are carried in registers; wy(j+1) and r(j-1)
// come from the lane's own vector or one lane shuffle; the next row's loads
// are issued before the current row is computed. A chunk recomputes r of the
// row before its first (values only, nothing stored), and row nx writes
// gVx(nx) from the carried r(nx-1). Three arrays read, three written.
//   * Addresses are a wave-uniform 64-bit row base plus a 32-bit lane offset.
//   * gP / gVx rows (pitch ny, ny % VJ == 0) are aligned vectors, stored
//     non-temporally; gVy rows have pitch ny+1, so they use element-aligned
//     vectors and the lane that starts at column ny does that column singly.
//   * A value outside the array is never loaded: lanes past the row alias its
//     last vector (clamped address) and every zero (w on boundary faces, r
//     outside the cells) is a select, never a product.
// The same kernel with one point per lane (VJ = 1, 62 owned columns) runs the
// rows the vector form cannot: ny % VJ != 0 or ny < 2*VJ. No LDS, no atomics,
// no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "igg/acoustic.hpp"
#include "igg/acoustic_adj.hpp"
#include "igg/common.hpp"

namespace igg {
namespace {

constexpr int ADJ_WAVES = 4;      // waves per workgroup
constexpr int64_t ADJ_CH = 2;     // rows of i per wave (swept 2..16: profiles/acoustic_adjoint/NOTES.md)

template <typename T>
struct AcAdjArgs {
  T* __restrict__ gp;
  T* __restrict__ gvx;
  T* __restrict__ gvy;
  const T* __restrict__ gp2;
  const T* __restrict__ gvx2;
  const T* __restrict__ gvy2;
  int64_t nx, ny, ch;
  T a, b, rdx, rdy;  // dt*K, dt/rho, 1/dx, 1/dy
};

template <typename T, int VJ>
struct AcVec {
  typedef T type __attribute__((ext_vector_type(VJ)));
  typedef T utype __attribute__((ext_vector_type(VJ), aligned(sizeof(T))));  // element aligned
};
template <typename T>
struct AcVec<T, 1> {
  struct type {
    T v;
    __device__ __forceinline__ T& operator[](int) { return v; }
    __device__ __forceinline__ const T& operator[](int) const { return v; }
  };
  typedef type utype;
};

template <typename T, int VJ>
__device__ __forceinline__ typename AcVec<T, VJ>::type ac_zero() {
  typename AcVec<T, VJ>::type v;
#pragma unroll
  for (int e = 0; e < VJ; ++e) v[e] = T(0);
  return v;
}
template <typename T, int VJ>
__device__ __forceinline__ typename AcVec<T, VJ>::type ac_load(const T* p) {
  return *reinterpret_cast<const typename AcVec<T, VJ>::type*>(p);
}
template <typename T, int VJ>
__device__ __forceinline__ typename AcVec<T, VJ>::type ac_load_u(const T* p) {
  return *reinterpret_cast<const typename AcVec<T, VJ>::utype*>(p);
}
template <typename T, int VJ>
__device__ __forceinline__ void ac_store(T* p, const typename AcVec<T, VJ>::type& v) {
  *reinterpret_cast<typename AcVec<T, VJ>::type*>(p) = v;
}
template <typename T, int VJ>
__device__ __forceinline__ void ac_store_u(T* p, const typename AcVec<T, VJ>::type& v) {
  *reinterpret_cast<typename AcVec<T, VJ>::utype*>(p) = v;
}
template <typename T, int VJ>
__device__ __forceinline__ void ac_store_nt(T* p, const typename AcVec<T, VJ>::type& v) {
  if constexpr (VJ == 1) {
    __builtin_nontemporal_store(v.v, p);
  } else {
    __builtin_nontemporal_store(v, reinterpret_cast<typename AcVec<T, VJ>::type*>(p));
  }
}

template <typename T, int VJ>
__global__ void __launch_bounds__(64 * ADJ_WAVES) acoustic2d_adjoint_kernel(const AcAdjArgs<T> a) {
  // No FMA contraction: a chunk's recomputed r(i0-1) must equal, bit for bit,
  // what the chunk before it formed in its loop, and both the host twin's.
#pragma clang fp contract(off)
  using V = typename AcVec<T, VJ>::type;
  constexpr int64_t OWNV = 62 * VJ;
  const int lane = threadIdx.x & 63;
  const int64_t wave =
      static_cast<int64_t>(blockIdx.x) * ADJ_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nx = a.nx, ny = a.ny, sy = ny + 1;
  const int64_t nseg = (ny + 1 + OWNV - 1) / OWNV;
  const int64_t seg = wave % nseg, chunk = wave / nseg;
  const int64_t i0 = chunk * a.ch;
  if (i0 > nx) return;  // wave-uniform
  const int64_t i1 = min(i0 + a.ch, nx + 1);
  const int64_t j0 = seg * OWNV + static_cast<int64_t>(lane - 1) * VJ;  // first column of this lane
  const bool own = lane >= 1 && lane <= 62 && j0 <= ny;
  const bool cells = j0 >= 0 && j0 + VJ <= ny;  // VJ cell / x-face columns
  const bool last = j0 == ny;                   // only the boundary y-face column ny
  // wave-uniform first column the wave touches (seg * OWNV <= ny, so jb <= ny - VJ)
  // and the lane's clamped vector start relative to it
  const int64_t jb = max<int64_t>(seg * OWNV - VJ, 0);
  const unsigned jo = static_cast<unsigned>(min<int64_t>(max<int64_t>(j0, 0), ny - VJ) - jb);
  bool yin[VJ];  // element is an inner y-face column
#pragma unroll
  for (int e = 0; e < VJ; ++e) yin[e] = j0 + e >= 1 && j0 + e <= ny - 1;

  const T* __restrict__ gp2 = a.gp2;
  const T* __restrict__ gvx2 = a.gvx2;
  const T* __restrict__ gvy2 = a.gvy2;
  const T ca = a.a, cb = a.b, rdx = a.rdx, rdy = a.rdy;

  auto ldc = [&](const T* base, int64_t row) { return ac_load<T, VJ>(base + (row * ny + jb) + jo); };
  auto ldy = [&](int64_t row) {  // gVy2(row, j0..j0+VJ-1); the column-ny lane holds gVy2(row, ny) in element 0
    V v = ac_load_u<T, VJ>(gvy2 + (row * sy + jb) + jo);
    if (last) {
      v = ac_zero<T, VJ>();
      v[0] = gvy2[row * sy + ny];
    }
    return v;
  };
  auto x_inner = [&](int64_t i) { return i >= 1 && i <= nx - 1; };
  auto wx_of = [&](const V& g, int64_t i) {
    V w;
    const bool in = x_inner(i);
#pragma unroll
    for (int e = 0; e < VJ; ++e) w[e] = acadj_w(g[e], cb, rdx, in);
    return w;
  };
  // r of the lane's cells from the row's gP2, wx above and below and gVy2;
  // 0 in the lanes that hold no cells.
  auto r_of = [&](const V& gp, const V& wx_hi, const V& wx_lo, const V& gy) {
    V wy, r;
#pragma unroll
    for (int e = 0; e < VJ; ++e) wy[e] = acadj_w(gy[e], cb, rdy, yin[e]);
    const T up = __shfl_down(wy[0], 1);
#pragma unroll
    for (int e = 0; e < VJ; ++e) {
      const T wy_hi = e + 1 < VJ ? wy[e + 1 < VJ ? e + 1 : e] : up;
      const T v = acadj_r(gp[e], wx_hi[e], wx_lo[e], wy_hi, wy[e]);
      r[e] = cells ? v : T(0);
    }
    return r;
  };

  // Row state: gVx2(i) and its w, r(i-1).
  V gx_i = ldc(gvx2, i0);
  V wx_i = wx_of(gx_i, i0);
  V r_prev = ac_zero<T, VJ>();
  if (i0 >= 1) {
    const V gy = ldy(i0 - 1), gxp = ldc(gvx2, i0 - 1), gpp = ldc(gp2, i0 - 1);
    r_prev = r_of(gpp, wx_i, wx_of(gxp, i0 - 1), gy);
  }
  // Prefetched loads of row i.
  V gy = ac_zero<T, VJ>(), gx_n = ac_zero<T, VJ>(), gpc = ac_zero<T, VJ>();
  if (i0 < nx) {
    gy = ldy(i0);
    gx_n = ldc(gvx2, i0 + 1);
    gpc = ldc(gp2, i0);
  }
  for (int64_t i = i0; i < i1; ++i) {
    if (i < nx) {
      V gy1 = ac_zero<T, VJ>(), gx_n1 = ac_zero<T, VJ>(), gpc1 = ac_zero<T, VJ>();
      if (i + 1 < nx && i + 1 < i1) {  // prefetch row i+1
        gy1 = ldy(i + 1);
        gx_n1 = ldc(gvx2, i + 2);
        gpc1 = ldc(gp2, i + 1);
      }
      const V wx_n = wx_of(gx_n, i + 1);
      const V r = r_of(gpc, wx_n, wx_i, gy);
      const T rl_lane = __shfl_up(r[VJ - 1], 1);  // r(i, j0-1); 0 from a lane without cells
      if (own) {
        V gvyo;
#pragma unroll
        for (int e = 0; e < VJ; ++e) {
          const T rl = e == 0 ? rl_lane : r[e > 0 ? e - 1 : 0];
          gvyo[e] = acadj_v(gy[e], ca, r[e], rl, rdy);
        }
        if (cells) {
          V gvxo;
#pragma unroll
          for (int e = 0; e < VJ; ++e) gvxo[e] = acadj_v(gx_i[e], ca, r[e], r_prev[e], rdx);
          ac_store_nt<T, VJ>(a.gp + (i * ny + jb) + jo, r);
          ac_store_nt<T, VJ>(a.gvx + (i * ny + jb) + jo, gvxo);
          ac_store_u<T, VJ>(a.gvy + (i * sy + jb) + jo, gvyo);
        } else if (last) {
          a.gvy[i * sy + ny] = gvyo[0];  // r(i, ny) = 0
        }
      }
      gx_i = gx_n;
      wx_i = wx_n;
      r_prev = r;
      gy = gy1;
      gx_n = gx_n1;
      gpc = gpc1;
    } else if (own && cells) {  // i == nx: r(nx) = 0
      V gvxo;
#pragma unroll
      for (int e = 0; e < VJ; ++e) gvxo[e] = acadj_v(gx_i[e], ca, T(0), r_prev[e], rdx);
      ac_store<T, VJ>(a.gvx + (i * ny + jb) + jo, gvxo);
    }
  }
}

template <typename T, int VJ>
void launch_form(const AcAdjArgs<T>& k, hipStream_t stream) {
  const int64_t ownv = 62 * VJ;
  const int64_t nseg = (k.ny + 1 + ownv - 1) / ownv, nch = (k.nx + 1 + k.ch - 1) / k.ch;
  const int64_t blocks = (nseg * nch + ADJ_WAVES - 1) / ADJ_WAVES;
  if (blocks > 0x7fffffffLL) fail("acoustic2d_adjoint: grid too large");
  hipLaunchKernelGGL((acoustic2d_adjoint_kernel<T, VJ>), dim3(static_cast<unsigned>(blocks)), dim3(64 * ADJ_WAVES), 0,
                     stream, k);
  IGG_HIP_CHECK(hipGetLastError());
}

template <typename T>
void launch_typed(const AcousticAdjointArgs& a, int64_t ch, hipStream_t stream) {
  AcAdjArgs<T> k{};
  k.gp = reinterpret_cast<T*>(a.gp);
  k.gvx = reinterpret_cast<T*>(a.gvx);
  k.gvy = reinterpret_cast<T*>(a.gvy);
  k.gp2 = reinterpret_cast<const T*>(a.gp2);
  k.gvx2 = reinterpret_cast<const T*>(a.gvx2);
  k.gvy2 = reinterpret_cast<const T*>(a.gvy2);
  k.nx = a.nx, k.ny = a.ny, k.ch = ch;
  k.a = static_cast<T>(a.dtk), k.b = static_cast<T>(a.dt_rho);
  k.rdx = static_cast<T>(a.rdx), k.rdy = static_cast<T>(a.rdy);
  constexpr int VJ = 16 / static_cast<int>(sizeof(T));
  if (a.ny % VJ == 0 && a.ny >= 2 * VJ) launch_form<T, VJ>(k, stream);
  else launch_form<T, 1>(k, stream);
}

}  // namespace

static int64_t g_adjoint_ch = 0;  // 0: ADJ_CH
void acoustic2d_adjoint_set_chunk(int64_t rows) { g_adjoint_ch = rows > 0 ? rows : 0; }
int64_t acoustic2d_adjoint_chunk() { return g_adjoint_ch > 0 ? g_adjoint_ch : ADJ_CH; }

void launch_acoustic2d_adjoint(const AcousticAdjointArgs& a, hipStream_t stream) {
  check_acoustic2d_adjoint(a);
  const int64_t ch = a.chunk > 0 ? a.chunk : g_adjoint_ch > 0 ? g_adjoint_ch : ADJ_CH;
  if (a.elem_bytes == 8) launch_typed<double>(a, ch, stream);
  else launch_typed<float>(a, ch, stream);
}

}  // namespace igg
