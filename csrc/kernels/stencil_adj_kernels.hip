// Adjoint of the 3-D diffusion step for gfx950 (igg/stencil_adj.hpp):
//   adjoint_t   gT  = S^T g           reads g and Cp (or Q), writes gT
//   adjoint_cp  gCp = dS(T)/dCp^T g   reads T (stencil), Cp and g, writes gCp
// Both move the forward step's three arrays and are as bandwidth bound, so
// they take the plain vector kernel's layout (stencil_kernels.hip
// diffusion3d_vkernel, igg/vsweep.hpp): each lane owns one 16-byte vector of
// the row, z neighbours come from the lane neighbours (only the two
// segment-edge values are loaded), a wave holds RY rows and marches along x
// with three planes of the stencil field in registers, addresses are a
// wave-uniform base plus a 32-bit lane offset, the output is stored
// non-temporally. The stencil field is u = q*g for adjoint_t and T for
// adjoint_cp. What differs from the forward sweep:
//   * u is formed on load, so every neighbour row and edge value of adjoint_t
//     takes g and Cp both;
//   * the output box is the whole array: every store is a whole aligned vector;
//   * a value beyond the array is never loaded: its address is clamped into
//     the array and 0 selected in its place;
//   * boundary cells get u = 0 by the same select (never by a multiply, so
//     Cp == 0 or a NaN there changes nothing).
// One tiling per element type for rows that are a multiple of the vector
// (VZ = 4 float32, 2 float64) and the same kernel with one point per lane
// (VZ = 1) for every other row length. No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "igg/stencil.hpp"
#include "igg/stencil_adj.hpp"
#include "igg/xcd.hpp"

namespace igg {
namespace {

constexpr int ADJ_BY = 4;  // waves per workgroup, one above the other along y
constexpr int ADJ_RY = 4;  // rows per wave

// 0: adjoint_t from Cp, 1: adjoint_t from Q, 2: adjoint_cp, 3: adjoint_cp accumulated
enum AdjMode : int { T_CP = 0, T_Q = 1, CP_SET = 2, CP_ADD = 3 };

template <typename T>
struct AdjArgs {
  T* __restrict__ out;        // gT or gCp
  const T* __restrict__ g;
  const T* __restrict__ c;    // Cp, or Q (T_Q)
  const T* __restrict__ t;    // the forward input (adjoint_cp only)
  int64_t n0, n1, n2;
  T rdx2, rdy2, rdz2, dtlam;
  int64_t ntz, nty, ch;       // z and y tiles, planes per x chunk
};

template <typename T, int VZ>
struct AdjVec {
  typedef T type __attribute__((ext_vector_type(VZ)));
};
template <typename T>
struct AdjVec<T, 1> {
  struct type {
    T v;
    __device__ __forceinline__ T& operator[](int) { return v; }
    __device__ __forceinline__ const T& operator[](int) const { return v; }
  };
};

template <typename T, int VZ>
__device__ __forceinline__ typename AdjVec<T, VZ>::type adj_load(const T* p) {
  return *reinterpret_cast<const typename AdjVec<T, VZ>::type*>(p);
}

template <typename T, int VZ>
__device__ __forceinline__ void adj_store(T* p, const typename AdjVec<T, VZ>::type& v) {
  if constexpr (VZ == 1) {
    __builtin_nontemporal_store(v.v, p);
  } else {
    __builtin_nontemporal_store(v, reinterpret_cast<typename AdjVec<T, VZ>::type*>(p));
  }
}

template <typename T, int VZ, int MODE>
__global__ void __launch_bounds__(64 * ADJ_BY)
diffusion3d_adjoint_kernel(const AdjArgs<T> a) {
  using V = typename AdjVec<T, VZ>::type;
  constexpr int RY = ADJ_RY;
  constexpr bool CPK = MODE >= CP_SET;
  int64_t b = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t tz = b % a.ntz;
  b /= a.ntz;
  const int64_t ty = b % a.nty;
  const int64_t cx = b / a.nty;

  const int lane = threadIdx.x & 63;
  const int wy = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n0 = a.n0, n1 = a.n1, n2 = a.n2;
  const int64_t s1 = n2, s0 = n1 * n2;
  const int64_t zt = tz * (64 * VZ);  // wave-uniform segment origin, < n2
  const int64_t y0 = ty * (ADJ_BY * RY) + wy * RY;
  const int64_t xs = cx * a.ch;
  const int64_t xe = min(xs + a.ch, n0);
  const int nv = static_cast<int>(min<int64_t>(RY, n1 - y0));
  if (nv <= 0) return;
  // A lane's vector lies wholly in the row or wholly past it (n2 % VZ == 0);
  // a lane past the row aliases the row's last vector and stores nothing.
  const int64_t z0 = zt + lane * VZ;
  const bool lane_in = z0 < n2;
  const int zl = static_cast<int>(min(z0, n2 - VZ) - zt);
  bool zin[VZ];  // element is an interior z of the row
#pragma unroll
  for (int e = 0; e < VZ; ++e) zin[e] = z0 + e >= 1 && z0 + e < n2 - 1;
  // the two values next to the wave's segment: loaded by its first and last
  // lane from a clamped address, 0 where they are no interior z
  const bool load_prev = lane == 0, load_next = lane == 63;
  const int zpi = static_cast<int>(max<int64_t>(zt - 1, 0) - zt);
  const int zni = static_cast<int>(min<int64_t>(zt + 64 * VZ, n2 - 1) - zt);
  const bool prev_in = zt - 1 >= 1, next_in = zt + 64 * VZ < n2 - 1;

  int64_t rowb[RY];  // wave-uniform row bases (element index of the segment origin)
  bool rowin[RY];    // row is an interior y
#pragma unroll
  for (int r = 0; r < RY; ++r) {
    const int64_t y = y0 + min(r, nv - 1);
    rowb[r] = y * s1 + zt;
    rowin[r] = y >= 1 && y < n1 - 1;
  }
  const int64_t ym_y = y0 - 1, yp_y = y0 + nv;
  const int64_t rowm = max<int64_t>(ym_y, 0) * s1 + zt, rowp = min(yp_y, n1 - 1) * s1 + zt;
  const bool rowm_in = ym_y >= 1, rowp_in = yp_y < n1 - 1;

  const T* __restrict__ gp = a.g;
  const T* __restrict__ cp = a.c;
  const T* __restrict__ tp = a.t;
  const T dtlam = a.dtlam;

  // The stencil field's vector at (plane base `off`, row base `row`): u with
  // 0 selected wherever the cell is no interior cell (adjoint_t; `gout` gets
  // g), or T as it is (adjoint_cp: what T holds outside the interior's star
  // reaches no result).
  auto load_w = [&](int64_t off, int64_t row, bool xy_in, V& gout) -> V {
    if constexpr (CPK) {
      return adj_load<T, VZ>(tp + off + row + zl);
    } else {
      const V gv = adj_load<T, VZ>(gp + off + row + zl);
      const V cv = adj_load<T, VZ>(cp + off + row + zl);
      V w;
#pragma unroll
      for (int e = 0; e < VZ; ++e) {
        if constexpr (MODE == T_Q) w[e] = adj_u_q(gv[e], cv[e], xy_in && zin[e]);
        else w[e] = adj_u(gv[e], cv[e], dtlam, xy_in && zin[e]);
      }
      gout = gv;
      return w;
    }
  };
  // One segment-edge value (element offset zi of the row), in the lanes `take`.
  auto edge_w = [&](int64_t off, int64_t row, int zi, bool take, bool in) -> T {
    if (!take) return T(0);
    if constexpr (CPK) {
      return tp[off + row + zi];
    } else {
      const T gs = gp[off + row + zi], cs = cp[off + row + zi];
      if constexpr (MODE == T_Q) return adj_u_q(gs, cs, in);
      else return adj_u(gs, cs, dtlam, in);
    }
  };
  auto x_interior = [&](int64_t x) { return x >= 1 && x < n0 - 1; };
  auto x_off = [&](int64_t x) { return min(max<int64_t>(x, 0), n0 - 1) * s0; };

  V wm[RY], wc[RY], wp[RY], gc[RY], gn[RY];
#pragma unroll
  for (int r = 0; r < RY; ++r) {
    V unused;
    wm[r] = load_w(x_off(xs - 1), rowb[r], x_interior(xs - 1) && rowin[r], unused);
    wc[r] = load_w(x_off(xs), rowb[r], x_interior(xs) && rowin[r], gc[r]);
  }
  for (int64_t x = xs; x < xe; ++x) {
    const int64_t off = x * s0;
    const bool xin = x_interior(x);
#pragma unroll
    for (int r = 0; r < RY; ++r) wp[r] = load_w(x_off(x + 1), rowb[r], x_interior(x + 1) && rowin[r], gn[r]);
    V unused;
    const V ym = load_w(off, rowm, xin && rowm_in, unused);
    const V yp = load_w(off, rowp, xin && rowp_in, unused);
    T em[RY], ep[RY];
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      em[r] = edge_w(off, rowb[r], zpi, load_prev, xin && rowin[r] && prev_in);
      ep[r] = edge_w(off, rowb[r], zni, load_next, xin && rowin[r] && next_in);
    }
    V pg[RY], pc[RY], po[RY];  // adjoint_cp: g, Cp and (accumulated) gCp of the plane
    if constexpr (CPK) {
#pragma unroll
      for (int r = 0; r < RY; ++r) {
        pg[r] = adj_load<T, VZ>(gp + off + rowb[r] + zl);
        pc[r] = adj_load<T, VZ>(cp + off + rowb[r] + zl);
        if constexpr (MODE == CP_ADD) po[r] = adj_load<T, VZ>(a.out + off + rowb[r] + zl);
      }
    }
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      const V& c = wc[r];
      const V& yv = (r == 0) ? ym : wc[r > 0 ? r - 1 : 0];
      const V& yn = (r + 1 < nv) ? wc[(r + 1 < RY) ? r + 1 : r] : yp;
      T prev = __shfl_up(c[VZ - 1], 1);
      T next = __shfl_down(c[0], 1);
      if (load_prev) prev = em[r];
      if (load_next) next = ep[r];
      V out;
#pragma unroll
      for (int e = 0; e < VZ; ++e) {
        const T zm = e == 0 ? prev : c[e > 0 ? e - 1 : 0];
        const T zp = e == VZ - 1 ? next : c[e + 1 < VZ ? e + 1 : e];
        if constexpr (CPK) {
          const T v = adj_cp_point(pg[r][e], pc[r][e], dtlam, c[e], wm[r][e], wp[r][e], yv[e], yn[e], zm, zp,
                                   a.rdx2, a.rdy2, a.rdz2);
          const bool in = xin && rowin[r] && zin[e];
          if constexpr (MODE == CP_ADD) out[e] = in ? po[r][e] + v : po[r][e];
          else out[e] = in ? v : T(0);
        } else {
          out[e] = adj_t_point(gc[r][e], c[e], wm[r][e], wp[r][e], yv[e], yn[e], zm, zp, a.rdx2, a.rdy2, a.rdz2);
        }
      }
      if (r < nv && lane_in) adj_store<T, VZ>(a.out + off + rowb[r] + zl, out);
    }
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      wm[r] = wc[r];
      wc[r] = wp[r];
      if constexpr (!CPK) gc[r] = gn[r];
    }
  }
}

template <typename T, int VZ, int MODE>
void launch_form(AdjArgs<T> ka, int chunk, hipStream_t stream) {
  const void* kern = reinterpret_cast<const void*>(&diffusion3d_adjoint_kernel<T, VZ, MODE>);
  ka.ntz = (ka.n2 + 64 * VZ - 1) / (64 * VZ);
  ka.nty = (ka.n1 + ADJ_BY * ADJ_RY - 1) / (ADJ_BY * ADJ_RY);
  const int64_t tiles = ka.ntz * ka.nty;
  int64_t ch = chunk;
  if (ch <= 0) {
    // equal chunks along the march, about one residency round of workgroups
    // (a chunk re-reads two planes, so none is shorter than 4)
    const int64_t target = diffusion3d_target_blocks(kern, 64 * ADJ_BY, 0);
    const int64_t want = std::max<int64_t>(4, (ka.n0 * tiles + target - 1) / target);
    const int64_t nch = std::max<int64_t>(1, (ka.n0 + want - 1) / want);
    ch = (ka.n0 + nch - 1) / nch;
  }
  ka.ch = std::min<int64_t>(ch, ka.n0);
  const int64_t blocks = tiles * ((ka.n0 + ka.ch - 1) / ka.ch);
  if (blocks > 0x7fffffffLL) fail("diffusion3d_adjoint: grid too large");
  hipLaunchKernelGGL((diffusion3d_adjoint_kernel<T, VZ, MODE>), dim3(static_cast<unsigned>(blocks)),
                     dim3(64 * ADJ_BY), 0, stream, ka);
  IGG_HIP_CHECK(hipGetLastError());
}

template <typename T, int MODE>
void launch_mode(const AdjArgs<T>& ka, int chunk, hipStream_t stream) {
  constexpr int VZ = 16 / static_cast<int>(sizeof(T));
  if (ka.n2 % VZ == 0) launch_form<T, VZ, MODE>(ka, chunk, stream);
  else launch_form<T, 1, MODE>(ka, chunk, stream);
}

template <typename T>
void launch_t(const DiffusionAdjointArgs& a, hipStream_t stream) {
  AdjArgs<T> k{};
  k.g = reinterpret_cast<const T*>(a.g);
  k.n0 = a.n[0]; k.n1 = a.n[1]; k.n2 = a.n[2];
  k.rdx2 = static_cast<T>(a.rd2[0]);
  k.rdy2 = static_cast<T>(a.rd2[1]);
  k.rdz2 = static_cast<T>(a.rd2[2]);
  k.dtlam = static_cast<T>(a.dt_lam);
  if (a.gt) {
    k.out = reinterpret_cast<T*>(a.gt);
    k.t = nullptr;
    if (a.q) {
      k.c = reinterpret_cast<const T*>(a.q);
      launch_mode<T, T_Q>(k, a.chunk, stream);
    } else {
      k.c = reinterpret_cast<const T*>(a.cp);
      launch_mode<T, T_CP>(k, a.chunk, stream);
    }
  }
  if (a.gcp) {
    k.out = reinterpret_cast<T*>(a.gcp);
    k.c = reinterpret_cast<const T*>(a.cp);
    k.t = reinterpret_cast<const T*>(a.t);
    if (a.accumulate) launch_mode<T, CP_ADD>(k, a.chunk, stream);
    else launch_mode<T, CP_SET>(k, a.chunk, stream);
  }
}

}  // namespace

AdjointTile diffusion3d_adjoint_tile(int64_t n2, int elem_bytes) {
  const int vz = 16 / elem_bytes;
  return {n2 % vz == 0 ? vz : 1, ADJ_BY * ADJ_RY};
}

void launch_diffusion3d_adjoint(const DiffusionAdjointArgs& a, hipStream_t stream) {
  check_diffusion3d_adjoint(a);
  const int64_t cells = a.n[0] * a.n[1] * a.n[2];
  if (cells == 0) return;
  if (a.n[0] < 3 || a.n[1] < 3 || a.n[2] < 3) {
    // no interior: S is the identity
    const size_t bytes = static_cast<size_t>(cells) * a.elem_bytes;
    if (a.gt)
      IGG_HIP_CHECK(hipMemcpyAsync(reinterpret_cast<void*>(a.gt), reinterpret_cast<const void*>(a.g), bytes,
                                   hipMemcpyDeviceToDevice, stream));
    if (a.gcp && !a.accumulate) IGG_HIP_CHECK(hipMemsetAsync(reinterpret_cast<void*>(a.gcp), 0, bytes, stream));
    return;
  }
  if (a.elem_bytes == 8) launch_t<double>(a, stream);
  else launch_t<float>(a, stream);
}

}  // namespace igg
