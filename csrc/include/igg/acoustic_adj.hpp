// Adjoint (transpose) of the 2-D staggered acoustic step (igg/acoustic.hpp):
// the point arithmetic shared by the kernels (acoustic_adj_kernels.hip) and
// their host twin (acoustic_adj_host.cpp).
//
// Forward S, with a = dt*K, b = dt/rho:
//   P2  = P - a*((Vx[i+1]-Vx[i])*rdx + (Vy[j+1]-Vy[j])*rdy)        all cells
//   Vx2 = Vx - b*(P2[i]-P2[i-1])*rdx   x-faces 1..nx-1, faces 0 and nx copied
//   Vy2 = Vy - b*(P2[j]-P2[j-1])*rdy   y-faces 1..ny-1, faces 0 and ny copied
// S is linear, so its transpose (gP2, gVx2, gVy2) -> (gP, gVx, gVy) needs no
// forward state:
//   wx(i,j) = (b*gVx2(i,j))*rdx  on x-faces 1..nx-1, else 0
//   wy(i,j) = (b*gVy2(i,j))*rdy  on y-faces 1..ny-1, else 0
//   r(i,j)  = gP2(i,j) + ((wx(i+1,j)-wx(i,j)) + (wy(i,j+1)-wy(i,j)))
//   gP(i,j)  = r(i,j)
//   gVx(i,j) = gVx2(i,j) + (a*(r(i,j)-r(i-1,j)))*rdx    r = 0 outside the cells
//   gVy(i,j) = gVy2(i,j) + (a*(r(i,j)-r(i,j-1)))*rdy    r = 0 outside the cells
// r plays the part P2 plays forward: formed once per cell, used by the faces on
// both sides. The forward step masks at its output (boundary faces copied);
// the transpose masks at its input (w = 0 on boundary faces) and at the array's
// edge (r = 0 outside). Every zero is a select, never a product, so what a
// boundary face holds (NaN, Inf) reaches that face's own result and no other.
//
// Every operation is rounded on its own (no contraction), so the host
// functions give bit for bit what the kernels give wherever a point is
// computed: the host path is the tests' oracle.
#pragma once

#if defined(__HIPCC__)
#define IGG_ACADJ_HD __host__ __device__ __forceinline__
#else
#define IGG_ACADJ_HD inline
#endif

namespace igg {

// w of one face: `inner` false selects 0 whatever g holds.
template <typename T>
IGG_ACADJ_HD T acadj_w(T g, T b, T rd, bool inner) {
#pragma clang fp contract(off)
  const T w = (b * g) * rd;
  return inner ? w : T(0);
}

// r of one cell from gP2 there and w on its four faces (x high, x low, y high, y low).
template <typename T>
IGG_ACADJ_HD T acadj_r(T gp2, T wx_hi, T wx_lo, T wy_hi, T wy_lo) {
#pragma clang fp contract(off)
  return gp2 + ((wx_hi - wx_lo) + (wy_hi - wy_lo));
}

// gV of one face from gV2 there and r of the cells on its high and low side
// (0 passed for a cell outside the array).
template <typename T>
IGG_ACADJ_HD T acadj_v(T gv2, T a, T r_hi, T r_lo, T rd) {
#pragma clang fp contract(off)
  return gv2 + (a * (r_hi - r_lo)) * rd;
}

}  // namespace igg
