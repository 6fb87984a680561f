// Adjoint (transpose) of the diffusion step: the point arithmetic shared by
// the kernels (stencil_adj_kernels.hip) and their host twins
// (stencil_adj_host.cpp).
//
// Forward, as the model's loop uses it: S(T)[i] = fma(q[i], lap(T)[i], T[i]) on
// interior cells [1, n-1)^3 with q = dtlam/Cp (devmath.hpp diffusion_point),
// and S(T)[b] = T[b] on boundary cells. S is linear in T, so its transpose
// needs no forward state:
//   u[i]  = q[i] * g[i] on interior cells, 0 on boundary cells and outside
//   dX    = fma(-2, u[i], u[i+eX]) + u[i-eX]                  X = x, y, z
//   gT[i] = g[i] + fma(dz, rdz2, fma(dy, rdy2, dx * rdx2))    on ALL cells
// (a boundary cell is copied, not updated: it receives gradient from its
// interior neighbour and sends none through the stencil). The derivative with
// respect to Cp needs the forward input T:
//   gCp[i] = -(u[i] / Cp[i]) * lap(T)[i] on interior cells, 0 on boundary cells.
//
// Every operation is rounded on its own (the build has no contraction) and an
// FMA happens only where it is spelled out, so the host functions give bit
// for bit what the kernels give: the host path is the tests' oracle.
#pragma once

#if defined(__HIPCC__)
#define IGG_ADJ_HD __host__ __device__ __forceinline__
#else
#define IGG_ADJ_HD inline
#endif

namespace igg {

IGG_ADJ_HD double adj_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
IGG_ADJ_HD float adj_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// u of one cell from Cp (one division, one multiply) or from the quotient
// array; `interior` false selects 0 whatever g, cp and q hold (NaN, Cp == 0).
template <typename T>
IGG_ADJ_HD T adj_u(T g, T cp, T dtlam, bool interior) {
  const T u = (dtlam / cp) * g;
  return interior ? u : T(0);
}
template <typename T>
IGG_ADJ_HD T adj_u_q(T g, T q, bool interior) {
  const T u = q * g;
  return interior ? u : T(0);
}

// gT of one cell from g there and u on its 7-point star.
template <typename T>
IGG_ADJ_HD T adj_t_point(T g, T u, T uxm, T uxp, T uym, T uyp, T uzm, T uzp, T rdx2, T rdy2, T rdz2) {
  const T m2 = T(-2);
  const T dx = adj_fma(m2, u, uxp) + uxm;
  const T dy = adj_fma(m2, u, uyp) + uym;
  const T dz = adj_fma(m2, u, uzp) + uzm;
  return g + adj_fma(dz, rdz2, adj_fma(dy, rdy2, dx * rdx2));
}

// gCp of one interior cell; lap is formed exactly as in diffusion_point.
template <typename T>
IGG_ADJ_HD T adj_cp_point(T g, T cp, T dtlam, T c, T xm, T xp, T ym, T yp, T zm, T zp, T rdx2, T rdy2, T rdz2) {
  const T m2 = T(-2);
  const T dx = adj_fma(m2, c, xp) + xm;
  const T dy = adj_fma(m2, c, yp) + ym;
  const T dz = adj_fma(m2, c, zp) + zm;
  const T lap = adj_fma(dz, rdz2, adj_fma(dy, rdy2, dx * rdx2));
  const T u = (dtlam / cp) * g;
  return -(u / cp) * lap;
}

}  // namespace igg
