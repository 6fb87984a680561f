// Host (CPU) twin of the adjoint acoustic kernels (acoustic_adj_kernels.hip):
// the same point functions (igg/acoustic_adj.hpp), threaded over rows of x.
// It is the CPU path of ops.stencil.acoustic2d_adjoint_ and the bitwise oracle
// of the kernels.
#include "igg/acoustic.hpp"
#include "igg/acoustic_adj.hpp"
#include "igg/copy.hpp"

namespace igg {

void check_acoustic2d_adjoint(const AcousticAdjointArgs& a) {
  if (a.elem_bytes != 4 && a.elem_bytes != 8)
    fail("acoustic2d_adjoint: element size must be 4 or 8 bytes (got ", a.elem_bytes, ")");
  if (a.nx < 1 || a.ny < 1) fail("acoustic2d_adjoint: empty grid");
  if (a.chunk < 0) fail("acoustic2d_adjoint: negative chunk");
  const uintptr_t p[6] = {a.gp, a.gvx, a.gvy, a.gp2, a.gvx2, a.gvy2};
  for (int k = 0; k < 6; ++k)
    if (!p[k]) fail("acoustic2d_adjoint: null array");
  for (int o = 0; o < 3; ++o)
    for (int k = o + 1; k < 6; ++k)
      if (p[o] == p[k]) fail("acoustic2d_adjoint: an output must not alias another array");
}

namespace {

template <typename T>
void host_adjoint(const AcousticAdjointArgs& a) {
  const int64_t nx = a.nx, ny = a.ny, sy = ny + 1;
  const T ca = static_cast<T>(a.dtk), cb = static_cast<T>(a.dt_rho);
  const T rdx = static_cast<T>(a.rdx), rdy = static_cast<T>(a.rdy);
  const T* gp2 = reinterpret_cast<const T*>(a.gp2);
  const T* gvx2 = reinterpret_cast<const T*>(a.gvx2);
  const T* gvy2 = reinterpret_cast<const T*>(a.gvy2);
  T* gp = reinterpret_cast<T*>(a.gp);
  T* gvx = reinterpret_cast<T*>(a.gvx);
  T* gvy = reinterpret_cast<T*>(a.gvy);
  // w of a face; 0 on a boundary face, nothing read there
  auto wx = [&](int64_t i, int64_t j) -> T {
    return (i >= 1 && i <= nx - 1) ? acadj_w(gvx2[i * ny + j], cb, rdx, true) : T(0);
  };
  auto wy = [&](int64_t i, int64_t j) -> T {
    return (j >= 1 && j <= ny - 1) ? acadj_w(gvy2[i * sy + j], cb, rdy, true) : T(0);
  };
  // r of a cell; 0 outside the cells
  auto r = [&](int64_t i, int64_t j) -> T {
    if (i < 0 || i >= nx || j < 0 || j >= ny) return T(0);
    return acadj_r(gp2[i * ny + j], wx(i + 1, j), wx(i, j), wy(i, j + 1), wy(i, j));
  };
  host_parallel_for(nx + 1, 16, [&](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i)
      for (int64_t j = 0; j <= ny; ++j) {
        const T rc = r(i, j);
        if (i < nx && j < ny) gp[i * ny + j] = rc;
        if (j < ny) gvx[i * ny + j] = acadj_v(gvx2[i * ny + j], ca, rc, r(i - 1, j), rdx);
        if (i < nx) gvy[i * sy + j] = acadj_v(gvy2[i * sy + j], ca, rc, r(i, j - 1), rdy);
      }
  });
}

}  // namespace

void host_acoustic2d_adjoint(const AcousticAdjointArgs& a) {
  check_acoustic2d_adjoint(a);
  if (a.elem_bytes == 8) host_adjoint<double>(a);
  else host_adjoint<float>(a);
}

}  // namespace igg
