// Host (CPU) twins of the adjoint diffusion kernels (stencil_adj_kernels.hip):
// the same point functions (igg/stencil_adj.hpp) in the same order, threaded
// over x planes. They are the CPU path of ops.stencil.diffusion3d_adjoint_ and
// the bitwise oracle of the kernels.
#include <cstring>

#include "igg/copy.hpp"
#include "igg/stencil.hpp"
#include "igg/stencil_adj.hpp"

namespace igg {

void check_diffusion3d_adjoint(const DiffusionAdjointArgs& a) {
  if (a.elem_bytes != 4 && a.elem_bytes != 8) fail("diffusion3d_adjoint: only float32/float64 are supported");
  for (int d = 0; d < 3; ++d)
    if (a.n[d] < 0) fail("diffusion3d_adjoint: negative extent along dim ", d);
  if (a.chunk < 0) fail("diffusion3d_adjoint: negative chunk");
  if (!a.g) fail("diffusion3d_adjoint: g is null");
  if (a.gt && !a.cp && !a.q) fail("diffusion3d_adjoint: gT needs Cp or Q");
  if (a.gcp && (!a.t || !a.cp)) fail("diffusion3d_adjoint: gCp needs T and Cp");
  if (a.gt && a.gt == a.g) fail("diffusion3d_adjoint: gT must not alias g");
  if (a.gcp && (a.gcp == a.g || a.gcp == a.cp || a.gcp == a.t || a.gcp == a.q || a.gcp == a.gt))
    fail("diffusion3d_adjoint: gCp must not alias another array");
}

namespace {

template <typename T>
void host_adjoint(const DiffusionAdjointArgs& a) {
  const int64_t n0 = a.n[0], n1 = a.n[1], n2 = a.n[2];
  const int64_t s1 = n2, s0 = n1 * n2;
  const T rdx2 = static_cast<T>(a.rd2[0]), rdy2 = static_cast<T>(a.rd2[1]), rdz2 = static_cast<T>(a.rd2[2]),
          dtlam = static_cast<T>(a.dt_lam);
  const T* g = reinterpret_cast<const T*>(a.g);
  const T* cp = reinterpret_cast<const T*>(a.cp);
  const T* q = reinterpret_cast<const T*>(a.q);
  const T* t = reinterpret_cast<const T*>(a.t);
  T* gt = reinterpret_cast<T*>(a.gt);
  T* gcp = reinterpret_cast<T*>(a.gcp);
  auto interior = [&](int64_t x, int64_t y, int64_t z) {
    return x >= 1 && x < n0 - 1 && y >= 1 && y < n1 - 1 && z >= 1 && z < n2 - 1;
  };
  // u of a cell; 0 for a boundary cell and beyond the array, nothing read there
  auto u = [&](int64_t x, int64_t y, int64_t z) -> T {
    if (!interior(x, y, z)) return T(0);
    const int64_t i = x * s0 + y * s1 + z;
    return q ? adj_u_q(g[i], q[i], true) : adj_u(g[i], cp[i], dtlam, true);
  };
  if (gt) {
    host_parallel_for(n0, 1, [&](int64_t x0, int64_t x1) {
      for (int64_t x = x0; x < x1; ++x)
        for (int64_t y = 0; y < n1; ++y)
          for (int64_t z = 0; z < n2; ++z) {
            const int64_t i = x * s0 + y * s1 + z;
            gt[i] = adj_t_point(g[i], u(x, y, z), u(x - 1, y, z), u(x + 1, y, z), u(x, y - 1, z), u(x, y + 1, z),
                                u(x, y, z - 1), u(x, y, z + 1), rdx2, rdy2, rdz2);
          }
    });
  }
  if (gcp) {
    host_parallel_for(n0, 1, [&](int64_t x0, int64_t x1) {
      for (int64_t x = x0; x < x1; ++x)
        for (int64_t y = 0; y < n1; ++y)
          for (int64_t z = 0; z < n2; ++z) {
            const int64_t i = x * s0 + y * s1 + z;
            if (!interior(x, y, z)) {
              if (!a.accumulate) gcp[i] = T(0);
              continue;
            }
            const T v = adj_cp_point(g[i], cp[i], dtlam, t[i], t[i - s0], t[i + s0], t[i - s1], t[i + s1], t[i - 1],
                                     t[i + 1], rdx2, rdy2, rdz2);
            gcp[i] = a.accumulate ? gcp[i] + v : v;
          }
    });
  }
}

}  // namespace

void host_diffusion3d_adjoint(const DiffusionAdjointArgs& a) {
  check_diffusion3d_adjoint(a);
  const int64_t cells = a.n[0] * a.n[1] * a.n[2];
  if (cells == 0) return;
  if (a.n[0] < 3 || a.n[1] < 3 || a.n[2] < 3) {
    // no interior: S is the identity
    const size_t bytes = static_cast<size_t>(cells) * a.elem_bytes;
    if (a.gt) std::memcpy(reinterpret_cast<void*>(a.gt), reinterpret_cast<const void*>(a.g), bytes);
    if (a.gcp && !a.accumulate) std::memset(reinterpret_cast<void*>(a.gcp), 0, bytes);
    return;
  }
  if (a.elem_bytes == 8) host_adjoint<double>(a);
  else host_adjoint<float>(a);
}

}  // namespace igg
