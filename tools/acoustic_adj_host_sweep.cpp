// Stand-alone sweep of the adjoint acoustic host twin (csrc/acoustic_adj_host.cpp)
// for a host sanitizer run: every (nx, ny) of a small range, float32 and
// float64, on heap arrays of exactly the fields' sizes, so that a read or a
// write beyond an array is an error. The transposed-matrix identity
// <Sᵀg, x> == <g, Sx> is checked on the way, on dyadic data (exact). Host code only.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ \
//       -Icsrc/include -I$ROCM_PATH/include tools/acoustic_adj_host_sweep.cpp csrc/acoustic_adj_host.cpp \
//       csrc/host_copy.cpp -lpthread -o /tmp/acoustic_adj_host_sweep
//   /tmp/acoustic_adj_host_sweep
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "igg/acoustic.hpp"
#include "igg/common.hpp"

using namespace igg;

namespace {

template <typename T>
std::vector<T> ints(size_t n, unsigned& seed) {
  std::vector<T> v(n);
  for (auto& x : v) {
    seed = seed * 1664525u + 1013904223u;
    x = static_cast<T>(static_cast<int>((seed >> 16) % 17) - 8);
  }
  return v;
}

template <typename T>
double dot(const std::vector<T>& a, const std::vector<T>& b) {
  double s = 0;
  for (size_t i = 0; i < a.size(); ++i) s += static_cast<double>(a[i]) * static_cast<double>(b[i]);
  return s;
}

// the forward step, plainly (a = 1/4, b = 1/2, 1/dx = 2, 1/dy = 4: exact on small integers)
template <typename T>
void forward(int64_t nx, int64_t ny, const std::vector<T>& p, const std::vector<T>& vx, const std::vector<T>& vy,
             std::vector<T>& p2, std::vector<T>& vx2, std::vector<T>& vy2) {
  const T a = T(0.25), b = T(0.5), rdx = T(2), rdy = T(4);
  for (int64_t i = 0; i < nx; ++i)
    for (int64_t j = 0; j < ny; ++j)
      p2[i * ny + j] = p[i * ny + j] - a * ((vx[(i + 1) * ny + j] - vx[i * ny + j]) * rdx +
                                            (vy[i * (ny + 1) + j + 1] - vy[i * (ny + 1) + j]) * rdy);
  vx2 = vx;
  vy2 = vy;
  for (int64_t i = 1; i < nx; ++i)
    for (int64_t j = 0; j < ny; ++j) vx2[i * ny + j] = vx[i * ny + j] - b * (p2[i * ny + j] - p2[(i - 1) * ny + j]) * rdx;
  for (int64_t i = 0; i < nx; ++i)
    for (int64_t j = 1; j < ny; ++j)
      vy2[i * (ny + 1) + j] = vy[i * (ny + 1) + j] - b * (p2[i * ny + j] - p2[i * ny + j - 1]) * rdy;
}

template <typename T>
long sweep() {
  long n = 0;
  unsigned seed = 12345;
  for (int64_t nx = 1; nx <= 9; ++nx)
    for (int64_t ny = 1; ny <= 70; ny += (ny < 10 ? 1 : 15)) {
      const size_t np = nx * ny, nvx = (nx + 1) * ny, nvy = nx * (ny + 1);
      auto gp2 = ints<T>(np, seed), gvx2 = ints<T>(nvx, seed), gvy2 = ints<T>(nvy, seed);
      auto p = ints<T>(np, seed), vx = ints<T>(nvx, seed), vy = ints<T>(nvy, seed);
      std::vector<T> gp(np), gvx(nvx), gvy(nvy), p2(np), vx2(nvx), vy2(nvy);
      AcousticAdjointArgs a{reinterpret_cast<uintptr_t>(gp.data()),   reinterpret_cast<uintptr_t>(gvx.data()),
                            reinterpret_cast<uintptr_t>(gvy.data()),  reinterpret_cast<uintptr_t>(gp2.data()),
                            reinterpret_cast<uintptr_t>(gvx2.data()), reinterpret_cast<uintptr_t>(gvy2.data()),
                            nx, ny, 0.25, 0.5, 2.0, 4.0, static_cast<int>(sizeof(T)), 0};
      host_acoustic2d_adjoint(a);
      forward(nx, ny, p, vx, vy, p2, vx2, vy2);
      const double lhs = dot(gp, p) + dot(gvx, vx) + dot(gvy, vy);
      const double rhs = dot(gp2, p2) + dot(gvx2, vx2) + dot(gvy2, vy2);
      if (lhs != rhs) {
        std::fprintf(stderr, "transpose identity broken at %ld x %ld: %g != %g\n", (long)nx, (long)ny, lhs, rhs);
        std::exit(1);
      }
      ++n;
    }
  return n;
}

}  // namespace

int main() {
  const long n = sweep<float>() + sweep<double>();
  // refused arguments throw before anything is written
  long refused = 0;
  float x[4] = {0, 0, 0, 0};
  const uintptr_t px = reinterpret_cast<uintptr_t>(x);
  for (int k = 0; k < 4; ++k) {
    AcousticAdjointArgs a{px, px + 4, px + 8, px + 12, px + 12, px + 12, 1, 1, 1.0, 1.0, 1.0, 1.0, 4, 0};
    if (k == 0) a.nx = 0;
    if (k == 1) a.elem_bytes = 2;
    if (k == 2) a.gp = a.gp2;
    if (k == 3) a.chunk = -1;
    try {
      host_acoustic2d_adjoint(a);
    } catch (const Error&) {
      ++refused;
    }
  }
  if (refused != 4) {
    std::fprintf(stderr, "only %ld of 4 bad calls were refused\n", refused);
    return 1;
  }
  std::printf("acoustic adjoint host twin: %ld shapes, transpose identity exact, 4 bad calls refused\n", n);
  return 0;
}
