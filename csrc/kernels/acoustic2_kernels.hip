// Two acoustic time steps in one pass over memory (see include/igg/acoustic.hpp
// launch_acoustic2d_twostep): reads P, Vx, Vy of step n once and writes P2, Vx2,
// Vy2 of step n+2; the field of step n+1 lives in registers only.
//
// Layout of acoustic2d_vmarch_kernel (acoustic_kernels.hip): a wave = 64 lanes
// of one 16-byte vector each (VJ = 4 columns f32, 2 f64), 62 owned vectors plus
// one halo vector per side; P/Vx rows are vector aligned (ny % VJ == 0), Vy rows
// (pitch ny+1) use element-aligned vector accesses and the lane that starts at
// column ny carries the last Vy face column with scalar accesses. Loads are
// clamped into the arrays, only owned lanes store.
//
// Dependencies along y over two steps: P'' of column j needs Vy' of j and j+1,
// Vy' of j needs P' of j-1 and j, P' of j needs Vy of j and j+1 - a reach of two
// columns to the left and two (Vy) / one (P, Vx) to the right, which the halo
// vectors cover for VJ >= 2. Values the halo lanes compute at their outer end
// (from a clamped shuffle or a clamped load) are wrong and never consumed: the
// comments at the shuffles say which elements are exact.
//
// March along x: at position r the wave forms the intermediate row r (P', Vx',
// Vy') from the prefetched inputs, then output row r-1 from the intermediate
// rows r-1 and r and P'' of row r-2. A chunk that writes rows [i0, i1) starts at
// row i0-2 (clipped at 0): P'(i0-2) makes Vx'(i0-1) exact, which makes P''(i0-1)
// exact, which Vx''(i0) needs. Boundary faces (Vx faces 0 / nx, Vy faces 0 / ny)
// are copied in both steps, i.e. keep their input values.
//
// Every value is computed with the expressions of vmarch_rows, rounded per
// operation (no FMA contraction), so a value is bitwise the same wherever it is
// computed - in the lead-in of one chunk or the march of another, in a halo
// lane or in the lane that owns it, here or in two single-step launches.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "igg/acoustic.hpp"
#include "igg/common.hpp"

namespace igg {
namespace {

constexpr int WAVES2 = 4;          // waves per workgroup
// Rows of x written per wave. A chunk reads two more rows than it writes, and
// the counters show them fetched past L2 ((chunk + 2) / chunk of the input);
// short chunks still win on waves in flight. Swept 1..128 at 8192^2 f32 and
// 4096^2 f64: 4..12 within a few per cent of each other, slower below 3 and
// above 32 (profiles/acoustic_twostep/NOTES.md).
constexpr int64_t TWOSTEP_CH = 8;

template <typename T, int VJ>
__global__ void __launch_bounds__(64 * WAVES2) acoustic2d_twostep_kernel(AcousticArgs a, int64_t ch) {
#pragma clang fp contract(off)
  typedef T V __attribute__((ext_vector_type(VJ)));
  typedef T VU __attribute__((ext_vector_type(VJ), aligned(sizeof(T))));
  constexpr int64_t OWNV = 62 * VJ;
  const int lane = threadIdx.x & 63;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * WAVES2 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nx = a.nx, ny = a.ny, sy = ny + 1;
  const int64_t nseg = (ny + 1 + OWNV - 1) / OWNV;
  const int64_t seg = wave % nseg, chunk = wave / nseg;
  const int64_t i0 = chunk * ch;  // output rows [i0, i1), row nx = the last x-faces
  if (i0 > nx) return;            // wave-uniform
  const int64_t i1 = min(i0 + ch, nx + 1);
  const int64_t j0 = seg * OWNV + static_cast<int64_t>(lane - 1) * VJ;  // first column of this lane
  const bool own = lane >= 1 && lane <= 62 && j0 <= ny;
  const bool cells = j0 + VJ <= ny && j0 >= 0;  // VJ cell / x-face columns
  const bool last = j0 == ny;                   // only the boundary y-face column ny
  const int64_t jl = min<int64_t>(max<int64_t>(j0, 0), ny - VJ);  // clamped vector start
  const T* __restrict__ p = reinterpret_cast<const T*>(a.p);
  const T* __restrict__ vx = reinterpret_cast<const T*>(a.vx);
  const T* __restrict__ vy = reinterpret_cast<const T*>(a.vy);
  T* __restrict__ p2 = reinterpret_cast<T*>(a.p2);
  T* __restrict__ vx2 = reinterpret_cast<T*>(a.vx2);
  T* __restrict__ vy2 = reinterpret_cast<T*>(a.vy2);
  const T dtk = static_cast<T>(a.dtk), dt_rho = static_cast<T>(a.dt_rho);
  const T rdx = static_cast<T>(a.rdx), rdy = static_cast<T>(a.rdy);
  auto ldv = [&](const T* base, int64_t row) { return *reinterpret_cast<const V*>(base + row * ny + jl); };
  auto ldy = [&](int64_t row) {  // Vy(row, j0..j0+VJ-1); the column-ny lane holds Vy(row, ny) in element 0
    V v = *reinterpret_cast<const VU*>(vy + row * sy + jl);
    if (last) {
      v = V(T(0));
      v[0] = vy[row * sy + ny];
    }
    return v;
  };
  auto next = [&](const V& h) {  // the value of column j+1 per element (lane 63: its last element is not exact)
    V n;
    const T up = __shfl_down(h[0], 1);
#pragma unroll
    for (int e = 0; e < VJ; ++e) n[e] = e + 1 < VJ ? h[e + 1 < VJ ? e + 1 : e] : up;
    return n;
  };
  auto prev = [&](const V& h) {  // the value of column j-1 per element (lane 0: its first element is not exact)
    V n;
    const T dn = __shfl_up(h[VJ - 1], 1);
#pragma unroll
    for (int e = 0; e < VJ; ++e) n[e] = e == 0 ? dn : h[e > 0 ? e - 1 : 0];
    return n;
  };
  if (i0 == nx) {  // a chunk of the last x-face row alone: boundary faces, copied
    if (own && cells) *reinterpret_cast<V*>(vx2 + nx * ny + j0) = ldv(vx, nx);
    return;
  }
  const int64_t rs = max<int64_t>(i0 - 2, 0);  // first intermediate row (lead-in), rs <= i0 < nx
  const int64_t re = min(i1, nx);              // last intermediate row (Vx' only if re == nx)
  // Inputs of row r: Vx(r) carried, Vx(r+1), P(r), Vy(r) prefetched one row ahead.
  V vx_i = ldv(vx, rs);
  V vy_h = ldy(rs), vx_n = ldv(vx, rs + 1), pp = ldv(p, rs);
  // Intermediate row r-1 and P'' of row r-2.
  V p1 = V(T(0)), vx1 = V(T(0)), vy1 = V(T(0)), q_prev = V(T(0));
  for (int64_t r = rs; r <= re; ++r) {
    V vy_h1 = V(T(0)), vx_n1 = V(T(0)), pp1 = V(T(0));
    if (r + 1 < nx && r + 1 <= re) {  // prefetch row r+1
      vy_h1 = ldy(r + 1);
      vx_n1 = ldv(vx, r + 2);
      pp1 = ldv(p, r + 1);
    }
    // Intermediate row r. Exact: P', Vx' in lanes 0..62 (and lane 63 but its
    // last element), Vy' in lanes 1..62, lane 0 but its first element, lane 63
    // but its last. Vx'(rs) of a chunk with rs > 0 lacks P'(rs-1): not exact,
    // and consumed only by P''(rs), which nothing exact depends on.
    V pc = V(T(0)), vxc = vx_i, vyc = V(T(0));
    if (r < nx) {
      const V vy_n = next(vy_h);
#pragma unroll
      for (int e = 0; e < VJ; ++e) pc[e] = pp[e] - dtk * ((vx_n[e] - vx_i[e]) * rdx + (vy_n[e] - vy_h[e]) * rdy);
      const V pl = prev(pc);
#pragma unroll
      for (int e = 0; e < VJ; ++e) {
        const int64_t j = j0 + e;
        vyc[e] = (j >= 1 && j <= ny - 1) ? vy_h[e] - dt_rho * (pc[e] - pl[e]) * rdy : vy_h[e];
        vxc[e] = (r >= 1) ? vx_i[e] - dt_rho * (pc[e] - p1[e]) * rdx : vx_i[e];
      }
    }  // r == nx: Vx'(nx) = Vx(nx), a boundary face
    if (r > rs) {
      // Output row o = r-1 < nx. P'' exact in lanes 1..62 and the last element
      // of lane 0 (from row i0-1 on, or from row 0 if the march starts there).
      const int64_t o = r - 1;
      const V vy1n = next(vy1);
      V q;
#pragma unroll
      for (int e = 0; e < VJ; ++e) q[e] = p1[e] - dtk * ((vxc[e] - vx1[e]) * rdx + (vy1n[e] - vy1[e]) * rdy);
      const V ql = prev(q);
      if (o >= i0 && own) {
        if (cells) {
          V vyo, vxo;
#pragma unroll
          for (int e = 0; e < VJ; ++e) {
            const int64_t j = j0 + e;
            vyo[e] = (j >= 1 && j <= ny - 1) ? vy1[e] - dt_rho * (q[e] - ql[e]) * rdy : vy1[e];
            vxo[e] = (o >= 1) ? vx1[e] - dt_rho * (q[e] - q_prev[e]) * rdx : vx1[e];
          }
          __builtin_nontemporal_store(q, reinterpret_cast<V*>(p2 + o * ny + j0));
          __builtin_nontemporal_store(vxo, reinterpret_cast<V*>(vx2 + o * ny + j0));
          *reinterpret_cast<VU*>(vy2 + o * sy + j0) = vyo;
        } else if (last) {
          vy2[o * sy + ny] = vy1[0];  // boundary face: Vy'(o, ny) = Vy(o, ny)
        }
      }
      q_prev = q;
    }
    if (r == nx && i1 == nx + 1 && own && cells)  // the last x-faces are boundary faces
      *reinterpret_cast<V*>(vx2 + nx * ny + j0) = vx_i;
    p1 = pc;
    vx1 = vxc;
    vy1 = vyc;
    vx_i = vx_n;
    vy_h = vy_h1;
    vx_n = vx_n1;
    pp = pp1;
  }
}

}  // namespace

bool acoustic2d_twostep_ok(const AcousticArgs& a) {
  if (a.elem_bytes != 4 && a.elem_bytes != 8) return false;
  const int vj = a.elem_bytes == 4 ? 4 : 2;  // 16 B per lane
  return a.nx >= 1 && a.ny % vj == 0 && a.ny >= 2 * vj;
}

void launch_acoustic2d_twostep(const AcousticArgs& a, int64_t chunk, hipStream_t stream) {
  if (a.elem_bytes != 4 && a.elem_bytes != 8)
    fail("acoustic2d_twostep: element size must be 4 or 8 bytes (got ", a.elem_bytes, ")");
  const int vj = a.elem_bytes == 4 ? 4 : 2;
  if (!acoustic2d_twostep_ok(a))
    fail("acoustic2d_twostep: needs nx >= 1, ny % ", vj, " == 0 and ny >= ", 2 * vj, " (got ", a.nx, " x ", a.ny, ")");
  if (chunk < 0) fail("acoustic2d_twostep: chunk must be >= 0 (got ", chunk, ")");
  for (uintptr_t out : {a.p2, a.vx2, a.vy2})
    for (uintptr_t in : {a.p, a.vx, a.vy})
      if (out == in) fail("acoustic2d_twostep: an output aliases an input (the pass reads rows it has already written)");
  const int64_t ch = std::min<int64_t>(chunk > 0 ? chunk : TWOSTEP_CH, a.nx + 1);
  const int64_t ownv = 62 * vj;
  const int64_t nseg = (a.ny + 1 + ownv - 1) / ownv, nch = (a.nx + 1 + ch - 1) / ch;
  const int64_t blocks = (nseg * nch + WAVES2 - 1) / WAVES2;
  if (blocks > 0x7fffffff) fail("acoustic2d_twostep: grid of ", blocks, " workgroups (raise chunk)");
  const dim3 grid(static_cast<unsigned>(blocks));
  if (a.elem_bytes == 8)
    hipLaunchKernelGGL((acoustic2d_twostep_kernel<double, 2>), grid, dim3(64 * WAVES2), 0, stream, a, ch);
  else
    hipLaunchKernelGGL((acoustic2d_twostep_kernel<float, 4>), grid, dim3(64 * WAVES2), 0, stream, a, ch);
  IGG_HIP_CHECK(hipGetLastError());
}

}  // namespace igg
