// Three diffusion time steps in one pass over memory for gfx950: t2 =
// step(step(step(t))) on the whole inner box of a rank without neighbours,
// bitwise what three launch_diffusion3d calls leave (every point goes through
// diffusion_point_q, devmath.hpp; boundary planes, rows and z points keep t's
// values in both intermediate fields, as they do in the ping-pong loop).
//
// The two-step pass (stencil2_kernels.hip) moves about 1 write + 2 reads per
// TWO steps and runs at the memory roof; here two intermediate fields stay on
// chip, so about the same bytes buy THREE steps.
//
// Only the case the headline runs: the tile spans the row (n2 <= tile width:
// no z ring, no edge threads) and the pass reads Q = dtlam/Cp (no division).
// Longer rows, or a model without Q, keep the two-step pass.
//
// Shape: the two-step march along dim 0 with one more stage. A workgroup of
// BY x BZ waves owns TYE = BY*RY rows of the plane: the two outer rows on
// either side are the rings of the intermediate fields, the TYE-4 inner rows
// are written, and tiles advance by TYE-4 rows. At march position p a wave
//   1. forms intermediate-1 plane p from T planes p-1, p, p+1 (y neighbours
//      beyond the wave's rows and the segment-edge z values are loaded);
//   2. forms intermediate-2 plane p-1 from intermediate-1 planes p-2, p-1, p,
//      on all but the tile's two outer rows (rows 0 and TYE-1 feed nothing);
//   3. forms output plane p-2 from intermediate-2 planes p-3, p-2, p-1, on the
//      TYE-4 written rows;
//   4. issues the loads of position p+1 (T plane p+2, Q plane p+1).
// Each wave's first and last row and its segment-edge z values of both
// intermediate fields travel through LDS (one buffer per phase of the march
// and field), with one barrier per position. An x chunk [xs, xe) starts with
// the four-position lead-in p = xs-2 .. xs+1.
//
// Waves: wave wid owns rows (wid / BZ) * RY .. of the tile and one 64-lane
// segment of the row; the odd rows of waves take their segments rotated by
// BZ/2 (wz = (wid + (wy & 1) * BZ/2) % BZ). Only a wave that holds an end of
// the row (z = 0 or n2-1), a boundary row or a boundary plane selects between
// T's value and the update; the others take a select-free path behind one
// wave-uniform branch per row update, and the rotation gives every SIMD one
// wave of either kind (waves s and s+4 usually share SIMD s).
//
// The kernel body is igg/stencil3_impl.hpp.
#include <hip/hip_runtime.h>

#include "igg/stencil3_impl.hpp"

namespace igg {
namespace {

using twostep::K2Args;

template <typename T, int BY, int RY, int VZ, int BZ>
__global__ void __launch_bounds__(64 * BY * BZ)
diffusion3d_threestep_kernel(const K2Args<T> a) {
  threestep::body<T, BY, RY, VZ, BZ>(a);
}

struct Form {
  const char* name;
  int by, ry, bz;
};

// Lanes hold 16 bytes, as in the two-step pass: form 0 spans a 512-point f64 /
// 1024-point f32 row.
constexpr Form FORMS[] = {
    {"t3_by2_ry4_bz4", 2, 4, 4},  // 0: 8 rows x 512 (f64) tile, 4 rows written, 512 threads
};
constexpr int NFORMS = sizeof(FORMS) / sizeof(FORMS[0]);

template <typename T, int BY, int RY, int BZ>
void launch3(const DiffusionArgs& a, hipStream_t stream) {
  constexpr int VZ = 16 / static_cast<int>(sizeof(T));
  threestep::launch_form<T, BY, RY, BZ>(&diffusion3d_threestep_kernel<T, BY, RY, VZ, BZ>, a, stream);
}

template <typename T>
void dispatch3(const DiffusionArgs& a, hipStream_t s) {
  switch (a.form) {
    case 0: launch3<T, 2, 4, 4>(a, s); break;
    default: fail("diffusion3d_threestep: no form ", a.form);
  }
}

}  // namespace

int diffusion3d_threestep_num_forms() { return NFORMS; }
const char* diffusion3d_threestep_form_name(int form) {
  return (form >= 0 && form < NFORMS) ? FORMS[form].name : "invalid";
}

bool diffusion3d_threestep_ok(const DiffusionArgs& a) {
  if (a.form < 0 || a.form >= NFORMS) return false;
  if (a.q == 0) return false;  // the pass has no dividing form
  if (a.elem_bytes != 4 && a.elem_bytes != 8) return false;
  const int vz = 16 / a.elem_bytes;
  if (a.n[0] < 3 || a.n[1] < 3 || a.n[2] < 3) return false;
  if (a.n[2] % vz != 0) return false;  // aligned 16-byte vectors along every row
  if (a.n[2] > int64_t(64) * vz * FORMS[a.form].bz) return false;  // the tile spans the row
  // the kernel's indices and its byte offsets within a plane are 32-bit
  const int64_t lim = int64_t(1) << 31;
  return a.n[0] < lim - 8 && a.n[1] < lim - 8 && a.n[1] * a.n[2] < lim / a.elem_bytes;
}

void launch_diffusion3d_threestep(const DiffusionArgs& a, hipStream_t stream) {
  if (!diffusion3d_threestep_ok(a))
    fail("diffusion3d_threestep: form ", a.form, " cannot run this shape (", a.n[0], ", ", a.n[1], ", ", a.n[2],
         ") at ", a.elem_bytes, " bytes per element", a.q == 0 ? " without the quotient array" : "",
         "; run the two-step pass or single steps");
  if (a.elem_bytes == 8) dispatch3<double>(a, stream);
  else dispatch3<float>(a, stream);
}

}  // namespace igg
