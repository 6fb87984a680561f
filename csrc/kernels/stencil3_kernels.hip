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
// Form 1 (Q in LDS): a wave holds of Q only the plane stage 1 reads; the lane
// parks each value in an LDS slot of its own after stage 1 and reads it back
// for stages 2 and 3 (no barrier: nobody else touches the slot). T's values
// around a wave's rows and segment come from the neighbouring waves' registers
// through LDS as well, one position ahead, as those of the intermediate fields
// do; only the row beyond the tile is loaded. The registers that frees go into
// a fifth row per wave: a 10-row tile writes 6 rows, 4.0 row updates per
// written row and pass instead of 4.5, and every row of T and Q is pulled from
// L2 2.0 and 1.67 times per written row instead of 2.5 and 2.0.
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

template <typename T, int BY, int RY, int VZ, int BZ>
__global__ void __launch_bounds__(64 * BY * BZ)
diffusion3d_threestep_qlds_kernel(const K2Args<T> a) {
  threestep::body_qlds<T, BY, RY, VZ, BZ>(a);
}

struct Form {
  const char* name;
  int by, ry, bz;
  bool qlds;  // Q parked in LDS between the stages
};

// Lanes hold 16 bytes, as in the two-step pass: form 0 spans a 512-point f64 /
// 1024-point f32 row.
constexpr Form FORMS[] = {
    {"t3_by2_ry4_bz4", 2, 4, 4, false},      // 0: 8 rows x 512 (f64) tile, 4 rows written, 512 threads, 116 KiB LDS
    {"t3_by2_ry5_bz4_qlds", 2, 5, 4, true},  // 1: 10 rows x 512 (f64) tile, 6 rows written, 512 threads, 143 KiB LDS
};
constexpr int NFORMS = sizeof(FORMS) / sizeof(FORMS[0]);

template <typename T, int BY, int RY, int BZ, bool QL>
auto kernel3() {
  constexpr int VZ = 16 / static_cast<int>(sizeof(T));
  if constexpr (QL) return &diffusion3d_threestep_qlds_kernel<T, BY, RY, VZ, BZ>;
  else return &diffusion3d_threestep_kernel<T, BY, RY, VZ, BZ>;
}

// What a form does: launch (stream) or, with stream == nullptr and `target`
// set, only report the workgroups a launch with a.rounds aims at.
template <typename T, int BY, int RY, int BZ, bool QL = false>
void launch3(const DiffusionArgs& a, hipStream_t stream, int64_t* target) {
  if (target)
    *target = diffusion3d_target_blocks(reinterpret_cast<const void*>(kernel3<T, BY, RY, BZ, QL>()), 64 * BY * BZ, a.rounds);
  else
    threestep::launch_form<T, BY, RY, BZ>(kernel3<T, BY, RY, BZ, QL>(), a, stream);
}

template <typename T>
void dispatch3(const DiffusionArgs& a, hipStream_t s, int64_t* target = nullptr) {
  switch (a.form) {
    case 0: launch3<T, 2, 4, 4>(a, s, target); break;
    case 1: launch3<T, 2, 5, 4, true>(a, s, target); break;
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

ThreestepPlan diffusion3d_threestep_plan(const DiffusionArgs& a, int64_t target) {
  if (a.form < 0 || a.form >= NFORMS) fail("diffusion3d_threestep: no form ", a.form);
  if (a.n[0] < 3 || a.n[1] < 3) fail("diffusion3d_threestep: every extent must be >= 3");
  return threestep::plan(a.n[0], a.n[1], FORMS[a.form].by * FORMS[a.form].ry - 4, target);
}

int64_t diffusion3d_threestep_target(const DiffusionArgs& a) {
  int64_t target = 0;
  if (a.elem_bytes == 8) dispatch3<double>(a, nullptr, &target);
  else if (a.elem_bytes == 4) dispatch3<float>(a, nullptr, &target);
  else fail("diffusion3d_threestep: 4 or 8 bytes per element");
  return target;
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
