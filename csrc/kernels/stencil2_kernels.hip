// Two diffusion time steps in one pass over memory (temporal blocking) for
// gfx950: t2 = step(step(t)) on the whole inner box of a rank without
// neighbours, bitwise what two launch_diffusion3d calls leave (every point goes
// through diffusion_point_q, devmath.hpp; the boundary planes keep t's values
// in the intermediate field, as they do in the ping-pong loop).
//
// The single-step loop moves 3 arrays per step (read T, read Cp, write T2);
// here the intermediate field never reaches memory: about 1 write + (1 + ring)
// reads of T and Cp per TWO steps.
//
// Shape: a 2.5-D march along dim 0 like diffusion3d_vkernel. A workgroup of
// BY x BZ waves owns TYE = BY*RY rows x W = 64*VZ*BZ points of the (dim 1,
// dim 2) plane: the outer rows are the 1-wide ring of the intermediate field,
// the TYE-2 inner rows are written. Tiles advance by TYE-2 rows (rows have no
// alignment to keep) and by W points (vector accesses stay aligned). At march
// position p a lane
//   1. forms the intermediate plane p at its own points from T planes p-1, p,
//      p+1 (registers; y neighbours beyond the wave's rows and the two z
//      segment-edge values are loaded, as in the single-step kernel);
//   2. issues the loads of the next position (T plane p+2, Cp plane p+1);
//   3. forms output plane p-1 from intermediate planes p-2, p-1, p: x
//      neighbours and the wave's own rows are registers, z neighbours lane
//      neighbours; the first/last row of every wave and the wave-edge z values
//      of intermediate plane p-1 come from LDS (one buffer per phase of the
//      march, one barrier per position);
//   4. puts those parts of plane p into the next LDS buffer.
// dtlam/Cp is divided once per point and kept for the second use, or read
// from the quotient array (DiffusionArgs::q) and not divided at all. Where a
// tile does not span the row, the intermediate values at z = zt-1 and zt+W
// (the z ring) are formed by 2*TYE "edge" threads with scalar loads. An x chunk
// [xs, xe) starts with the two-position lead-in p = xs-1, xs.
//
// The kernel body is igg/stencil2_impl.hpp. This unit holds one kernel per
// (form, dtype) - the general one - and the dispatch; the specialisations are
// instantiated in stencil2q_kernels.hip.
#include <hip/hip_runtime.h>

#include "igg/stencil2_impl.hpp"

namespace igg {
namespace {

using twostep::K2Args;

// The general kernel of a form: any shape, z ring included, reads Cp (the
// body and the specialisations: stencil2_impl.hpp, stencil2q_kernels.hip).
template <typename T, int BY, int RY, int VZ, int BZ>
__global__ void __launch_bounds__(64 * BY * BZ)
diffusion3d_twostep_kernel(const K2Args<T> a) {
  twostep::body<T, BY, RY, VZ, BZ, false, false>(a);
}

struct Form {
  const char* name;
  int by, ry, bz;
};

// Lanes hold 16 bytes (VZ = 2 f64 / 4 f32), so a tile is 128*BZ f64 or 256*BZ
// f32 points wide: form 0 spans a 512-point f64 / 1024-point f32 row (no z
// ring). RY = 4 is the most the register file holds without scratch at two
// waves per SIMD (RY = 5 and 6 spill).
constexpr Form FORMS[] = {
    {"t2_by2_ry4_bz4", 2, 4, 4},  // 0: 8 rows x 512 (f64) tile, 512 threads
    {"t2_by4_ry4_bz2", 4, 4, 2},  // 1: 16 rows x 256, 512 threads
    {"t2_by4_ry4_bz1", 4, 4, 1},  // 2: 16 rows x 128, 256 threads (two workgroups per CU)
};
constexpr int NFORMS = sizeof(FORMS) / sizeof(FORMS[0]);

template <typename T, int BY, int RY, int BZ>
void launch_general(const DiffusionArgs& a, hipStream_t stream) {
  constexpr int VZ = 16 / static_cast<int>(sizeof(T));
  // a tile that spans the row, or the quotient input: the other unit's kernels
  if (a.q != 0 || a.n[2] <= twostep::tile_width<T, BZ>()) return launch_diffusion3d_twostep_special(a, stream);
  twostep::launch_form<T, BY, RY, BZ>(&diffusion3d_twostep_kernel<T, BY, RY, VZ, BZ>, a, false, stream);
}

template <typename T>
void dispatch2(const DiffusionArgs& a, hipStream_t s) {
  switch (a.form) {
    case 0: launch_general<T, 2, 4, 4>(a, s); break;
    case 1: launch_general<T, 4, 4, 2>(a, s); break;
    case 2: launch_general<T, 4, 4, 1>(a, s); break;
    default: fail("diffusion3d_twostep: no form ", a.form);
  }
}

}  // namespace

int diffusion3d_twostep_num_forms() { return NFORMS; }
const char* diffusion3d_twostep_form_name(int form) {
  return (form >= 0 && form < NFORMS) ? FORMS[form].name : "invalid";
}

bool diffusion3d_twostep_ok(const DiffusionArgs& a) {
  if (a.form < 0 || a.form >= NFORMS) return false;
  if (a.elem_bytes != 4 && a.elem_bytes != 8) return false;
  const int vz = 16 / a.elem_bytes;
  if (a.n[0] < 3 || a.n[1] < 3 || a.n[2] < 3) return false;
  if (a.n[2] % vz != 0) return false;  // aligned 16-byte vectors along every row
  // the kernel's indices and its byte offsets within a plane are 32-bit
  const int64_t lim = int64_t(1) << 31;
  return a.n[0] < lim - 8 && a.n[1] < lim && a.n[2] < lim && a.n[1] * a.n[2] < lim / a.elem_bytes;
}

void launch_diffusion3d_twostep(const DiffusionArgs& a, hipStream_t stream) {
  if (!diffusion3d_twostep_ok(a))
    fail("diffusion3d_twostep: form ", a.form, " cannot run this shape (", a.n[0], ", ", a.n[1], ", ", a.n[2],
         ") at ", a.elem_bytes, " bytes per element; run two single steps");
  if (a.elem_bytes == 8) dispatch2<double>(a, stream);
  else dispatch2<float>(a, stream);
}

}  // namespace igg
