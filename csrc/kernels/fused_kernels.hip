// Fused halo-exchange diffusion kernel for gfx950 (see igg/fused.hpp): the
// restrict-argument plain sweeps (stencil variants 21+) and the entry points.
// The kernel templates live in igg/fused_impl.hpp; the fused instantiations in
// fused_t{0,11,9,14}_{f64,f32}.hip (one tiling family and type each).
#include "igg/fused_impl.hpp"

namespace igg {

int64_t* g_hx_stamps = nullptr;
int g_hx_force_sel = -1;

namespace {

// The sweep without any exchange feature (FEAT=0): the plain inner-box
// update through this kernel's restrict-argument form, measured 13-26 us
// faster than diffusion3d_vkernel with the same tiling (profiles/r1_fused/
// feature_bisect_v11.log); bitwise identical arithmetic.
template <typename T>
void dispatch_plain(const DiffusionArgs& d, int v, hipStream_t s) {
  const HaloIOArgs none{};
  switch (v) {  // igg/variants.hpp: the tilings with both z-edge store forms, then those with one
#define IGG_ROW_HZ(C, ID, BY, RY, VZ, PF, BZ, F)                                                          \
  IGG_IF_##C(case ID:                                                                                     \
             d.halo_z ? launch_hx<T, BY, RY, VZ, PF, BZ, false, (F) | HZ>(d, none, s)                     \
                      : launch_hx<T, BY, RY, VZ, PF, BZ, false, (F)>(d, none, s);                         \
             break;)
#define IGG_ROW(C, ID, BY, RY, VZ, PF, BZ, F) \
  IGG_IF_##C(case ID: launch_hx<T, BY, RY, VZ, PF, BZ, false, (F)>(d, none, s); break;)
    IGG_RESTRICT_TILINGS_HZ(IGG_ROW_HZ)
    IGG_RESTRICT_TILINGS(IGG_ROW)
#undef IGG_ROW
#undef IGG_ROW_HZ
    default: fail("diffusion3d (restrict form): tiling ", v, " not instantiated");
  }
}

// Tile of fused variant v (igg/variants.hpp); false: none, or not in this build.
bool fused_row(int v, FusedTile* t) {
  switch (v) {
#define IGG_ROW(C, V, BY, RY, VZ, PF, BZ, XF) \
  case V: *t = FusedTile{BY, RY, VZ, BZ, ((XF) & ZDPP) != 0}; return IGG_IS_##C;
    IGG_FUSED_VARIANTS(IGG_ROW)
#undef IGG_ROW
    default: return false;
  }
}

template <typename T>
bool fused_any_family(const DiffusionArgs& a, const HaloIOArgs& io, int v, int mode, hipStream_t s) {
  return fused_family_t0<T>(a, io, v, mode, s) || fused_family_t11<T>(a, io, v, mode, s) ||
         fused_family_t9<T>(a, io, v, mode, s) || fused_family_t14<T>(a, io, v, mode, s);
}

}  // namespace

void launch_diffusion3d_inner_hx(const DiffusionArgs& a, int tiling, hipStream_t stream) {
  if (a.n[0] < 3 || a.n[1] < 3 || a.n[2] < 3) fail("diffusion3d: every extent must be >= 3");
  if (a.elem_bytes == 8) dispatch_plain<double>(a, tiling, stream);
  else if (a.elem_bytes == 4) dispatch_plain<float>(a, tiling, stream);
  else fail("diffusion3d: only float32/float64 are supported");
}

void fused_debug(int64_t* stamps, int force_sel) {
  g_hx_stamps = stamps;
  g_hx_force_sel = force_sel;
}

bool diffusion3d_fused_variant_ok(int v) {
  FusedTile t;
  return fused_row(v, &t);
}

std::vector<int> diffusion3d_fused_variants() {
#define IGG_ROW(C, V, BY, RY, VZ, PF, BZ, XF) V,
  std::vector<int> vs{IGG_FUSED_VARIANTS(IGG_ROW)};
#undef IGG_ROW
  std::sort(vs.begin(), vs.end());
  return vs;
}

FusedTile diffusion3d_fused_tile(int v) {
  FusedTile t;
  if (!fused_row(v, &t)) fail("diffusion3d (fused halo): variant ", v, " has no fused instantiation");
  return t;
}

void launch_diffusion3d_fused(const DiffusionArgs& a, const HaloIOArgs& io, int variant, int mode,
                              hipStream_t stream) {
  if (a.n[0] < 3 || a.n[1] < 3 || a.n[2] < 3) fail("diffusion3d: every extent must be >= 3");
  if (mode < 0 || mode > 63 || (mode & 16))
    fail("diffusion3d (fused halo): send mode must be 0..63 without bit 16 (step sync: FusedHalo)");
  if (a.elem_bytes != 8 && a.elem_bytes != 4) fail("diffusion3d: only float32/float64 are supported");
  const bool ok = a.elem_bytes == 8 ? fused_any_family<double>(a, io, variant, mode, stream)
                                    : fused_any_family<float>(a, io, variant, mode, stream);
  if (!ok) fail("diffusion3d (fused halo): variant ", variant, " has no fused instantiation");
}

}  // namespace igg
