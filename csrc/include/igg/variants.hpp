#pragma once
// The catalogue of the single-step diffusion kernels: every number that names a
// kernel is written here once, with the kernel's template arguments. The tables
// and switches of stencil_kernels.hip, fused_kernels.hip and
// igg/fused_families.hpp are expansions of these row lists: a new tiling is one
// new row (of IGG_RESTRICT_TILINGS* and IGG_HX_VARIANTS for a plain variant, of
// its family's IGG_FUSED_T* for a fused one) and nothing else. Index spaces:
//   * plain variants 0..44 (the autotune, IGG_STENCIL_VARIANT, bench.py,
//     launch_diffusion3d): 0..20 are kernels of stencil_kernels.hip, 21..44 run
//     the inner box through a restrict-form tiling, other boxes through a fallback;
//   * restrict-form tiling ids: the no-exchange sweeps of the fused kernel
//     (launch_diffusion3d_inner_hx, native.diffusion3d_hx_tiling, profiles/);
//   * fused variants (launch_diffusion3d_fused, bench.py's fused candidates).
// One number can mean different things: plain 44 is tiling 0 at two workgroups
// per CU, fused 44 is tiling 14 with the edge-lane z exchange; plain 9 / 11 / 14
// are vector kernels, tiling and fused 9 / 11 / 14 their restrict forms. The
// numbers stay: bench.py and the recorded profiles name them.
// First column, the build class: CORE rows are in every build (the autotune's
// SHORTLIST of ops/stencil.py, the fused A/B's forms, what those fall back to,
// the scalar fallback 1 and the one-row slab kernel 18); PROBES rows were
// measured in rounds 1-4 and never won, and are compiled only with
// `build.py --probes` (IGG_PROBES). IGG_IF_<class>(code) keeps code in the
// builds of the class. The FEAT bits of a row: igg/fused_impl.hpp.
#define IGG_IF_CORE(...) __VA_ARGS__
#define IGG_IS_CORE true
#ifdef IGG_PROBES
#define IGG_IF_PROBES(...) __VA_ARGS__
#define IGG_IS_PROBES true
#else
#define IGG_IF_PROBES(...)
#define IGG_IS_PROBES false
#endif

// Kernels of stencil_kernels.hip: X(class, index, name, S scalar / V vector kernel, BY,
// RY, VZ, PF, NT, BZ). 0: best on MI355X for 512^3 f64 (benchmarks/stencil_sweep.py).
#define IGG_PLAIN_KERNELS(X)                                                        \
  X(CORE, 0, "v4_by4_ry4_nt", V, 4, 4, 4, false, true, 1)                           \
  X(CORE, 1, "s_by4_ry8", S, 4, 8, 1, false, false, 1) /* scalar fallback */           \
  X(CORE, 2, "v2_by4_ry4_pf_nt", V, 4, 4, 2, true, true, 1)                         \
  X(PROBES, 3, "v4_by4_ry4", V, 4, 4, 4, false, false, 1)                           \
  X(PROBES, 4, "v4_by4_ry4_pf_nt", V, 4, 4, 4, true, true, 1)                       \
  X(CORE, 5, "v4_by4_ry2_nt", V, 4, 2, 4, false, true, 1)                           \
  X(PROBES, 6, "v8_by4_ry2_nt", V, 4, 2, 8, false, true, 1)                         \
  X(PROBES, 7, "v4_by2_ry4_nt", V, 2, 4, 4, false, true, 1)                         \
  X(PROBES, 8, "v4_by8_ry2_nt", V, 8, 2, 4, false, true, 1)                         \
  X(CORE, 9, "v4_by4_ry8_nt", V, 4, 8, 4, false, true, 1)                           \
  X(PROBES, 10, "v8_by2_ry2_nt", V, 2, 2, 8, false, true, 1)                        \
  X(CORE, 11, "v2_by4_ry8_nt", V, 4, 8, 2, false, true, 1)                          \
  X(PROBES, 12, "v4_bz2_by8_ry4_nt", V, 8, 4, 4, false, true, 2) /* 1024 threads */    \
  X(PROBES, 13, "v4_bz2_by4_ry4_nt", V, 4, 4, 4, false, true, 2)                    \
  X(CORE, 14, "v4_bz2_by2_ry8_nt", V, 2, 8, 4, false, true, 2)                      \
  X(PROBES, 15, "v2_bz2_by4_ry8_nt", V, 4, 8, 2, false, true, 2)                    \
  X(PROBES, 16, "v4_bz2_by8_ry2_nt", V, 8, 2, 4, false, true, 2)                    \
  X(PROBES, 17, "v2_bz4_by4_ry4_nt", V, 4, 4, 2, false, true, 4)                    \
  X(CORE, 18, "s_by4_ry1", S, 4, 1, 1, false, false, 1) /* low-VGPR: thin send planes */ \
  X(PROBES, 19, "v2_by4_ry1_nt", V, 4, 1, 2, false, true, 1) /* low-VGPR vector */     \
  X(PROBES, 20, "v4_by4_ry2", V, 4, 2, 4, false, false, 1)

// Restrict-form tilings: X(class, id, BY, RY, VZ, PF, BZ, extra FEAT). The first
// list has the partial-line and the whole-line (HZ, halo_z) z-edge store form:
// the autotune times both (models/diffusion3d.py).
#define IGG_RESTRICT_TILINGS_HZ(X)                                                  \
  X(CORE, 0, 4, 4, 4, false, 1, 0)                                                  \
  X(CORE, 11, 4, 8, 2, false, 1, 0)                                                 \
  X(CORE, 100, 2, 8, 2, false, 1, 0)                                                \
  X(CORE, 124, 4, 8, 2, false, 1, ZSEG | OCC1)                                      \
  X(CORE, 141, 2, 8, 2, false, 4, 0) /* full-row z tiles, profiles/r2_fullrow/ */   \
  X(CORE, 150, 4, 4, 4, false, 1, OCC2) /* f32 1024^3: +2.5 %, profiles/r6_vsweep/ */ \
  X(PROBES, 9, 4, 8, 4, false, 1, 0)                                                \
  X(PROBES, 14, 2, 8, 4, false, 2, 0)
// One form (halo_z ignored): other tilings, non-temporal Cp (11x), lane-distributed
// z-segment edges (12x), timing probes with wrong results (13x), wider z tiles
// (14x), the reversed march (200, 211, 300, 324), temporal stores (411, 611).
#define IGG_RESTRICT_TILINGS(X)                                                     \
  X(PROBES, 2, 4, 4, 2, true, 1, 0)                                                 \
  X(PROBES, 101, 4, 6, 2, false, 1, 0)                                              \
  X(PROBES, 102, 4, 8, 2, true, 1, 0)                                               \
  X(PROBES, 103, 4, 4, 2, false, 1, 0)                                              \
  X(PROBES, 104, 4, 2, 4, false, 1, 0)                                              \
  X(PROBES, 105, 8, 4, 2, false, 1, 0)                                              \
  X(PROBES, 110, 4, 8, 2, false, 1, NT_CP)                                          \
  X(PROBES, 111, 4, 4, 4, false, 1, NT_CP)                                          \
  X(PROBES, 112, 4, 8, 4, false, 1, NT_CP)                                          \
  X(PROBES, 113, 2, 8, 4, false, 2, NT_CP)                                          \
  X(PROBES, 120, 4, 8, 2, false, 1, ZSEG)                                           \
  X(PROBES, 121, 4, 8, 4, false, 1, ZSEG)                                           \
  X(PROBES, 122, 2, 8, 2, false, 1, ZSEG)                                           \
  X(PROBES, 123, 4, 4, 4, false, 1, ZSEG)                                           \
  X(PROBES, 125, 4, 10, 2, false, 1, ZSEG | OCC1)                                   \
  X(PROBES, 126, 4, 12, 2, false, 1, ZSEG | OCC1)                                   \
  X(PROBES, 130, 4, 8, 2, false, 1, ZSEG | OCC1 | PROBE_NO_ZSEG)                    \
  X(PROBES, 131, 4, 8, 2, false, 1, ZSEG | OCC1 | PROBE_NO_YROWS)                   \
  X(PROBES, 132, 4, 8, 2, false, 1, ZSEG | OCC1 | PROBE_NO_ZSEG | PROBE_NO_YROWS)   \
  X(PROBES, 140, 4, 8, 2, false, 4, 0)                                              \
  X(PROBES, 142, 4, 4, 2, false, 4, 0)                                              \
  X(PROBES, 143, 4, 4, 4, false, 2, 0)                                              \
  X(PROBES, 144, 4, 8, 4, false, 2, 0)                                              \
  X(PROBES, 145, 2, 8, 2, false, 4, ZSEG)                                           \
  X(PROBES, 200, 4, 4, 4, false, 1, PROBE_REVERSE)                                  \
  X(PROBES, 211, 4, 8, 2, false, 1, PROBE_REVERSE)                                  \
  X(PROBES, 300, 2, 8, 2, false, 1, PROBE_REVERSE)                                  \
  X(PROBES, 324, 4, 8, 2, false, 1, ZSEG | OCC1 | PROBE_REVERSE)                    \
  X(PROBES, 411, 4, 8, 2, false, 1, PROBE_T_STORE)                                  \
  X(PROBES, 611, 4, 8, 2, false, 1, PROBE_T_STORE | PROBE_REVERSE)

// Plain variants 21..44: X(class, index, name, tiling id, fallback). The inner box
// goes through the tiling's restrict form (13-26 us faster than diffusion3d_vkernel
// with the same tiling, profiles/r1_fused/), any other box list through kernel
// `fallback`, whose tile width the variant reports; its vector is the tiling's.
#define IGG_HX_VARIANTS(X)                                                          \
  X(CORE, 21, "hx_v4_by4_ry4_nt", 0, 0)                                             \
  X(PROBES, 22, "hx_v2_by4_ry4_pf_nt", 2, 2)                                        \
  X(PROBES, 23, "hx_v4_by4_ry8_nt", 9, 9)                                           \
  X(CORE, 24, "hx_v2_by4_ry8_nt", 11, 11)                                           \
  X(PROBES, 25, "hx_v4_bz2_by2_ry8_nt", 14, 14)                                     \
  X(CORE, 26, "hx_v2_by2_ry8_nt", 100, 11)                                          \
  X(PROBES, 27, "hx_v2_by4_ry6_nt", 101, 11)                                        \
  X(PROBES, 28, "hx_v2_by4_ry8_pf_nt", 102, 11)                                     \
  X(PROBES, 29, "hx_v2_by4_ry4_nt", 103, 2)                                         \
  X(PROBES, 30, "hx_v4_by4_ry2_nt", 104, 5)                                         \
  X(PROBES, 31, "hx_v2_by8_ry4_nt", 105, 11)                                        \
  X(PROBES, 32, "hx_v2_by4_ry8_nt_ntc", 110, 11) /* non-temporal Cp loads */        \
  X(PROBES, 33, "hx_v4_by4_ry4_nt_ntc", 111, 0)                                     \
  X(PROBES, 34, "hx_v4_by4_ry8_nt_ntc", 112, 9)                                     \
  X(PROBES, 35, "hx_v4_bz2_by2_ry8_nt_ntc", 113, 14)                                \
  X(PROBES, 36, "hx_v2_by4_ry8_nt_zl", 120, 11) /* lane-distributed z-segment edge loads */ \
  X(PROBES, 37, "hx_v4_by4_ry8_nt_zl", 121, 9)                                      \
  X(PROBES, 38, "hx_v2_by2_ry8_nt_zl", 122, 11)                                     \
  X(PROBES, 39, "hx_v4_by4_ry4_nt_zl", 123, 0)                                      \
  X(CORE, 40, "hx_v2_by4_ry8_nt_zl_occ1", 124, 11) /* + one workgroup per CU, profiles/r1_zl/ */ \
  X(PROBES, 41, "hx_v2_by4_ry10_nt_zl_occ1", 125, 11)                               \
  X(PROBES, 42, "hx_v2_by4_ry12_nt_zl_occ1", 126, 11)                               \
  X(CORE, 43, "hx_v2_bz4_by2_ry8_nt", 141, 11)                                      \
  X(CORE, 44, "hx_v4_by4_ry4_nt_occ2", 150, 0)

// Fused variants: X(class, index, BY, RY, VZ, PF, BZ, extra FEAT), one list per
// family, the units fused_<family>_{f64,f32}.hip that instantiate its rows (t9:
// tiling 9 with the side-only z forms, profiles/r4_shapes/ pass 4).
#define IGG_FUSED_T0(X)                                                             \
  X(CORE, 0, 4, 4, 4, false, 1, 0)                                                  \
  X(CORE, 50, 4, 4, 4, false, 1, OCC1)                                              \
  X(PROBES, 45, 4, 4, 4, false, 1, Z_EDGE_LANE)
#define IGG_FUSED_T11(X)                                                            \
  X(PROBES, 11, 4, 8, 2, false, 1, 0)                                               \
  X(PROBES, 41, 4, 8, 2, false, 1, ZSEG | OCC1 | Z_LDS)                             \
  X(CORE, 40, 4, 8, 2, false, 1, ZSEG | OCC1)                                       \
  X(CORE, 42, 4, 8, 2, false, 1, ZSEG | OCC1 | Z_EDGE_LANE)
#define IGG_FUSED_T9(X)                                                             \
  X(CORE, 9, 4, 8, 4, false, 1, ZSIDES)                                             \
  X(CORE, 48, 4, 8, 4, false, 1, ZSIDES | ZDPP)
#define IGG_FUSED_T14(X)                                                            \
  X(PROBES, 2, 4, 4, 2, true, 1, 0) /* tiling 2's only fused form is built in this unit */ \
  X(CORE, 14, 2, 8, 4, false, 2, 0)                                                 \
  X(CORE, 44, 2, 8, 4, false, 2, Z_EDGE_LANE) /* the f32 form cannot hide per-row v_readlane, profiles/r2_f32_fused/ */
#define IGG_FUSED_VARIANTS(X) IGG_FUSED_T0(X) IGG_FUSED_T11(X) IGG_FUSED_T9(X) IGG_FUSED_T14(X)

namespace igg {

// Host tables: a variant has vz / bz of its own kernel and tiling -1 (0..20), or
// a tiling id and a fallback (21..44).
struct VariantRow {
  int index;
  const char* name;
  int vz, bz, tiling, fallback;
  bool compiled;
};
struct TilingRow { int id, vz; bool compiled; };
#define IGG_ROW(C, I, NAME, K, BY, RY, VZ, PF, NT, BZ) {I, NAME, VZ, BZ, -1, I, IGG_IS_##C},
#define IGG_ROW_HX(C, I, NAME, TILING, FALLBACK) {I, NAME, 0, 0, TILING, FALLBACK, IGG_IS_##C},
inline constexpr VariantRow VARIANTS[] = {IGG_PLAIN_KERNELS(IGG_ROW) IGG_HX_VARIANTS(IGG_ROW_HX)};
#undef IGG_ROW
#undef IGG_ROW_HX
#define IGG_ROW(C, ID, BY, RY, VZ, PF, BZ, F) {ID, VZ, IGG_IS_##C},
inline constexpr TilingRow TILINGS[] = {IGG_RESTRICT_TILINGS_HZ(IGG_ROW) IGG_RESTRICT_TILINGS(IGG_ROW)};
#undef IGG_ROW
constexpr int NVARIANTS = sizeof(VARIANTS) / sizeof(VARIANTS[0]);

constexpr const TilingRow* restrict_tiling(int id) {  // nullptr: no such tiling
  for (const TilingRow& t : TILINGS)
    if (t.id == id) return &t;
  return nullptr;
}

// Indices dense and ascending; tiling ids unique; every 21+ row names a tiling
// and a fallback kernel that exist and are compiled whenever the row is.
constexpr bool catalogue_ok() {
  for (int i = 0; i < NVARIANTS; ++i) {
    const VariantRow& r = VARIANTS[i];
    if (r.index != i) return false;
    if (r.tiling < 0) continue;
    const TilingRow* t = restrict_tiling(r.tiling);
    if (!t || r.fallback < 0 || r.fallback >= i || VARIANTS[r.fallback].tiling >= 0) return false;
    if (r.compiled && !(t->compiled && VARIANTS[r.fallback].compiled)) return false;
  }
  for (const TilingRow& t : TILINGS)
    if (restrict_tiling(t.id) != &t) return false;
  return true;
}
static_assert(catalogue_ok(), "an index out of order, a tiling id twice, or a 21+ row with a bad tiling or fallback");

}  // namespace igg
