#pragma once
// Fused halo-exchange kernel families (tiling x exchange forms) for the
// fused_t*_<dt>.hip translation units: each unit explicitly instantiates ONE
// family for ONE element type, so the build compiles them in parallel. A
// family's variants are the rows of its list IGG_FUSED_T* in igg/variants.hpp.
#include "igg/fused_impl.hpp"

namespace igg {

#define IGG_ROW(C, V, BY, RY, VZ, PF, BZ, XF) \
  IGG_IF_##C(case V: launch_mode<T, BY, RY, VZ, PF, BZ, XF>(d, io, mode, s); break;)
#define IGG_FUSED_FAMILY(NAME, ROWS)                                                                     \
  template <typename T>                                                                                  \
  bool NAME(const DiffusionArgs& d, const HaloIOArgs& io, int v, int mode, hipStream_t s) {              \
    switch (v) {                                                                                         \
      ROWS(IGG_ROW)                                                                                      \
      default: return false;                                                                             \
    }                                                                                                    \
    return true;                                                                                         \
  }
IGG_FUSED_FAMILY(fused_family_t0, IGG_FUSED_T0)
IGG_FUSED_FAMILY(fused_family_t11, IGG_FUSED_T11)
IGG_FUSED_FAMILY(fused_family_t9, IGG_FUSED_T9)
IGG_FUSED_FAMILY(fused_family_t14, IGG_FUSED_T14)
#undef IGG_FUSED_FAMILY
#undef IGG_ROW

}  // namespace igg
