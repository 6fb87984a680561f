// Fused halo-exchange diffusion kernels, tiling 9 with side-only z forms: the rows of IGG_FUSED_T9 (igg/variants.hpp), double.
// One (family, element type) per translation unit: igg/fused_families.hpp.
#include "igg/fused_families.hpp"

namespace igg {
template bool fused_family_t9<double>(const DiffusionArgs&, const HaloIOArgs&, int, int, hipStream_t);
}  // namespace igg
