// Fused halo-exchange diffusion kernels, tiling 14: the rows of IGG_FUSED_T14 (igg/variants.hpp), float.
// One (family, element type) per translation unit: igg/fused_families.hpp.
#include "igg/fused_families.hpp"

namespace igg {
template bool fused_family_t14<float>(const DiffusionArgs&, const HaloIOArgs&, int, int, hipStream_t);
}  // namespace igg
