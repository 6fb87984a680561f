// Fused halo-exchange diffusion kernels, tiling 11: the rows of IGG_FUSED_T11 (igg/variants.hpp), double.
// One (family, element type) per translation unit: igg/fused_families.hpp.
#include "igg/fused_families.hpp"

namespace igg {
template bool fused_family_t11<double>(const DiffusionArgs&, const HaloIOArgs&, int, int, hipStream_t);
}  // namespace igg
