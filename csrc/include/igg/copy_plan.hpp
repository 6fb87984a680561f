// Host-side plan of one batched copy: the box as the kernel will see it and
// the path it takes (copy_kernels.hip). Plain host C++, shared by the
// launchers and by the tests (native.copy2d_plan / copy3d_plan), so what the
// tests assert about a descriptor is what the launch does with it.
#pragma once

#include <cstdint>

#include "igg/copy.hpp"

namespace igg {

// Launch geometry of copy2d_batch_kernel / copy3d_batch_kernel.
constexpr int COPY_BLOCK = 256;
constexpr int COPY_EPT = 4;                              // elements per thread per chunk
constexpr int64_t COPY_CHUNK = COPY_BLOCK * COPY_EPT;    // elements of a row per workgroup
constexpr int COPY_GROWS = 8;                            // outer rows per lane (gather paths)

// IGG_COPY_GATHER (copy_kernels.hip): the plan functions take it as an argument.
extern bool g_copy_gather;

enum class CopyPath { flat, gather, chunk };

inline const char* copy_path_name(CopyPath p) {
  return p == CopyPath::flat ? "flat" : p == CopyPath::gather ? "gather" : "chunk";
}

struct CopyPlan2 {
  Copy2D box;
  CopyPath path = CopyPath::flat;
  int vec_bytes = 0;   // always 0: the 2-D kernel has no vector rows
  int64_t blocks = 0;  // 0 for an empty copy (the launcher skips it)
};

struct CopyPlan3 {
  Copy3D box;  // normalized
  CopyPath path = CopyPath::flat;
  int vec_bytes = 0;  // gather: a row is one aligned access of 4, 8 or 16 bytes; 0: scalar
  int64_t blocks = 0;
};

// Merge extents that are adjacent in memory on both sides, then order the box
// for the kernel's shapes. The element order of the copy does not change.
Copy3D normalized(Copy3D c);

// A row of `c` (normalized) is one 4-, 8- or 16-byte access, aligned on both sides.
bool aligned_rows(const Copy3D& c, int elem_bytes, const ParityShift& par);

CopyPlan2 plan_copy2d(const Copy2D& c, int elem_bytes, bool gather);
CopyPlan3 plan_copy3d(const Copy3D& c, int elem_bytes, const ParityShift& par, bool gather);

}  // namespace igg
