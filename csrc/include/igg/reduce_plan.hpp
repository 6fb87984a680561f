// Host-side plan of one reduction job: the owned box of a field as the kernel
// will see it and the path it takes (reduce_kernels.hip). Plain host C++,
// shared by the launcher and by the tests (native.reduce_plan), so what the
// tests assert about a plan is what the launch does with it.
//
// The kernel sees every box as n[0] x n[1] rows of n[2] elements and covers it
// with TILES: a tile is one load per lane of a 256-lane workgroup, LX lanes
// along a row and LY = 256 / LX rows (LX the power of two that holds a row, at
// most 256). A workgroup takes REDUCE_UNROLL consecutive tiles per iteration,
// grid-stride. The number of workgroups is a function of the box alone - never
// of the device (CU count, occupancy) - so the order of every addition, and
// with it every bit of the result, is the same on every run and device mode.
#pragma once

#include <cstdint>
#include <vector>

namespace igg {

constexpr int REDUCE_BLOCK = 256;        // lanes per workgroup
constexpr int REDUCE_UNROLL = 4;         // independent loads per lane and input in flight
constexpr int REDUCE_MAX_BLOCKS = 1024;  // workgroups per job (cap)
constexpr int REDUCE_MAX_JOBS = 32;      // jobs per launch (descriptor table)

// flat: one unit-stride run, 16-B loads, any element-aligned base (the head
//   vector is aligned down and masked);
// rows: unit inner stride, 16-B-aligned base and row pitches, 16-B loads
//   aligned down at the head of each row, masked at head and tail;
// element: any strides and alignment, one element per load.
enum class ReducePath { flat, rows, element };

inline const char* reduce_path_name(ReducePath p) {
  return p == ReducePath::flat ? "flat" : p == ReducePath::rows ? "rows" : "element";
}

struct ReducePlan {
  ReducePath path = ReducePath::element;
  int64_t n[3] = {1, 1, 1};    // merged extents, outer .. inner
  int64_t s[3] = {0, 0, 1};    // strides of the first input in elements
  int64_t sb[3] = {0, 0, 1};   // strides of the second input (two-input ops)
  int64_t offset = 0;          // elements from the first input's base to the box's first element
  int64_t offset_b = 0;
  int64_t total = 0;           // elements of the box
  int vec = 1;                 // elements per load: 16 / elem_size, or 1 (element path)
  int head = 0;                // elements by which a row's first load starts before the row
  int64_t nv = 0;              // loads per row
  int lx_log2 = 0;             // log2 of LX
  int64_t cx = 0;              // tiles along a row
  int64_t g1 = 0;              // row groups (LY rows each) per index of n[0]
  int64_t tiles = 0;
  int64_t blocks = 0;          // 0: an empty box (the launcher skips it)
};

// `shape`, `strides` (elements), `lo`, `hi` (the box, half-open) have one entry
// per dimension (1 .. 3). `strides_b` / `base_b` describe the second input of
// a two-input op (same shape and box); empty: none. Extents that are
// contiguous in the box - for both inputs - are merged, so a fully owned dense
// array is one flat run.
ReducePlan plan_reduce(const std::vector<int64_t>& shape, const std::vector<int64_t>& strides,
                       const std::vector<int64_t>& lo, const std::vector<int64_t>& hi, int elem_size,
                       uintptr_t base_address, const std::vector<int64_t>& strides_b = {},
                       uintptr_t base_b = 0);

}  // namespace igg
