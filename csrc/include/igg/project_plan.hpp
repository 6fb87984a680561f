// Host-side plan of one projection job: a reduction over SOME axes of a box
// that keeps the others (project_kernels.hip, ops/reduce.py project_g). Plain
// host C++, shared by the launcher and by the tests (native.project_plan), so
// what the tests assert about a plan is what the launch does with it.
//
// The plan orders the axes of the box by stride (outer .. inner), marks each
// kept (K) or reduced (R), drops extents of one and merges neighbours of the
// same kind that are contiguous in the box. The kind of the innermost axis
// picks the kernel family:
//
//   family 1, inner axis kept (R.R.K, K.R.K, R.K.K): slots [KO, R0, R1, KI].
//     Lanes lie along KI, one load (16 B or one element) each, and own the
//     outputs of that load. The reduced range R0 x R1 is cut into `slices`;
//     a UNIT is one (KO index, slice) pair, a workgroup holds LX lanes along
//     the row times 256 / LX units.
//   family 2, inner axis reduced (K.R.R, R.K.R, K.K.R): slots [K0, K1, RO, RI].
//     A GROUP of G lanes lies along a row of RI; a row is `cx` chunks of G
//     loads, an output has RO x cx TILES, cut into `slices`; a unit is one
//     (slice, output) pair and belongs to one group, 256 / G units a workgroup.
//
// Every (slice, output) pair gives one partial (value, NaN flag) at
// partials[slice * nout + p], p the output's C-order index over the kept
// extents in MEMORY order; `keep_pstride` maps a kept axis' index to p. The
// second stage combines an output's slices in index order. Slices, units and
// the number of workgroups are functions of the box and the keep-set alone -
// never of the device - so one box gives the same bits on every run.
#pragma once

#include <cstdint>
#include <vector>

namespace igg {

constexpr int PROJECT_BLOCK = 256;        // lanes per workgroup
constexpr int PROJECT_UNROLL1 = 8;        // family 1: independent loads per lane and input in flight (two inputs;
                                          // a one-input op takes twice as many: the same bytes)
constexpr int PROJECT_UNROLL2 = 4;        // family 2
constexpr int PROJECT_MAX_BLOCKS = 1024;  // workgroups of the first stage (cap; they walk their units grid-stride)
constexpr int PROJECT_MAX_SLICES = 256;   // partials per output (cap)
constexpr int PROJECT_MIN_GROUP_LOG2 = 2; // family 2: the shortest group is 4 lanes

struct ProjectPlan {
  int family = 2;
  bool vector = false;           // 16-B loads aligned down at the head of each row; else one element per load
  char pattern[4] = {0, 0, 0, 0};  // merged axes outer .. inner, e.g. "KRK"
  int64_t n[4] = {1, 1, 1, 1};   // extents of the family's slots
  int64_t s[4] = {0, 0, 0, 1};   // strides of the first input in elements
  int64_t sb[4] = {0, 0, 0, 1};  // strides of the second input (two-input ops)
  int64_t offset = 0;            // elements from the first input's base to the box's first element
  int64_t offset_b = 0;
  int64_t total = 0;             // elements of the box
  int64_t nout = 0;              // outputs: the product of the kept extents
  int vec = 1;                   // elements per load
  int head = 0;                  // elements by which a row's first load starts before the row
  int64_t nv = 0;                // loads per row
  int lanes_log2 = 0;            // log2 of LX (family 1) or G (family 2)
  int64_t cx = 0;                // chunks of LX / G loads along a row
  int64_t reduced = 0;           // family 1: R0 * R1 reduced indices; family 2: RO * cx tiles
  int64_t slices = 0;
  int64_t units = 0;
  int64_t block_units = 0;       // workgroup-sized pieces of work
  int64_t blocks = 0;            // 0: an empty box (no first stage)
  int index_bits = 64;           // width of the offsets in the inner loop
  int nkeep = 0;                 // kept axes, in the field's axis order
  int64_t keep_n[2] = {1, 1};
  int64_t keep_pstride[2] = {0, 0};
};

// `shape`, `strides` (elements), `lo`, `hi` (the box, half-open) have one entry
// per dimension (2 .. 3); `keep` lists the kept axes, strictly increasing, at
// least one and not all. `strides_b` / `base_b` describe the second input of a
// two-input op (same shape and box); empty: none.
ProjectPlan plan_project(const std::vector<int64_t>& shape, const std::vector<int64_t>& strides,
                         const std::vector<int64_t>& lo, const std::vector<int64_t>& hi,
                         const std::vector<int>& keep, int elem_size, uintptr_t base_address,
                         const std::vector<int64_t>& strides_b = {}, uintptr_t base_b = 0);

}  // namespace igg
