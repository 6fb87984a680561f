// Projections on the GPU (project_kernels.hip, project.cpp): the hot path of
// ops/reduce.py project_g - reduce a box of a field over some of its axes and
// keep the others, placed into a global-shaped destination.
//
// Two launches, no data passed between workgroups inside a launch:
//   stage 1: every (slice, output) pair of the plan (igg/project_plan.hpp) is
//            accumulated in f64 by one lane (family 1) or one group of lanes
//            (family 2) and stored as ONE partial (value, NaN flag);
//   stage 2: one lane per cell of the destination: a cell of this box combines
//            its slices in index order, every other cell takes the identity.
// No atomics, nothing that depends on the device: the same box gives the same
// bits on every run.
#pragma once

#include <cstdint>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "igg/project_plan.hpp"
#include "igg/reduce.hpp"

namespace igg {

// The first stage's kernel argument. Pointers address the first element of
// the box; n / s / sb are the slots of the plan's family.
struct ProjectJob {
  const void* a;
  const void* b;
  int64_t s[4];
  int64_t sb[4];
  int64_t n[4];
  int64_t reduced;
  int64_t nout;
  uint32_t nv, head, lanes_log2, cx, slices, units, block_units;
};

// The destination: `nkeep` kept axes in the field's axis order. The box's
// index i of kept axis k lands at global index (start[k] + i) mod extent[k],
// element dst[sum(g[k] * stride[k])]; the destination has extent[0] x
// extent[1] cells (extent[1] = 1 with one kept axis).
struct ProjectStage2 {
  double* dst;
  double* flags;       // travel form of the MAX-type ops: dst = value with NaN as -inf, flags = 1.0 / 0.0
  int64_t extent[2], start[2], stride[2];
  int64_t own[2];      // kept extents of the box (0: nothing owned)
  int64_t pstride[2];  // of the box's index in the output's partial index
  int64_t nout;
  uint32_t slices;
  int max_type;
  int negate;          // R_MIN, final form: -max(-x), identity +inf
};

struct ProjectDest {
  uintptr_t dst = 0, flags = 0;
  std::vector<int64_t> start, extent, stride;  // one entry per kept axis
};

// dst = op over the reduced axes of the box of one field (f64), enqueued on
// `stream`. The workspace of the current device must not be shared by
// concurrent streams.
void project_field(int op, const ReduceField& f, const std::vector<int>& keep, int elem_size,
                   const ProjectDest& dest, hipStream_t stream);

// The per-device workspace of partials: grows only; a call that has to grow
// it inside a stream capture is an error; freed by finalize_global_grid.
void* project_workspace(size_t bytes, hipStream_t stream);
size_t project_workspace_bytes();
void project_free_workspace();

// project_kernels.hip
void launch_project_stage1(int op, int elem_size, const ProjectPlan& plan, const ProjectJob& job, void* partials,
                           hipStream_t stream);
void launch_project_stage2(const ProjectStage2& args, const void* partials, hipStream_t stream);

}  // namespace igg
