// Reductions over boxes of fields on the GPU (reduce_kernels.hip, reduce.cpp):
// the hot path of ops/reduce.py (sums, norms, maxima over the owned cells of
// the implicit global grid).
//
// Two launches per batch of up to REDUCE_MAX_JOBS fields, no data passed
// between workgroups inside a launch:
//   stage 1: every workgroup of a job walks its tiles in a fixed grid-stride
//            order, accumulates in f64 per lane, combines its lanes by
//            cross-lane moves and its waves through LDS (one barrier) and
//            stores ONE partial (value, NaN flag) into the workspace;
//   stage 2: one workgroup per job combines the job's partials in index order
//            and writes out[job].
// No atomics, no fences, nothing that depends on the device: the same box
// gives the same bits on every run (the block count comes from the plan).
#pragma once

#include <cstdint>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "igg/reduce_plan.hpp"

namespace igg {

// SUM-type ops propagate NaN on their own; the MAX-type ops carry a NaN flag
// (fmax drops NaN). R_MIN is computed as max(-x): stage 2 negates it back
// unless the caller asks for the travel form.
enum ReduceOp : int { R_SUM = 0, R_SUMSQ, R_MAX, R_MIN, R_MAXABS, R_DOT, R_SUMSQ_DIFF, R_MAXABS_DIFF, R_NUM_OPS };

inline bool reduce_two_inputs(int op) { return op == R_DOT || op == R_SUMSQ_DIFF || op == R_MAXABS_DIFF; }
inline bool reduce_max_type(int op) { return op == R_MAX || op == R_MIN || op == R_MAXABS || op == R_MAXABS_DIFF; }

// One job of the descriptor table (a kernel argument, like the copy kernel's
// regions). Pointers address the first element of the box.
struct ReduceJob {
  const void* a;
  const void* b;
  int64_t s[3];
  int64_t sb[3];
  int64_t n2;
  uint32_t n1, nv, head, cx, g1, lx_log2, tiles, nblocks;
};

struct ReduceBatch {
  int n;
  uint32_t block_start[REDUCE_MAX_JOBS + 1];
  ReduceJob job[REDUCE_MAX_JOBS];
};

struct ReduceStage2 {
  int n;
  int max_type;
  int negate;      // R_MIN, final form: out = -max(-x)
  double* out;     // out[job]
  double* flags;   // travel form of the MAX-type ops: out = value with NaN as -inf, flags[job] = 1.0 / 0.0
  uint32_t nblocks[REDUCE_MAX_JOBS];
};

struct ReduceField {
  uintptr_t a = 0, b = 0;
  std::vector<int64_t> shape, stride_a, stride_b, lo, hi;
};

// out[k] = op over the box of field k (f64), enqueued on `stream`. With
// `flags` the MAX-type ops write the travel form (see ReduceStage2). The
// workspace of the current device must not be shared by concurrent streams.
void reduce_fields(int op, const std::vector<ReduceField>& fields, int elem_size, double* out, double* flags,
                   hipStream_t stream);

// The per-device workspace of partials: allocated on first use (never inside
// a stream capture: that is an error), sized for REDUCE_MAX_JOBS jobs at the
// block cap; freed by finalize_global_grid.
void* reduce_workspace(hipStream_t stream);
size_t reduce_workspace_bytes();
void reduce_free_workspace();

// reduce_kernels.hip
void launch_reduce_stage1(int op, int elem_size, bool vector_loads, const ReduceBatch& batch, void* partials,
                          hipStream_t stream);
void launch_reduce_stage2(const ReduceStage2& args, const void* partials, hipStream_t stream);

}  // namespace igg
