// spread_g: the transpose of sample_g, point values added into the grid
// (spread_kernels.hip, spread.cpp; parallel/spread_g.py).
//
// A point u is what sample_axis makes of it: per dimension a lower corner g, a
// weight t and a validity. The lower corner takes the factor 1 - t, the upper
// one ((g + 1), wrapped where periodic) the factor t; a corner's weight is
// ((fx*fy)*fz) and a corner with a zero factor receives nothing. Which local
// cells stand for a corner depends on `copies`:
//   SPREAD_ALL    every local cell whose global index is the corner's: the run
//                 table of scatter_g (halo and overlap copies included);
//   SPREAD_OWNER  on the rank that owns the lower corner (sample_axis), its
//                 local cells lo and hi, exactly those sample_kernel reads.
// The work is split in two. The plan lists every (cell, point, weight) target,
// sorted by (cell, point), as CSR segments by touched cell; apply gives every
// touched cell to one lane, which folds its segment in order in float64 and
// does one read-modify-write. No atomics: the order of the additions is fixed,
// so the result is bitwise reproducible and the host twins (spread.cpp) give
// the same bits. All arithmetic is float64 with separately rounded operations
// (the build has no contraction). The expressions below are shared by the
// kernels and the host twins.
#pragma once

#include <cstdint>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "igg/sample.hpp"

namespace igg {

constexpr int SPREAD_BLOCK = 256;        // lanes per workgroup (4 waves)
constexpr int SPREAD_MAX_BLOCKS = 4096;  // 16 per CU; grid-stride beyond
constexpr int SPREAD_MAX_FIELDS = 8;     // fields per launch (more: further launches)
constexpr int SPREAD_MAX_RUNS = 4;       // runs of one dimension (scatter_g._runs)
constexpr int SPREAD_ALL = 0, SPREAD_OWNER = 1;

// One dimension: sample_g's table (E, m, per; the owned segments are used by
// SPREAD_OWNER) and the local range as runs: local i0 .. i0 + len - 1 hold the
// global indices g0, g0 + 1, ... (used by SPREAD_ALL).
struct SpreadDim {
  SampleDim own;
  int32_t nrun = 0;
  int32_t i0[SPREAD_MAX_RUNS] = {0, 0, 0, 0}, len[SPREAD_MAX_RUNS] = {0, 0, 0, 0}, g0[SPREAD_MAX_RUNS] = {0, 0, 0, 0};
};

struct SpreadPlanArgs {
  int32_t nd = 0;      // 1..3
  int32_t copies = 0;  // SPREAD_ALL / SPREAD_OWNER
  SpreadDim dim[3];
  const double* P = nullptr;  // point p, axis d at P[p*ps0 + d*ps1]
  int64_t ps0 = 0, ps1 = 0;
  int64_t npts = 0;
  int64_t* count = nullptr;      // count pass: targets of point p
  const int64_t* cum = nullptr;  // fill pass: the inclusive running sum of count
  int64_t nentries = 0;          // fill pass: cum[npts - 1]; nothing is written at or beyond it
  int64_t* key = nullptr;        // fill pass: linear C-order index of the target cell,
  int64_t* point = nullptr;      //            the point,
  double* weight = nullptr;      //            the weight; entries of a point in corner order
};

// What a point is in one dimension: its two corners (global indices under
// SPREAD_ALL, local ones under SPREAD_OWNER), their factors and how many local
// cells each reaches.
struct SpreadAxis {
  int32_t c[2];
  double f[2];
  int32_t n[2];
};

IGG_HD int32_t spread_run_hits(const SpreadDim& D, int32_t g) {
  int32_t hits = 0;
#pragma unroll
  for (int r = 0; r < SPREAD_MAX_RUNS; ++r)
    hits += (r < D.nrun && g >= D.g0[r] && g - D.g0[r] < D.len[r]) ? 1 : 0;
  return hits;
}

// Returns the point's validity in this dimension.
IGG_HD bool spread_axis(const SpreadDim& D, int copies, double u, SpreadAxis& a) {
  if (copies == SPREAD_OWNER) {
    const SampleAxis s = sample_axis(D.own, u);
    a.c[0] = static_cast<int32_t>(s.lo), a.c[1] = static_cast<int32_t>(s.hi);
    a.f[0] = 1.0 - s.t, a.f[1] = s.t;
    a.n[0] = (s.owned && a.f[0] != 0.0) ? 1 : 0;
    a.n[1] = (s.owned && a.f[1] != 0.0) ? 1 : 0;
    return s.valid;
  }
  // the whole index range as one segment at local index 0: lo is the global lower corner
  SampleDim G;
  G.E = D.own.E, G.m = D.own.E + 1, G.per = D.own.per, G.nseg = 1;
  G.g0[0] = 0, G.g1[0] = D.own.E, G.i0[0] = 0;
  const SampleAxis s = sample_axis(G, u);
  const int32_t g = static_cast<int32_t>(s.lo);
  a.c[0] = g;
  a.c[1] = (D.own.per && g + 1 >= D.own.E) ? 0 : g + 1;
  a.f[0] = 1.0 - s.t, a.f[1] = s.t;
  a.n[0] = a.f[0] != 0.0 ? spread_run_hits(D, a.c[0]) : 0;
  a.n[1] = a.f[1] != 0.0 ? spread_run_hits(D, a.c[1]) : 0;
  return s.valid;
}

// Target k (< n[0] + n[1]) of a dimension: the lower corner's cells first, each corner's in run order.
IGG_HD void spread_pick(const SpreadDim& D, int copies, const SpreadAxis& a, int32_t k, int32_t& idx, double& fac) {
  const bool up = k >= a.n[0];
  const int32_t kk = up ? k - a.n[0] : k;
  const int32_t g = up ? a.c[1] : a.c[0];
  fac = up ? a.f[1] : a.f[0];
  idx = copies == SPREAD_OWNER ? g : 0;
  int32_t seen = 0;
#pragma unroll
  for (int r = 0; r < SPREAD_MAX_RUNS; ++r) {
    const bool hit = copies != SPREAD_OWNER && r < D.nrun && g >= D.g0[r] && g - D.g0[r] < D.len[r];
    idx = (hit && seen == kk) ? D.i0[r] + (g - D.g0[r]) : idx;
    seen += hit ? 1 : 0;
  }
}

// The three axes of point p (a dimension the field does not have: one target,
// index 0, factor 1 - a multiplication by 1 is exact). Returns the number of
// targets: 0 for a point that is invalid in any dimension.
IGG_HD int64_t spread_point(const SpreadPlanArgs& A, int64_t p, SpreadAxis ax[3]) {
  bool valid = true;
  int64_t n = 1;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (d < A.nd) {
      valid = spread_axis(A.dim[d], A.copies, A.P[p * A.ps0 + d * A.ps1], ax[d]) && valid;
    } else {
      ax[d].c[0] = 0, ax[d].c[1] = 0, ax[d].f[0] = 1.0, ax[d].f[1] = 1.0, ax[d].n[0] = 1, ax[d].n[1] = 0;
    }
    n *= ax[d].n[0] + ax[d].n[1];
  }
  return valid ? n : 0;
}

// The fill pass of point p: its entries from `begin` on, x outermost.
IGG_HD void spread_fill_point(const SpreadPlanArgs& A, int64_t p, int64_t begin) {
  SpreadAxis ax[3];
  if (spread_point(A, p, ax) == 0) return;
  const int32_t nx = ax[0].n[0] + ax[0].n[1], ny = ax[1].n[0] + ax[1].n[1], nz = ax[2].n[0] + ax[2].n[1];
  const int64_t m1 = A.nd > 1 ? A.dim[1].own.m : 1, m2 = A.nd > 2 ? A.dim[2].own.m : 1;
  int64_t e = begin;
  for (int32_t kx = 0; kx < nx; ++kx) {
    int32_t ix, iy, iz;
    double fx, fy, fz;
    spread_pick(A.dim[0], A.copies, ax[0], kx, ix, fx);
    for (int32_t ky = 0; ky < ny; ++ky) {
      spread_pick(A.dim[1], A.copies, ax[1], ky, iy, fy);
      const double fxy = fx * fy;
      for (int32_t kz = 0; kz < nz; ++kz) {
        spread_pick(A.dim[2], A.copies, ax[2], kz, iz, fz);
        if (e < A.nentries) {
          A.key[e] = (static_cast<int64_t>(ix) * m1 + iy) * m2 + iz;
          A.point[e] = p;
          A.weight[e] = fxy * fz;
        }
        ++e;
      }
    }
  }
}

struct SpreadField {
  void* base;
  int64_t stride[3];  // elements, per axis of the field
};

struct SpreadArgs {
  int32_t nd = 0;  // 1..3
  int32_t nf = 0;  // 1..SPREAD_MAX_FIELDS
  int64_t m[3] = {1, 1, 1};  // the fields' shape (1: a dimension they do not have)
  int64_t numel = 1;         // its product
  SpreadField field[SPREAD_MAX_FIELDS];
  int64_t ncells = 0;              // touched cells
  const int64_t* cells = nullptr;  // their linear C-order indices, ascending
  const int64_t* start = nullptr;  // ncells + 1: cell i has the entries start[i] .. start[i+1] - 1
  const int64_t* point = nullptr;  // per entry, sorted by (cell, point)
  const double* weight = nullptr;
  const double* V = nullptr;  // field f, point p at V[f*v_fs + p*v_ps]
  int64_t v_fs = 0, v_ps = 1;
  const int64_t* row = nullptr;  // optional: V moves by *row * row_stride,
  int64_t nrows = 0;             // and nothing is done if *row >= nrows
  int64_t row_stride = 0;
};

// Cell i of the plan, every field: fold the segment in order, one read-modify-write.
template <typename T>
IGG_HD void spread_cell(const SpreadArgs& A, const double* V, int64_t i) {
  const int64_t c = A.cells[i];
  int64_t i0, i1, i2;
  if (A.numel <= INT32_MAX) {  // (uniform: a 32-bit division where the field allows it)
    const uint32_t c32 = static_cast<uint32_t>(c), m1 = static_cast<uint32_t>(A.m[1]), m2 = static_cast<uint32_t>(A.m[2]);
    const uint32_t q = c32 / m2;
    i2 = c32 - q * m2, i0 = q / m1, i1 = q - static_cast<uint32_t>(i0) * m1;
  } else {
    const int64_t q = c / A.m[2];
    i2 = c - q * A.m[2], i0 = q / A.m[1], i1 = q - i0 * A.m[1];
  }
  const int64_t b = A.start[i], e = A.start[i + 1];
  if (e <= b) return;
  for (int f = 0; f < A.nf; ++f) {
    const double* Vf = V + f * A.v_fs;
    double s = A.weight[b] * Vf[A.point[b] * A.v_ps];
    for (int64_t j = b + 1; j < e; ++j) s = s + A.weight[j] * Vf[A.point[j] * A.v_ps];
    T* q = static_cast<T*>(A.field[f].base) + (i0 * A.field[f].stride[0] + i1 * A.field[f].stride[1] + i2 * A.field[f].stride[2]);
    *q = static_cast<T>(static_cast<double>(*q) + s);
  }
}

// A finished plan on the host.
struct SpreadPlan {
  std::vector<int64_t> cells, start, point;
  std::vector<double> weight;
};

// Checks shared by the entry points; `who` names the caller in the message.
void check_spread_plan(const char* who, const SpreadPlanArgs& a);
void check_spread(const char* who, const SpreadArgs& a);

// Plan passes on device memory, one lane per point: count[p], then (with the
// running sum of the counts) the entries. Nothing is allocated and nothing
// synchronises. max_blocks caps the grid (0: SPREAD_MAX_BLOCKS).
void spread_count(const SpreadPlanArgs& a, int max_blocks, hipStream_t stream);
void spread_fill(const SpreadPlanArgs& a, int max_blocks, hipStream_t stream);
// Enqueue one apply launch (elem_size 4 or 8: f32 or f64 fields), one lane per touched cell.
void spread_apply(const SpreadArgs& a, int elem_size, int max_blocks, hipStream_t stream);

// The same on host memory: the whole plan (sorted with std::stable_sort), and the apply pass.
SpreadPlan host_spread_plan(const SpreadPlanArgs& a);
void host_spread_apply(const SpreadArgs& a, int elem_size);

// spread_kernels.hip
void launch_spread_count(const SpreadPlanArgs& a, int blocks, hipStream_t stream);
void launch_spread_fill(const SpreadPlanArgs& a, int blocks, hipStream_t stream);
void launch_spread_apply(const SpreadArgs& a, int elem_size, int blocks, hipStream_t stream);

}  // namespace igg
