// Argument checks, launchers and host twins of spread_g (igg/spread.hpp).
#include "igg/spread.hpp"

#include <algorithm>
#include <numeric>

#include "igg/common.hpp"

namespace igg {

void check_spread_plan(const char* who, const SpreadPlanArgs& a) {
  if (a.nd < 1 || a.nd > 3) fail(who, ": fields must have 1 to 3 dimensions (got ", a.nd, ")");
  if (a.copies != SPREAD_ALL && a.copies != SPREAD_OWNER) fail(who, ": copies must be 0 (all) or 1 (owner)");
  if (a.npts < 0) fail(who, ": negative point count");
  for (int d = 0; d < a.nd; ++d) {
    const SpreadDim& S = a.dim[d];
    const SampleDim& D = S.own;
    if (D.E < 2) fail(who, ": global extent ", D.E, " in dimension ", d, " (at least 2 is needed)");
    if (D.m < 1) fail(who, ": local size ", D.m, " in dimension ", d);
    if (D.nseg < 0 || D.nseg > 2) fail(who, ": ", D.nseg, " segments in dimension ", d);
    // every target lies in the field, so that no cell index leaves it
    for (int s = 0; s < D.nseg; ++s)
      if (D.g0[s] < 0 || D.g1[s] <= D.g0[s] || D.g1[s] > D.E || D.i0[s] < 0 ||
          int64_t{D.i0[s]} + (D.g1[s] - D.g0[s]) > D.m)
        fail(who, ": segment ", s, " of dimension ", d, " lies outside of the field or the global extent");
    if (S.nrun < 0 || S.nrun > SPREAD_MAX_RUNS)
      fail(who, ": ", S.nrun, " runs in dimension ", d, " (at most ", SPREAD_MAX_RUNS, ")");
    for (int r = 0; r < S.nrun; ++r)
      if (S.g0[r] < 0 || S.len[r] < 1 || int64_t{S.g0[r]} + S.len[r] > D.E || S.i0[r] < 0 ||
          int64_t{S.i0[r]} + S.len[r] > D.m)
        fail(who, ": run ", r, " of dimension ", d, " lies outside of the field or the global extent");
  }
  if (a.npts && !a.P) fail(who, ": null pointer");
}

void check_spread(const char* who, const SpreadArgs& a) {
  if (a.nd < 1 || a.nd > 3) fail(who, ": fields must have 1 to 3 dimensions (got ", a.nd, ")");
  if (a.nf < 1 || a.nf > SPREAD_MAX_FIELDS) fail(who, ": 1 to ", SPREAD_MAX_FIELDS, " fields per call (got ", a.nf, ")");
  if (a.ncells < 0) fail(who, ": negative cell count");
  int64_t numel = 1;
  for (int d = 0; d < 3; ++d) {
    if (a.m[d] < 1 || a.m[d] > INT32_MAX || (d >= a.nd && a.m[d] != 1)) fail(who, ": size ", a.m[d], " in dimension ", d);
    if (numel > INT64_MAX / a.m[d]) fail(who, ": the field has too many elements");
    numel *= a.m[d];
  }
  if (numel != a.numel) fail(who, ": the element count does not match the shape");
  if (a.ncells == 0) return;
  if (!a.cells || !a.start || !a.point || !a.weight || !a.V) fail(who, ": null pointer");
  for (int f = 0; f < a.nf; ++f) {
    if (!a.field[f].base) fail(who, ": null field pointer");
    for (int d = 0; d < a.nd; ++d)
      if (a.field[f].stride[d] < 0) fail(who, ": negative stride");
  }
  if (a.v_fs < 0 || a.v_ps < 0) fail(who, ": negative stride of the values");
  if (a.row && (a.nrows < 0 || a.row_stride < 0)) fail(who, ": negative row count or row stride");
}

namespace {

int blocks_for(int64_t n, int max_blocks) {
  const int64_t cap = max_blocks > 0 ? max_blocks : SPREAD_MAX_BLOCKS;
  const int64_t want = (n + SPREAD_BLOCK - 1) / SPREAD_BLOCK;
  return static_cast<int>(want < cap ? want : cap);
}

}  // namespace

void spread_count(const SpreadPlanArgs& a, int max_blocks, hipStream_t stream) {
  check_spread_plan("spread_count", a);
  if (a.npts == 0) return;
  if (!a.count) fail("spread_count: null pointer");
  launch_spread_count(a, blocks_for(a.npts, max_blocks), stream);
}

void spread_fill(const SpreadPlanArgs& a, int max_blocks, hipStream_t stream) {
  check_spread_plan("spread_fill", a);
  if (a.nentries < 0) fail("spread_fill: negative entry count");
  if (a.npts == 0 || a.nentries == 0) return;
  if (!a.cum || !a.key || !a.point || !a.weight) fail("spread_fill: null pointer");
  launch_spread_fill(a, blocks_for(a.npts, max_blocks), stream);
}

void spread_apply(const SpreadArgs& a, int elem_size, int max_blocks, hipStream_t stream) {
  if (elem_size != 4 && elem_size != 8)
    fail("spread_apply: float32 and float64 fields only (element size ", elem_size, ")");
  check_spread("spread_apply", a);
  if (a.ncells == 0) return;
  launch_spread_apply(a, elem_size, blocks_for(a.ncells, max_blocks), stream);
}

SpreadPlan host_spread_plan(const SpreadPlanArgs& a0) {
  check_spread_plan("host_spread_plan", a0);
  SpreadPlanArgs a = a0;
  const size_t npts = static_cast<size_t>(a.npts);
  std::vector<int64_t> cum(npts);
  int64_t total = 0;
  for (size_t p = 0; p < npts; ++p) {
    SpreadAxis ax[3];
    total += spread_point(a, static_cast<int64_t>(p), ax);
    cum[p] = total;
  }
  std::vector<int64_t> key(total), point(total);
  std::vector<double> weight(total);
  a.cum = cum.data(), a.nentries = total;
  a.key = key.data(), a.point = point.data(), a.weight = weight.data();
  for (size_t p = 0; p < npts; ++p) spread_fill_point(a, static_cast<int64_t>(p), p ? cum[p - 1] : 0);
  // entries are in point order: a stable sort by cell leaves every segment sorted by point
  std::vector<int64_t> order(total);
  std::iota(order.begin(), order.end(), int64_t{0});
  std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return key[x] < key[y]; });
  SpreadPlan plan;
  plan.point.resize(total), plan.weight.resize(total);
  for (int64_t e = 0; e < total; ++e) {
    const int64_t s = order[e];
    if (e == 0 || key[s] != plan.cells.back()) plan.cells.push_back(key[s]), plan.start.push_back(e);
    plan.point[e] = point[s], plan.weight[e] = weight[s];
  }
  plan.start.push_back(total);
  return plan;
}

namespace {

template <typename T>
void host_spread_apply_t(const SpreadArgs& A) {
  const double* V = A.V;
  if (A.row) {
    const int64_t r = *A.row;
    if (r < 0 || r >= A.nrows) return;
    V += r * A.row_stride;
  }
  for (int64_t i = 0; i < A.ncells; ++i) spread_cell<T>(A, V, i);
}

}  // namespace

void host_spread_apply(const SpreadArgs& a, int elem_size) {
  if (elem_size != 4 && elem_size != 8)
    fail("host_spread_apply: float32 and float64 fields only (element size ", elem_size, ")");
  check_spread("host_spread_apply", a);
  if (a.ncells == 0) return;
  if (elem_size == 4)
    host_spread_apply_t<float>(a);
  else
    host_spread_apply_t<double>(a);
}

}  // namespace igg
