// Host-side plan of the projection kernels (igg/project_plan.hpp).
#include "igg/project_plan.hpp"

#include <algorithm>

#include "igg/common.hpp"

namespace igg {

namespace {
struct Axis {
  int64_t n, s, sb;
  bool kept;
  int axis;  // of the field (the first of a merged run)
};

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
}  // namespace

ProjectPlan plan_project(const std::vector<int64_t>& shape, const std::vector<int64_t>& strides,
                         const std::vector<int64_t>& lo, const std::vector<int64_t>& hi,
                         const std::vector<int>& keep, int elem_size, uintptr_t base_address,
                         const std::vector<int64_t>& strides_b, uintptr_t base_b) {
  const size_t nd = shape.size();
  if (nd < 2 || nd > 3) fail("plan_project: 2 or 3 dimensions (got ", nd, ")");
  if (strides.size() != nd || lo.size() != nd || hi.size() != nd)
    fail("plan_project: shape, strides, lo and hi must have one entry per dimension");
  const bool two = !strides_b.empty();
  if (two && strides_b.size() != nd) fail("plan_project: the second input's strides must have one entry per dimension");
  if (elem_size != 4 && elem_size != 8) fail("plan_project: 4- or 8-byte elements (got ", elem_size, ")");
  if (keep.empty() || keep.size() >= nd) fail("plan_project: keep must name at least one axis and not all of them");
  for (size_t k = 0; k < keep.size(); ++k)
    if (keep[k] < 0 || keep[k] >= static_cast<int>(nd) || (k > 0 && keep[k] <= keep[k - 1]))
      fail("plan_project: keep must be strictly increasing axes of the field");
  ProjectPlan p;
  p.total = 1;
  p.nout = 1;
  p.nkeep = static_cast<int>(keep.size());
  std::vector<Axis> axes;
  for (size_t d = 0; d < nd; ++d) {
    if (lo[d] < 0 || hi[d] > shape[d] || lo[d] > hi[d])
      fail("plan_project: box [", lo[d], ", ", hi[d], ") outside of extent ", shape[d], " in dimension ", d);
    if (strides[d] < 0 || (two && strides_b[d] < 0)) fail("plan_project: negative stride");
    const int64_t n = hi[d] - lo[d];
    const bool kept = std::find(keep.begin(), keep.end(), static_cast<int>(d)) != keep.end();
    p.total *= n;
    if (kept) p.nout *= n;
    p.offset += lo[d] * strides[d];
    if (two) p.offset_b += lo[d] * strides_b[d];
    if (n != 1) axes.push_back({n, strides[d], two ? strides_b[d] : strides[d], kept, static_cast<int>(d)});
  }
  if (p.total == 0) {  // nothing owned: the second stage writes the identity everywhere
    p.nout = 0;
    p.keep_n[0] = p.keep_n[1] = 0;
    return p;
  }
  // memory order, outer .. inner (by the first input; ties keep the axis order)
  std::stable_sort(axes.begin(), axes.end(), [](const Axis& a, const Axis& b) { return a.s > b.s; });
  // an output's index p among the partials: C order over the kept extents in memory order
  for (size_t k = 0; k < keep.size(); ++k) {
    const int d = keep[k];
    p.keep_n[k] = hi[d] - lo[d];
    int64_t ps = 0;
    for (size_t i = 0; i < axes.size(); ++i) {
      if (axes[i].axis != d) continue;
      ps = 1;
      for (size_t j = i + 1; j < axes.size(); ++j)
        if (axes[j].kept) ps *= axes[j].n;
    }
    p.keep_pstride[k] = ps;
  }
  // merge neighbours of one kind that are contiguous in the box, for both inputs
  std::vector<Axis> m;
  for (const Axis& a : axes) {
    if (!m.empty() && m.back().kept == a.kept && m.back().s == a.n * a.s && m.back().sb == a.n * a.sb) {
      m.back().n *= a.n, m.back().s = a.s, m.back().sb = a.sb;
    } else {
      m.push_back(a);
    }
  }
  for (size_t i = 0; i < m.size(); ++i) p.pattern[i] = m[i].kept ? 'K' : 'R';
  // the slots of the family: [KO, R0, R1, KI] or [K0, K1, RO, RI]; a slot without an axis has extent 1
  const bool inner_kept = !m.empty() && m.back().kept;
  p.family = inner_kept ? 1 : 2;
  auto put = [&](int slot, const Axis& a) { p.n[slot] = a.n, p.s[slot] = a.s, p.sb[slot] = a.sb; };
  if (!m.empty()) {
    put(3, m.back());
    int kslot = inner_kept ? 0 : 1, rslot = 2;
    for (size_t i = m.size() - 1; i-- > 0;) {  // inner .. outer: the inner of two like axes gets the inner slot
      if (m[i].kept) {
        put(kslot, m[i]);
        kslot -= 1;
      } else {
        put(rslot, m[i]);
        rslot -= 1;
      }
    }
  }
  // the loads
  const int vec = 16 / elem_size;
  const uintptr_t first = base_address + static_cast<uintptr_t>(p.offset) * elem_size;
  const uintptr_t first_b = two ? base_b + static_cast<uintptr_t>(p.offset_b) * elem_size : first;
  auto pitch_ok = [&](int64_t s) { return (s * elem_size) % 16 == 0; };
  bool vector = p.s[3] == 1 && p.sb[3] == 1 && base_address % 16 == 0 && (!two || base_b % 16 == 0) &&
                first % elem_size == 0 && first_b % elem_size == 0 && first % 16 == first_b % 16;
  for (int k = 0; k < 3; ++k) vector = vector && pitch_ok(p.s[k]) && pitch_ok(p.sb[k]);
  p.vector = vector;
  if (vector) {
    p.vec = vec;
    p.head = static_cast<int>((first % 16) / elem_size);
    p.nv = ceil_div(p.head + p.n[3], vec);
  } else {
    p.vec = 1, p.head = 0, p.nv = p.n[3];
  }
  // 32-bit offsets in the loops: the farthest element of the box, plus the steps a loop takes past its end
  // before it notices (at most PROJECT_UNROLL1 of the largest stride), must fit
  int64_t span = 16, span_b = 16, smax = 1;
  for (int k = 0; k < 4; ++k) {
    span += (p.n[k] - 1) * p.s[k], span_b += (p.n[k] - 1) * p.sb[k];
    smax = std::max({smax, p.s[k], p.sb[k]});
  }
  if (p.total > (int64_t{1} << 46) || span > (int64_t{1} << 46) || span_b > (int64_t{1} << 46))
    fail("plan_project: box too large (", p.total, " elements)");
  p.index_bits = (vector && std::max(span, span_b) + PROJECT_UNROLL1 * smax < (int64_t{1} << 31)) ? 32 : 64;
  // lanes, slices, units, workgroups
  const int64_t target_lanes = int64_t{PROJECT_MAX_BLOCKS} * PROJECT_BLOCK;
  // (family 2: with outputs enough for every wave of the grid a group stays inside its wave - no LDS, no barrier)
  const int min_log2 = inner_kept ? 0 : PROJECT_MIN_GROUP_LOG2;
  const int max_log2 = (inner_kept || p.nout < int64_t{PROJECT_MAX_BLOCKS} * (PROJECT_BLOCK / 64)) ? 8 : 6;
  p.lanes_log2 = min_log2;
  while (p.lanes_log2 < max_log2 && (int64_t{1} << p.lanes_log2) < p.nv) ++p.lanes_log2;
  const int64_t lanes = int64_t{1} << p.lanes_log2, per_block = PROJECT_BLOCK / lanes;
  p.cx = ceil_div(p.nv, lanes);
  if (inner_kept) {
    p.reduced = p.n[1] * p.n[2];
    const int64_t want = ceil_div(ceil_div(target_lanes, p.cx * lanes), p.n[0]);
    p.slices = std::max<int64_t>(1, std::min<int64_t>({want, p.reduced, PROJECT_MAX_SLICES}));
    p.units = p.n[0] * p.slices;
    p.block_units = p.cx * ceil_div(p.units, per_block);
  } else {
    p.reduced = p.n[2] * p.cx;
    const int64_t want = ceil_div(ceil_div(target_lanes, lanes), p.nout);
    p.slices = std::max<int64_t>(1, std::min<int64_t>({want, p.reduced, PROJECT_MAX_SLICES}));
    p.units = p.nout * p.slices;
    p.block_units = ceil_div(p.units, per_block);
  }
  // (the kernels decode units and rows in 32 bits)
  if (p.units > 0x7fffffffLL || p.block_units > 0x7fffffffLL || p.nv > 0x7fffffffLL || p.nout > 0x7fffffffLL)
    fail("plan_project: box too large (", p.total, " elements)");
  p.blocks = std::min<int64_t>(p.block_units, PROJECT_MAX_BLOCKS);
  return p;
}

}  // namespace igg
