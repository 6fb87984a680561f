// Host-side plan of the reduction kernels (igg/reduce_plan.hpp).
#include "igg/reduce_plan.hpp"

#include <algorithm>

#include "igg/common.hpp"

namespace igg {

namespace {
struct Dim {
  int64_t n, s, sb;
};
}  // namespace

ReducePlan plan_reduce(const std::vector<int64_t>& shape, const std::vector<int64_t>& strides,
                       const std::vector<int64_t>& lo, const std::vector<int64_t>& hi, int elem_size,
                       uintptr_t base_address, const std::vector<int64_t>& strides_b, uintptr_t base_b) {
  const size_t nd = shape.size();
  if (nd < 1 || nd > 3) fail("plan_reduce: 1 to 3 dimensions (got ", nd, ")");
  if (strides.size() != nd || lo.size() != nd || hi.size() != nd)
    fail("plan_reduce: shape, strides, lo and hi must have one entry per dimension");
  const bool two = !strides_b.empty();
  if (two && strides_b.size() != nd) fail("plan_reduce: the second input's strides must have one entry per dimension");
  if (elem_size != 4 && elem_size != 8) fail("plan_reduce: 4- or 8-byte elements (got ", elem_size, ")");
  ReducePlan p;
  p.total = 1;
  std::vector<Dim> dims;
  for (size_t d = 0; d < nd; ++d) {
    if (lo[d] < 0 || hi[d] > shape[d] || lo[d] > hi[d])
      fail("plan_reduce: box [", lo[d], ", ", hi[d], ") outside of extent ", shape[d], " in dimension ", d);
    if (strides[d] < 0 || (two && strides_b[d] < 0)) fail("plan_reduce: negative stride");
    const int64_t n = hi[d] - lo[d];
    p.total *= n;
    p.offset += lo[d] * strides[d];
    if (two) p.offset_b += lo[d] * strides_b[d];
    if (n != 1) dims.push_back({n, strides[d], two ? strides_b[d] : strides[d]});
  }
  if (p.total == 0) return p;
  // merge extents that are adjacent in memory inside the box, for both inputs
  std::vector<Dim> m;
  for (const Dim& d : dims) {
    if (!m.empty() && m.back().s == d.n * d.s && m.back().sb == d.n * d.sb) {
      m.back().n *= d.n, m.back().s = d.s, m.back().sb = d.sb;
    } else {
      m.push_back(d);
    }
  }
  if (m.empty()) m.push_back({1, 1, 1});  // a single element
  for (size_t k = 0; k < m.size(); ++k) {
    const size_t at = 3 - m.size() + k;
    p.n[at] = m[k].n, p.s[at] = m[k].s, p.sb[at] = m[k].sb;
  }
  const int vec = 16 / elem_size;
  const uintptr_t first = base_address + static_cast<uintptr_t>(p.offset) * elem_size;
  const uintptr_t first_b = two ? base_b + static_cast<uintptr_t>(p.offset_b) * elem_size : first;
  const bool unit = p.s[2] == 1 && p.sb[2] == 1 && first % elem_size == 0 && first_b % elem_size == 0 &&
                    first % 16 == first_b % 16;  // one head mask serves both inputs
  auto pitch_ok = [&](int64_t s) { return (s * elem_size) % 16 == 0; };
  if (unit && m.size() == 1) {
    p.path = ReducePath::flat;
  } else if (unit && base_address % 16 == 0 && (!two || base_b % 16 == 0) && pitch_ok(p.s[0]) && pitch_ok(p.s[1]) &&
             pitch_ok(p.sb[0]) && pitch_ok(p.sb[1])) {
    p.path = ReducePath::rows;
  } else {
    p.path = ReducePath::element;
  }
  if (p.path == ReducePath::element) {
    p.vec = 1, p.head = 0, p.nv = p.n[2];
  } else {
    p.vec = vec;
    p.head = static_cast<int>((first % 16) / elem_size);
    p.nv = (p.head + p.n[2] + vec - 1) / vec;
  }
  while (p.lx_log2 < 8 && (int64_t{1} << p.lx_log2) < p.nv) ++p.lx_log2;
  const int64_t lx = int64_t{1} << p.lx_log2, ly = REDUCE_BLOCK / lx;
  p.cx = (p.nv + lx - 1) / lx;
  p.g1 = (p.n[1] + ly - 1) / ly;
  // (the kernel decodes tile and row numbers in 32 bits)
  if (p.n[0] > 0x7fffffffLL || p.n[1] > 0x7fffffffLL || p.nv > 0x7fffffffLL ||
      static_cast<double>(p.n[0]) * static_cast<double>(p.g1) * static_cast<double>(p.cx) > 2.0e9)
    fail("plan_reduce: box too large (", p.total, " elements)");
  p.tiles = p.n[0] * p.g1 * p.cx;
  p.blocks = std::min<int64_t>((p.tiles + REDUCE_UNROLL - 1) / REDUCE_UNROLL, REDUCE_MAX_BLOCKS);
  return p;
}

}  // namespace igg
