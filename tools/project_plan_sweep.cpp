// Stand-alone sweep of the projection plan (csrc/project_plan.cpp) for a host
// sanitizer run: boxes, keep-sets, layouts, element sizes and base offsets,
// with the plan's own invariants checked on the way. Host code only.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Icsrc/include tools/project_plan_sweep.cpp csrc/project_plan.cpp -o /tmp/project_plan_sweep
//   /tmp/project_plan_sweep
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "igg/common.hpp"
#include "igg/project_plan.hpp"

using namespace igg;

namespace {
long g_plans = 0, g_refused = 0;

void require(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "plan invariant broken: %s\n", what);
    std::exit(1);
  }
}

void one(const std::vector<int64_t>& shape, const std::vector<int64_t>& strides, const std::vector<int64_t>& lo,
         const std::vector<int64_t>& hi, const std::vector<int>& keep, int es, uintptr_t base, bool two) {
  ProjectPlan p;
  try {
    p = two ? plan_project(shape, strides, lo, hi, keep, es, base, strides, base + 16)
            : plan_project(shape, strides, lo, hi, keep, es, base);
  } catch (const Error&) {
    ++g_refused;
    return;
  }
  ++g_plans;
  if (p.total == 0) {
    require(p.blocks == 0 && p.nout == 0, "an empty box has no first stage");
    return;
  }
  int64_t total = 1;
  for (int k = 0; k < 4; ++k) total *= p.n[k];
  require(total == p.total, "the slots hold the box");
  require(p.family == 1 ? p.nout == p.n[0] * p.n[3] : p.nout == p.n[0] * p.n[1], "outputs");
  require(p.slices >= 1 && p.slices <= PROJECT_MAX_SLICES && p.slices <= p.reduced, "slices");
  require(p.blocks >= 1 && p.blocks <= PROJECT_MAX_BLOCKS && p.blocks <= p.block_units, "blocks");
  require(p.nv * p.vec >= p.head + p.n[3] && (p.nv - 1) * p.vec < p.head + p.n[3], "loads per row");
  require(p.cx * (int64_t{1} << p.lanes_log2) >= p.nv, "chunks cover the row");
  require(p.head >= 0 && p.head < p.vec, "head");
  require(!p.vector || p.s[3] == 1, "vector loads need a unit stride");
  // every slice gets at least one index, the slices tile the reduced range
  int64_t covered = 0;
  for (int64_t s = 0; s < p.slices; ++s) {
    const int64_t b = s * p.reduced / p.slices, e = (s + 1) * p.reduced / p.slices;
    require(e > b, "an empty slice");
    covered += e - b;
  }
  require(covered == p.reduced, "the slices tile the reduced range");
}
}  // namespace

int main() {
  const std::vector<std::vector<int64_t>> shapes3 = {{6, 8, 12}, {5, 7, 9}, {1, 9, 33}, {70, 33, 9}, {3, 4, 300},
                                                     {512, 512, 512}, {1024, 1024, 1024}, {4096, 4096, 4096}};
  const std::vector<std::vector<int>> keeps3 = {{0}, {1}, {2}, {0, 1}, {0, 2}, {1, 2}, {}, {0, 1, 2}, {2, 0}, {3}};
  for (const auto& shape : shapes3) {
    std::vector<int> order = {0, 1, 2};
    do {
      std::vector<int64_t> strides(3);
      int64_t acc = 1;
      for (int k = 2; k >= 0; --k) strides[order[k]] = acc, acc *= shape[order[k]];
      for (int cut = 0; cut < 4; ++cut) {
        std::vector<int64_t> lo(3), hi(3);
        for (int d = 0; d < 3; ++d) {
          lo[d] = std::min<int64_t>(cut == 3 ? 0 : cut, shape[d]);
          hi[d] = std::max<int64_t>(lo[d], shape[d] - (cut == 3 ? 0 : cut));
        }
        for (const auto& keep : keeps3)
          for (int es : {4, 8, 2})
            for (uintptr_t off : {0, 4, 8, 12, 16})
              for (bool two : {false, true}) one(shape, strides, lo, hi, keep, es, (uintptr_t{1} << 30) + off, two);
      }
    } while (std::next_permutation(order.begin(), order.end()));
  }
  for (const std::vector<int64_t>& shape : {std::vector<int64_t>{7, 11}, {1, 5}, {4096, 3}, {1 << 20, 1 << 12}})
    for (const std::vector<int64_t>& strides : {std::vector<int64_t>{shape[1], 1}, {1, shape[0]}, {shape[1] + 3, 1}})
      for (int cut = 0; cut < 3; ++cut)
        for (const auto& keep : std::vector<std::vector<int>>{{0}, {1}, {0, 1}, {}})
          for (int es : {4, 8})
            for (uintptr_t off : {0, 4, 8})
              one(shape, strides, {std::min<int64_t>(cut, shape[0]), std::min<int64_t>(cut, shape[1])},
                  {std::max<int64_t>(std::min<int64_t>(cut, shape[0]), shape[0] - cut),
                   std::max<int64_t>(std::min<int64_t>(cut, shape[1]), shape[1] - cut)},
                  keep, es, (uintptr_t{1} << 30) + off, false);
  one({4, 4}, {4, 1}, {0, 0}, {5, 4}, {0}, 8, 1 << 20, false);        // a box outside of the field
  one({4, 4}, {4, -1}, {0, 0}, {4, 4}, {0}, 8, 1 << 20, false);       // a negative stride
  one({4}, {1}, {0}, {4}, {0}, 8, 1 << 20, false);                    // one dimension
  std::printf("project plan sweep: %ld plans, %ld refused, all invariants hold\n", g_plans, g_refused);
  return 0;
}
