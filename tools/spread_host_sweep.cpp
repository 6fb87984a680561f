// Stand-alone sweep of the spread_g host twins (csrc/spread.cpp) for a host
// sanitizer run: 1-D to 3-D shapes of a small range, periodic and not, one rank
// and the tables of ranks of a 2-rank split, both `copies`, float32 and
// float64, on heap arrays of exactly the fields' and the plan's sizes, so that
// a read or a write beyond an array is an error. On the way it checks that the
// plan is sorted by (cell, point), that every cell lies in the field, and the
// transposed identity <A, spread(V)> == <sample(A), V> on dyadic data (exact)
// for the owner's cells. Host code only.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -D__HIP_PLATFORM_AMD__ -Icsrc/include -I$ROCM_PATH/include tools/spread_host_sweep.cpp csrc/spread.cpp \
//       csrc/sample.cpp -o /tmp/spread_host_sweep
//   /tmp/spread_host_sweep
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "igg/common.hpp"
#include "igg/sample.hpp"
#include "igg/spread.hpp"

using namespace igg;

// The device launchers live in the kernel units, which this host-only program does not link.
namespace igg {
void launch_spread_count(const SpreadPlanArgs&, int, hipStream_t) { fail("host-only build"); }
void launch_spread_fill(const SpreadPlanArgs&, int, hipStream_t) { fail("host-only build"); }
void launch_spread_apply(const SpreadArgs&, int, int, hipStream_t) { fail("host-only build"); }
void launch_sample(const SampleArgs&, int, int, hipStream_t) { fail("host-only build"); }
}  // namespace igg

namespace {

unsigned g_seed = 12345u;
unsigned next() { return g_seed = g_seed * 1664525u + 1013904223u; }

[[noreturn]] void die(const char* what, int nd, const int* m, int per, int copies) {
  std::fprintf(stderr, "spread_host_sweep: %s (nd %d, shape %d %d %d, periodic %d, copies %d)\n", what, nd, m[0],
               nd > 1 ? m[1] : 1, nd > 2 ? m[2] : 1, per, copies);
  std::exit(1);
}

// One dimension of a rank: local size m, `per`iodic or not, rank c of D, grid overlap 2 (as scatter_g._runs and
// gather_g._segments give them for an unstaggered field).
SpreadDim make_dim(int m, int per, int c, int D) {
  const int o = 2, ng = D * (m - o);
  SpreadDim S;
  SampleDim& d = S.own;
  d.m = m, d.per = per, d.E = per ? ng : ng + o;
  if (!per) {
    S.nrun = 1, S.i0[0] = 0, S.len[0] = m, S.g0[0] = c * (m - o);
    const int a = c == 0 ? 0 : 1, b = c == D - 1 ? m : m - 1;
    d.nseg = 1, d.g0[0] = c * (m - o) + a, d.g1[0] = c * (m - o) + b, d.i0[0] = a;
    return S;
  }
  int i = 0, g = ((c * (m - o) - 1) % ng + ng) % ng;
  while (i < m) {
    const int ln = ng - g < m - i ? ng - g : m - i;
    S.i0[S.nrun] = i, S.len[S.nrun] = ln, S.g0[S.nrun] = g, ++S.nrun;
    i += ln, g = 0;
  }
  const int g0 = ((c * (m - o) - 1 + 1) % ng + ng) % ng, n = m - 2;  // owned: local 1 .. m - 2
  if (g0 + n <= ng) {
    d.nseg = 1, d.g0[0] = g0, d.g1[0] = g0 + n, d.i0[0] = 1;
  } else {
    d.nseg = 2, d.g0[0] = g0, d.g1[0] = ng, d.i0[0] = 1;
    d.g0[1] = 0, d.g1[1] = g0 + n - ng, d.i0[1] = 1 + (ng - g0);
  }
  return S;
}

template <typename T>
void one_case(int nd, const int* m, int per, int D, int c, int copies) {
  SpreadPlanArgs pa;
  pa.nd = nd, pa.copies = copies;
  int64_t numel = 1;
  for (int d = 0; d < nd; ++d) {
    pa.dim[d] = make_dim(m[d], d == 0 ? per : 0, d == 0 ? c : 0, d == 0 ? D : 1);
    numel *= m[d];
  }
  const int64_t npts = 40;
  std::vector<double> P(static_cast<size_t>(npts * nd));  // exactly npts * nd doubles
  for (int64_t p = 0; p < npts; ++p)
    for (int d = 0; d < nd; ++d) {
      const int E = pa.dim[d].own.E;
      // quarters of the index range, beyond it on both sides, and a few non-finite coordinates
      double u = static_cast<double>(static_cast<int>(next() >> 8) % (4 * (E + 4))) / 4.0 - 2.0;
      if (p == 7 && d == 0) u = __builtin_nan("");
      if (p == 9 && d == nd - 1) u = __builtin_inf();
      P[static_cast<size_t>(p * nd + d)] = u;
    }
  pa.P = P.data(), pa.ps0 = nd, pa.ps1 = 1, pa.npts = npts;
  const SpreadPlan plan = host_spread_plan(pa);
  const int64_t ncells = static_cast<int64_t>(plan.cells.size());
  if (plan.start.size() != plan.cells.size() + 1 || plan.start.back() != static_cast<int64_t>(plan.point.size()))
    die("the segment starts do not match the entries", nd, m, per, copies);
  for (int64_t i = 0; i < ncells; ++i) {
    if (plan.cells[i] < 0 || plan.cells[i] >= numel) die("a cell outside of the field", nd, m, per, copies);
    if (i && plan.cells[i] <= plan.cells[i - 1]) die("cells not ascending", nd, m, per, copies);
    if (plan.start[i + 1] <= plan.start[i]) die("an empty segment", nd, m, per, copies);
    for (int64_t e = plan.start[i] + 1; e < plan.start[i + 1]; ++e)
      if (plan.point[e] < plan.point[e - 1] || (copies == SPREAD_ALL && plan.point[e] == plan.point[e - 1]))
        die("a segment not sorted by point", nd, m, per, copies);
  }
  // two fields of exactly numel elements (the second in the reversed layout), small integers / 4
  std::vector<T> A(static_cast<size_t>(numel)), B(static_cast<size_t>(numel)), A0;
  for (auto& x : A) x = static_cast<T>(static_cast<int>(next() >> 16) % 17 - 8) / 4;
  for (auto& x : B) x = static_cast<T>(static_cast<int>(next() >> 16) % 17 - 8) / 4;
  A0 = A;
  std::vector<double> V(static_cast<size_t>(2 * npts));
  for (auto& v : V) v = static_cast<double>(static_cast<int>(next() >> 16) % 9 - 4);
  SpreadArgs sa;
  sa.nd = nd, sa.nf = 2, sa.numel = numel;
  int64_t c_st[3] = {0, 0, 0}, r_st[3] = {0, 0, 0}, run = 1;
  for (int d = nd - 1; d >= 0; --d) c_st[d] = run, run *= m[d];
  run = 1;
  for (int d = 0; d < nd; ++d) r_st[d] = run, run *= m[d];
  for (int d = 0; d < nd; ++d) sa.m[d] = m[d], sa.field[0].stride[d] = c_st[d], sa.field[1].stride[d] = r_st[d];
  for (int d = nd; d < 3; ++d) sa.field[0].stride[d] = 0, sa.field[1].stride[d] = 0;
  sa.field[0].base = A.data(), sa.field[1].base = B.data();
  sa.ncells = ncells, sa.cells = plan.cells.data(), sa.start = plan.start.data();
  sa.point = plan.point.data(), sa.weight = plan.weight.data();
  sa.V = V.data(), sa.v_fs = npts, sa.v_ps = 1;
  const int64_t row = 1;  // V as the second of two rows of a table of one field's width: row 1 is the second field's
  host_spread_apply(sa, static_cast<int>(sizeof(T)));
  sa.row = &row, sa.nrows = 1, sa.row_stride = npts;
  std::vector<T> A1 = A;
  host_spread_apply(sa, static_cast<int>(sizeof(T)));  // the rows are used up: nothing happens
  if (std::memcmp(A1.data(), A.data(), A.size() * sizeof(T)) != 0) die("a used-up row counter added", nd, m, per, copies);
  if (copies != SPREAD_OWNER) return;
  // <A0, spread(V)> == <sample(A0), V> over the points this rank owns: exact on this data
  SampleArgs s;
  s.nd = nd, s.nf = 1, s.me0 = 0;
  for (int d = 0; d < nd; ++d) s.dim[d] = pa.dim[d].own;
  s.field[0].base = A0.data();
  for (int d = 0; d < 3; ++d) s.field[0].stride[d] = d < nd ? c_st[d] : 0;
  s.P = P.data(), s.ps0 = nd, s.ps1 = 1, s.npts = npts;
  std::vector<uint64_t> out(static_cast<size_t>(npts));
  s.out = out.data(), s.out_fs = npts;
  host_sample(s, static_cast<int>(sizeof(T)));
  double lhs = 0, rhs = 0;
  for (int64_t i = 0; i < numel; ++i)
    lhs += static_cast<double>(A0[static_cast<size_t>(i)]) *
           (static_cast<double>(A[static_cast<size_t>(i)]) - static_cast<double>(A0[static_cast<size_t>(i)]));
  for (int64_t p = 0; p < npts; ++p) {
    double v;
    std::memcpy(&v, &out[static_cast<size_t>(p)], 8);
    rhs += v * V[static_cast<size_t>(p)];  // (0 bits where the rank does not own the point or the point is invalid)
  }
  if (lhs != rhs) die("<A, spread(V)> != <sample(A), V>", nd, m, per, copies);
}

}  // namespace

int main() {
  int cases = 0;
  try {
    for (int nd = 1; nd <= 3; ++nd)
      for (int m0 = 4; m0 <= 7; ++m0)
        for (int m1 = 3; m1 <= (nd > 1 ? 5 : 3); ++m1)
          for (int m2 = 3; m2 <= (nd > 2 ? 4 : 3); ++m2)
            for (int per = 0; per <= 1; ++per)
              for (int D = 1; D <= 2; ++D)
                for (int c = 0; c < D; ++c)
                  for (int copies = 0; copies <= 1; ++copies) {
                    const int m[3] = {m0, m1, m2};
                    one_case<double>(nd, m, per, D, c, copies);
                    one_case<float>(nd, m, per, D, c, copies);
                    cases += 2;
                  }
  } catch (const Error& e) {
    std::fprintf(stderr, "spread_host_sweep: %s\n", e.what());
    return 1;
  }
  std::printf("spread_host_sweep: %d cases OK\n", cases);
  return 0;
}
