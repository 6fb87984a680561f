// Launcher and workspace of the projection kernels (igg/project.hpp).
#include "igg/project.hpp"

#include <map>
#include <mutex>

#include "igg/common.hpp"

namespace igg {

namespace {
struct Workspace {
  void* p = nullptr;
  size_t bytes = 0;
};
std::mutex g_ws_mu;
std::map<int, Workspace> g_ws;  // device -> partials
}  // namespace

size_t project_workspace_bytes() {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  size_t n = 0;
  for (const auto& [dev, w] : g_ws) n += w.bytes;
  return n;
}

void* project_workspace(size_t bytes, hipStream_t stream) {
  int dev = 0;
  IGG_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_ws_mu);
  Workspace& w = g_ws[dev];
  if (w.bytes >= bytes && w.p) return w.p;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  IGG_HIP_CHECK(hipStreamIsCapturing(stream, &cs));
  if (cs != hipStreamCaptureStatusNone)
    fail("project: this projection has to grow the workspace of its device (", w.bytes, " -> ", bytes,
         " bytes) and cannot do so inside a stream capture: call it once before capturing");
  if (w.p) {
    IGG_HIP_CHECK(hipDeviceSynchronize());  // no kernel may still use the partials
    IGG_HIP_CHECK(hipFree(w.p));
    w.p = nullptr, w.bytes = 0;
  }
  const size_t grown = static_cast<size_t>(round_up(static_cast<int64_t>(bytes), 1 << 16));
  IGG_HIP_CHECK(hipMalloc(&w.p, grown));
  w.bytes = grown;
  return w.p;
}

void project_free_workspace() {
  std::map<int, Workspace> ws;
  {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    ws.swap(g_ws);
  }
  if (ws.empty()) return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (const auto& [dev, w] : ws) {
    if (!w.p) continue;
    (void)hipSetDevice(dev);
    (void)hipDeviceSynchronize();  // no kernel may still use the partials
    (void)hipFree(w.p);
  }
  (void)hipSetDevice(cur);
}

void project_field(int op, const ReduceField& f, const std::vector<int>& keep, int elem_size,
                   const ProjectDest& dest, hipStream_t stream) {
  if (op < 0 || op >= R_NUM_OPS) fail("project: unknown op ", op);
  const bool two = reduce_two_inputs(op);
  if (!f.a || (two && !f.b)) fail("project: null field pointer");
  if (!dest.dst) fail("project: no destination");
  const ProjectPlan p = two ? plan_project(f.shape, f.stride_a, f.lo, f.hi, keep, elem_size, f.a, f.stride_b, f.b)
                            : plan_project(f.shape, f.stride_a, f.lo, f.hi, keep, elem_size, f.a);
  const size_t nk = keep.size();
  if (dest.start.size() != nk || dest.extent.size() != nk || dest.stride.size() != nk)
    fail("project: the destination needs a start, an extent and a stride per kept axis");
  ProjectStage2 s2;
  s2.dst = reinterpret_cast<double*>(dest.dst);
  s2.flags = reinterpret_cast<double*>(dest.flags);
  for (int k = 0; k < 2; ++k)
    s2.extent[k] = 1, s2.start[k] = 0, s2.stride[k] = 0, s2.own[k] = p.total > 0 ? 1 : 0, s2.pstride[k] = 0;
  for (size_t k = 0; k < nk; ++k) {
    const size_t at = 2 - nk + k;  // one kept axis: the inner slot
    if (dest.extent[k] < 1 || dest.start[k] < 0 || dest.start[k] >= dest.extent[k] || dest.stride[k] < 0)
      fail("project: destination start ", dest.start[k], " / extent ", dest.extent[k], " of kept axis ", keep[k]);
    if (p.keep_n[k] > dest.extent[k])
      fail("project: ", p.keep_n[k], " owned cells do not fit the destination's extent ", dest.extent[k]);
    s2.extent[at] = dest.extent[k], s2.start[at] = dest.start[k], s2.stride[at] = dest.stride[k];
    s2.own[at] = p.keep_n[k], s2.pstride[at] = p.keep_pstride[k];
  }
  s2.nout = p.nout;
  s2.slices = static_cast<uint32_t>(p.slices);
  s2.max_type = reduce_max_type(op) ? 1 : 0;
  s2.negate = (op == R_MIN && !dest.flags) ? 1 : 0;
  void* ws = nullptr;
  if (p.blocks > 0) {
    ws = project_workspace(static_cast<size_t>(p.slices) * static_cast<size_t>(p.nout) * 2 * sizeof(double), stream);
    ProjectJob j;
    j.a = reinterpret_cast<const char*>(f.a) + p.offset * elem_size;
    j.b = two ? reinterpret_cast<const char*>(f.b) + p.offset_b * elem_size : j.a;
    for (int k = 0; k < 4; ++k) j.s[k] = p.s[k], j.sb[k] = p.sb[k], j.n[k] = p.n[k];
    j.reduced = p.reduced;
    j.nout = p.nout;
    j.nv = static_cast<uint32_t>(p.nv);
    j.head = static_cast<uint32_t>(p.head);
    j.lanes_log2 = static_cast<uint32_t>(p.lanes_log2);
    j.cx = static_cast<uint32_t>(p.cx);
    j.slices = static_cast<uint32_t>(p.slices);
    j.units = static_cast<uint32_t>(p.units);
    j.block_units = static_cast<uint32_t>(p.block_units);
    launch_project_stage1(op, elem_size, p, j, ws, stream);
  }
  launch_project_stage2(s2, ws, stream);
}

}  // namespace igg
