// Launcher and workspace of the reduction kernels (igg/reduce.hpp).
#include "igg/reduce.hpp"

#include <map>
#include <mutex>

#include "igg/common.hpp"

namespace igg {

namespace {
std::mutex g_ws_mu;
std::map<int, void*> g_ws;  // device -> partials

constexpr size_t WS_BYTES = size_t{REDUCE_MAX_JOBS} * REDUCE_MAX_BLOCKS * 2 * sizeof(double);
}  // namespace

size_t reduce_workspace_bytes() {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  return g_ws.size() * WS_BYTES;
}

void* reduce_workspace(hipStream_t stream) {
  int dev = 0;
  IGG_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_ws_mu);
  auto it = g_ws.find(dev);
  if (it != g_ws.end()) return it->second;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  IGG_HIP_CHECK(hipStreamIsCapturing(stream, &cs));
  if (cs != hipStreamCaptureStatusNone)
    fail("reduce: the first reduction on a device allocates its workspace and cannot run inside a stream "
         "capture: call a reduction once before capturing");
  void* p = nullptr;
  IGG_HIP_CHECK(hipMalloc(&p, WS_BYTES));
  g_ws[dev] = p;
  return p;
}

void reduce_free_workspace() {
  std::map<int, void*> ws;
  {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    ws.swap(g_ws);
  }
  if (ws.empty()) return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (const auto& [dev, p] : ws) {
    (void)hipSetDevice(dev);
    (void)hipDeviceSynchronize();  // no kernel may still use the partials
    (void)hipFree(p);
  }
  (void)hipSetDevice(cur);
}

void reduce_fields(int op, const std::vector<ReduceField>& fields, int elem_size, double* out, double* flags,
                   hipStream_t stream) {
  if (op < 0 || op >= R_NUM_OPS) fail("reduce: unknown op ", op);
  if (fields.empty()) return;
  if (!out) fail("reduce: no output");
  const bool two = reduce_two_inputs(op);
  void* ws = reduce_workspace(stream);
  ReduceBatch batch;
  ReduceStage2 s2;
  size_t k = 0;
  while (k < fields.size()) {
    // one launch: consecutive fields with the same kind of loads, at most REDUCE_MAX_JOBS
    batch.n = 0;
    uint32_t blocks = 0;
    bool vec = false;
    const size_t first = k;
    for (; k < fields.size() && batch.n < REDUCE_MAX_JOBS; ++k) {
      const ReduceField& f = fields[k];
      if (!f.a || (two && !f.b)) fail("reduce: null field pointer");
      const ReducePlan p = two ? plan_reduce(f.shape, f.stride_a, f.lo, f.hi, elem_size, f.a, f.stride_b, f.b)
                               : plan_reduce(f.shape, f.stride_a, f.lo, f.hi, elem_size, f.a);
      const bool v = p.vec > 1;
      if (batch.n > 0 && v != vec) break;
      vec = v;
      ReduceJob& j = batch.job[batch.n];
      j.a = reinterpret_cast<const char*>(f.a) + p.offset * elem_size;
      j.b = two ? reinterpret_cast<const char*>(f.b) + p.offset_b * elem_size : j.a;
      for (int d = 0; d < 3; ++d) j.s[d] = p.s[d], j.sb[d] = p.sb[d];
      j.n2 = p.n[2];
      j.n1 = static_cast<uint32_t>(p.n[1]);
      j.nv = static_cast<uint32_t>(p.nv);
      j.head = static_cast<uint32_t>(p.head);
      j.cx = static_cast<uint32_t>(p.cx);
      j.g1 = static_cast<uint32_t>(p.g1);
      j.lx_log2 = static_cast<uint32_t>(p.lx_log2);
      j.tiles = static_cast<uint32_t>(p.tiles);
      j.nblocks = static_cast<uint32_t>(p.blocks);
      batch.block_start[batch.n] = blocks;
      s2.nblocks[batch.n] = j.nblocks;
      blocks += j.nblocks;
      ++batch.n;
    }
    batch.block_start[batch.n] = blocks;
    if (blocks > 0) launch_reduce_stage1(op, elem_size, vec, batch, ws, stream);
    s2.n = batch.n;
    s2.max_type = reduce_max_type(op) ? 1 : 0;
    s2.negate = (op == R_MIN && !flags) ? 1 : 0;
    s2.out = out + first;
    s2.flags = flags ? flags + first : nullptr;
    launch_reduce_stage2(s2, ws, stream);
  }
}

}  // namespace igg
