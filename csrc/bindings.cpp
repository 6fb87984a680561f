// pybind11 bindings of the native IGG runtime (_igg_native).
//
// The Python layer passes raw pointers, extents and strides of torch tensors
// (CPU or HIP) plus the current HIP stream handle; nothing here links libtorch,
// so the runtime is a self-contained C++/HIP library with a thin binding.
#include <pybind11/functional.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <chrono>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "igg/acoustic.hpp"
#include "igg/coherence.hpp"
#include "igg/comm.hpp"
#include "igg/copy.hpp"
#include "igg/copy_plan.hpp"
#include "igg/fault.hpp"
#include "igg/fused.hpp"
#include "igg/gather.hpp"
#include "igg/halo.hpp"
#include "igg/ipc.hpp"
#include "igg/project.hpp"
#include "igg/reduce.hpp"
#include "igg/sample.hpp"
#include "igg/select.hpp"
#include "igg/spread.hpp"
#include "igg/stencil.hpp"
#include "igg/topology.hpp"
#include "igg/trace.hpp"
#include "igg/vmm.hpp"
#include "igg/zedge.hpp"

namespace igg {
void launch_zcol_probe(int dir, const void* src, void* dst, int64_t rows, int64_t pitch, int aux,
                       hipStream_t stream);
void launch_stream_probe(int kind, double* out, const double* a, const double* b, int64_t n, int blocks,
                         hipStream_t stream);
}

namespace py = pybind11;
using namespace igg;

namespace {

// A job of the converting lattice copies as Python passes it: (src, dst, counts, src strides, dst strides).
using SelectTuple =
    std::tuple<uintptr_t, uintptr_t, std::array<int64_t, 3>, std::array<int64_t, 3>, std::array<int64_t, 3>>;

std::vector<SelectDesc> select_descs(const std::vector<SelectTuple>& jobs) {
  std::vector<SelectDesc> v;
  v.reserve(jobs.size());
  for (const auto& t : jobs) {
    SelectDesc j;
    j.src = std::get<0>(t), j.dst = std::get<1>(t);
    for (int d = 0; d < 3; ++d) j.c[d] = std::get<2>(t)[d], j.S[d] = std::get<3>(t)[d], j.T[d] = std::get<4>(t)[d];
    v.push_back(j);
  }
  return v;
}

// sample_g's arguments as Python passes them: per dimension (E, periodic, m,
// [(g0, g1, i0), ...]), per field (pointer, strides in elements).
using SampleDimTuple = std::tuple<int64_t, int, int64_t, std::vector<std::array<int64_t, 3>>>;
using SampleFieldTuple = std::pair<uintptr_t, std::vector<int64_t>>;

// One SampleArgs per SAMPLE_MAX_FIELDS fields, each handed to `run`.
template <typename Run>
void sample_calls(const char* who, const std::vector<SampleDimTuple>& dims, const std::vector<SampleFieldTuple>& fields,
                  uintptr_t points, int64_t ps0, int64_t ps1, int64_t npts, uintptr_t out, int64_t out_fs, bool me0,
                  uintptr_t row, int64_t nrows, int64_t row_stride, Run run) {
  SampleArgs a;
  a.nd = static_cast<int32_t>(dims.size());
  if (a.nd < 1 || a.nd > 3) fail(who, ": fields must have 1 to 3 dimensions (got ", dims.size(), ")");
  if (fields.empty()) fail(who, ": at least one field is needed");
  for (int d = 0; d < a.nd; ++d) {
    SampleDim& D = a.dim[d];
    const auto& segs = std::get<3>(dims[d]);
    if (segs.size() > 2) fail(who, ": at most two owned segments per dimension");
    auto narrow = [&](int64_t v) {
      if (v < 0 || v > INT32_MAX) fail(who, ": ", v, " in the table of dimension ", d, " is negative or above 2^31 - 1");
      return static_cast<int32_t>(v);
    };
    D.E = narrow(std::get<0>(dims[d])), D.per = std::get<1>(dims[d]) ? 1 : 0, D.m = narrow(std::get<2>(dims[d]));
    D.nseg = static_cast<int32_t>(segs.size());
    for (int s = 0; s < D.nseg; ++s)
      D.g0[s] = narrow(segs[s][0]), D.g1[s] = narrow(segs[s][1]), D.i0[s] = narrow(segs[s][2]);
  }
  a.me0 = me0 ? 1 : 0;
  a.P = reinterpret_cast<const double*>(points), a.ps0 = ps0, a.ps1 = ps1, a.npts = npts;
  a.out_fs = out_fs;
  a.row = reinterpret_cast<const int64_t*>(row), a.nrows = nrows, a.row_stride = row_stride;
  for (size_t f0 = 0; f0 < fields.size(); f0 += SAMPLE_MAX_FIELDS) {
    a.nf = static_cast<int32_t>(std::min<size_t>(fields.size() - f0, SAMPLE_MAX_FIELDS));
    for (int f = 0; f < a.nf; ++f) {
      const auto& [ptr, strides] = fields[f0 + f];
      if (static_cast<int>(strides.size()) != a.nd) fail(who, ": one stride per dimension of the field");
      a.field[f].base = reinterpret_cast<const void*>(ptr);
      for (int d = 0; d < 3; ++d) a.field[f].stride[d] = d < a.nd ? strides[d] : 0;
    }
    a.out = reinterpret_cast<uint64_t*>(out) + static_cast<int64_t>(f0) * out_fs;
    run(a);
  }
}

// spread_g's table as Python passes it: per dimension (E, periodic, m, [(g0, g1,
// i0), ...] owned segments, [(i0, len, g0), ...] runs of the local range).
using SpreadDimTuple =
    std::tuple<int64_t, int, int64_t, std::vector<std::array<int64_t, 3>>, std::vector<std::array<int64_t, 3>>>;

SpreadPlanArgs spread_plan_args(const char* who, const std::vector<SpreadDimTuple>& dims, int copies, uintptr_t points,
                                int64_t ps0, int64_t ps1, int64_t npts) {
  SpreadPlanArgs a;
  a.nd = static_cast<int32_t>(dims.size());
  if (a.nd < 1 || a.nd > 3) fail(who, ": fields must have 1 to 3 dimensions (got ", dims.size(), ")");
  a.copies = copies;
  for (int d = 0; d < a.nd; ++d) {
    SpreadDim& S = a.dim[d];
    SampleDim& D = S.own;
    const auto& segs = std::get<3>(dims[d]);
    const auto& runs = std::get<4>(dims[d]);
    if (segs.size() > 2) fail(who, ": at most two owned segments per dimension");
    if (runs.size() > SPREAD_MAX_RUNS) fail(who, ": at most ", SPREAD_MAX_RUNS, " runs per dimension");
    auto narrow = [&](int64_t v) {
      if (v < 0 || v > INT32_MAX) fail(who, ": ", v, " in the table of dimension ", d, " is negative or above 2^31 - 1");
      return static_cast<int32_t>(v);
    };
    D.E = narrow(std::get<0>(dims[d])), D.per = std::get<1>(dims[d]) ? 1 : 0, D.m = narrow(std::get<2>(dims[d]));
    D.nseg = static_cast<int32_t>(segs.size());
    for (int s = 0; s < D.nseg; ++s)
      D.g0[s] = narrow(segs[s][0]), D.g1[s] = narrow(segs[s][1]), D.i0[s] = narrow(segs[s][2]);
    S.nrun = static_cast<int32_t>(runs.size());
    for (int r = 0; r < S.nrun; ++r)
      S.i0[r] = narrow(runs[r][0]), S.len[r] = narrow(runs[r][1]), S.g0[r] = narrow(runs[r][2]);
  }
  a.P = reinterpret_cast<const double*>(points), a.ps0 = ps0, a.ps1 = ps1, a.npts = npts;
  return a;
}

// One SpreadArgs per SPREAD_MAX_FIELDS fields, each handed to `run`.
template <typename Run>
void spread_calls(const char* who, const std::vector<int64_t>& shape, const std::vector<SampleFieldTuple>& fields,
                  int64_t ncells, uintptr_t cells, uintptr_t start, uintptr_t point, uintptr_t weight, uintptr_t values,
                  int64_t v_fs, int64_t v_ps, uintptr_t row, int64_t nrows, int64_t row_stride, Run run) {
  SpreadArgs a;
  a.nd = static_cast<int32_t>(shape.size());
  if (a.nd < 1 || a.nd > 3) fail(who, ": fields must have 1 to 3 dimensions (got ", shape.size(), ")");
  if (fields.empty()) fail(who, ": at least one field is needed");
  for (int d = 0; d < a.nd; ++d) {
    if (shape[d] < 1 || shape[d] > INT32_MAX) fail(who, ": size ", shape[d], " in dimension ", d);
    a.m[d] = shape[d];
    a.numel *= shape[d];
  }
  a.ncells = ncells;
  a.cells = reinterpret_cast<const int64_t*>(cells), a.start = reinterpret_cast<const int64_t*>(start);
  a.point = reinterpret_cast<const int64_t*>(point), a.weight = reinterpret_cast<const double*>(weight);
  a.v_fs = v_fs, a.v_ps = v_ps;
  a.row = reinterpret_cast<const int64_t*>(row), a.nrows = nrows, a.row_stride = row_stride;
  for (size_t f0 = 0; f0 < fields.size(); f0 += SPREAD_MAX_FIELDS) {
    a.nf = static_cast<int32_t>(std::min<size_t>(fields.size() - f0, SPREAD_MAX_FIELDS));
    for (int f = 0; f < a.nf; ++f) {
      const auto& [ptr, strides] = fields[f0 + f];
      if (static_cast<int>(strides.size()) != a.nd) fail(who, ": one stride per dimension of the field");
      a.field[f].base = reinterpret_cast<void*>(ptr);
      for (int d = 0; d < 3; ++d) a.field[f].stride[d] = d < a.nd ? strides[d] : 0;
    }
    a.V = reinterpret_cast<const double*>(values) + static_cast<int64_t>(f0) * v_fs;
    run(a);
  }
}

// DLPack (v0.8 ABI, the layout torch.utils.dlpack consumes): a native device
// allocation of a given memory kind handed to torch as a 1-D uint8 tensor
// whose deleter frees it. Lets a model keep its fields in fine-grained memory
// (docs/COHERENCE.md) without linking libtorch.
struct DLDevice { int32_t device_type; int32_t device_id; };
struct DLDataType { uint8_t code; uint8_t bits; uint16_t lanes; };
struct DLTensor {
  void* data;
  DLDevice device;
  int32_t ndim;
  DLDataType dtype;
  int64_t* shape;
  int64_t* strides;
  uint64_t byte_offset;
};
struct DLManagedTensor {
  DLTensor dl_tensor;
  void* manager_ctx;
  void (*deleter)(DLManagedTensor*);
};
constexpr int32_t kDLROCM = 10;

struct DlpackAlloc {
  int64_t shape[1];
  int device;
};

// Freeing a field whose tensor was garbage-collected: kernels queued on any
// stream may still use it, and a device synchronisation right here would
// invalidate a hipGraph capture in progress on this thread. So the
// release is DEFERRED: the buffer joins a list that is drained (one device
// synchronisation, then hipFree) at the next native allocation, at
// finalize_global_grid / model close, or at exit - never inside a capture.
std::mutex g_deferred_mu;
std::vector<std::pair<void*, int>> g_deferred;  // (pointer, device)

void flush_deferred_frees() {
  std::vector<std::pair<void*, int>> v;
  {
    std::lock_guard<std::mutex> lk(g_deferred_mu);
    v.swap(g_deferred);
  }
  if (v.empty()) return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  int synced = -1;
  for (const auto& [p, dev] : v) {
    if (dev != synced) {
      (void)hipSetDevice(dev);
      (void)hipDeviceSynchronize();  // no kernel may still use the buffers
      synced = dev;
    }
    if (vmm_find(p, nullptr, nullptr)) vmm_free(p);  // a MemKind::Vmm field
    else (void)hipFree(p);
  }
  (void)hipSetDevice(cur);
}

void dlpack_free(DLManagedTensor* t) {
  if (!t) return;
  auto* ctx = static_cast<DlpackAlloc*>(t->manager_ctx);
  {
    std::lock_guard<std::mutex> lk(g_deferred_mu);
    g_deferred.emplace_back(t->dl_tensor.data, ctx->device);
  }
  delete ctx;
  delete t;
}

py::capsule alloc_dlpack(size_t bytes, int kind) {
  if (bytes == 0) fail("alloc_dlpack: zero bytes");
  flush_deferred_frees();  // allocation time is a safe point (no capture in progress)
  int dev = 0;
  IGG_HIP_CHECK(hipGetDevice(&dev));
  void* p = ipc_malloc(bytes, static_cast<MemKind>(kind));
  auto* ctx = new DlpackAlloc{{static_cast<int64_t>(bytes)}, dev};
  auto* t = new DLManagedTensor{};
  t->dl_tensor.data = p;
  t->dl_tensor.device = {kDLROCM, dev};
  t->dl_tensor.ndim = 1;
  t->dl_tensor.dtype = {1 /* kDLUInt */, 8, 1};
  t->dl_tensor.shape = ctx->shape;
  t->dl_tensor.strides = nullptr;
  t->dl_tensor.byte_offset = 0;
  t->manager_ctx = ctx;
  t->deleter = dlpack_free;
  // Unconsumed capsules free their tensor; torch renames a consumed one to
  // "used_dltensor" and owns the deleter from then on.
  return py::capsule(t, "dltensor", [](PyObject* cap) {
    if (PyCapsule_IsValid(cap, "dltensor")) dlpack_free(static_cast<DLManagedTensor*>(PyCapsule_GetPointer(cap, "dltensor")));
  });
}

hipStream_t as_stream(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

using FieldTuple = std::tuple<uintptr_t, int, std::array<int64_t, 3>, std::array<int64_t, 3>, int, bool>;

Field to_field(const FieldTuple& t) {
  Field f;
  f.ptr = std::get<0>(t);
  f.ndims = std::get<1>(t);
  f.size = std::get<2>(t);
  f.stride = std::get<3>(t);
  f.elem_bytes = std::get<4>(t);
  f.device = std::get<5>(t);
  return f;
}

std::vector<Field> to_fields(const std::vector<FieldTuple>& ts) {
  std::vector<Field> fs;
  fs.reserve(ts.size());
  for (const auto& t : ts) fs.push_back(to_field(t));
  return fs;
}

GridInfo make_grid(int64_t me, int64_t nprocs, const Int3& nxyz, const Int3& overlaps,
                   const std::array<Int3, 2>& neighbors, const std::vector<int64_t>& peers,
                   const Int3& halowidths) {
  GridInfo g;
  g.halowidths = halowidths;
  g.me = me;
  g.nprocs = nprocs;
  g.nxyz = nxyz;
  g.overlaps = overlaps;
  g.neighbors = neighbors;
  if (!peers.empty()) {
    if (peers.size() != 27) fail("GridInfo: peers must have 27 entries (dir_key order)");
    for (int k = 0; k < 27; ++k) g.peers[k] = peers[k];
    g.has_peers = true;
  }
  return g;
}

// Transport implemented in Python (torch.distributed gloo/nccl point-to-point).
class PyTransport : public Transport {
 public:
  PyTransport(py::function fn, bool host, bool dev, std::string name)
      : fn_(std::move(fn)), host_(host), dev_(dev), name_(std::move(name)) {}
  bool device_capable() const override { return dev_; }
  bool host_capable() const override { return host_; }
  std::string name() const override { return name_; }
  void exchange(const std::vector<P2POp>& recvs, const std::vector<P2POp>& sends, bool device,
                hipStream_t stream) override {
    auto conv = [](const std::vector<P2POp>& ops) {
      py::list l;
      for (const auto& o : ops)
        l.append(py::make_tuple(reinterpret_cast<uintptr_t>(o.ptr), o.bytes, o.peer, o.tag));
      return l;
    };
    fn_(conv(recvs), conv(sends), device, reinterpret_cast<uintptr_t>(stream));
  }

 private:
  py::function fn_;
  bool host_, dev_;
  std::string name_;
};

// Pre-converted field list: the update_halo hot path converts tuples once per
// plan, not per call.
struct FieldSet {
  std::vector<Field> f;
};

AccumType accum_type(const std::string& dtype) {
  static const std::pair<const char*, AccumType> names[] = {
      {"float32", AccumType::F32}, {"float64", AccumType::F64}, {"int8", AccumType::I8},
      {"int16", AccumType::I16},   {"int32", AccumType::I32},   {"int64", AccumType::I64},
      {"uint8", AccumType::U8},    {"float16", AccumType::F16}, {"bfloat16", AccumType::BF16},
      {"complex64", AccumType::C64}, {"complex128", AccumType::C128}};
  for (const auto& n : names)
    if (dtype == n.first) return n.second;
  fail("accumulate: unsupported element type '", dtype, "'");
}

std::vector<Accum3D> to_accums(const std::vector<std::array<int64_t, 9>>& boxes,
                               const std::vector<std::pair<uintptr_t, uintptr_t>>& ptrs,
                               const std::vector<std::string>& ops) {
  if (boxes.size() != ptrs.size() || boxes.size() != ops.size())
    fail("accum3d: one (src, dst) pair and one operation per box");
  std::vector<Accum3D> v;
  for (size_t k = 0; k < boxes.size(); ++k) {
    const auto& b = boxes[k];
    v.push_back({{reinterpret_cast<const char*>(ptrs[k].first), reinterpret_cast<char*>(ptrs[k].second), b[0], b[1],
                  b[2], b[3], b[4], b[5], b[6], b[7], b[8]},
                 accum_op_from_name(ops[k].c_str())});
  }
  return v;
}

std::vector<Box> to_boxes(const std::vector<std::pair<Int3, Int3>>& bs) {
  std::vector<Box> out;
  for (const auto& b : bs) {
    Box x;
    for (int d = 0; d < 3; ++d) { x.lo[d] = b.first[d]; x.hi[d] = b.second[d]; }
    out.push_back(x);
  }
  return out;
}

std::pair<Int3, Int3> from_box(const Box& b) {
  return {{b.lo[0], b.lo[1], b.lo[2]}, {b.hi[0], b.hi[1], b.hi[2]}};
}

}  // namespace

PYBIND11_MODULE(_igg_native, m) {
  m.doc() = "Native MI355X runtime of the implicit global grid (HIP kernels + RCCL).";
  py::register_exception<Error>(m, "IGGError", PyExc_RuntimeError);

  m.attr("PROC_NULL") = PROC_NULL;
  m.attr("NDIMS") = NDIMS;
  m.attr("NNEIGHBORS") = NNEIGHBORS;
  m.attr("ALLOC_GRANULARITY") = ALLOC_GRANULARITY;
  m.attr("THREADCOPY_THRESHOLD") = THREADCOPY_THRESHOLD;

  // --- topology
  m.def("dims_create", &dims_create, py::arg("nprocs"), py::arg("dims"));
  m.def("cart_coords", &cart_coords, py::arg("rank"), py::arg("dims"));
  m.def("cart_rank", &cart_rank, py::arg("coords"), py::arg("dims"));
  m.def("cart_shift", &cart_shift, py::arg("rank"), py::arg("dim"), py::arg("disp"),
        py::arg("dims"), py::arg("periods"));
  m.def("global_size", &global_size);
  m.def("coord_g", &coord_g);

  // --- device
  m.def("device_count", []() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
  });
  m.def("set_device", [](int d) { IGG_HIP_CHECK(hipSetDevice(d)); });
  m.def("get_device", []() {
    int d = 0;
    IGG_HIP_CHECK(hipGetDevice(&d));
    return d;
  });
  m.def("device_synchronize", []() {
    py::gil_scoped_release nogil;
    IGG_HIP_CHECK(hipDeviceSynchronize());
  });
  // Bounded, low-latency wait for everything enqueued on stream `s` so far:
  // an event recorded there is polled (GIL released) until it completes or
  // `timeout` seconds pass (returns false; the caller aborts communicators).
  // Unlike a helper thread around hipDeviceSynchronize it returns within
  // microseconds of completion, so a timed region pays no wake-up latency.
  m.def("stream_wait_bounded", [](uintptr_t s, double timeout) {
    thread_local hipEvent_t ev = nullptr;
    if (!ev) IGG_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    IGG_HIP_CHECK(hipEventRecord(ev, as_stream(s)));
    py::gil_scoped_release nogil;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t e = hipEventQuery(ev);
      if (e == hipSuccess) return true;
      if (e != hipErrorNotReady) IGG_HIP_CHECK(e);
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout) return false;
      std::this_thread::yield();
    }
  }, py::arg("stream"), py::arg("timeout"));
  m.def("stream_synchronize", [](uintptr_t s) {
    py::gil_scoped_release nogil;
    IGG_HIP_CHECK(hipStreamSynchronize(as_stream(s)));
  });
  m.def("memcpy_d2h", [](uintptr_t src, size_t n) {
    std::string out(n, '\0');
    IGG_HIP_CHECK(hipMemcpy(out.data(), reinterpret_cast<void*>(src), n, hipMemcpyDeviceToHost));
    return py::bytes(out);
  });
  m.def("clear_last_error", []() {
    const hipError_t e = hipGetLastError();  // reads and resets the thread's sticky error
    return e == hipSuccess ? std::string() : std::string(hipGetErrorString(e));
  }, "Reset the HIP runtime's last-error state (after a failed capture); returns the error it held.");
  m.def("rccl_version", &rccl_version);
  m.def("abandoned_waits", &abandoned_waits,
        "Bounded first-contact calls this process gave up on (their helper threads are still stuck in the "
        "runtime): a process with any should be replaced, not reused (fault.hpp).");
  m.def("first_contact_timeout", &first_contact_timeout);
  m.def("install_crash_handler", &install_crash_handler,
        "Print a native backtrace on SIGSEGV/SIGBUS/SIGABRT, then chain to the previous handler "
        "(faulthandler's Python stack).");
  m.def("trace_enabled", &trace_enabled);
  m.def("trace_push", [](const std::string& n) { trace_push(n.c_str()); });
  m.def("trace_pop", &trace_pop);
  m.def("trace_mark", [](const std::string& n) { trace_mark(n.c_str()); });

  // --- intra-node peer memory (put transport primitives)
  m.def("ipc_malloc", [](size_t bytes, int kind) {
    return reinterpret_cast<uintptr_t>(ipc_malloc(bytes, static_cast<MemKind>(kind)));
  });
  m.def("ipc_free", [](uintptr_t p) { ipc_free(reinterpret_cast<void*>(p)); });
  m.def("flush_deferred_frees", &flush_deferred_frees,
        "Free the native field buffers whose tensors were released (one device synchronisation); "
        "called at finalize / model close. Never call it inside a hipGraph capture.");
  m.def("deferred_frees", []() {
    std::lock_guard<std::mutex> lk(g_deferred_mu);
    return g_deferred.size();
  });
  m.def("alloc_dlpack", &alloc_dlpack, py::arg("bytes"), py::arg("kind"),
        "Zeroed device allocation of a MemKind as a DLPack capsule (1-D uint8; torch.utils.dlpack.from_dlpack).");
  m.def("ipc_get_handle", [](uintptr_t p) { return py::bytes(ipc_get_handle(reinterpret_cast<void*>(p))); });
  m.def("alloc_bytes", [](uintptr_t p) { return alloc_bytes(reinterpret_cast<const void*>(p)); }, py::arg("ptr"),
        "Size of the device allocation holding `ptr` (hipMemGetAddressRange).");
  m.attr("IPC_MAX_BYTES") = py::int_(IPC_MAX_BYTES);
  m.def("ipc_open", [](const std::string& h) { return reinterpret_cast<uintptr_t>(ipc_open(h)); });
  m.def("ipc_close", [](uintptr_t p) { ipc_close(reinterpret_cast<void*>(p)); });
  m.def("stream_write_u64", [](uintptr_t s, uintptr_t p, uint64_t v) {
    stream_write_u64(as_stream(s), reinterpret_cast<void*>(p), v);
  });
  m.def("stream_wait_u64_geq", [](uintptr_t s, uintptr_t p, uint64_t v) {
    stream_wait_u64_geq(as_stream(s), reinterpret_cast<void*>(p), v);
  });
  m.def("can_stream_wait_value", &can_stream_wait_value);
  m.def("gpu_spin", [](double seconds, uintptr_t s) { launch_spin(seconds, as_stream(s)); },
        py::arg("seconds"), py::arg("stream"));
  m.def("read_u64", [](uintptr_t p) {
    uint64_t v = 0;
    IGG_HIP_CHECK(hipMemcpy(&v, reinterpret_cast<void*>(p), 8, hipMemcpyDeviceToHost));
    return v;
  });
  // Streams restricted to a subset of CUs (MI355X CU masking): the halo stream
  // can own a few CUs so communication kernels (RCCL's spin on each other and
  // need all their workgroups resident) never wait behind a compute kernel
  // that fills every CU. Returns the hipStream_t as an integer.
  m.def("stream_create_cu_mask", [](const std::vector<uint32_t>& mask, int priority) {
    hipStream_t s = nullptr;
    if (mask.empty()) {
      IGG_HIP_CHECK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority));
    } else {
      IGG_HIP_CHECK(hipExtStreamCreateWithCUMask(&s, static_cast<uint32_t>(mask.size()), mask.data()));
    }
    return reinterpret_cast<uintptr_t>(s);
  }, py::arg("mask"), py::arg("priority") = 0);
  m.def("stream_destroy", [](uintptr_t s) { IGG_HIP_CHECK(hipStreamDestroy(as_stream(s))); });
  m.def("stream_get_cu_mask", [](uintptr_t s, int words) {
    std::vector<uint32_t> m(static_cast<size_t>(words), 0u);
    IGG_HIP_CHECK(hipExtStreamGetCUMask(as_stream(s), static_cast<uint32_t>(words), m.data()));
    return m;
  });
  m.def("cu_count", []() {
    int dev = 0, cus = 0;
    IGG_HIP_CHECK(hipGetDevice(&dev));
    IGG_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    return cus;
  });
  // Stream-ordered blocking copies for the host-staged transport: wait for all
  // prior work on `stream`, copy, wait again.
  m.def("memcpy_d2h_stream", [](uintptr_t dst, uintptr_t src, size_t n, uintptr_t s) {
    py::gil_scoped_release nogil;
    IGG_HIP_CHECK(hipStreamSynchronize(as_stream(s)));
    IGG_HIP_CHECK(hipMemcpyAsync(reinterpret_cast<void*>(dst), reinterpret_cast<const void*>(src), n,
                                 hipMemcpyDeviceToHost, as_stream(s)));
    IGG_HIP_CHECK(hipStreamSynchronize(as_stream(s)));
  });
  m.def("memcpy_h2d_stream", [](uintptr_t dst, uintptr_t src, size_t n, uintptr_t s) {
    py::gil_scoped_release nogil;
    IGG_HIP_CHECK(hipStreamSynchronize(as_stream(s)));
    IGG_HIP_CHECK(hipMemcpyAsync(reinterpret_cast<void*>(dst), reinterpret_cast<const void*>(src), n,
                                 hipMemcpyHostToDevice, as_stream(s)));
    IGG_HIP_CHECK(hipStreamSynchronize(as_stream(s)));
  });

  // --- field geometry helpers (test hooks)
  m.def("ol", [](const GridInfo& g, int dim, const FieldTuple& f) { return ol(g, dim, to_field(f)); });
  m.def("max_halo_elems", [](const FieldTuple& f) { return max_halo_elems(to_field(f)); });
  m.def("send_index", [](const GridInfo& g, int side, int dim, const FieldTuple& f) {
    return send_index(g, side, dim, to_field(f));
  });
  m.def("recv_index", [](const GridInfo& g, int side, int dim, const FieldTuple& f) {
    return recv_index(g, side, dim, to_field(f));
  });
  m.def("face_info", [](const FieldTuple& f, int dim, int64_t index) {
    const Face fc = face(to_field(f), dim, index);
    return py::make_tuple(reinterpret_cast<uintptr_t>(fc.base), fc.n_outer, fc.n_inner, fc.s_outer,
                          fc.s_inner, fc.contiguous, fc.bytes);
  });

  m.def("slab_info", [](const FieldTuple& f, int dim, int64_t lo, int64_t w) {
    const Field fd = to_field(f);
    if (dim < 0 || dim >= NDIMS || w < 1 || lo < 0 || lo + w > fd.size[dim]) fail("slab_info: planes out of range");
    const Face fc = slab(fd, dim, lo, w);
    return py::make_tuple(reinterpret_cast<uintptr_t>(fc.base), fc.n_outer, fc.n_mid, fc.n_inner, fc.s_outer,
                          fc.s_mid, fc.s_inner, fc.contiguous, fc.bytes);
  });

  py::class_<GridInfo>(m, "GridInfo")
      .def(py::init(&make_grid), py::arg("me"), py::arg("nprocs"), py::arg("nxyz"),
           py::arg("overlaps"), py::arg("neighbors"), py::arg("peers") = std::vector<int64_t>{},
           py::arg("halowidths") = Int3{1, 1, 1})
      .def_readonly("peers", &GridInfo::peers)
      .def_readonly("has_peers", &GridInfo::has_peers)
      .def_readwrite("me", &GridInfo::me)
      .def_readwrite("nprocs", &GridInfo::nprocs)
      .def_readwrite("nxyz", &GridInfo::nxyz)
      .def_readwrite("overlaps", &GridInfo::overlaps)
      .def_readwrite("halowidths", &GridInfo::halowidths)
      .def_readwrite("neighbors", &GridInfo::neighbors);

  // --- copies
  m.def("copy2d",
        [](const std::vector<std::tuple<uintptr_t, uintptr_t, int64_t, int64_t, int64_t, int64_t,
                                        int64_t, int64_t>>& cs,
           int elem_bytes, bool device, uintptr_t stream, bool system) {
          std::vector<Copy2D> v;
          for (const auto& c : cs)
            v.push_back({reinterpret_cast<const char*>(std::get<0>(c)),
                         reinterpret_cast<char*>(std::get<1>(c)), std::get<2>(c), std::get<3>(c),
                         std::get<4>(c), std::get<5>(c), std::get<6>(c), std::get<7>(c)});
          if (device) launch_copy2d(v, elem_bytes, as_stream(stream), system);
          else host_copy2d(v, elem_bytes);
        },
        py::arg("copies"), py::arg("elem_bytes"), py::arg("device"), py::arg("stream") = 0,
        py::arg("system") = false,
        "Batched strided 2-D copies; system: the put transport's system-scope (sc0 sc1) stores.");

  m.def("copy3d",
        [](const std::vector<std::array<int64_t, 9>>& boxes, const std::vector<std::pair<uintptr_t, uintptr_t>>& ptrs,
           int elem_bytes, bool device, uintptr_t stream, bool system) {
          if (boxes.size() != ptrs.size()) fail("copy3d: one (src, dst) pair per box");
          std::vector<Copy3D> v;
          for (size_t k = 0; k < boxes.size(); ++k) {
            const auto& b = boxes[k];
            v.push_back({reinterpret_cast<const char*>(ptrs[k].first), reinterpret_cast<char*>(ptrs[k].second),
                         b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8]});
          }
          if (device) launch_copy3d(v, elem_bytes, as_stream(stream), system);
          else host_copy3d(v, elem_bytes);
        },
        py::arg("boxes"), py::arg("ptrs"), py::arg("elem_bytes"), py::arg("device"), py::arg("stream") = 0,
        py::arg("system") = false,
        "Batched strided 3-extent copies (slab kernel): boxes are (n_outer, n_mid, n_inner, src strides, dst "
        "strides), strides in elements.");

  m.def("copy2d_plan",
        [](const std::tuple<uintptr_t, uintptr_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>& c,
           int elem_bytes) {
          const CopyPlan2 p = plan_copy2d(
              {reinterpret_cast<const char*>(std::get<0>(c)), reinterpret_cast<char*>(std::get<1>(c)),
               std::get<2>(c), std::get<3>(c), std::get<4>(c), std::get<5>(c), std::get<6>(c), std::get<7>(c)},
              elem_bytes, g_copy_gather);
          py::dict d;
          d["box"] = py::make_tuple(p.box.n_outer, p.box.n_inner, p.box.src_so, p.box.src_si, p.box.dst_so,
                                    p.box.dst_si);
          d["path"] = copy_path_name(p.path);
          d["vec_bytes"] = p.vec_bytes;
          d["blocks"] = p.blocks;
          return d;
        },
        py::arg("copy"), py::arg("elem_bytes"),
        "What launch_copy2d does with one copy: box (n_outer, n_inner, src strides, dst strides), path "
        "(flat / gather / chunk), vec_bytes (0) and blocks.");

  m.def("copy3d_plan",
        [](const std::array<int64_t, 9>& b, const std::pair<uintptr_t, uintptr_t>& ptrs, int elem_bytes) {
          const CopyPlan3 p = plan_copy3d(
              {reinterpret_cast<const char*>(ptrs.first), reinterpret_cast<char*>(ptrs.second), b[0], b[1], b[2],
               b[3], b[4], b[5], b[6], b[7], b[8]},
              elem_bytes, ParityShift{}, g_copy_gather);
          py::dict d;
          d["box"] = py::make_tuple(p.box.n_outer, p.box.n_mid, p.box.n_inner, p.box.src_so, p.box.src_sm,
                                    p.box.src_si, p.box.dst_so, p.box.dst_sm, p.box.dst_si);
          d["path"] = copy_path_name(p.path);
          d["vec_bytes"] = p.vec_bytes;
          d["blocks"] = p.blocks;
          return d;
        },
        py::arg("box"), py::arg("ptrs"), py::arg("elem_bytes"),
        "What launch_copy3d does with one box: the normalised box (extents, src strides, dst strides), path "
        "(flat / gather / chunk), vec_bytes (0, 4, 8 or 16) and blocks.");

  // --- accumulation (the transposed halo exchange's kernels)
  m.def("accum3d",
        [](const std::vector<std::array<int64_t, 9>>& boxes, const std::vector<std::pair<uintptr_t, uintptr_t>>& ptrs,
           const std::vector<std::string>& ops, const std::string& dtype, uintptr_t stream) {
          launch_accum3d(to_accums(boxes, ptrs, ops), accum_type(dtype), as_stream(stream));
        },
        py::arg("boxes"), py::arg("ptrs"), py::arg("ops"), py::arg("dtype"), py::arg("stream") = 0,
        "Batched strided accumulation on the GPU: boxes and (src, dst) pointers as for copy3d, one operation "
        "per box ('add': dst += src; 'take': dst = src, src = 0; 'add_take': both; 'zero': dst = 0); dtype "
        "'float32' or 'float64'. Descriptors of one call must not share cells.");
  m.def("host_accum3d",
        [](const std::vector<std::array<int64_t, 9>>& boxes, const std::vector<std::pair<uintptr_t, uintptr_t>>& ptrs,
           const std::vector<std::string>& ops, const std::string& dtype) {
          host_accum3d(to_accums(boxes, ptrs, ops), accum_type(dtype));
        },
        py::arg("boxes"), py::arg("ptrs"), py::arg("ops"), py::arg("dtype"),
        "accum3d on host memory, one descriptor after the other; every torch dtype that adds, bool excepted.");
  m.def("accum3d_plan",
        [](const std::array<int64_t, 9>& b, const std::pair<uintptr_t, uintptr_t>& ptrs, const std::string& dtype) {
          const CopyPlan3 p = plan_accum3d(
              {reinterpret_cast<const char*>(ptrs.first), reinterpret_cast<char*>(ptrs.second), b[0], b[1], b[2],
               b[3], b[4], b[5], b[6], b[7], b[8]},
              accum_elem_bytes(accum_type(dtype)), g_copy_gather);
          py::dict d;
          d["box"] = py::make_tuple(p.box.n_outer, p.box.n_mid, p.box.n_inner, p.box.src_so, p.box.src_sm,
                                    p.box.src_si, p.box.dst_so, p.box.dst_sm, p.box.dst_si);
          d["path"] = copy_path_name(p.path);
          d["vec_bytes"] = p.vec_bytes;
          d["blocks"] = p.blocks;
          return d;
        },
        py::arg("box"), py::arg("ptrs"), py::arg("dtype"),
        "What accum3d does with one box: the normalised box, path (flat / gather / chunk), vec_bytes (gather: "
        "the row as one access of 4, 8 or 16 bytes; chunk: 16 where both sides are aligned; else 0) and blocks.");
  m.attr("MAX_BATCH") = MAX_BATCH;

  // --- reductions (ops/reduce.py)
  m.attr("REDUCE_MAX_BLOCKS") = REDUCE_MAX_BLOCKS;
  m.attr("REDUCE_MAX_JOBS") = REDUCE_MAX_JOBS;
  m.attr("REDUCE_UNROLL") = REDUCE_UNROLL;
  m.def("reduce_plan",
        [](const std::vector<int64_t>& shape, const std::vector<int64_t>& strides, const std::vector<int64_t>& lo,
           const std::vector<int64_t>& hi, int elem_size, uintptr_t base_address,
           const std::vector<int64_t>& strides_b, uintptr_t base_b) {
          const ReducePlan p = plan_reduce(shape, strides, lo, hi, elem_size, base_address, strides_b, base_b);
          py::dict d;
          d["path"] = reduce_path_name(p.path);
          d["box"] = py::make_tuple(p.n[0], p.n[1], p.n[2]);
          d["strides"] = py::make_tuple(p.s[0], p.s[1], p.s[2]);
          d["offset"] = p.offset;
          d["total"] = p.total;
          d["vec"] = p.vec;
          d["head"] = p.head;
          d["loads_per_row"] = p.nv;
          d["lanes_per_row"] = int64_t{1} << p.lx_log2;
          d["tiles"] = p.tiles;
          d["blocks"] = p.blocks;
          return d;
        },
        py::arg("shape"), py::arg("strides"), py::arg("lo"), py::arg("hi"), py::arg("elem_size"),
        py::arg("base_address"), py::arg("strides_b") = std::vector<int64_t>{}, py::arg("base_b") = 0,
        "What a reduction does with the box [lo, hi) of one field: the merged box (extents, strides in elements), "
        "path (flat / rows / element), elements per load, head mask, tiles and blocks.");
  m.def("reduce",
        [](int op,
           const std::vector<std::tuple<uintptr_t, uintptr_t, std::vector<int64_t>, std::vector<int64_t>,
                                        std::vector<int64_t>, std::vector<int64_t>, std::vector<int64_t>>>& fields,
           int elem_size, uintptr_t out, uintptr_t flags, uintptr_t stream) {
          std::vector<ReduceField> fs;
          fs.reserve(fields.size());
          for (const auto& t : fields) {
            ReduceField f;
            f.a = std::get<0>(t), f.b = std::get<1>(t);
            f.shape = std::get<2>(t), f.stride_a = std::get<3>(t), f.stride_b = std::get<4>(t);
            f.lo = std::get<5>(t), f.hi = std::get<6>(t);
            fs.push_back(std::move(f));
          }
          reduce_fields(op, fs, elem_size, reinterpret_cast<double*>(out), reinterpret_cast<double*>(flags),
                        as_stream(stream));
        },
        py::arg("op"), py::arg("fields"), py::arg("elem_size"), py::arg("out"), py::arg("flags") = 0,
        py::arg("stream") = 0,
        "out[k] (f64, device) = op over the box of field k: fields are (a, b, shape, strides_a, strides_b, lo, hi), "
        "ops 0 sum, 1 sumsq, 2 max, 3 min, 4 maxabs, 5 dot, 6 sumsq_diff, 7 maxabs_diff. With `flags` the max-type "
        "ops write the travel form: value with NaN as -inf (min: of -x) and a NaN flag.");
  m.def("reduce_workspace_bytes", &reduce_workspace_bytes, "Bytes of the reductions' device workspaces.");
  m.def("reduce_free_workspace", &reduce_free_workspace,
        "Free the reductions' workspaces (one device synchronisation each); finalize_global_grid calls it.");

  // --- projections (ops/reduce.py project_g)
  m.attr("PROJECT_MAX_BLOCKS") = PROJECT_MAX_BLOCKS;
  m.attr("PROJECT_MAX_SLICES") = PROJECT_MAX_SLICES;
  m.def("project_plan",
        [](const std::vector<int64_t>& shape, const std::vector<int64_t>& strides, const std::vector<int64_t>& lo,
           const std::vector<int64_t>& hi, const std::vector<int>& keep, int elem_size, uintptr_t base_address,
           const std::vector<int64_t>& strides_b, uintptr_t base_b) {
          const ProjectPlan p = plan_project(shape, strides, lo, hi, keep, elem_size, base_address, strides_b, base_b);
          py::dict d;
          d["family"] = p.family;
          d["path"] = p.vector ? "vector" : "element";
          d["pattern"] = std::string(p.pattern);
          d["box"] = py::make_tuple(p.n[0], p.n[1], p.n[2], p.n[3]);
          d["strides"] = py::make_tuple(p.s[0], p.s[1], p.s[2], p.s[3]);
          d["offset"] = p.offset;
          d["total"] = p.total;
          d["outputs"] = p.nout;
          d["vec"] = p.vec;
          d["head"] = p.head;
          d["loads_per_row"] = p.nv;
          d["lanes"] = int64_t{1} << p.lanes_log2;
          d["chunks_per_row"] = p.cx;
          d["reduced"] = p.reduced;
          d["slices"] = p.slices;
          d["units"] = p.units;
          d["block_units"] = p.block_units;
          d["blocks"] = p.blocks;
          d["index_bits"] = p.index_bits;
          py::list ps;
          for (int k = 0; k < p.nkeep; ++k) ps.append(p.keep_pstride[k]);
          d["partial_strides"] = py::tuple(ps);
          return d;
        },
        py::arg("shape"), py::arg("strides"), py::arg("lo"), py::arg("hi"), py::arg("keep"), py::arg("elem_size"),
        py::arg("base_address"), py::arg("strides_b") = std::vector<int64_t>{}, py::arg("base_b") = 0,
        "What a projection does with the box [lo, hi) of one field that keeps the axes `keep`: family (1 inner axis "
        "kept, 2 inner axis reduced), path (vector / element), the merged pattern (outer .. inner, K kept, R "
        "reduced), the extents and strides of the family's slots ([KO, R0, R1, KI] or [K0, K1, RO, RI]), elements "
        "per load, head mask, lanes along a row, slices, units, blocks, the width of the loop offsets and the "
        "stride of each kept axis in an output's partial index.");
  m.def("project",
        [](int op, uintptr_t a, uintptr_t b, const std::vector<int64_t>& shape, const std::vector<int64_t>& strides_a,
           const std::vector<int64_t>& strides_b, const std::vector<int64_t>& lo, const std::vector<int64_t>& hi,
           const std::vector<int>& keep, int elem_size, uintptr_t dst, uintptr_t flags,
           const std::vector<int64_t>& dst_start, const std::vector<int64_t>& dst_extent,
           const std::vector<int64_t>& dst_stride, uintptr_t stream) {
          ReduceField f;
          f.a = a, f.b = b, f.shape = shape, f.stride_a = strides_a, f.stride_b = strides_b, f.lo = lo, f.hi = hi;
          ProjectDest d;
          d.dst = dst, d.flags = flags, d.start = dst_start, d.extent = dst_extent, d.stride = dst_stride;
          project_field(op, f, keep, elem_size, d, as_stream(stream));
        },
        py::arg("op"), py::arg("a"), py::arg("b"), py::arg("shape"), py::arg("strides_a"), py::arg("strides_b"),
        py::arg("lo"), py::arg("hi"), py::arg("keep"), py::arg("elem_size"), py::arg("dst"), py::arg("flags"),
        py::arg("dst_start"), py::arg("dst_extent"), py::arg("dst_stride"), py::arg("stream") = 0,
        "dst (f64, device) = op over the axes of the box [lo, hi) that `keep` does not name (ops as in reduce). The "
        "destination has dst_extent cells per kept axis at dst_stride (elements); the box's index i of a kept axis "
        "lands at (dst_start + i) mod dst_extent, every other cell takes the op's identity. With `flags` (same "
        "layout) the max-type ops write the travel form: value with NaN as -inf (min: of -x) and a NaN flag.");
  m.def("project_workspace_bytes", &project_workspace_bytes, "Bytes of the projections' device workspaces.");
  m.def("project_free_workspace", &project_free_workspace,
        "Free the projections' workspaces (one device synchronisation each); finalize_global_grid calls it.");

  // --- converting lattice copy (parallel/gather_g.py)
  m.attr("SELECT_MAX_BLOCKS") = SELECT_MAX_BLOCKS;
  m.attr("SELECT_MAX_JOBS") = SELECT_MAX_JOBS;
  m.def("select_plan",
        [](const std::array<int64_t, 3>& counts, const std::array<int64_t, 3>& src_strides,
           const std::array<int64_t, 3>& dst_strides) {
          const SelectPlan p = plan_select(counts.data(), src_strides.data(), dst_strides.data());
          py::dict d;
          d["path"] = select_path_name(p.path);
          d["index_bits"] = p.index_bits;
          d["total"] = p.total;
          d["rows"] = p.rows;
          d["src_span"] = p.src_span;
          d["dst_span"] = p.dst_span;
          d["blocks"] = p.blocks;
          return d;
        },
        py::arg("counts"), py::arg("src_strides"), py::arg("dst_strides"),
        "What select_convert does with one job (counts and strides in elements, outer .. inner): path (rows / "
        "element), index_bits (32 / 64), elements, rows, spans and blocks (0: empty, skipped).");
  m.def("select_convert",
        [](const std::vector<SelectTuple>& jobs, uintptr_t stream) { select_convert(select_descs(jobs), as_stream(stream)); },
        py::arg("jobs"), py::arg("stream") = 0,
        "dst[i0*T0 + i1*T1 + i2*T2] (f32, device) = float(src[i0*S0 + i1*S1 + i2*S2]) (f64, device), i_d < c_d, for "
        "every job (src, dst, counts, src strides, dst strides); strides in elements.");
  m.def("select_widen",
        [](const std::vector<SelectTuple>& jobs, uintptr_t stream) { select_widen(select_descs(jobs), as_stream(stream)); },
        py::arg("jobs"), py::arg("stream") = 0,
        "dst[i0*T0 + i1*T1 + i2*T2] (f64, device) = double(src[i0*S0 + i1*S1 + i2*S2]) (f32, device), i_d < c_d, for "
        "every job (src, dst, counts, src strides, dst strides); strides in elements. The plan is select_plan's.");

  // --- point sampling (parallel/sample_g.py)
  m.attr("SAMPLE_BLOCK") = SAMPLE_BLOCK;
  m.attr("SAMPLE_POINTS") = SAMPLE_POINTS;
  m.attr("SAMPLE_MAX_BLOCKS") = SAMPLE_MAX_BLOCKS;
  m.attr("SAMPLE_MAX_FIELDS") = SAMPLE_MAX_FIELDS;
  m.def("sample",
        [](const std::vector<SampleDimTuple>& dims, const std::vector<SampleFieldTuple>& fields, int elem_size,
           uintptr_t points, int64_t ps0, int64_t ps1, int64_t npts, uintptr_t out, int64_t out_fs, bool me0,
           uintptr_t row, int64_t nrows, int64_t row_stride, uintptr_t stream, int max_blocks) {
          sample_calls("sample", dims, fields, points, ps0, ps1, npts, out, out_fs, me0, row, nrows, row_stride,
                       [&](const SampleArgs& a) { sample(a, elem_size, max_blocks, as_stream(stream)); });
        },
        py::arg("dims"), py::arg("fields"), py::arg("elem_size"), py::arg("points"), py::arg("ps0"), py::arg("ps1"),
        py::arg("npts"), py::arg("out"), py::arg("out_fs"), py::arg("me0"), py::arg("row") = 0, py::arg("nrows") = 0,
        py::arg("row_stride") = 0, py::arg("stream") = 0, py::arg("max_blocks") = 0,
        "out[f*out_fs + p] (f64 bits, device) = field f (f32 / f64, device; (pointer, strides in elements)) "
        "interpolated multilinearly at point p, whose coordinate of axis d is the double at points[p*ps0 + d*ps1], in "
        "the field's global index space. dims: per axis (E, periodic, m, [(g0, g1, i0), ...]) - the global extent, "
        "the local size and this rank's owned segments. A point whose cell this rank does not own gives 0 bits, an "
        "invalid point the canonical quiet NaN if me0 and 0 otherwise. With `row` (a device int64) the output moves "
        "by *row * row_stride elements and nothing is written if *row >= nrows. One launch per SAMPLE_MAX_FIELDS "
        "fields; max_blocks caps the grid (0: SAMPLE_MAX_BLOCKS).");
  m.def("host_sample",
        [](const std::vector<SampleDimTuple>& dims, const std::vector<SampleFieldTuple>& fields, int elem_size,
           uintptr_t points, int64_t ps0, int64_t ps1, int64_t npts, uintptr_t out, int64_t out_fs, bool me0,
           uintptr_t row, int64_t nrows, int64_t row_stride) {
          sample_calls("host_sample", dims, fields, points, ps0, ps1, npts, out, out_fs, me0, row, nrows, row_stride,
                       [&](const SampleArgs& a) { host_sample(a, elem_size); });
        },
        py::arg("dims"), py::arg("fields"), py::arg("elem_size"), py::arg("points"), py::arg("ps0"), py::arg("ps1"),
        py::arg("npts"), py::arg("out"), py::arg("out_fs"), py::arg("me0"), py::arg("row") = 0, py::arg("nrows") = 0,
        py::arg("row_stride") = 0,
        "`sample` on host memory with the same expressions: the CPU path and the GPU tests' reference.");

  // --- point spreading (parallel/spread_g.py)
  m.attr("SPREAD_BLOCK") = SPREAD_BLOCK;
  m.attr("SPREAD_MAX_BLOCKS") = SPREAD_MAX_BLOCKS;
  m.attr("SPREAD_MAX_FIELDS") = SPREAD_MAX_FIELDS;
  m.attr("SPREAD_MAX_RUNS") = SPREAD_MAX_RUNS;
  m.def("spread_count",
        [](const std::vector<SpreadDimTuple>& dims, int copies, uintptr_t points, int64_t ps0, int64_t ps1,
           int64_t npts, uintptr_t count, uintptr_t stream, int max_blocks) {
          SpreadPlanArgs a = spread_plan_args("spread_count", dims, copies, points, ps0, ps1, npts);
          a.count = reinterpret_cast<int64_t*>(count);
          spread_count(a, max_blocks, as_stream(stream));
        },
        py::arg("dims"), py::arg("copies"), py::arg("points"), py::arg("ps0"), py::arg("ps1"), py::arg("npts"),
        py::arg("count"), py::arg("stream") = 0, py::arg("max_blocks") = 0,
        "count[p] (int64, device) = the number of local cells that point p reaches. dims: per axis (E, periodic, m, "
        "[(g0, g1, i0), ...] owned segments, [(i0, len, g0), ...] runs of the local range); copies: 0 every local "
        "cell whose global index is a corner's (the runs), 1 the owner's two cells (the segments). An invalid point "
        "and a corner with a zero factor reach nothing. max_blocks caps the grid (0: SPREAD_MAX_BLOCKS).");
  m.def("spread_fill",
        [](const std::vector<SpreadDimTuple>& dims, int copies, uintptr_t points, int64_t ps0, int64_t ps1,
           int64_t npts, uintptr_t cum, int64_t nentries, uintptr_t key, uintptr_t point, uintptr_t weight,
           uintptr_t stream, int max_blocks) {
          SpreadPlanArgs a = spread_plan_args("spread_fill", dims, copies, points, ps0, ps1, npts);
          a.cum = reinterpret_cast<const int64_t*>(cum), a.nentries = nentries;
          a.key = reinterpret_cast<int64_t*>(key), a.point = reinterpret_cast<int64_t*>(point);
          a.weight = reinterpret_cast<double*>(weight);
          spread_fill(a, max_blocks, as_stream(stream));
        },
        py::arg("dims"), py::arg("copies"), py::arg("points"), py::arg("ps0"), py::arg("ps1"), py::arg("npts"),
        py::arg("cum"), py::arg("nentries"), py::arg("key"), py::arg("point"), py::arg("weight"),
        py::arg("stream") = 0, py::arg("max_blocks") = 0,
        "The entries of every point, from cum[p - 1] on (cum: the inclusive running sum of spread_count's counts, "
        "nentries its last value; nothing is written at or beyond nentries): key (the target cell's linear C-order "
        "index in the field's shape), point and weight ((fx*fy)*fz in float64), the x corners outermost.");
  m.def("host_spread_plan",
        [](const std::vector<SpreadDimTuple>& dims, int copies, uintptr_t points, int64_t ps0, int64_t ps1,
           int64_t npts) {
          const SpreadPlan p =
              host_spread_plan(spread_plan_args("host_spread_plan", dims, copies, points, ps0, ps1, npts));
          auto raw = [](const void* d, size_t n) { return py::bytes(static_cast<const char*>(d), n); };
          return py::make_tuple(raw(p.cells.data(), p.cells.size() * 8), raw(p.start.data(), p.start.size() * 8),
                                raw(p.point.data(), p.point.size() * 8), raw(p.weight.data(), p.weight.size() * 8));
        },
        py::arg("dims"), py::arg("copies"), py::arg("points"), py::arg("ps0"), py::arg("ps1"), py::arg("npts"),
        "The finished plan from host points, with the kernels' expressions and std::stable_sort: (cells, start, "
        "point, weight) as the bytes of int64, int64, int64 and float64 arrays - the touched cells ascending, "
        "ncells + 1 segment starts, and the entries sorted by (cell, point).");
  m.def("spread_apply",
        [](const std::vector<int64_t>& shape, const std::vector<SampleFieldTuple>& fields, int elem_size,
           int64_t ncells, uintptr_t cells, uintptr_t start, uintptr_t point, uintptr_t weight, uintptr_t values,
           int64_t v_fs, int64_t v_ps, uintptr_t row, int64_t nrows, int64_t row_stride, uintptr_t stream,
           int max_blocks) {
          spread_calls("spread_apply", shape, fields, ncells, cells, start, point, weight, values, v_fs, v_ps, row,
                       nrows, row_stride,
                       [&](const SpreadArgs& a) { spread_apply(a, elem_size, max_blocks, as_stream(stream)); });
        },
        py::arg("shape"), py::arg("fields"), py::arg("elem_size"), py::arg("ncells"), py::arg("cells"),
        py::arg("start"), py::arg("point"), py::arg("weight"), py::arg("values"), py::arg("v_fs"), py::arg("v_ps"),
        py::arg("row") = 0, py::arg("nrows") = 0, py::arg("row_stride") = 0, py::arg("stream") = 0,
        py::arg("max_blocks") = 0,
        "For every touched cell i of the plan and every field f (f32 / f64, device; (pointer, strides in elements)): "
        "s = the fold in entry order, in float64, of weight[e] * values[f*v_fs + point[e]*v_ps] over e in [start[i], "
        "start[i+1]); field[cells[i]] = T(double(field[cells[i]]) + s), cells[i] being the linear C-order index in "
        "`shape`. With `row` (a device int64) the values move by *row * row_stride and nothing is done if *row >= "
        "nrows. One launch per SPREAD_MAX_FIELDS fields, one lane per cell; max_blocks caps the grid.");
  m.def("host_spread_apply",
        [](const std::vector<int64_t>& shape, const std::vector<SampleFieldTuple>& fields, int elem_size,
           int64_t ncells, uintptr_t cells, uintptr_t start, uintptr_t point, uintptr_t weight, uintptr_t values,
           int64_t v_fs, int64_t v_ps, uintptr_t row, int64_t nrows, int64_t row_stride) {
          spread_calls("host_spread_apply", shape, fields, ncells, cells, start, point, weight, values, v_fs, v_ps,
                       row, nrows, row_stride, [&](const SpreadArgs& a) { host_spread_apply(a, elem_size); });
        },
        py::arg("shape"), py::arg("fields"), py::arg("elem_size"), py::arg("ncells"), py::arg("cells"),
        py::arg("start"), py::arg("point"), py::arg("weight"), py::arg("values"), py::arg("v_fs"), py::arg("v_ps"),
        py::arg("row") = 0, py::arg("nrows") = 0, py::arg("row_stride") = 0,
        "`spread_apply` on host memory with the same expressions: the CPU path and the GPU tests' reference.");

  // --- transports
  py::class_<Transport, std::shared_ptr<Transport>>(m, "Transport")
      .def_property_readonly("name", &Transport::name)
      .def_property_readonly("device_capable", &Transport::device_capable)
      .def_property_readonly("host_capable", &Transport::host_capable)
      .def("exchange",
           [](Transport& t, const std::vector<std::tuple<uintptr_t, size_t, int, int>>& recvs,
              const std::vector<std::tuple<uintptr_t, size_t, int, int>>& sends, bool device, uintptr_t s) {
             auto conv = [](const std::vector<std::tuple<uintptr_t, size_t, int, int>>& ops) {
               std::vector<P2POp> v;
               v.reserve(ops.size());
               for (const auto& x : ops)
                 v.push_back({reinterpret_cast<void*>(std::get<0>(x)), std::get<1>(x), std::get<2>(x), std::get<3>(x)});
               return v;
             };
             t.exchange(conv(recvs), conv(sends), device, as_stream(s));
           },
           py::arg("recvs"), py::arg("sends"), py::arg("device"), py::arg("stream") = 0,
           "One point-to-point phase: every receive, then every send, as (pointer, bytes, peer, tag); messages may "
           "have any, unequal sizes. Device memory is ordered on `stream`.");
  py::class_<PyTransport, Transport, std::shared_ptr<PyTransport>>(m, "PyTransport")
      .def(py::init<py::function, bool, bool, std::string>(), py::arg("fn"), py::arg("host"),
           py::arg("device"), py::arg("name"));
  py::class_<PeerMesh, std::shared_ptr<PeerMesh>>(m, "PeerMesh")
      .def(py::init([](int rank, int nranks, py::function allgather) {
             // Called from C++ (GIL held: exchanges run with the GIL).
             PeerMesh::AllGather ag = [allgather](const std::string& mine) {
               py::gil_scoped_acquire gil;
               py::list out = allgather(py::bytes(mine));
               std::vector<std::string> v;
               for (auto h : out) v.push_back(h.cast<std::string>());
               return v;
             };
             return std::make_shared<PeerMesh>(rank, nranks, ag);
           }),
           py::arg("rank"), py::arg("nranks"), py::arg("allgather"))
      .def_property_readonly("rank", &PeerMesh::rank)
      .def_property_readonly("nranks", &PeerMesh::nranks)
      .def_property_readonly("arena_bytes", &PeerMesh::arena_bytes)
      .def_property_readonly("epoch", [](const PeerMesh& m) { return m.read_flag(PutFlags::EPOCH); })
      .def_property_readonly("flag_words", &PeerMesh::flag_words)
      .def("flag", &PeerMesh::read_flag)
      .def("check_error", &PeerMesh::check_error)
      .def("clear_error", &PeerMesh::clear_error)
      .def("close", &PeerMesh::close);
  // --- HIP virtual memory management (allocations >= 2 GiB across processes)
  m.def("vmm_granularity", &vmm_granularity, py::arg("device"));
  m.def("vmm_alloc",
        [](size_t bytes) {
          size_t mapped = 0;
          void* p = vmm_alloc(bytes, &mapped);
          return py::make_tuple(reinterpret_cast<uintptr_t>(p), mapped);
        },
        py::arg("bytes"), "(pointer, mapped bytes) of new hipMemCreate memory on the current device");
  m.def("vmm_export_fd", [](uintptr_t p) { return vmm_export_fd(reinterpret_cast<void*>(p)); }, py::arg("ptr"));
  m.def("vmm_import_fd",
        [](int fd, size_t size, double seconds) {
          py::gil_scoped_release nogil;
          return reinterpret_cast<uintptr_t>(vmm_import_fd(fd, size, seconds));
        },
        py::arg("fd"), py::arg("size"), py::arg("seconds"));
  m.def("vmm_free", [](uintptr_t p) { vmm_free(reinterpret_cast<void*>(p)); }, py::arg("ptr"));
  m.def(
      "range_export_fd",
      [](uintptr_t p) {
        void* base = nullptr;
        size_t size = 0;
        const int fd = range_export_fd(reinterpret_cast<void*>(p), &base, &size);
        return py::make_tuple(fd, reinterpret_cast<uintptr_t>(base), size);
      },
      py::arg("ptr"), "(fd, base, size): dma-buf descriptor of the hipMalloc allocation holding ptr");
  m.def("fd_listen", &fd_listen, py::arg("name"));
  m.def("fd_serve",
        [](int listener, int fd, int clients, double seconds) {
          py::gil_scoped_release nogil;
          fd_serve(listener, fd, clients, seconds);
        },
        py::arg("listener"), py::arg("fd"), py::arg("clients"), py::arg("seconds"));
  m.def("fd_fetch",
        [](const std::string& name, double seconds) {
          py::gil_scoped_release nogil;
          return fd_fetch(name, seconds);
        },
        py::arg("name"), py::arg("seconds"));
  m.def("fd_close", &fd_close, py::arg("fd"));
  py::class_<CoherenceProbe, std::shared_ptr<CoherenceProbe>>(m, "CoherenceProbe")
      .def(py::init<std::shared_ptr<PeerMesh>, size_t>(), py::arg("mesh"), py::arg("bytes"),
           "Collective over a 2-rank mesh (reader 0, writer 1): arenas of `bytes` (igg/coherence.hpp).")
      .def("warm", [](CoherenceProbe& p, uintptr_t s) { p.warm(as_stream(s)); }, py::arg("stream"))
      .def("write",
           [](CoherenceProbe& p, uint64_t v, bool in_kernel, uintptr_t s, bool plain) {
             p.write(v, in_kernel, as_stream(s), plain);
           },
           py::arg("value"), py::arg("in_kernel"), py::arg("stream"), py::arg("plain") = false)
      .def("check",
           [](CoherenceProbe& p, uint64_t v, bool in_kernel, uintptr_t s) {
             py::gil_scoped_release nogil;
             return p.check(v, in_kernel, as_stream(s));
           },
           py::arg("value"), py::arg("in_kernel"), py::arg("stream"))
      .def("control",
           [](CoherenceProbe& p, uint64_t v, uint64_t target, bool l2, uintptr_t s) {
             p.control(v, target, l2, as_stream(s));
           },
           py::arg("value"), py::arg("target"), py::arg("l2"), py::arg("stream"))
      .def("mismatches",
           [](CoherenceProbe& p, uintptr_t s) {
             py::gil_scoped_release nogil;
             return p.mismatches(as_stream(s));
           },
           py::arg("stream"))
      .def_property_readonly("workgroups", &CoherenceProbe::workgroups)
      .def_property_readonly("words", &CoherenceProbe::words);
  py::class_<PutTransport, Transport, std::shared_ptr<PutTransport>>(m, "PutTransport")
      .def(py::init<std::shared_ptr<PeerMesh>>(), py::arg("mesh"))
      .def_property_readonly("mesh", &PutTransport::mesh_ptr);
  py::class_<RcclComm, Transport, std::shared_ptr<RcclComm>>(m, "RcclComm")
      .def_static("unique_id", []() {
        auto v = RcclComm::unique_id();
        return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
      })
      .def(py::init([](py::bytes uid, int nranks, int rank, double timeout) {
             std::string s = uid;
             std::vector<uint8_t> v(s.begin(), s.end());
             py::gil_scoped_release nogil;  // bounded rendezvous (polled)
             return std::make_shared<RcclComm>(v, nranks, rank, timeout);
           }),
           py::arg("uid"), py::arg("nranks"), py::arg("rank"), py::arg("timeout") = 0.0,
           "Bounded RCCL bootstrap (non-blocking communicator polled for `timeout` s; <= 0: "
           "IGG_FIRST_CONTACT_TIMEOUT, default 120); aborts and raises on expiry.")
      .def("barrier", [](RcclComm& c, uintptr_t s) { c.barrier(as_stream(s)); })
      .def("allreduce",
           [](RcclComm& c, uintptr_t send, uintptr_t recv, size_t count, int dtype, int op, uintptr_t s) {
             c.allreduce(reinterpret_cast<const void*>(send), reinterpret_cast<void*>(recv), count, dtype, op,
                         as_stream(s));
           },
           py::arg("send"), py::arg("recv"), py::arg("count"), py::arg("dtype"), py::arg("op"), py::arg("stream"))
      .def("broadcast",
           [](RcclComm& c, uintptr_t send, uintptr_t recv, size_t count, int dtype, int root, uintptr_t s) {
             c.broadcast(reinterpret_cast<const void*>(send), reinterpret_cast<void*>(recv), count, dtype, root,
                         as_stream(s));
           },
           py::arg("send"), py::arg("recv"), py::arg("count"), py::arg("dtype"), py::arg("root"), py::arg("stream"))
      .def("check_async_error", &RcclComm::check_async_error)
      .def("abort", &RcclComm::abort)
      .def_property_readonly("rank", &RcclComm::rank)
      .def_property_readonly("nranks", &RcclComm::nranks)
      .def("p2p",
           [](RcclComm& c, const std::vector<std::tuple<uintptr_t, size_t, int>>& recvs,
              const std::vector<std::tuple<uintptr_t, size_t, int>>& sends, uintptr_t s) {
             std::vector<P2POp> r, sd;
             for (const auto& x : recvs)
               r.push_back({reinterpret_cast<void*>(std::get<0>(x)), std::get<1>(x), std::get<2>(x), 0});
             for (const auto& x : sends)
               sd.push_back({reinterpret_cast<void*>(std::get<0>(x)), std::get<1>(x), std::get<2>(x), 0});
             c.exchange(r, sd, true, as_stream(s));
           });

  // --- halo engine
  py::class_<FieldSet>(m, "FieldSet")
      .def(py::init([](const std::vector<FieldTuple>& ts) { return FieldSet{to_fields(ts)}; }))
      .def("__len__", [](const FieldSet& s) { return s.f.size(); });
  py::class_<HaloEngine>(m, "HaloEngine")
      .def(py::init<const GridInfo&>())
      .def_property_readonly("grid", [](HaloEngine& e) { return e.grid(); })
      .def("set_grid", &HaloEngine::set_grid)
      .def("set_transport", &HaloEngine::set_transport, py::arg("transport"), py::arg("device"))
      .def("clear_transport", [](HaloEngine& e, bool device) { e.set_transport(nullptr, device); })
      .def("transport_name", [](HaloEngine& e, bool device) {
        auto t = e.transport(device);
        return t ? t->name() : std::string("none");
      })
      .def("exchange",
           [](HaloEngine& e, const std::vector<FieldTuple>& fs, uintptr_t s) {
             e.exchange(to_fields(fs), as_stream(s));
           })
      .def("set_mode", [](HaloEngine& e, int m) { e.set_mode(static_cast<HaloMode>(m)); })
      .def_property_readonly("mode", [](HaloEngine& e) { return static_cast<int>(e.mode()); })
      .def("set_pack_mode",
           [](HaloEngine& e, int dim, int m) {
             if (dim < 0 || dim >= NDIMS || m < 0 || m > 1) throw std::invalid_argument("set_pack_mode: bad dim/mode");
             e.set_pack_mode(dim, static_cast<PackMode>(m));
           })
      .def("pack_mode", [](HaloEngine& e, int dim) { return static_cast<int>(e.pack_mode(dim)); })
      .def("resolved_mode", [](HaloEngine& e, const FieldSet& fs) {
        return static_cast<int>(e.resolved_mode(fs.f));
      })
      .def_property_readonly("last_message_count", &HaloEngine::last_message_count)
      .def("exchange_set",
           [](HaloEngine& e, const FieldSet& fs, uintptr_t s, int mode) { e.exchange(fs.f, as_stream(s), mode); },
           py::arg("fields"), py::arg("stream"), py::arg("mode") = -1)
      .def("accumulate_set",
           [](HaloEngine& e, const FieldSet& fs, const std::string& dtype, uintptr_t s,
              std::shared_ptr<Transport> dev_transport) {
             e.accumulate(fs.f, accum_type(dtype), as_stream(s), dev_transport);
           },
           py::arg("fields"), py::arg("dtype"), py::arg("stream"), py::arg("dev_transport") = nullptr)
      .def("exchange_dim",
           [](HaloEngine& e, const std::vector<FieldTuple>& fs, int dim, uintptr_t s) {
             e.exchange_dim(to_fields(fs), dim, as_stream(s));
           })
      .def("pool_ensure",
           [](HaloEngine& e, const std::vector<FieldTuple>& fs, bool device) {
             e.pool().ensure(to_fields(fs), device);
           })
      .def("pool_free", [](HaloEngine& e) { e.pool().free_all(); })
      .def("pool_allocated", [](HaloEngine& e, bool device) { return e.pool().allocated(device); })
      .def("pool_nslots", [](HaloEngine& e, bool device) { return e.pool().nslots(device); })
      .def("pool_capacity",
           [](HaloEngine& e, size_t slot, bool device) { return e.pool().capacity(slot, device); })
      .def("pool_ptrs", [](HaloEngine& e, size_t slot, bool device) {
        auto& p = e.pool();
        return py::make_tuple(reinterpret_cast<uintptr_t>(p.send(slot, 0, device)),
                              reinterpret_cast<uintptr_t>(p.send(slot, 1, device)),
                              reinterpret_cast<uintptr_t>(p.recv(slot, 0, device)),
                              reinterpret_cast<uintptr_t>(p.recv(slot, 1, device)));
      });

  // --- gather
  py::class_<Gatherer>(m, "Gatherer")
      .def(py::init<>())
      .def("gather",
           [](Gatherer& g, const FieldTuple& a, uintptr_t dst, int root, const Int3& dims,
              RcclComm& comm, uintptr_t s) {
             g.gather(to_field(a), reinterpret_cast<void*>(dst), root, dims, comm, as_stream(s));
           })
      .def("free", &Gatherer::free)
      .def_property_readonly("capacity", &Gatherer::capacity);
  py::class_<PullGatherer>(m, "PullGatherer")
      .def(py::init([](int rank, int nranks, py::function allgather) {
             PullGatherer::AllGather ag = [allgather](const std::string& mine) {
               py::gil_scoped_acquire gil;
               py::list out = allgather(py::bytes(mine));
               std::vector<std::string> v;
               for (auto h : out) v.push_back(h.cast<std::string>());
               return v;
             };
             return std::make_unique<PullGatherer>(rank, nranks, ag);
           }),
           py::arg("rank"), py::arg("nranks"), py::arg("allgather"))
      .def("start", [](PullGatherer& g, const FieldTuple& a, uintptr_t dst, int root, const Int3& dims,
                       uintptr_t s, bool snapshot) {
             g.start(to_field(a), reinterpret_cast<void*>(dst), root, dims, as_stream(s), snapshot);
           },
           py::arg("a"), py::arg("dst"), py::arg("root"), py::arg("dims"), py::arg("stream"),
           py::arg("snapshot") = false)
      .def("wait", [](PullGatherer& g, uintptr_t s) { g.wait(as_stream(s)); }, py::arg("stream"))
      .def_property_readonly("pending", &PullGatherer::pending)
      .def_property_readonly("last_kind", [](const PullGatherer& g) { return std::string(g.last_kind()); })
      .def("free", &PullGatherer::free);
  m.def("gather_reorder", [](uintptr_t src, uintptr_t dst, const Int3& s, const Int3& dims,
                             int eb, uintptr_t stream) {
    launch_gather_reorder(reinterpret_cast<const void*>(src), reinterpret_cast<void*>(dst), s, dims,
                          eb, as_stream(stream));
  });

  // --- stencils
  m.def("diffusion3d_variants", []() {
    std::vector<std::string> v;
    for (int i = 0; i < diffusion3d_num_variants(); ++i) v.push_back(diffusion3d_variant_name(i));
    return v;
  });
  m.def("diffusion3d_variant_tile", &diffusion3d_variant_tile);
  m.def("zcol_probe",
        [](int dir, uintptr_t src, uintptr_t dst, int64_t rows, int64_t pitch, int aux, uintptr_t stream) {
          launch_zcol_probe(dir, reinterpret_cast<const void*>(src), reinterpret_cast<void*>(dst), rows, pitch, aux,
                            as_stream(stream));
        },
        py::arg("dir"), py::arg("src"), py::arg("dst"), py::arg("rows"), py::arg("pitch"), py::arg("aux"),
        py::arg("stream") = 0,
        "z-face column probe: dir 0 pack (strided reads), 1 unpack (strided writes), 8-B elements; aux = cache "
        "policy bits of the strided access (1 sc0, 2 nt, 16 sc1).");
  m.def("stream_probe", [](int kind, uintptr_t out, uintptr_t a, uintptr_t b, int64_t n, int blocks,
                           uintptr_t stream) {
    launch_stream_probe(kind, reinterpret_cast<double*>(out), reinterpret_cast<const double*>(a),
                        reinterpret_cast<const double*>(b), n, blocks, as_stream(stream));
  });
  m.def("acoustic2d",
        [](uintptr_t p2, uintptr_t vx2, uintptr_t vy2, uintptr_t p, uintptr_t vx, uintptr_t vy, int64_t nx,
           int64_t ny, double dtk, double dt_rho, double rdx, double rdy, int elem_bytes, bool device,
           uintptr_t stream) {
          TraceRange tr("igg.acoustic2d");
          AcousticArgs a{p2, vx2, vy2, p, vx, vy, nx, ny, dtk, dt_rho, rdx, rdy, elem_bytes};
          if (device) {
            launch_acoustic2d(a, as_stream(stream));
          } else {
            py::gil_scoped_release nogil;
            host_acoustic2d(a);
          }
        },
        py::arg("p2"), py::arg("vx2"), py::arg("vy2"), py::arg("p"), py::arg("vx"), py::arg("vy"), py::arg("nx"),
        py::arg("ny"), py::arg("dtk"), py::arg("dt_rho"), py::arg("rdx"), py::arg("rdy"), py::arg("elem_bytes"),
        py::arg("device"), py::arg("stream") = 0);
  py::class_<FusedAcoustic, std::shared_ptr<FusedAcoustic>>(m, "FusedAcoustic")
      .def(py::init([](std::shared_ptr<PeerMesh> mesh, int64_t nx, int64_t ny, int elem_bytes,
                       const std::array<std::array<int, 2>, 2>& nb) {
             return std::make_shared<FusedAcoustic>(mesh, nx, ny, elem_bytes, nb);
           }),
           py::arg("mesh"), py::arg("nx"), py::arg("ny"), py::arg("elem_bytes"), py::arg("neighbors"))
      .def("set_fields", &FusedAcoustic::set_fields, py::arg("vx_a"), py::arg("vx_b"), py::arg("vy_a"),
           py::arg("vy_b"))
      .def("step",
           [](FusedAcoustic& f, uintptr_t p2, uintptr_t vx2, uintptr_t vy2, uintptr_t p, uintptr_t vx, uintptr_t vy,
              int64_t nx, int64_t ny, double dtk, double dt_rho, double rdx, double rdy, int elem_bytes,
              uintptr_t stream, bool entry) {
             TraceRange tr("igg.acoustic2d_fused");
             AcousticArgs a{p2, vx2, vy2, p, vx, vy, nx, ny, dtk, dt_rho, rdx, rdy, elem_bytes};
             f.step(a, as_stream(stream), entry);
           },
           py::arg("p2"), py::arg("vx2"), py::arg("vy2"), py::arg("p"), py::arg("vx"), py::arg("vy"), py::arg("nx"),
           py::arg("ny"), py::arg("dtk"), py::arg("dt_rho"), py::arg("rdx"), py::arg("rdy"), py::arg("elem_bytes"),
           py::arg("stream"), py::arg("entry") = false)
      .def("drain", [](FusedAcoustic& f, uintptr_t s) { f.drain(as_stream(s)); }, py::arg("stream"),
           "Exit barrier after in-kernel synchronised steps (collective; no-op after a sync-kernel step).")
      .def("check_error", &FusedAcoustic::check_error)
      .def("clear_error", &FusedAcoustic::clear_error,
           "Reset this rank's sticky timeout word (after a failed exchange was handled).")
      .def("set_step_sync", &FusedAcoustic::set_step_sync, py::arg("mode"),
           "Step synchronisation: -1 default, 0 inside the fused kernel, 1 sync kernel (same on every rank).")
      .def_property_readonly("in_kernel_sync", &FusedAcoustic::in_kernel_sync)
      .def("flag", [](FusedAcoustic& f, int i) { return f.flag(i); }, py::arg("index"),
           "Word `index` of this rank's flag block (PutFlags: 0 EPOCH = completed steps, 2 COUNT).")
      .def("close", &FusedAcoustic::close);
  // Two acoustic time steps in one pass (acoustic2_kernels.hip): GPU only.
  m.def("acoustic2d_twostep",
        [](uintptr_t p2, uintptr_t vx2, uintptr_t vy2, uintptr_t p, uintptr_t vx, uintptr_t vy, int64_t nx,
           int64_t ny, double dtk, double dt_rho, double rdx, double rdy, int elem_bytes, int64_t chunk,
           uintptr_t stream) {
          TraceRange tr("igg.acoustic2d_twostep");
          AcousticArgs a{p2, vx2, vy2, p, vx, vy, nx, ny, dtk, dt_rho, rdx, rdy, elem_bytes};
          launch_acoustic2d_twostep(a, chunk, as_stream(stream));
        },
        py::arg("p2"), py::arg("vx2"), py::arg("vy2"), py::arg("p"), py::arg("vx"), py::arg("vy"), py::arg("nx"),
        py::arg("ny"), py::arg("dtk"), py::arg("dt_rho"), py::arg("rdx"), py::arg("rdy"), py::arg("elem_bytes"),
        py::arg("chunk") = 0, py::arg("stream") = 0);
  m.def("acoustic2d_twostep_ok",
        [](int64_t nx, int64_t ny, int elem_bytes) {
          AcousticArgs a{0, 0, 0, 0, 0, 0, nx, ny, 0.0, 0.0, 1.0, 1.0, elem_bytes};
          return acoustic2d_twostep_ok(a);
        },
        py::arg("nx"), py::arg("ny"), py::arg("elem_bytes"));
  m.def("acoustic2d_set_variant", &acoustic2d_set_variant);
  m.def("acoustic2d_set_chunk", &acoustic2d_set_chunk);
  // Transpose of the step (acoustic_adj_kernels.hip / acoustic_adj_host.cpp):
  // (gP2, gVx2, gVy2) -> (gP, gVx, gVy).
  m.def("acoustic2d_adjoint",
        [](uintptr_t gp, uintptr_t gvx, uintptr_t gvy, uintptr_t gp2, uintptr_t gvx2, uintptr_t gvy2, int64_t nx,
           int64_t ny, double dtk, double dt_rho, double rdx, double rdy, int elem_bytes, bool device,
           uintptr_t stream, int64_t chunk) {
          TraceRange tr("igg.acoustic2d_adjoint");
          AcousticAdjointArgs a{gp, gvx, gvy, gp2, gvx2, gvy2, nx, ny, dtk, dt_rho, rdx, rdy, elem_bytes, chunk};
          if (device) {
            launch_acoustic2d_adjoint(a, as_stream(stream));
          } else {
            check_acoustic2d_adjoint(a);
            py::gil_scoped_release nogil;
            host_acoustic2d_adjoint(a);
          }
        },
        py::arg("gp"), py::arg("gvx"), py::arg("gvy"), py::arg("gp2"), py::arg("gvx2"), py::arg("gvy2"),
        py::arg("nx"), py::arg("ny"), py::arg("dtk"), py::arg("dt_rho"), py::arg("rdx"), py::arg("rdy"),
        py::arg("elem_bytes"), py::arg("device"), py::arg("stream") = 0, py::arg("chunk") = 0);
  m.def("acoustic2d_adjoint_set_chunk", &acoustic2d_adjoint_set_chunk, py::arg("rows"),
        "Rows of x per wave of the adjoint acoustic kernel where a call passes chunk = 0 (0: the built-in default).");
  m.def("acoustic2d_adjoint_chunk", &acoustic2d_adjoint_chunk,
        "Rows of x per wave that a call with chunk = 0 gets.");
  m.def("diffusion3d_set_rounds", &diffusion3d_set_rounds);
  m.def("diffusion3d_get_rounds", &diffusion3d_get_rounds);
  m.def("diffusion3d",
        [](uintptr_t t2, uintptr_t t, uintptr_t cp, const Int3& n, const std::array<double, 3>& rd2,
           double dtlam, int elem_bytes, const std::vector<std::pair<Int3, Int3>>& boxes,
           bool device, int variant, uintptr_t stream, int rounds, bool halo_z) {
          TraceRange tr("igg.diffusion3d");
          DiffusionArgs a{t2, t, cp, {n[0], n[1], n[2]}, {rd2[0], rd2[1], rd2[2]}, dtlam, elem_bytes, rounds, halo_z};
          const auto bx = to_boxes(boxes);
          if (device) {
            launch_diffusion3d(a, bx, variant, as_stream(stream));
          } else {
            py::gil_scoped_release nogil;
            host_diffusion3d(a, bx);
          }
        },
        py::arg("t2"), py::arg("t"), py::arg("cp"), py::arg("n"), py::arg("rd2"), py::arg("dtlam"),
        py::arg("elem_bytes"), py::arg("boxes"), py::arg("device"), py::arg("variant") = 0,
        py::arg("stream") = 0, py::arg("rounds") = 0, py::arg("halo_z") = false);
  // Transpose of the step (stencil_adj_kernels.hip / stencil_adj_host.cpp): gT = S^T g
  // where gt != 0, the derivative with respect to Cp where gcp != 0.
  m.def("diffusion3d_adjoint",
        [](uintptr_t gt, uintptr_t gcp, uintptr_t g, uintptr_t cp, uintptr_t q, uintptr_t t, const Int3& n,
           const std::array<double, 3>& rd2, double dtlam, int elem_bytes, bool accumulate, bool device,
           uintptr_t stream, int chunk) {
          TraceRange tr("igg.diffusion3d_adjoint");
          DiffusionAdjointArgs a;
          a.gt = gt, a.gcp = gcp, a.g = g, a.cp = cp, a.q = q, a.t = t;
          for (int d = 0; d < 3; ++d) a.n[d] = n[d], a.rd2[d] = rd2[d];
          a.dt_lam = dtlam, a.elem_bytes = elem_bytes, a.accumulate = accumulate, a.chunk = chunk;
          if (device) {
            launch_diffusion3d_adjoint(a, as_stream(stream));
          } else {
            py::gil_scoped_release nogil;
            host_diffusion3d_adjoint(a);
          }
        },
        py::arg("gt"), py::arg("gcp"), py::arg("g"), py::arg("cp"), py::arg("q"), py::arg("t"), py::arg("n"),
        py::arg("rd2"), py::arg("dtlam"), py::arg("elem_bytes"), py::arg("accumulate"), py::arg("device"),
        py::arg("stream") = 0, py::arg("chunk") = 0);
  // (points per lane, rows per workgroup tile) of the adjoint kernels for rows of n2 points
  m.def("diffusion3d_adjoint_tile",
        [](int64_t n2, int elem_bytes) {
          if (elem_bytes != 4 && elem_bytes != 8) fail("diffusion3d_adjoint_tile: element size 4 or 8");
          const AdjointTile t = diffusion3d_adjoint_tile(n2, elem_bytes);
          return std::make_pair(t.vz, t.rows);
        },
        py::arg("n2"), py::arg("elem_bytes"));
  // Inner-box sweep through one restrict-form tiling id (igg/variants.hpp
  // IGG_RESTRICT_TILINGS*); the measurement-only tilings (incl. the timing probes
  // 130-132 of profiles/r2_refetch/refetch_probe.py) exist only in a --probes build.
  m.def("diffusion3d_hx_tiling",
        [](uintptr_t t2, uintptr_t t, uintptr_t cp, const Int3& n, const std::array<double, 3>& rd2,
           double dtlam, int elem_bytes, int tiling, uintptr_t stream, int rounds, bool halo_z) {
          DiffusionArgs a{t2, t, cp, {n[0], n[1], n[2]}, {rd2[0], rd2[1], rd2[2]}, dtlam, elem_bytes, rounds, halo_z};
          launch_diffusion3d_inner_hx(a, tiling, as_stream(stream));
        },
        py::arg("t2"), py::arg("t"), py::arg("cp"), py::arg("n"), py::arg("rd2"), py::arg("dtlam"),
        py::arg("elem_bytes"), py::arg("tiling"), py::arg("stream") = 0, py::arg("rounds") = 0,
        py::arg("halo_z") = false);
  // Two time steps in one pass (stencil2_kernels.hip): whole inner box, GPU only.
  m.def("diffusion3d_twostep",
        [](uintptr_t t2, uintptr_t t, uintptr_t cp, const Int3& n, const std::array<double, 3>& rd2,
           double dtlam, int elem_bytes, int form, uintptr_t stream, int rounds, bool halo_z, uintptr_t q) {
          TraceRange tr("igg.diffusion3d_twostep");
          DiffusionArgs a{t2, t, cp, {n[0], n[1], n[2]}, {rd2[0], rd2[1], rd2[2]}, dtlam, elem_bytes, rounds, halo_z,
                          form, q};
          launch_diffusion3d_twostep(a, as_stream(stream));
        },
        py::arg("t2"), py::arg("t"), py::arg("cp"), py::arg("n"), py::arg("rd2"), py::arg("dtlam"),
        py::arg("elem_bytes"), py::arg("form") = 0, py::arg("stream") = 0, py::arg("rounds") = 0,
        py::arg("halo_z") = false, py::arg("q") = 0);
  // q = dtlam / cp as the two-step pass divides (stencil2q_kernels.hip): its optional input `q`. GPU only.
  m.def("quotient",
        [](uintptr_t q, uintptr_t cp, int64_t n, double dtlam, int elem_bytes, uintptr_t stream) {
          TraceRange tr("igg.quotient");
          launch_quotient(q, cp, n, dtlam, elem_bytes, as_stream(stream));
        },
        py::arg("q"), py::arg("cp"), py::arg("n"), py::arg("dtlam"), py::arg("elem_bytes"), py::arg("stream") = 0);
  m.def("diffusion3d_twostep_ok",
        [](const Int3& n, int elem_bytes, int form) {
          DiffusionArgs a{0, 0, 0, {n[0], n[1], n[2]}, {1.0, 1.0, 1.0}, 0.0, elem_bytes, 0, false, form};
          return diffusion3d_twostep_ok(a);
        },
        py::arg("n"), py::arg("elem_bytes"), py::arg("form") = 0);
  m.def("diffusion3d_twostep_forms", []() {
    std::vector<std::string> v;
    for (int i = 0; i < diffusion3d_twostep_num_forms(); ++i) v.push_back(diffusion3d_twostep_form_name(i));
    return v;
  });
  // Three time steps in one pass (stencil3_kernels.hip): rows within a tile, reads q. GPU only.
  m.def("diffusion3d_threestep",
        [](uintptr_t t2, uintptr_t t, uintptr_t q, const Int3& n, const std::array<double, 3>& rd2, double dtlam,
           int elem_bytes, int form, uintptr_t stream, int rounds, bool halo_z) {
          TraceRange tr("igg.diffusion3d_threestep");
          DiffusionArgs a{t2, t, 0, {n[0], n[1], n[2]}, {rd2[0], rd2[1], rd2[2]}, dtlam, elem_bytes, rounds, halo_z,
                          form, q};
          launch_diffusion3d_threestep(a, as_stream(stream));
        },
        py::arg("t2"), py::arg("t"), py::arg("q"), py::arg("n"), py::arg("rd2"), py::arg("dtlam"),
        py::arg("elem_bytes"), py::arg("form") = 0, py::arg("stream") = 0, py::arg("rounds") = 0,
        py::arg("halo_z") = false);
  m.def("diffusion3d_threestep_ok",
        [](const Int3& n, int elem_bytes, int form) {
          // (the quotient array: any non-null value, the shape is what is asked about)
          DiffusionArgs a{0, 0, 0, {n[0], n[1], n[2]}, {1.0, 1.0, 1.0}, 0.0, elem_bytes, 0, false, form, 1};
          return diffusion3d_threestep_ok(a);
        },
        py::arg("n"), py::arg("elem_bytes"), py::arg("form") = 0);
  // (tiles, planes per x chunk, workgroups) of a launch of `form` on shape n aiming at `target` workgroups:
  // host arithmetic. _target: what a launch with `rounds` aims at (rounds > 0 asks the device).
  m.def("diffusion3d_threestep_plan",
        [](const Int3& n, int form, int64_t target) {
          DiffusionArgs a{0, 0, 0, {n[0], n[1], n[2]}, {1.0, 1.0, 1.0}, 0.0, 8, 0, false, form, 1};
          const ThreestepPlan p = diffusion3d_threestep_plan(a, target);
          return std::make_tuple(p.tiles, p.chunk, p.workgroups);
        },
        py::arg("n"), py::arg("form"), py::arg("target"));
  m.def("diffusion3d_threestep_target",
        [](int elem_bytes, int form, int rounds) {
          DiffusionArgs a{0, 0, 0, {3, 3, 4}, {1.0, 1.0, 1.0}, 0.0, elem_bytes, rounds, false, form, 1};
          return diffusion3d_threestep_target(a);
        },
        py::arg("elem_bytes"), py::arg("form"), py::arg("rounds") = 0);
  m.def("diffusion3d_threestep_forms", []() {
    std::vector<std::string> v;
    for (int i = 0; i < diffusion3d_threestep_num_forms(); ++i) v.push_back(diffusion3d_threestep_form_name(i));
    return v;
  });
  m.def("diffusion3d_fused_variant_ok", &diffusion3d_fused_variant_ok);
  m.def("diffusion3d_fused_variants", &diffusion3d_fused_variants,
        "Every fused variant index of the catalogue, ascending, whether this build compiles it or not.");
  // (BY, RY, VZ, BZ, dpp) of a compiled fused variant: host arithmetic
  m.def("diffusion3d_fused_tile",
        [](int v) {
          const FusedTile t = diffusion3d_fused_tile(v);
          return std::make_tuple(t.by, t.ry, t.vz, t.bz, t.dpp);
        },
        py::arg("variant"));
  // The z-edge lane rule of the fused kernels (igg/zedge.hpp), as the kernel
  // evaluates it: (lo, hi, rl, rh, src, src_row, dst, dst_row) of one lane.
  m.def("fused_zedge_lane",
        [](bool dpp, int lane, int zh, int nv, bool in_lo, bool in_hi, bool out_lo, bool out_hi) {
          const ZEdgeLane z = zedge_lane(dpp, lane, zh, nv, in_lo, in_hi, out_lo, out_hi);
          return std::make_tuple(z.lo, z.hi, z.rl, z.rh, z.src, z.src_row, z.dst, z.dst_row);
        },
        py::arg("dpp"), py::arg("lane"), py::arg("zh"), py::arg("nv"), py::arg("in_lo"), py::arg("in_hi"),
        py::arg("out_lo"), py::arg("out_hi"));
  m.def("fused_zedge_zh", &zedge_zh, py::arg("n2"), py::arg("vz"));
  m.def("fused_zedge_one_wave", &zedge_one_wave, py::arg("n2"), py::arg("vz"));
  m.def("fused_zedge_dpp_rows_fit", &zedge_dpp_rows_fit, py::arg("zh"), py::arg("ry"));
  m.def("fused_zedge_dpp_ok", &zedge_dpp_ok, py::arg("n2"), py::arg("vz"), py::arg("ry"));
  m.def("diffusion3d_variant_compiled", &stencil_variant_compiled,
        "Whether stencil variant v is compiled in this build (measurement-only ones: build.py --probes).");
  m.def("probes_build", []() {
#ifdef IGG_PROBES
    return true;
#else
    return false;
#endif
  });
  m.def("fused_debug", [](uintptr_t stamps, int force_sel) {
    fused_debug(reinterpret_cast<int64_t*>(stamps), force_sel);
  }, py::arg("stamps"), py::arg("force_sel") = -1);
  py::class_<FusedHalo, std::shared_ptr<FusedHalo>>(m, "FusedHalo")
      .def(py::init([](std::shared_ptr<PeerMesh> mesh, const Int3& n, int elem_bytes,
                       const std::array<std::array<int, 2>, 3>& nb) {
             return std::make_shared<FusedHalo>(mesh, std::array<int64_t, 3>{n[0], n[1], n[2]}, elem_bytes, nb);
           }),
           py::arg("mesh"), py::arg("n"), py::arg("elem_bytes"), py::arg("neighbors"))
      .def("step",
           [](FusedHalo& f, uintptr_t t2, uintptr_t t, uintptr_t cp, const std::array<double, 3>& rd2,
              double dtlam, int variant, int64_t step, bool primed, uintptr_t stream, int rounds, int mode,
              bool entry, bool halo_z) {
             TraceRange tr("igg.diffusion3d_fused");
             DiffusionArgs a{t2, t, cp, {0, 0, 0}, {rd2[0], rd2[1], rd2[2]}, dtlam, 0, rounds, halo_z};
             f.step_shape(a);
             f.step(a, variant, mode, step, primed, as_stream(stream), entry);
           },
           py::arg("t2"), py::arg("t"), py::arg("cp"), py::arg("rd2"), py::arg("dtlam"), py::arg("variant"),
           py::arg("step"), py::arg("primed"), py::arg("stream"), py::arg("rounds") = 0, py::arg("mode") = 0,
           py::arg("entry") = false, py::arg("halo_z") = false)
      .def("sync", [](FusedHalo& f, uintptr_t s) { f.sync(as_stream(s)); })
      .def("drain", [](FusedHalo& f, uintptr_t s) { f.drain(as_stream(s)); }, py::arg("stream"),
           "Exit barrier after in-kernel synchronised steps (collective; no-op after a sync-kernel step).")
      .def("set_fields", &FusedHalo::set_fields, py::arg("a"), py::arg("b"))
      .def_property_readonly("has_fields", &FusedHalo::has_fields)
      .def("io", [](FusedHalo& f, int64_t step, bool primed, uintptr_t t2, bool direct_z) {
        const HaloIOArgs io = f.io(step, primed, t2, direct_z);
        py::list in, out;
        for (int d = 0; d < 3; ++d) {
          in.append(py::make_tuple(io.in[d][0], io.in[d][1]));
          out.append(py::make_tuple(io.out[d][0], io.out[d][1]));
        }
        return py::make_tuple(in, out, io.zpitch, io.zrow);
      }, py::arg("step"), py::arg("primed"), py::arg("t2") = 0, py::arg("direct_z") = false)
      .def("region_offset", &FusedHalo::region_offset)
      .def_property_readonly("half_elems", &FusedHalo::half_elems)
      .def_property_readonly("zpitch", &FusedHalo::zpitch)
      .def_property_readonly("n_peers", &FusedHalo::n_peers)
      .def("check_error", [](FusedHalo& f) { f.mesh().check_error(); })
      .def("clear_error", [](FusedHalo& f) { f.mesh().clear_error(); },
           "Reset this rank's sticky timeout word (after a failed exchange was handled).")
      .def("set_step_sync", &FusedHalo::set_step_sync, py::arg("mode"),
           "Step synchronisation: -1 default, 0 inside the fused kernel, 1 sync kernel (same on every rank).")
      .def_property_readonly("in_kernel_sync", [](const FusedHalo& f) { return f.in_kernel_sync(0); },
                             "Whether a step with the default send mode synchronises inside the kernel.")
      .def("in_kernel_sync_for", &FusedHalo::in_kernel_sync, py::arg("mode"),
           "Whether a step with send mode `mode` synchronises inside the kernel (bit 16 asks for it).")
      .def("flag", [](FusedHalo& f, int i) { return f.mesh().read_flag(i); }, py::arg("index"),
           "Word `index` of this rank's flag block (PutFlags: 0 EPOCH = completed steps, 2 COUNT).")
      .def("close", [](FusedHalo& f) { f.close(); });
  m.def("split_boundary", [](const Int3& n, const std::array<std::array<bool, 2>, 3>& active,
                             const Int3& w) {
    std::vector<Box> slabs;
    Box interior;
    int64_t nn[3] = {n[0], n[1], n[2]}, ww[3] = {w[0], w[1], w[2]};
    bool aa[3][2];
    for (int d = 0; d < 3; ++d) { aa[d][0] = active[d][0]; aa[d][1] = active[d][1]; }
    split_boundary(nn, aa, ww, slabs, interior);
    std::vector<std::pair<Int3, Int3>> out;
    for (const Box& b : slabs) out.push_back(from_box(b));
    return py::make_tuple(out, from_box(interior));
  });
}
