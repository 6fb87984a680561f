// Converting lattice copies on the GPU (select_kernels.hip, select.cpp): the
// one thing gather_g needs that a byte mover cannot do. A job reads the
// lattice src[i0*S0 + i1*S1 + i2*S2], i_d < c_d, of an f64 field and writes
// static_cast<float> of it to dst[i0*T0 + i1*T1 + i2*T2]; strides are in
// elements and a selection step is already folded into S. The sender packs
// its pieces of a global selection this way (compact dst: half the bytes
// travel), the root writes its own block straight into its box of the global
// array (dst strides of that array).
//
// scatter_g needs the mirror image at the receiver: select_widen reads an f32
// lattice (a compact staging buffer, or a box of a float32 global array) and
// writes static_cast<double> of it into an f64 field - exact, and again only
// half the bytes travelled. Same jobs, same batches, same plan.
//
// One launch takes up to SELECT_MAX_JOBS jobs, each with its own block range
// (as ReduceBatch). The path of a job comes from a host plan (plan_select),
// shared by the launcher and the tests (native.select_plan).
#pragma once

#include <cstdint>
#include <vector>

#include <hip/hip_runtime_api.h>

namespace igg {

constexpr int SELECT_BLOCK = 256;        // lanes per workgroup (4 waves)
constexpr int SELECT_MAX_BLOCKS = 2048;  // workgroups per job: 8 per CU, 8 waves per SIMD; grid-stride beyond
constexpr int SELECT_MAX_JOBS = 16;      // jobs per launch (a rank has up to 8 pieces)
constexpr int SELECT_UNROLL = 4;         // independent 32-B loads per lane in flight (rows path)

// rows: S2 == 1 and T2 == 1. A wave takes a row; 16-B f32x4 stores aligned on
//   the destination, head and tail elements stored singly; the source needs
//   only its element's alignment.
// element: anything else (a step along the contiguous axis, a permuted
//   layout): one output per lane over the flattened lattice.
enum class SelectPath { rows, element };

inline const char* select_path_name(SelectPath p) { return p == SelectPath::rows ? "rows" : "element"; }

struct SelectPlan {
  SelectPath path = SelectPath::element;
  int index_bits = 32;   // 64: some span of the job does not fit 31 bits
  int64_t total = 0;     // elements
  int64_t rows = 0;      // c0 * c1
  int64_t src_span = 0;  // elements between the first and the last selected one
  int64_t dst_span = 0;
  int64_t blocks = 0;    // 0: an empty job (the launcher skips it)
};

// Counts, source strides and destination strides, outer .. inner. Strides must
// not be negative.
SelectPlan plan_select(const int64_t c[3], const int64_t S[3], const int64_t T[3]);

template <typename In, typename Out>
struct SelectJobT {
  const In* src;  // the first selected element
  Out* dst;
  int64_t c[3], S[3], T[3];
  int rows;  // SelectPath::rows
};

template <typename Job>
struct SelectBatchT {
  int n;
  uint32_t block_start[SELECT_MAX_JOBS + 1];
  Job job[SELECT_MAX_JOBS];
};

using SelectJob = SelectJobT<double, float>;  // select_convert: f64 in, f32 out
using SelectBatch = SelectBatchT<SelectJob>;
using WidenJob = SelectJobT<float, double>;  // select_widen: f32 in, f64 out
using WidenBatch = SelectBatchT<WidenJob>;

struct SelectDesc {
  uintptr_t src = 0, dst = 0;
  int64_t c[3] = {1, 1, 1}, S[3] = {0, 0, 1}, T[3] = {0, 0, 1};
};

// Enqueue every job on `stream` (any count, SELECT_MAX_JOBS per launch; jobs
// of one launch share the index width). Nothing is allocated and nothing
// synchronises.
void select_convert(const std::vector<SelectDesc>& jobs, hipStream_t stream);

// The same for f32 in, f64 out (rows path: 16-B f64x2 stores aligned on the
// destination, at most one head and three tail elements stored singly, the
// lanes of a wave exchanging their floats so that each store instruction is
// contiguous; the source needs only its element's alignment).
void select_widen(const std::vector<SelectDesc>& jobs, hipStream_t stream);

// select_kernels.hip
void launch_select_convert(const SelectBatch& batch, bool wide, hipStream_t stream);
void launch_select_widen(const WidenBatch& batch, bool wide, hipStream_t stream);

}  // namespace igg
