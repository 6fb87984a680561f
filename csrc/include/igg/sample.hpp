// sample_g: a field's values at arbitrary points of the global grid
// (sample_kernels.hip, sample.cpp; parallel/sample_g.py).
//
// A point u lives in the global index space of the field (the fractional form
// of indices_g). Per dimension it has a lower corner g and a weight t; the
// rank that owns g (one of its owned segments holds it) also holds the upper
// corner at local index i + 1, so it interpolates alone and every other rank
// writes the bit pattern 0: an integer sum over the ranks reproduces the
// owner's 64 bits. All arithmetic is float64 with separately rounded
// operations (the build has no contraction); the expressions below are shared
// by the kernel and by host_sample, which is the CPU path and the tests' oracle.
#pragma once

#include <cstdint>
#include <vector>

#include <hip/hip_runtime_api.h>

#if defined(__HIPCC__)
#define IGG_HD __host__ __device__ inline
#else
#define IGG_HD inline
#endif

namespace igg {

constexpr int SAMPLE_BLOCK = 256;        // lanes per workgroup (4 waves)
constexpr int SAMPLE_POINTS = 2;         // points per lane in flight
constexpr int SAMPLE_MAX_BLOCKS = 4096;  // 16 per CU; grid-stride beyond
constexpr int SAMPLE_MAX_FIELDS = 8;     // fields per launch (more: further launches)
constexpr uint64_t SAMPLE_NAN = 0x7FF8000000000000ull;  // the canonical quiet NaN

// One dimension of the field's global index space and this rank's part of it.
// (32-bit: an extent is far below 2^31, and the table lives in scalar registers)
struct SampleDim {
  int32_t E = 1;     // global extent
  int32_t m = 1;     // local size
  int32_t per = 0;   // periodic
  int32_t nseg = 0;  // owned segments: global [g0, g1) at local i0, i0 + 1, ...
  int32_t g0[2] = {0, 0}, g1[2] = {0, 0}, i0[2] = {0, 0};
};

struct SampleField {
  const void* base;
  int64_t stride[3];  // elements, per axis of the field
};

struct SampleArgs {
  int32_t nd = 0;   // 1..3
  int32_t nf = 0;   // 1..SAMPLE_MAX_FIELDS
  int32_t me0 = 0;  // this rank writes the NaN of invalid points
  int32_t pad = 0;
  SampleDim dim[3];
  SampleField field[SAMPLE_MAX_FIELDS];
  const double* P = nullptr;  // point p, axis d at P[p*ps0 + d*ps1]
  int64_t ps0 = 0, ps1 = 0;
  int64_t npts = 0;
  uint64_t* out = nullptr;   // field f, point p at out[f*out_fs + p] (bits of a double)
  int64_t out_fs = 0;
  const int64_t* row = nullptr;  // optional: the output moves by *row * row_stride,
  int64_t nrows = 0;             // and nothing is written if *row >= nrows
  int64_t row_stride = 0;
};

// What a point is in one dimension.
struct SampleAxis {
  int64_t lo, hi;  // local indices of the two corners (hi clamped into the field)
  double t;        // weight of the upper corner
  bool valid, owned;
};

IGG_HD SampleAxis sample_axis(const SampleDim& D, double u) {
  const double E = static_cast<double>(D.E);
  const bool fin = u == u && __builtin_fabs(u) != __builtin_inf();
  SampleAxis a;
  double f;
  if (D.per) {
    a.valid = fin;
    const double uu = fin ? u : 0.0;
    double w = uu - E * __builtin_floor(uu / E);
    if (w >= E) w -= E;
    if (w < 0.0) w += E;
    f = __builtin_floor(w);
    if (f > E - 1.0) f = E - 1.0;
    if (f < 0.0) f = 0.0;  // (only where |u| is so large that the fold has lost every digit)
    a.t = w - f;
  } else {
    a.valid = fin && u >= 0.0 && u <= E - 1.0;
    const double uu = a.valid ? u : 0.0;
    f = __builtin_floor(uu);
    if (f > E - 2.0) f = E - 2.0;
    a.t = uu - f;
  }
  const int32_t g = static_cast<int32_t>(f);  // 0 <= f <= E - 1
  const bool in0 = D.nseg > 0 && g >= D.g0[0] && g < D.g1[0];
  const bool in1 = D.nseg > 1 && g >= D.g0[1] && g < D.g1[1];
  a.owned = in0 || in1;
  const int32_t lo = in0 ? D.i0[0] + (g - D.g0[0]) : in1 ? D.i0[1] + (g - D.g0[1]) : 0;
  a.lo = lo;
  a.hi = lo + 1 < D.m ? lo + 1 : D.m - 1;
  return a;
}

// A corner of weight zero never reaches the result.
IGG_HD double sample_lerp(double a, double b, double t) {
  return t == 0.0 ? a : t == 1.0 ? b : (1.0 - t) * a + t * b;
}

// What lands in the output: the value's bits (every NaN as the canonical one,
// so that host and device agree whatever NaN their arithmetic produces), the
// canonical NaN of an invalid point on the rank with me0, 0 otherwise.
IGG_HD uint64_t sample_bits(double v, bool valid, bool owned, bool me0) {
  union { double d; uint64_t u; } c;
  c.d = v;
  if (v != v) c.u = SAMPLE_NAN;
  return !valid ? (me0 ? SAMPLE_NAN : 0ull) : owned ? c.u : 0ull;
}

// Checks shared by both entry points; `who` names the caller in the message.
void check_sample(const char* who, const SampleArgs& a);

// Enqueue one launch on `stream` (elem_size 4 or 8: f32 or f64 fields).
// Nothing is allocated and nothing synchronises. max_blocks caps the grid
// (0: SAMPLE_MAX_BLOCKS); the tests use it to run the grid-stride loop on few points.
void sample(const SampleArgs& a, int elem_size, int max_blocks, hipStream_t stream);

// The same on host memory, point after point.
void host_sample(const SampleArgs& a, int elem_size);

// sample_kernels.hip
void launch_sample(const SampleArgs& a, int elem_size, int blocks, hipStream_t stream);

}  // namespace igg
