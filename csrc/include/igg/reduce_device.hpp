// Device pieces shared by the reduction kernels (reduce_kernels.hip) and the
// projection kernels (project_kernels.hip): the streamed loads, one load's
// worth of elements, an op's f64 term and the combination of two partials.
// Include from .hip units only, after igg/reduce.hpp (the op codes).
#pragma once

#include <hip/hip_runtime.h>

#include "igg/reduce.hpp"

// Non-temporal loads of the streamed fields (measurement builds: -DIGG_REDUCE_NT=0).
#ifndef IGG_REDUCE_NT
#define IGG_REDUCE_NT 1
#endif

namespace igg {
namespace {

typedef double D2 __attribute__((ext_vector_type(2)));
typedef float F4 __attribute__((ext_vector_type(4)));

template <typename V>
__device__ inline V stream_load(const V* p) {
#if IGG_REDUCE_NT
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}

// One load's worth of elements.
template <typename T, int VEC>
struct Pack;
template <>
struct Pack<float, 4> {
  F4 v;
  __device__ void load(const float* p) { v = stream_load(reinterpret_cast<const F4*>(p)); }
  __device__ double get(int e) const { return static_cast<double>(v[e]); }
};
template <>
struct Pack<double, 2> {
  D2 v;
  __device__ void load(const double* p) { v = stream_load(reinterpret_cast<const D2*>(p)); }
  __device__ double get(int e) const { return v[e]; }
};
template <typename T>
struct Pack<T, 1> {
  T v;
  __device__ void load(const T* p) { v = stream_load(p); }
  __device__ double get(int) const { return static_cast<double>(v); }
};

template <int OP>
__device__ inline double term(double a, double b) {
  if (OP == R_SUM || OP == R_MAX) return a;
  if (OP == R_MIN) return -a;
  if (OP == R_SUMSQ) return a * a;
  if (OP == R_MAXABS) return __builtin_fabs(a);
  if (OP == R_DOT) return a * b;
  const double d = a - b;
  return OP == R_SUMSQ_DIFF ? d * d : __builtin_fabs(d);
}

template <bool MAXT>
__device__ inline double combine(double a, double b) {
  return MAXT ? __builtin_fmax(a, b) : a + b;
}

}  // namespace
}  // namespace igg
