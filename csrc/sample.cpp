// Argument checks, launcher and host reference of sample_g (igg/sample.hpp).
#include "igg/sample.hpp"

#include "igg/common.hpp"

namespace igg {

void check_sample(const char* who, const SampleArgs& a) {
  if (a.nd < 1 || a.nd > 3) fail(who, ": fields must have 1 to 3 dimensions (got ", a.nd, ")");
  if (a.nf < 1 || a.nf > SAMPLE_MAX_FIELDS) fail(who, ": 1 to ", SAMPLE_MAX_FIELDS, " fields per call (got ", a.nf, ")");
  if (a.npts < 0) fail(who, ": negative point count");
  for (int d = 0; d < a.nd; ++d) {
    const SampleDim& D = a.dim[d];
    if (D.E < 2) fail(who, ": global extent ", D.E, " in dimension ", d, " (at least 2 is needed)");
    if (D.m < 1) fail(who, ": local size ", D.m, " in dimension ", d);
    if (D.nseg < 0 || D.nseg > 2) fail(who, ": ", D.nseg, " segments in dimension ", d);
    // every owned cell lies in the field, so that no corner offset leaves it
    for (int s = 0; s < D.nseg; ++s)
      if (D.g0[s] < 0 || D.g1[s] <= D.g0[s] || D.g1[s] > D.E || D.i0[s] < 0 ||
          int64_t{D.i0[s]} + (D.g1[s] - D.g0[s]) > D.m)
        fail(who, ": segment ", s, " of dimension ", d, " lies outside of the field or the global extent");
  }
  if (a.npts == 0) return;
  if (!a.P || !a.out) fail(who, ": null pointer");
  for (int f = 0; f < a.nf; ++f) {
    if (!a.field[f].base) fail(who, ": null field pointer");
    for (int d = 0; d < a.nd; ++d)
      if (a.field[f].stride[d] < 0) fail(who, ": negative stride");
  }
  if (a.nf > 1 && a.out_fs < a.npts) fail(who, ": the outputs of two fields overlap");
  if (a.row && (a.nrows < 0 || a.row_stride < 0)) fail(who, ": negative row count or row stride");
}

void sample(const SampleArgs& a, int elem_size, int max_blocks, hipStream_t stream) {
  if (elem_size != 4 && elem_size != 8) fail("sample: float32 and float64 fields only (element size ", elem_size, ")");
  check_sample("sample", a);
  if (a.npts == 0) return;
  const int64_t per_block = int64_t{SAMPLE_BLOCK} * SAMPLE_POINTS;
  const int64_t cap = max_blocks > 0 ? max_blocks : SAMPLE_MAX_BLOCKS;
  const int64_t want = (a.npts + per_block - 1) / per_block;
  launch_sample(a, elem_size, static_cast<int>(want < cap ? want : cap), stream);
}

namespace {

template <typename T>
void host_sample_t(const SampleArgs& A) {
  uint64_t* out = A.out;
  if (A.row) {
    const int64_t r = *A.row;
    if (r < 0 || r >= A.nrows) return;
    out += r * A.row_stride;
  }
  const int nd = A.nd, nc = 1 << nd;
  for (int64_t p = 0; p < A.npts; ++p) {
    int64_t lo[3], hi[3];
    double t[3];
    bool valid = true, owned = true;
    for (int d = 0; d < nd; ++d) {
      const SampleAxis a = sample_axis(A.dim[d], A.P[p * A.ps0 + d * A.ps1]);
      valid = valid && a.valid, owned = owned && a.owned;
      lo[d] = a.lo, hi[d] = a.hi, t[d] = a.t;
    }
    if (!(valid && owned))
      for (int d = 0; d < nd; ++d) lo[d] = 0, hi[d] = 0;
    for (int f = 0; f < A.nf; ++f) {
      const T* base = static_cast<const T*>(A.field[f].base);
      double w[8];
      for (int c = 0; c < nc; ++c) {
        int64_t off = 0;
        for (int d = 0; d < nd; ++d) off += (((c >> (nd - 1 - d)) & 1) ? hi[d] : lo[d]) * A.field[f].stride[d];
        w[c] = static_cast<double>(base[off]);
      }
      for (int d = nd - 1; d >= 0; --d)
        for (int c = 0; c < (1 << d); ++c) w[c] = sample_lerp(w[2 * c], w[2 * c + 1], t[d]);
      out[f * A.out_fs + p] = sample_bits(w[0], valid, owned, A.me0 != 0);
    }
  }
}

}  // namespace

void host_sample(const SampleArgs& a, int elem_size) {
  if (elem_size != 4 && elem_size != 8)
    fail("host_sample: float32 and float64 fields only (element size ", elem_size, ")");
  check_sample("host_sample", a);
  if (a.npts == 0) return;
  if (elem_size == 4)
    host_sample_t<float>(a);
  else
    host_sample_t<double>(a);
}

}  // namespace igg
