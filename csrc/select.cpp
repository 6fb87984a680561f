// Launcher of the converting lattice copy (igg/select.hpp).
#include "igg/select.hpp"

#include "igg/common.hpp"

namespace igg {

void select_convert(const std::vector<SelectDesc>& jobs, hipStream_t stream) {
  size_t k = 0;
  while (k < jobs.size()) {
    SelectBatch batch;
    batch.n = 0;
    uint32_t blocks = 0;
    bool wide = false;
    for (; k < jobs.size() && batch.n < SELECT_MAX_JOBS; ++k) {
      const SelectDesc& in = jobs[k];
      const SelectPlan p = plan_select(in.c, in.S, in.T);
      if (p.blocks == 0) continue;  // an empty job
      if (!in.src || !in.dst) fail("select_convert: null pointer");
      if (in.src % sizeof(double) != 0 || in.dst % sizeof(float) != 0)
        fail("select_convert: source and destination must be aligned to their elements");
      SelectJob& j = batch.job[batch.n];
      j.src = reinterpret_cast<const double*>(in.src);
      j.dst = reinterpret_cast<float*>(in.dst);
      for (int d = 0; d < 3; ++d) j.c[d] = in.c[d], j.S[d] = in.S[d], j.T[d] = in.T[d];
      j.rows = p.path == SelectPath::rows ? 1 : 0;
      wide = wide || p.index_bits == 64;
      batch.block_start[batch.n] = blocks;
      blocks += static_cast<uint32_t>(p.blocks);
      ++batch.n;
    }
    if (batch.n == 0) continue;
    batch.block_start[batch.n] = blocks;
    launch_select_convert(batch, wide, stream);
  }
}

}  // namespace igg
