// Launchers of the converting lattice copies (igg/select.hpp).
#include "igg/select.hpp"

#include "igg/common.hpp"

namespace igg {
namespace {

// Jobs into batches of SELECT_MAX_JOBS, one launch each; empty jobs are skipped.
template <typename In, typename Out, typename Launch>
void run_batches(const char* name, const std::vector<SelectDesc>& jobs, hipStream_t stream, Launch launch) {
  size_t k = 0;
  while (k < jobs.size()) {
    SelectBatchT<SelectJobT<In, Out>> batch;
    batch.n = 0;
    uint32_t blocks = 0;
    bool wide = false;
    for (; k < jobs.size() && batch.n < SELECT_MAX_JOBS; ++k) {
      const SelectDesc& in = jobs[k];
      const SelectPlan p = plan_select(in.c, in.S, in.T);
      if (p.blocks == 0) continue;  // an empty job
      if (!in.src || !in.dst) fail(name, ": null pointer");
      if (in.src % sizeof(In) != 0 || in.dst % sizeof(Out) != 0)
        fail(name, ": source and destination must be aligned to their elements");
      SelectJobT<In, Out>& j = batch.job[batch.n];
      j.src = reinterpret_cast<const In*>(in.src);
      j.dst = reinterpret_cast<Out*>(in.dst);
      for (int d = 0; d < 3; ++d) j.c[d] = in.c[d], j.S[d] = in.S[d], j.T[d] = in.T[d];
      j.rows = p.path == SelectPath::rows ? 1 : 0;
      wide = wide || p.index_bits == 64;
      batch.block_start[batch.n] = blocks;
      blocks += static_cast<uint32_t>(p.blocks);
      ++batch.n;
    }
    if (batch.n == 0) continue;
    batch.block_start[batch.n] = blocks;
    launch(batch, wide, stream);
  }
}

}  // namespace

void select_convert(const std::vector<SelectDesc>& jobs, hipStream_t stream) {
  run_batches<double, float>("select_convert", jobs, stream, launch_select_convert);
}

void select_widen(const std::vector<SelectDesc>& jobs, hipStream_t stream) {
  run_batches<float, double>("select_widen", jobs, stream, launch_select_widen);
}

}  // namespace igg
