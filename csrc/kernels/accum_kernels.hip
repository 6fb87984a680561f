// Batched strided accumulation for gfx950 (igg/accum.hpp): the kernels of the
// transposed halo exchange. The launch geometry, the block -> (descriptor,
// row, chunk) decode and the three shapes are those of copy3d_batch_kernel
// (copy_kernels.hip) and come from the same host plan; what differs is the
// element work, chosen per descriptor (wave-uniform):
//   add       load dst and src, store dst + src
//   take      load src, store it to dst, store +0 to src
//   add_take  both
//   zero      store +0 to dst
// A cell has one writer per launch (the engine puts a second message into the
// same slab into a second launch), so there are no atomics and the result does
// not depend on the schedule. The additions are plain IEEE adds in the
// element type, one per cell, which is what host_accum3d does: the two agree
// bit for bit.
#include <hip/hip_runtime.h>

#include "igg/accum.hpp"
#include "igg/copy_plan.hpp"

namespace igg {

namespace {

constexpr int BLOCK = COPY_BLOCK;
constexpr int EPT = COPY_EPT;
constexpr int64_t CHUNK = COPY_CHUNK;
constexpr int GROWS = COPY_GROWS;

struct AccumBatch {
  Copy3D c[MAX_BATCH];
  int64_t block_start[MAX_BATCH + 1];
  int n;
  uint32_t flat_mask;    // as CopyBatch3
  uint32_t gather_mask;
  uint32_t vec_mask;     // gather: a row is one aligned access; chunk: 16-byte accesses
  uint32_t add_mask;     // bit c: dst is read and added to
  uint32_t take_mask;    // bit c: src is cleared
  uint32_t zero_mask;    // bit c: dst = 0, src is not read
};

template <typename T, int N>
struct VecOf {
  typedef T type __attribute__((ext_vector_type(N)));
};
template <typename T>
struct VecOf<T, 1> {
  typedef T type;
};

struct Ops {
  bool add, take, zero;  // wave-uniform
};

// One access of type V on each side.
template <typename V>
__device__ __forceinline__ void accum_one(char* s, char* d, const Ops& op) {
  V out{};
  if (!op.zero) {
    out = *reinterpret_cast<const V*>(s);
    if (op.add) out = *reinterpret_cast<const V*>(d) + out;
  }
  *reinterpret_cast<V*>(d) = out;
  if (op.take) *reinterpret_cast<V*>(s) = V{};
}

// GROWS rows (one per outer index) of one lane: every load before the first
// store, as move_rows of the copy kernel (rows past nr load row nr - 1 again
// and store nothing).
template <typename V>
__device__ __forceinline__ void accum_rows(char* s, char* d, int64_t s_step, int64_t d_step, int nr,
                                           const Ops& op) {
  V v[GROWS];
  if (op.zero) {
#pragma unroll
    for (int k = 0; k < GROWS; ++k) v[k] = V{};
  } else {
#pragma unroll
    for (int k = 0; k < GROWS; ++k) v[k] = *reinterpret_cast<const V*>(s + (k < nr ? k : nr - 1) * s_step);
    if (op.add) {
      V a[GROWS];
#pragma unroll
      for (int k = 0; k < GROWS; ++k) a[k] = *reinterpret_cast<const V*>(d + (k < nr ? k : nr - 1) * d_step);
#pragma unroll
      for (int k = 0; k < GROWS; ++k) v[k] = a[k] + v[k];
    }
  }
#pragma unroll
  for (int k = 0; k < GROWS; ++k)
    if (k < nr) *reinterpret_cast<V*>(d + k * d_step) = v[k];
  if (op.take) {
#pragma unroll
    for (int k = 0; k < GROWS; ++k)
      if (k < nr) *reinterpret_cast<V*>(s + k * s_step) = V{};
  }
}

template <typename T>
__global__ void __launch_bounds__(BLOCK) accum3d_batch_kernel(const AccumBatch batch) {
  const int64_t b = blockIdx.x;
  int c = 0;
  while (c + 1 < batch.n && b >= batch.block_start[c + 1]) ++c;
  const Copy3D& cp = batch.c[c];
  const int64_t local = b - batch.block_start[c];
  const Ops op{((batch.add_mask >> c) & 1u) != 0, ((batch.take_mask >> c) & 1u) != 0,
               ((batch.zero_mask >> c) & 1u) != 0};
  char* sbase = const_cast<char*>(cp.src);
  char* dbase = cp.dst;
  constexpr int64_t EB = sizeof(T);
  const bool vec = (batch.vec_mask >> c) & 1u;
  if ((batch.flat_mask >> c) & 1u) {
    // Edges of small fields, narrow slabs: one element per lane over the flattened box.
    const int64_t e = local * BLOCK + threadIdx.x;
    const int64_t plane = cp.n_mid * cp.n_inner;
    if (e < cp.n_outer * plane) {
      const int64_t o = e / plane, r = e - o * plane;
      const int64_t m = r / cp.n_inner, i = r - m * cp.n_inner;
      accum_one<T>(sbase + (o * cp.src_so + m * cp.src_sm + i * cp.src_si) * EB,
                   dbase + (o * cp.dst_so + m * cp.dst_sm + i * cp.dst_si) * EB, op);
    }
  } else if ((batch.gather_mask >> c) & 1u) {
    // Short rows, many of them (the z slab of a C-ordered field): a lane owns
    // the row `m` of GROWS consecutive outer indices. On the field's side every
    // row is a cache line of its own, so the launch is bound by line requests:
    // an add makes two per row and lane (load, store) on the field's side where
    // the copy makes one, a take likewise.
    const int64_t nmc = (cp.n_mid + 63) / 64;
    const int64_t og = local / nmc, mc = local - og * nmc;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t m = mc * 64 + lane;
    const int64_t o0 = (og * 4 + w) * GROWS;
    if (m < cp.n_mid && o0 < cp.n_outer) {
      char* s = sbase + (o0 * cp.src_so + m * cp.src_sm) * EB;
      char* d = dbase + (o0 * cp.dst_so + m * cp.dst_sm) * EB;
      const int64_t ss = cp.src_so * EB, ds = cp.dst_so * EB;
      const int nr = static_cast<int>(min<int64_t>(GROWS, cp.n_outer - o0));
      const int rb = vec ? static_cast<int>(cp.n_inner * EB) : 0;  // wave-uniform
      if (rb == 16) {
        accum_rows<typename VecOf<T, 16 / EB>::type>(s, d, ss, ds, nr, op);
      } else if (rb == 8) {
        accum_rows<typename VecOf<T, 8 / EB>::type>(s, d, ss, ds, nr, op);
      } else if (rb == 4 && EB == 4) {
        accum_rows<T>(s, d, ss, ds, nr, op);
      } else {
#pragma unroll 1
        for (int64_t i = 0; i < cp.n_inner; ++i)
          accum_rows<T>(s + i * cp.src_si * EB, d + i * cp.dst_si * EB, ss, ds, nr, op);
      }
    }
  } else {
    // Long rows (x and y slabs of a C-ordered field, packed buffers): a
    // workgroup does one CHUNK of one of the n_outer * n_mid rows.
    const int64_t nchunks = (cp.n_inner + CHUNK - 1) / CHUNK;
    const int64_t row = local / nchunks;
    const int64_t i0 = (local - row * nchunks) * CHUNK;
    const int64_t o = row / cp.n_mid, m = row - o * cp.n_mid;
    char* src = sbase + (o * cp.src_so + m * cp.src_sm) * EB;
    char* dst = dbase + (o * cp.dst_so + m * cp.dst_sm) * EB;
    const int64_t n = cp.n_inner;
    if (vec) {
      // unit stride and every row start 16-byte aligned on both sides: a lane
      // moves 16 bytes per access; the elements past the row's last full
      // 16 bytes go one by one
      constexpr int VPT = 16 / EB;        // elements per access
      constexpr int NV = EPT / VPT;       // accesses per lane and chunk
      typedef typename VecOf<T, VPT>::type V;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int64_t i = i0 + (static_cast<int64_t>(k) * BLOCK + threadIdx.x) * VPT;
        if (i + VPT <= n) {
          accum_one<V>(src + i * EB, dst + i * EB, op);
        } else {
          for (int64_t j = i; j < n; ++j) accum_one<T>(src + j * EB, dst + j * EB, op);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < EPT; ++k) {
        const int64_t i = i0 + k * BLOCK + threadIdx.x;
        if (i < n) accum_one<T>(src + i * cp.src_si * EB, dst + i * cp.dst_si * EB, op);
      }
    }
  }
}

template <typename T>
void launch_typed(const std::vector<Accum3D>& ops, hipStream_t stream) {
  size_t pos = 0;
  while (pos < ops.size()) {
    AccumBatch batch{};
    int64_t blocks = 0;
    while (pos < ops.size() && batch.n < MAX_BATCH) {
      const Accum3D& a = ops[pos++];
      const CopyPlan3 p = plan_accum3d(a.c, static_cast<int>(sizeof(T)), g_copy_gather);
      if (p.blocks <= 0) continue;
      if (!a.c.dst || !a.c.src) fail("launch_accum3d: null pointer");
      const uint32_t bit = 1u << batch.n;
      batch.c[batch.n] = p.box;
      batch.block_start[batch.n] = blocks;
      if (p.path == CopyPath::flat) batch.flat_mask |= bit;
      if (p.path == CopyPath::gather) batch.gather_mask |= bit;
      if (p.vec_bytes) batch.vec_mask |= bit;
      if (a.op == AccumOp::Zero) batch.zero_mask |= bit;
      else {
        if (static_cast<int>(a.op) & 1) batch.add_mask |= bit;
        if (static_cast<int>(a.op) & 2) batch.take_mask |= bit;
      }
      blocks += p.blocks;
      ++batch.n;
    }
    if (batch.n == 0) continue;
    batch.block_start[batch.n] = blocks;
    if (blocks > 0x7fffffffLL) fail("launch_accum3d: too many blocks (", blocks, ")");
    hipLaunchKernelGGL((accum3d_batch_kernel<T>), dim3(static_cast<unsigned>(blocks)), dim3(BLOCK), 0, stream,
                       batch);
    IGG_HIP_CHECK(hipGetLastError());
  }
}

}  // namespace

void launch_accum3d(const std::vector<Accum3D>& ops, AccumType type, hipStream_t stream) {
  if (ops.empty()) return;
  for (const Accum3D& a : ops) {
    const int eb = accum_elem_bytes(type);
    if (reinterpret_cast<uintptr_t>(a.c.src) % eb || reinterpret_cast<uintptr_t>(a.c.dst) % eb)
      fail("launch_accum3d: a pointer is not aligned to the element size");
  }
  switch (type) {
    case AccumType::F32: launch_typed<float>(ops, stream); break;
    case AccumType::F64: launch_typed<double>(ops, stream); break;
    default: fail("launch_accum3d: the GPU kernels take float32 and float64 only");
  }
}

}  // namespace igg
