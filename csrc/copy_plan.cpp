// Host-side plan of the batched copy kernels (igg/copy_plan.hpp).
#include "igg/copy_plan.hpp"

#include <cstring>

#include "igg/accum.hpp"

namespace igg {

Copy3D normalized(Copy3D c) {
  if (c.n_mid > 1 && c.src_sm == c.n_inner * c.src_si && c.dst_sm == c.n_inner * c.dst_si) {
    c.n_inner *= c.n_mid;
    c.n_mid = 1;
  } else if (c.n_inner == 1 && c.n_mid > 1) {
    c.n_inner = c.n_mid, c.src_si = c.src_sm, c.dst_si = c.dst_sm;
    c.n_mid = 1;
  }
  if (c.n_mid == 1) {
    c.n_mid = c.n_outer, c.src_sm = c.src_so, c.dst_sm = c.dst_so;
    c.n_outer = 1;
  }
  // (short rows keep n_outer when there are enough of them for a wave: the
  // one-row-per-lane shape takes its GROWS independent loads from it)
  if (c.n_outer > 1 && c.src_so == c.n_mid * c.src_sm && c.dst_so == c.n_mid * c.dst_sm &&
      (c.n_inner >= 64 || c.n_mid < 64)) {
    c.n_mid *= c.n_outer;
    c.n_outer = 1;
  }
  // now the box is n_outer x n_mid rows of n_inner, n_outer > 1 only with n_mid > 1
  if (c.n_outer == 1 && c.n_inner >= 64 && (c.src_si != 1 || c.dst_si != 1)) {
    // long strided rows (a one-plane z face in a batch with slabs): one
    // element per lane along the row, GROWS rows per lane
    c.n_outer = c.n_mid, c.src_so = c.src_sm, c.dst_so = c.dst_sm;
    c.n_mid = c.n_inner, c.src_sm = c.src_si, c.dst_sm = c.dst_si;
    c.n_inner = 1;
  }
  if (c.n_outer == 1) c.src_so = c.dst_so = 0;
  return c;
}

bool aligned_rows(const Copy3D& c, int eb, const ParityShift& par) {
  const int64_t rb = c.n_inner * eb;
  if (c.src_si != 1 || c.dst_si != 1 || (rb != 4 && rb != 8 && rb != 16)) return false;
  if (par.side != 0 && par.bytes % rb != 0) return false;
  auto ok = [&](const char* p, int64_t sm, int64_t so) {
    return reinterpret_cast<uintptr_t>(p) % rb == 0 && (sm * eb) % rb == 0 && (so * eb) % rb == 0;
  };
  return ok(c.src, c.src_sm, c.src_so) && ok(c.dst, c.dst_sm, c.dst_so);
}

CopyPlan2 plan_copy2d(const Copy2D& c, int /*elem_bytes*/, bool gather) {
  CopyPlan2 p;
  p.box = c;
  const int64_t total = c.n_outer * c.n_inner;
  if (c.n_outer <= 0 || c.n_inner <= 0) return p;
  const bool is_flat = c.n_inner < 64;
  const bool is_gather = !is_flat && (c.src_si != 1 || c.dst_si != 1) && gather;
  p.path = is_flat ? CopyPath::flat : is_gather ? CopyPath::gather : CopyPath::chunk;
  p.blocks = is_flat     ? (total + COPY_BLOCK - 1) / COPY_BLOCK
             : is_gather ? ((c.n_inner + 63) / 64) * ((c.n_outer + 4 * COPY_GROWS - 1) / (4 * COPY_GROWS))
                         : c.n_outer * ((c.n_inner + COPY_CHUNK - 1) / COPY_CHUNK);
  return p;
}

CopyPlan3 plan_copy3d(const Copy3D& in, int elem_bytes, const ParityShift& par, bool gather) {
  CopyPlan3 p;
  p.box = in;
  const int64_t total = in.n_outer * in.n_mid * in.n_inner;
  if (in.n_outer <= 0 || in.n_mid <= 0 || in.n_inner <= 0) return p;
  const Copy3D c = normalized(in);
  p.box = c;
  const bool is_gather = c.n_inner < 64 && c.n_mid >= 64 && gather;
  const bool is_flat = !is_gather && c.n_inner < 64;
  p.path = is_flat ? CopyPath::flat : is_gather ? CopyPath::gather : CopyPath::chunk;
  if (is_gather && aligned_rows(c, elem_bytes, par)) p.vec_bytes = static_cast<int>(c.n_inner * elem_bytes);
  p.blocks = is_flat     ? (total + COPY_BLOCK - 1) / COPY_BLOCK
             : is_gather ? ((c.n_mid + 63) / 64) * ((c.n_outer + 4 * COPY_GROWS - 1) / (4 * COPY_GROWS))
                         : c.n_outer * c.n_mid * ((c.n_inner + COPY_CHUNK - 1) / COPY_CHUNK);
  return p;
}

// ---------------------------------------------------------------- accumulation

const char* accum_op_name(AccumOp op) {
  switch (op) {
    case AccumOp::Add: return "add";
    case AccumOp::Take: return "take";
    case AccumOp::AddTake: return "add_take";
    case AccumOp::Zero: return "zero";
  }
  return "?";
}

AccumOp accum_op_from_name(const char* name) {
  for (AccumOp op : {AccumOp::Add, AccumOp::Take, AccumOp::AddTake, AccumOp::Zero})
    if (std::strcmp(name, accum_op_name(op)) == 0) return op;
  fail("accum3d: unknown operation '", name, "' (add, take, add_take or zero)");
}

int accum_elem_bytes(AccumType t) {
  switch (t) {
    case AccumType::I8: case AccumType::U8: return 1;
    case AccumType::I16: case AccumType::F16: case AccumType::BF16: return 2;
    case AccumType::F32: case AccumType::I32: return 4;
    case AccumType::F64: case AccumType::I64: case AccumType::C64: return 8;
    case AccumType::C128: return 16;
  }
  fail("accum3d: unknown element type ", static_cast<int>(t));
}

CopyPlan3 plan_accum3d(const Copy3D& in, int elem_bytes, bool gather) {
  CopyPlan3 p = plan_copy3d(in, elem_bytes, ParityShift{}, gather);
  if (p.blocks <= 0 || p.path != CopyPath::chunk) return p;
  const Copy3D& c = p.box;
  auto ok = [&](const char* q, int64_t sm, int64_t so) {
    return reinterpret_cast<uintptr_t>(q) % 16 == 0 && (sm * elem_bytes) % 16 == 0 && (so * elem_bytes) % 16 == 0;
  };
  if (c.src_si == 1 && c.dst_si == 1 && ok(c.src, c.src_sm, c.src_so) && ok(c.dst, c.dst_sm, c.dst_so))
    p.vec_bytes = 16;
  return p;
}

}  // namespace igg
