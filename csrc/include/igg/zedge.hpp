// The z-edge lane rule of the fused diffusion kernels (igg/fused_impl.hpp).
//
// A wave's rows keep their z-face values one per lane: the received halo value
// of row r is loaded by one lane and moved into the edge lane, the send value
// of row r is moved from the edge lane into one lane and stored from there.
// Which lane holds which row, and which side's source and destination a lane
// takes, is written down here for the host and the device:
//   * low edge (z = 0 / 1, edge lane 0): row r in lane r;
//   * high edge (z = n2-1 / n2-2, edge lane zh): row r in lane 32 + r
//     (readlane form), or in lane zh - r (DPP form, ZDPP: one row shift inside
//     the edge lane's 16-lane DPP row reaches it).
// Only rows r < nv exist (a partial last y tile has fewer than RY).
//
// The host side (the launch guards of launch_mode, the bindings'
// fused_zedge_lane that tests/test_fused_zedge_cpu.py enumerates) uses all of
// it. The kernel (hx_sweep) takes from here the side and row of a DPP lane's
// send destination (zedge_side, zedge_row), which is where the two edges can
// meet in one lane; its other lane expressions stay spelled out in place,
// because the register allocation of every fused form moved when they were
// routed through these functions (profiles/fused_z_edges/NOTES.md). They are
// the same expressions; the sweep of tests/test_gpu_fused_z_edges.py holds the
// kernel to them at every lane position.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IGG_ZEDGE_HD __host__ __device__ __forceinline__
#else
#define IGG_ZEDGE_HD inline
#endif

namespace igg {

// Lane of the high z edge (the vector holding n2 - vz) within its wave of
// 64 * vz points, and whether that wave also holds the low edge.
IGG_ZEDGE_HD int zedge_zh(int64_t n2, int vz) { return static_cast<int>(((n2 - vz) % (64 * vz)) / vz); }
IGG_ZEDGE_HD bool zedge_one_wave(int64_t n2, int vz) { return n2 <= 64 * vz + vz; }

// The DPP form needs the high edge's rows (lanes zh - r, r < ry) inside the
// edge lane's 16-lane DPP row, and one z edge per wave.
IGG_ZEDGE_HD bool zedge_dpp_rows_fit(int zh, int ry) { return ry <= 16 && zh % 16 >= ry - 1; }
IGG_ZEDGE_HD bool zedge_dpp_ok(int64_t n2, int vz, int ry) {
  return !zedge_one_wave(n2, vz) && zedge_dpp_rows_fit(zedge_zh(n2, vz), ry);
}

// Side a lane serves (0 low, 1 high, -1 none): lo / hi say whether it holds a
// row of the low / high edge, act_lo / act_hi which sides this wave receives
// from (or sends to). A DPP lane can hold a row of both edges: it serves the
// low side if that is active, else the high side - and takes the row of the
// side it serves (zedge_row: rl of the low edge, rh of the high), never the
// other's.
IGG_ZEDGE_HD int zedge_side(bool lo, bool hi, bool act_lo, bool act_hi) {
  return (lo && act_lo) ? 0 : ((hi && act_hi) ? 1 : -1);
}
IGG_ZEDGE_HD int zedge_row(int side, int rl, int rh) { return side == 1 ? rh : rl; }

// The whole rule for one lane as hx_sweep applies it (host view: the bindings).
struct ZEdgeLane {
  bool lo, hi;       // the lane holds a row of the low / high edge (rows < nv only) ...
  int rl, rh;        // ... namely this one
  int src, src_row;  // side and row of the received value this lane loads (-1: a dummy load)
  int dst, dst_row;  // side and row its send value is stored to (-1: no store)
};

// in_* / out_*: this wave receives from / sends to that z side.
IGG_ZEDGE_HD ZEdgeLane zedge_lane(bool dpp, int lane, int zh, int nv, bool in_lo, bool in_hi, bool out_lo,
                                  bool out_hi) {
  ZEdgeLane z;
  z.rl = lane & 31;
  z.rh = dpp ? zh - lane : z.rl;
  z.lo = lane < 32 && z.rl < nv;
  z.hi = dpp ? (z.rh >= 0 && z.rh < nv) : (lane >= 32 && z.rl < nv);
  z.src = zedge_side(z.lo, z.hi, in_lo, in_hi);
  z.src_row = z.src < 0 ? 0 : zedge_row(z.src, z.rl, z.rh);
  z.dst = zedge_side(z.lo, z.hi, out_lo, out_hi);
  z.dst_row = z.dst < 0 ? 0 : zedge_row(z.dst, z.rl, z.rh);
  return z;
}

}  // namespace igg
