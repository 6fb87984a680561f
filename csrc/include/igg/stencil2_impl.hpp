// Body and launch of the two-step diffusion pass (see stencil2_kernels.hip for
// the scheme), shared by the kernel units that instantiate it:
//   stencil2_kernels.hip   one kernel per (form, dtype): any shape, reads Cp;
//   stencil2q_kernels.hip  the specialisations: tiles that span the row (NOZ:
//                          no z ring, no edge threads) and the quotient input
//                          (QIN: reads Q = dtlam/Cp where the others read Cp).
// Every point goes through diffusion_point_q with the same operands in every
// instantiation, so all of them leave bitwise the same values.
//
// The march over dim 0 keeps no value in a place that depends on the position's
// parity or age: every plane-sized register array has three slots, plane j
// lives in slot (j - first) % 3 from its load or its computation to its last
// use, and the loop body is unrolled over the three phases, so a slot is a
// compile-time index and nothing is moved at the end of a position. T plane
// p+2 is loaded into the slot of plane p-1 after that plane's last use. The LDS
// parts of the intermediate plane are triple-buffered by the same phase. A
// chunk's length need not be a multiple of three: the unrolled group is left
// after any of its positions.
//
// Addresses: one unsigned 32-bit byte offset per lane (its place in the row)
// and wave-uniform row/plane pointers that advance by one plane per position;
// the loop holds no 64-bit multiply and no per-lane 64-bit arithmetic.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "igg/devmath.hpp"
#include "igg/stencil.hpp"
#include "igg/xcd.hpp"

namespace igg {
namespace twostep {

template <typename T>
struct K2Args {
  T* __restrict__ t2;
  const T* __restrict__ t;
  const T* __restrict__ cp;  // QIN kernels: the quotient array
  int64_t n0, n1, n2;
  T rdx2, rdy2, rdz2, dtlam;
  int halo_z;
  int64_t ntz, nty, ch, nblk;
};

template <typename T, int VZ>
struct Vec2 {
  typedef T type __attribute__((ext_vector_type(VZ)));
};

// whether a lane's vector [z0, z0+vz) holds a z-boundary point
__device__ __forceinline__ bool zany_of(int z0, int n2, int vz) { return z0 == 0 || z0 + vz - 1 >= n2 - 1; }

// The value of the lane below / above in the wave (lanes 0 / 63: unspecified,
// the callers replace it): a DPP move of the whole wave by one lane, on the
// VALU, where __shfl_up/__shfl_down go through the LDS crossbar.
template <int CTRL>
__device__ __forceinline__ int lane_shift(int x) {
  return __builtin_amdgcn_mov_dpp(x, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
__device__ __forceinline__ float lane_shift(float x) {
  return __int_as_float(lane_shift<CTRL>(__float_as_int(x)));
}
template <int CTRL>
__device__ __forceinline__ double lane_shift(double x) {
  return __hiloint2double(lane_shift<CTRL>(__double2hiint(x)), lane_shift<CTRL>(__double2loint(x)));
}
template <typename T>
__device__ __forceinline__ T lane_below(T x) { return lane_shift<0x138>(x); }  // wave_shr:1, lane i takes lane i-1
template <typename T>
__device__ __forceinline__ T lane_above(T x) { return lane_shift<0x130>(x); }  // wave_shl:1, lane i takes lane i+1

// Wave-uniform base + per-lane unsigned 32-bit byte offset. The offset is made
// opaque at the access, so that its extension to 64 bits happens there and
// folds into the scalar-base addressing form (global_load v, v_off, s[base]);
// extended once outside the loop it is held as a register pair, and every
// access forms a 64-bit per-lane address with a VALU add.
__device__ __forceinline__ uint32_t here(uint32_t off) {
  asm("" : "+v"(off));
  return off;
}
template <typename X>
__device__ __forceinline__ X ldg(const char* base, uint32_t off) {
  return *reinterpret_cast<const X*>(base + here(off));
}

template <typename T, int BY, int RY, int VZ, int BZ, bool NOZ, bool QIN>
__device__ __forceinline__ void body(const K2Args<T>& a) {
  using V = typename Vec2<T, VZ>::type;
  constexpr int WS = 64 * VZ;  // points of one wave's row segment
  constexpr int W = WS * BZ;
  constexpr int TYE = BY * RY, TYS = TYE - 2;
  constexpr uint32_t ES = sizeof(T);
  static_assert(2 * TYE <= 64, "edge threads live in wave 0");
  // intermediate plane parts shared between waves, [phase of the position]:
  // first / last row of every wave, and per row the values left ([0], z =
  // segment origin - 1) and right ([1], z = segment origin) of every segment
  // boundary j = 0..BZ
  // rows is [3][BY][2][W] behind one row of padding, addressed from one
  // per-lane index: rows[RP * phase + lb + k * W] is, for k = 0..3, the last
  // row of the wave below, this wave's first and last row, and the first row
  // of the wave above (k = 0 / 3 of the first / last wave: padding or the
  // next phase, only ever addressed for the tile's ring rows, which are not
  // computed in stage 3).
  constexpr int RP = BY * 2 * W;
  __shared__ __attribute__((aligned(16))) T rows[3 * RP + 2 * W];
  constexpr int ZR = (BZ + 1) * 2, ZP = TYE * ZR;  // zedge as [3][TYE][BZ + 1][2], flat
  __shared__ T zedge[3 * ZP];

  // Indices and in-plane byte offsets are 32-bit (diffusion3d_twostep_ok: a
  // plane is below 2 GiB); only plane pointers are 64-bit, and wave-uniform.
  int b = static_cast<int>(xcd_remap(blockIdx.x, a.nblk));
  int tz = 0;
  if (!NOZ) {
    const int ntz = static_cast<int>(a.ntz);
    tz = b % ntz;
    b /= ntz;
  }
  const int nty = static_cast<int>(a.nty);
  const int ty = b % nty;
  const int cx = b / nty;

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wz = wid % BZ, wy = wid / BZ;
  const int n0 = static_cast<int>(a.n0), n1 = static_cast<int>(a.n1), n2 = static_cast<int>(a.n2);
  const uint32_t s1b = n2 * ES, s0b = n1 * s1b;  // row / plane stride in bytes
  const int zt = tz * W;          // tile origin
  const int zw = zt + wz * WS;    // segment origin (wave-uniform)
  const int ye0 = ty * TYS;       // first (ring) row of the tile
  const int xs = 1 + cx * static_cast<int>(a.ch);
  const int xe = min(xs + static_cast<int>(a.ch), n0 - 1);

  // Lanes past the row alias its last vector (loads stay in bounds, nothing
  // stored).
  const int z0 = zw + lane * VZ;
  const int zlast = n2 - VZ;
  const int zc = min(z0, zlast);
  const bool zin = z0 < n2;
  // The segment's neighbours along z come from the lane neighbours, except in
  // the wave's edge lanes: lane 0 loads z-1 and lane 63 z+VZ (clamped to the
  // row; a clamped value only ever enters a z-boundary point, which keeps T's
  // value). One masked region serves both: `voe` is the lane's own offset, and
  // i63 selects the lane's side in zedge.
  const bool l0 = lane == 0, l63 = lane == 63, ledge = l0 || l63;
  const int i63 = l63 ? 1 : 0;
  // the edge lane's own side of its segment boundary in zedge, row 0 of the
  // wave: read there, written at the other side (zx + 1 - 2 * i63)
  const int zx = wy * RY * ZR + (wz + i63) * 2 + i63;
  const uint32_t vo = zc * ES;
  const uint32_t voe = (l63 ? min(zc + VZ, n2 - 1) : max(zc - 1, 0)) * ES;
  const int lb = wy * 2 * W + wz * WS + lane * VZ;  // the lane's place in the LDS rows (below)
  const bool vst = zin && (!zany_of(z0, n2, VZ) || a.halo_z);  // the lane stores whole vectors
  bool zb[VZ];  // boundary point along z: the intermediate value is T's
#pragma unroll
  for (int e = 0; e < VZ; ++e) zb[e] = z0 + e == 0 || z0 + e >= n2 - 1;

  // Rows past the array alias row n1-1 (a boundary row: never written).
  uint32_t rowo[RY];  // wave-uniform row offsets (bytes)
  bool rbnd[RY], rout[RY];
#pragma unroll
  for (int r = 0; r < RY; ++r) {
    const int yr = ye0 + wy * RY + r;
    const int lr = wy * RY + r;
    rowo[r] = min(yr, n1 - 1) * s1b;
    rbnd[r] = yr == 0 || yr >= n1 - 1;
    rout[r] = lr >= 1 && lr <= TYE - 2 && yr <= n1 - 2;
  }
  const uint32_t rowm = min(max(ye0 + wy * RY - 1, 0), n1 - 1) * s1b;
  const uint32_t rowp = min(ye0 + wy * RY + RY, n1 - 1) * s1b;

  // z-ring ("edge") threads: thread s*TYE + el forms the intermediate value
  // of tile row el at z = zt-1 (s = 0) or zt+W (s = 1) where that point exists
  const int et = static_cast<int>(threadIdx.x);
  const int es = et / TYE, el = et % TYE;
  const int ez = es == 0 ? zt - 1 : zt + W;
  const bool eact = !NOZ && et < 2 * TYE && (es == 0 ? zt > 0 : zt + W < n2);
  const int eyr = ye0 + el;
  const bool ebnd = eyr == 0 || eyr >= n1 - 1 || ez >= n2 - 1;
  uint32_t eo = 0, eom = 0, eop = 0, eozm = 0, eozp = 0;  // bytes within a plane
  if (eact) {
    const int y = min(eyr, n1 - 1);
    eo = y * s1b + ez * ES;
    eom = eo - (y > 0 ? s1b : 0u);
    eop = eo + (y < n1 - 1 ? s1b : 0u);
    eozm = eo - ES;                              // ez >= W - 1 > 0
    eozp = eo + (ez < n2 - 1 ? ES : 0u);
  }

  const char* const tb0 = reinterpret_cast<const char*>(a.t);
  const char* const cb0 = reinterpret_cast<const char*>(a.cp);
  const T rdx2 = a.rdx2, rdy2 = a.rdy2, rdz2 = a.rdz2, dtlam = a.dtlam;

  // March state, slot = (plane - (xs-1)) % 3: tt = T planes p-1, p, p+1; cq =
  // Cp (QIN: Q) planes, ym/yp/ev = T around the wave's rows and segment,
  // loaded one position ahead; im = intermediate planes p-2, p-1, p; qq =
  // dtlam/Cp of planes p-1, p (QIN: cq itself, which then lives three positions).
  V tt[3][RY], cq[3][RY], im[3][RY], qq[3][RY];
  V ym[3], yp[3];
  T ev[3][RY];
  // Plane pointers of the next position's loads, clamped at the last plane
  // (what is loaded there is unused): T planes p+1 and p+2, Cp plane p+1;
  // oo = byte offset of output plane p-1.
  const char *t1, *t2, *c1;
  int64_t oo;
  {
    const int p = xs - 1;  // >= 0; p+1 = xs <= n0-2
    const int64_t pl = s0b;
    const char* tm = tb0 + max(p - 1, 0) * pl;
    const char* tc = tb0 + p * pl;
    const char* cc = cb0 + p * pl;
    t1 = tc + pl;
    t2 = tb0 + min(p + 2, n0 - 1) * pl;
    c1 = cc + pl;
    oo = (p - 1) * pl;
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      tt[2][r] = ldg<V>(tm + rowo[r], vo);
      tt[0][r] = ldg<V>(tc + rowo[r], vo);
      tt[1][r] = ldg<V>(t1 + rowo[r], vo);
      cq[0][r] = ldg<V>(cc + rowo[r], vo);
      ev[0][r] = T(0);
      im[1][r] = tt[0][r];
      im[2][r] = tt[0][r];
      qq[2][r] = tt[0][r];
      if (QIN) cq[2][r] = tt[0][r];
    }
    if (ledge) {
#pragma unroll
      for (int r = 0; r < RY; ++r) ev[0][r] = ldg<T>(tc + rowo[r], voe);
    }
    ym[0] = ldg<V>(tc + rowm, vo);
    yp[0] = ldg<V>(tc + rowp, vo);
  }

  // One march position at phase PH = (p - (xs-1)) % 3.
  auto position = [&](auto phase, const int p) __attribute__((always_inline)) {
    constexpr int PH = decltype(phase)::value;
    constexpr int SA = (PH + 2) % 3, SB = PH, SN = (PH + 1) % 3;  // slots of planes p-1, p, p+1
    const bool pb = p == 0 || p == n0 - 1;  // boundary plane: intermediate = T

    // 1. intermediate plane p
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      const V& c = tt[SB][r];
      const V& yv = (r == 0) ? ym[SB] : tt[SB][r > 0 ? r - 1 : 0];
      const V& yn = (r == RY - 1) ? yp[SB] : tt[SB][r + 1 < RY ? r + 1 : r];
      T prev = lane_below(c[VZ - 1]);
      T next = lane_above(c[0]);
      if (l0) prev = ev[SB][r];
      if (l63) next = ev[SB][r];
#pragma unroll
      for (int e = 0; e < VZ; ++e) {
        const T zm = e == 0 ? prev : c[e > 0 ? e - 1 : 0];
        const T zp = e == VZ - 1 ? next : c[e + 1 < VZ ? e + 1 : e];
        const T q = QIN ? cq[SB][r][e] : dtlam / cq[SB][r][e];
        if (!QIN) qq[SB][r][e] = q;
        const T v = diffusion_point_q(c[e], tt[SA][r][e], tt[SN][r][e], yv[e], yn[e], zm, zp, q, rdx2, rdy2, rdz2);
        im[SB][r][e] = (pb || rbnd[r] || zb[e]) ? c[e] : v;
      }
    }
    T ein = T(0);
    if (eact) {
      // all seven T values are loaded here (they are in cache: the tile's
      // neighbour reads them as its own points); nothing is kept across
      // positions, the general kernels have no registers to spare
      const char* tc = t1 - (p + 1 <= n0 - 1 ? s0b : 0u);
      const char* cc = c1 - (p + 1 <= n0 - 1 ? s0b : 0u);
      const char* tm = tc - (p > 0 ? s0b : 0u);
      const T etc = ldg<T>(tc, eo);
      const T cpe = ldg<T>(cc, eo);
      const T v = diffusion_point_q(etc, ldg<T>(tm, eo), ldg<T>(t1, eo), ldg<T>(tc, eom), ldg<T>(tc, eop),
                                    ldg<T>(tc, eozm), ldg<T>(tc, eozp), QIN ? cpe : dtlam / cpe, rdx2, rdy2, rdz2);
      ein = (pb || ebnd) ? etc : v;
    }

    // 2. loads of position p+1: T plane p+2 takes the slot of plane p-1
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      tt[SA][r] = ldg<V>(t2 + rowo[r], vo);
      cq[SN][r] = ldg<V>(c1 + rowo[r], vo);
    }
    if (ledge) {
#pragma unroll
      for (int r = 0; r < RY; ++r) ev[SN][r] = ldg<T>(t1 + rowo[r], voe);
    }
    ym[SN] = ldg<V>(t1 + rowm, vo);
    yp[SN] = ldg<V>(t1 + rowp, vo);

    // 3. output plane x = p-1 from intermediate planes p-2, p-1, p
    if (p - 1 >= xs) {
      char* const ob = reinterpret_cast<char*>(a.t2) + oo;
#pragma unroll
      for (int r = 0; r < RY; ++r) {
        const int lr = wy * RY + r;
        if (!rout[r]) continue;  // wave-uniform
        const V& c = im[SA][r];
        V yv, yn;
        if (r == 0) yv = *reinterpret_cast<const V*>(&rows[RP * SA + lb]);
        else yv = im[SA][r > 0 ? r - 1 : 0];
        if (r == RY - 1) yn = *reinterpret_cast<const V*>(&rows[RP * SA + lb + 3 * W]);
        else yn = im[SA][r + 1 < RY ? r + 1 : r];
        T prev = lane_below(c[VZ - 1]);
        T next = lane_above(c[0]);
        const T zv = zedge[ZP * SA + r * ZR + zx];  // every lane reads; the edge lanes use it
        if (l0) prev = zv;
        if (l63) next = zv;
        V out;
#pragma unroll
        for (int e = 0; e < VZ; ++e) {
          const T zm = e == 0 ? prev : c[e > 0 ? e - 1 : 0];
          const T zp = e == VZ - 1 ? next : c[e + 1 < VZ ? e + 1 : e];
          const T q = QIN ? cq[SA][r][e] : qq[SA][r][e];
          const T v = diffusion_point_q(c[e], im[SN][r][e], im[SB][r][e], yv[e], yn[e], zm, zp, q, rdx2, rdy2, rdz2);
          out[e] = zb[e] ? c[e] : v;  // z boundary: T's value (written only with halo_z)
        }
        T* dst = reinterpret_cast<T*>(ob + rowo[r] + here(vo));
        if (vst) {
          __builtin_nontemporal_store(out, reinterpret_cast<V*>(dst));
        } else if (zin) {
#pragma unroll
          for (int e = 0; e < VZ; ++e)
            if (!zb[e]) dst[e] = out[e];
        }
      }
    }

    // 4. the shared parts of intermediate plane p
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      if (r == 0) *reinterpret_cast<V*>(&rows[RP * SB + lb + W]) = im[SB][r];
      if (r == RY - 1) *reinterpret_cast<V*>(&rows[RP * SB + lb + 2 * W]) = im[SB][r];
    }
    if (ledge) {
      // formed here from zx, not held in a register of its own across the march
      const int zo = static_cast<int>(here(static_cast<uint32_t>(zx))) + 1 - 2 * i63;
#pragma unroll
      for (int r = 0; r < RY; ++r) zedge[ZP * SB + r * ZR + zo] = l63 ? im[SB][r][VZ - 1] : im[SB][r][0];
    }
    if (eact) zedge[ZP * SB + el * ZR + (es == 0 ? 0 : BZ * 2 + 1)] = ein;
    __syncthreads();

    // the plane pointers of position p+1
    t1 = t2;
    if (p + 3 <= n0 - 1) t2 += s0b;
    if (p + 2 <= n0 - 1) c1 += s0b;
    oo += s0b;
  };

  for (int p = xs - 1;;) {
    position(std::integral_constant<int, 0>{}, p);
    if (p == xe) break;
    ++p;
    position(std::integral_constant<int, 1>{}, p);
    if (p == xe) break;
    ++p;
    position(std::integral_constant<int, 2>{}, p);
    if (p == xe) break;
    ++p;
  }
}

// Points along dim 2 of one workgroup tile.
template <typename T, int BZ>
constexpr int tile_width() {
  return 64 * (16 / static_cast<int>(sizeof(T))) * BZ;
}

template <typename T, int BY, int RY, int BZ, typename Kern>
void launch_form(Kern kern, const DiffusionArgs& a, bool qin, hipStream_t stream) {
  constexpr int W = tile_width<T, BZ>(), TYS = BY * RY - 2, BLOCK = 64 * BY * BZ;
  K2Args<T> k;
  k.t2 = reinterpret_cast<T*>(a.t2);
  k.t = reinterpret_cast<const T*>(a.t);
  k.cp = reinterpret_cast<const T*>(qin ? a.q : a.cp);
  k.n0 = a.n[0]; k.n1 = a.n[1]; k.n2 = a.n[2];
  k.rdx2 = static_cast<T>(a.rd2[0]);
  k.rdy2 = static_cast<T>(a.rd2[1]);
  k.rdz2 = static_cast<T>(a.rd2[2]);
  k.dtlam = static_cast<T>(a.dt_lam);
  k.halo_z = a.halo_z ? 1 : 0;
  k.ntz = (k.n2 + W - 1) / W;
  k.nty = (k.n1 - 2 + TYS - 1) / TYS;
  // Equal x chunks so that the grid is about `rounds` residency rounds; a
  // chunk pays a two-position lead-in, so it is at least 4 planes long.
  const int64_t len0 = k.n0 - 2, tiles = k.ntz * k.nty;
  const int64_t target = diffusion3d_target_blocks(reinterpret_cast<const void*>(kern), BLOCK, a.rounds);
  const int64_t ch_min = std::max<int64_t>(std::min<int64_t>(4, len0), (len0 * tiles + target - 1) / target);
  const int64_t nch = std::max<int64_t>(1, len0 / ch_min);
  k.ch = (len0 + nch - 1) / nch;
  k.nblk = tiles * ((len0 + k.ch - 1) / k.ch);
  if (k.nblk > 0x7fffffffLL) fail("diffusion3d_twostep: grid too large");
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(k.nblk)), dim3(BLOCK), 0, stream, k);
  IGG_HIP_CHECK(hipGetLastError());
}

}  // namespace twostep

// stencil2q_kernels.hip: the launch of a tile that spans the row (n2 <= the
// form's tile width) and/or of the quotient input (a.q != 0).
void launch_diffusion3d_twostep_special(const DiffusionArgs& a, hipStream_t stream);

}  // namespace igg
