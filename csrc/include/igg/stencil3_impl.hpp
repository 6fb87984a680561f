// Body and launch of the three-step diffusion pass (scheme: stencil3_kernels.hip).
// It is the two-step march of stencil2_impl.hpp with one more stage, for the
// case that kernel's NOZ/QIN specialisation runs: the tile spans the row (no z
// ring, no edge threads) and the pass reads Q = dtlam/Cp (no division). Every
// point goes through diffusion_point_q with the operands of the single-step
// kernel, so the pass leaves bitwise the values of three single steps.
//
// As there, every plane-sized register array has three slots, plane j lives in
// slot (j - first) % 3, and the loop body is unrolled over the three phases.
// Within a position the work goes row by row - intermediate-1 (p), then
// intermediate-2 (p-1, tile rows 1 .. TYE-2 only), then output (p-2, tile rows
// 2 .. TYE-3 only) of row r - and the loads of the next
// position follow the last use of the row they replace (T plane p+2 after
// stage 1, Q plane p+1 after stage 3), so of each intermediate field and of Q
// two planes and one row are live, not three planes and a fourth of Q.
#pragma once

#include "igg/stencil2_impl.hpp"

namespace igg {
namespace threestep {

using twostep::here;
using twostep::K2Args;
using twostep::lane_above;
using twostep::lane_below;
using twostep::ldg;
using twostep::Vec2;

// The value of the lane below / above in the wave, as lane_below / lane_above,
// but lane 0 / lane 63, which has no such neighbour, keeps `old`: the DPP move
// leaves its destination alone where the source lane does not exist.
template <int CTRL>
__device__ __forceinline__ int lane_shift_keep(int old, int x) {
  return __builtin_amdgcn_update_dpp(old, x, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float lane_shift_keep(float old, float x) {
  return __int_as_float(lane_shift_keep<CTRL>(__float_as_int(old), __float_as_int(x)));
}
template <int CTRL>
__device__ __forceinline__ double lane_shift_keep(double old, double x) {
  return __hiloint2double(lane_shift_keep<CTRL>(__double2hiint(old), __double2hiint(x)),
                          lane_shift_keep<CTRL>(__double2loint(old), __double2loint(x)));
}

// A chunk marches four positions before its first output plane; the shortest
// chunk worth that lead-in.
constexpr int MIN_CHUNK = 8;

template <typename T, int BY, int RY, int VZ, int BZ>
__device__ __forceinline__ void body(const K2Args<T>& a) {
  using V = typename Vec2<T, VZ>::type;
  constexpr int WS = 64 * VZ;  // points of one wave's row segment
  constexpr int W = WS * BZ;
  constexpr int TYE = BY * RY, TYS = TYE - 4;
  constexpr uint32_t ES = sizeof(T);
  static_assert(TYE > 4, "a tile writes TYE - 4 rows");
  static_assert(RY >= 2, "the edge values are loaded in two parts: the first RY / 2 rows, then the rest");
  // The parts of the two intermediate fields shared between waves, laid out as
  // in the two-step body: rowsN is [3][BY][2][W] behind one row of padding
  // (rowsN[RP * slot + lb + k * W], k = 0..3: the last row of the wave below,
  // this wave's first and last row, the first row of the wave above; k = 0 / 3
  // of the first / last wave is padding or another slot, never read: the tile's
  // outer rows take part in stage 1 only), zedgeN is [3][TYE][BZ + 1][2]: per
  // row the values left ([0]) and right ([1]) of every segment boundary.
  constexpr int RP = BY * 2 * W;
  __shared__ __attribute__((aligned(16))) T rows1[3 * RP + 2 * W];
  __shared__ __attribute__((aligned(16))) T rows2[3 * RP + 2 * W];
  constexpr int ZR = (BZ + 1) * 2, ZP = TYE * ZR;
  __shared__ T zedge1[3 * ZP];
  __shared__ T zedge2[3 * ZP];

  // Indices and in-plane byte offsets are 32-bit (diffusion3d_threestep_ok: a
  // plane is below 2 GiB); only plane pointers are 64-bit, and wave-uniform.
  const int b = static_cast<int>(xcd_remap(blockIdx.x, a.nblk));
  const int nty = static_cast<int>(a.nty);
  const int ty = b % nty;
  const int cx = b / nty;

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // Wave wid takes rows wy * RY .. of the tile and segment wz of the row; the
  // odd wy take their segments rotated by BZ/2. Waves s and s + 4 usually share
  // a SIMD, and the workgroup moves at the pace of its slowest SIMD (one barrier
  // per position): so a wave that holds an end of the row, the only kind that
  // selects (`wplain` below), shares its SIMD with one that holds none.
  const int wy = wid / BZ, wz = (wid + (wy & 1) * (BZ / 2)) % BZ;
  const int n0 = static_cast<int>(a.n0), n1 = static_cast<int>(a.n1), n2 = static_cast<int>(a.n2);
  const uint32_t s1b = n2 * ES, s0b = n1 * s1b;  // row / plane stride in bytes
  const int zw = wz * WS;                        // segment origin (wave-uniform)
  const int ye0 = ty * TYS - 1;                  // first ring row of the tile: rows ye0+2 .. ye0+TYE-3 are written
  const int xs = 1 + cx * static_cast<int>(a.ch);
  const int xe = min(xs + static_cast<int>(a.ch), n0 - 1);
  const int p0 = max(xs - 2, 0);  // first march position

  // Lanes past the row alias its last vector (loads stay in bounds, nothing
  // stored).
  const int z0 = zw + lane * VZ;
  const int zc = min(z0, n2 - VZ);
  const bool zin = z0 < n2;
  // T's z neighbours of the wave's edge lanes are loaded (lane 0: z-1, lane
  // 63: z+VZ, clamped to the row: a clamped value only enters a z-boundary
  // point, which keeps T's value); those of the intermediate fields come from
  // zedgeN, where i63 selects the lane's side.
  const bool l63 = lane == 63, ledge = ((lane + 1) & 63) < 2;  // ledge: lane 0 or 63, one compare
  const int i63 = l63 ? 1 : 0;
  const int zx = wy * RY * ZR + (wz + i63) * 2 + i63;  // read here, written at zx + 1 - 2 * i63
  const uint32_t vo = zc * ES;
  const uint32_t voe = (l63 ? min(zc + VZ, n2 - 1) : max(zc - 1, 0)) * ES;
  const int lb = wy * 2 * W + wz * WS + lane * VZ;  // the lane's place in the LDS rows
  const bool vst = zin && (!twostep::zany_of(z0, n2, VZ) || a.halo_z);  // the lane stores whole vectors
  const bool wvst = __ballot(zin && !vst) == 0;  // ... and so does every lane of the wave that stores at all
  bool zb[VZ];  // boundary point along z: both intermediate values are T's
#pragma unroll
  for (int e = 0; e < VZ; ++e) zb[e] = z0 + e == 0 || z0 + e >= n2 - 1;

  // Rows outside the array alias row 0 / n1-1 (boundary rows: never written).
  uint32_t rowo[RY];  // wave-uniform row offsets (bytes)
  uint32_t rbnd = 0, rout = 0;  // bit r: row r is a boundary row / is written
#pragma unroll
  for (int r = 0; r < RY; ++r) {
    const int yr = ye0 + wy * RY + r;
    const int lr = wy * RY + r;
    rowo[r] = min(max(yr, 0), n1 - 1) * s1b;
    rbnd |= (yr <= 0 || yr >= n1 - 1 ? 1u : 0u) << r;
    rout |= (lr >= 2 && lr <= TYE - 3 && yr <= n1 - 2 ? 1u : 0u) << r;
  }
  // Stage 2 (intermediate-2) is wanted on tile rows 1 .. TYE-2, stage 3 on rows
  // 2 .. TYE-3: row 0 of the first wave along y and row RY-1 of the last are
  // formed in stage 1 alone, and nothing of them is shared.
  const bool ylo = wy != 0, yhi = wy != BY - 1;
  // The plain class of waves: no lane holds an end of the row (z = 0 or n2-1)
  // and no row is a boundary row, so on an inner plane no point of the wave
  // keeps T's value. Lanes past the row do not count: no value of theirs
  // reaches a stored point.
  uint64_t zbm[VZ], zanym = 0;  // zb as lane masks: what the selects take
#pragma unroll
  for (int e = 0; e < VZ; ++e) zanym |= zbm[e] = __ballot(zb[e]);
  const bool wplain = (zanym & __ballot(zin)) == 0 && rbnd == 0;
  const uint32_t rowm = min(max(ye0 + wy * RY - 1, 0), n1 - 1) * s1b;
  const uint32_t rowp = min(max(ye0 + wy * RY + RY, 0), n1 - 1) * s1b;

  const char* const tb0 = reinterpret_cast<const char*>(a.t);
  const char* const qb0 = reinterpret_cast<const char*>(a.cp);
  const T rdx2 = a.rdx2, rdy2 = a.rdy2, rdz2 = a.rdz2;

  // March state, slot = (plane - p0) % 3: tt = T planes p-1, p, p+1; qq = Q
  // planes p-2 .. p (p+1 row by row into the slot of p-2); i1 = intermediate-1
  // planes p-2, p-1, p; i2 = intermediate-2 planes p-3, p-2, p-1. ym/yp/ev = T
  // of plane p around the wave's rows and segment: one slot, reloaded for plane
  // p+1 behind its use.
  V tt[3][RY], qq[3][RY], i1[3][RY], i2[3][RY];
  V ym, yp;
  T ev[RY];
  // Plane pointers of the next position's loads, clamped at the last plane
  // (what is loaded there is unused): T planes p+1 and p+2, Q plane p+1; oo =
  // byte offset of output plane p-2.
  const char *t1, *t2, *q1;
  int64_t oo;
  {
    const int64_t pl = s0b;
    const char* tm = tb0 + max(p0 - 1, 0) * pl;
    const char* tc = tb0 + p0 * pl;
    const char* qc = qb0 + p0 * pl;
    t1 = tc + pl;  // p0 + 1 <= n0 - 1
    t2 = tb0 + min(p0 + 2, n0 - 1) * pl;
    q1 = qc + pl;
    oo = (p0 - 2) * pl;
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      tt[2][r] = ldg<V>(tm + rowo[r], vo);
      tt[0][r] = ldg<V>(tc + rowo[r], vo);
      tt[1][r] = ldg<V>(t1 + rowo[r], vo);
      qq[0][r] = ldg<V>(qc + rowo[r], vo);
      ev[r] = T(0);
      // planes before the chunk: never used by a value that is stored
      qq[1][r] = qq[2][r] = tt[0][r];
      i1[1][r] = i1[2][r] = tt[0][r];
      i2[0][r] = i2[1][r] = i2[2][r] = tt[0][r];
    }
    if (ledge) {
#pragma unroll
      for (int r = 0; r < RY; ++r) ev[r] = ldg<T>(tc + rowo[r], voe);
    }
    ym = ldg<V>(tc + rowm, vo);
    yp = ldg<V>(tc + rowp, vo);
  }

  // One stencil update of row r of a plane held in registers `cc` (its x
  // neighbours xm / xp), whose parts beyond the wave come from `yv` / `yn`
  // (rows) and `zl` (the edge lanes' z neighbour). A point on the boundary keeps
  // c: a z-boundary point by a select on its lane mask, a boundary plane or row
  // (`keep`, wave-uniform) as a whole. A `plain` update (wave-uniform) holds no
  // such point and skips both: one scalar branch where the selects were. The
  // empty asm statements cannot be speculated, which keeps the compiler from
  // folding the branches back into selects that every wave would execute.
  auto update = [&](bool plain, const V& c, const V& xm, const V& xp, const V& yv, const V& yn, T zl, const V& q,
                    bool keep) __attribute__((always_inline)) {
    const T prev = lane_shift_keep<0x138>(zl, c[VZ - 1]);  // wave_shr:1, lane 0 keeps zl
    const T next = lane_shift_keep<0x130>(zl, c[0]);       // wave_shl:1, lane 63 keeps zl
    V out;
#pragma unroll
    for (int e = 0; e < VZ; ++e) {
      const T zm = e == 0 ? prev : c[e > 0 ? e - 1 : 0];
      const T zp = e == VZ - 1 ? next : c[e + 1 < VZ ? e + 1 : e];
      out[e] = diffusion_point_q(c[e], xm[e], xp[e], yv[e], yn[e], zm, zp, q[e], rdx2, rdy2, rdz2);
    }
    if (!plain) {  // wave-uniform
      asm volatile("");
#pragma unroll
      for (int e = 0; e < VZ; ++e) out[e] = __builtin_amdgcn_inverse_ballot_w64(zbm[e]) ? c[e] : out[e];
      if (keep) {  // rare
        asm volatile("");
        out = c;
      }
    }
    return out;
  };

  // One march position at phase PH = (p - p0) % 3.
  auto position = [&](auto phase, const int p) __attribute__((always_inline)) {
    constexpr int PH = decltype(phase)::value;
    const bool plain = wplain && p > 1 && p < n0 - 1;  // neither stage 1 nor stage 2 is on a boundary plane
    constexpr int SA = (PH + 2) % 3, SB = PH, SN = (PH + 1) % 3;  // slots of planes p-1 (and p-4), p (p-3), p+1 (p-2)
    const bool pb1 = p <= 0 || p >= n0 - 1;      // boundary plane: the intermediate value is T's
    const bool pb2 = p - 1 <= 0 || p >= n0;
    const bool st = p - 2 >= xs;                 // output plane p-2 belongs to the chunk
    char* const ob = reinterpret_cast<char*>(a.t2) + oo;
    // the edge lane's place in zedgeN to write, formed here from zx
    const int zo = static_cast<int>(here(static_cast<uint32_t>(zx))) + 1 - 2 * i63;

#pragma unroll
    for (int r = 0; r < RY; ++r) {
      // 1. intermediate-1 plane p, then T plane p+2 into the slot of plane p-1
      {
        const V& yv = (r == 0) ? ym : tt[SB][r > 0 ? r - 1 : 0];
        const V& yn = (r == RY - 1) ? yp : tt[SB][r + 1 < RY ? r + 1 : r];
        i1[SB][r] = update(plain, tt[SB][r], tt[SA][r], tt[SN][r], yv, yn, ev[r], qq[SB][r], pb1 | ((rbnd >> r) & 1) != 0);
        tt[SA][r] = ldg<V>(t2 + rowo[r], vo);
        // T of plane p+1 around the wave's rows and segment, behind the use of plane p's
        if (r == 0) ym = ldg<V>(t1 + rowm, vo);
        if (r == RY - 1) yp = ldg<V>(t1 + rowp, vo);
        if (r == RY / 2 - 1 && ledge) {
#pragma unroll
          for (int h = 0; h < RY / 2; ++h) ev[h] = ldg<T>(t1 + rowo[h], voe);
        }
      }
      // 2. intermediate-2 plane p-1 from intermediate-1 planes p-2, p-1, p; not
      // for the tile's outer rows (wave-uniform), whose intermediate-1 values
      // no other wave reads either
      if ((r > 0 || ylo) && (r < RY - 1 || yhi)) {
        if (r == 0) *reinterpret_cast<V*>(&rows1[RP * SB + lb + W]) = i1[SB][r];
        if (r == RY - 1) *reinterpret_cast<V*>(&rows1[RP * SB + lb + 2 * W]) = i1[SB][r];
        V yv, yn;
        if (r == 0) yv = *reinterpret_cast<const V*>(&rows1[RP * SA + lb]);
        else yv = i1[SA][r > 0 ? r - 1 : 0];
        if (r == RY - 1) yn = *reinterpret_cast<const V*>(&rows1[RP * SA + lb + 3 * W]);
        else yn = i1[SA][r + 1 < RY ? r + 1 : r];
        const T zl = zedge1[ZP * SA + r * ZR + zx];  // every lane reads; the edge lanes use it
        i2[SA][r] = update(plain, i1[SA][r], i1[SN][r], i1[SB][r], yv, yn, zl, qq[SA][r], pb2 | ((rbnd >> r) & 1) != 0);
        if (r == 0) *reinterpret_cast<V*>(&rows2[RP * SA + lb + W]) = i2[SA][r];
        if (r == RY - 1) *reinterpret_cast<V*>(&rows2[RP * SA + lb + 2 * W]) = i2[SA][r];
      }
      // 3. output plane p-2 from intermediate-2 planes p-3, p-2, p-1
      if (st && ((rout >> r) & 1) != 0) {  // wave-uniform
        V yv, yn;
        if (r == 0) yv = *reinterpret_cast<const V*>(&rows2[RP * SN + lb]);
        else yv = i2[SN][r > 0 ? r - 1 : 0];
        if (r == RY - 1) yn = *reinterpret_cast<const V*>(&rows2[RP * SN + lb + 3 * W]);
        else yn = i2[SN][r + 1 < RY ? r + 1 : r];
        const T zl = zedge2[ZP * SN + r * ZR + zx];
        // z boundary: T's value (written only with halo_z)
        const V out = update(plain, i2[SN][r], i2[SB][r], i2[SA][r], yv, yn, zl, qq[SN][r], false);
        T* dst = reinterpret_cast<T*>(ob + rowo[r] + here(vo));
        if (wvst) {  // wave-uniform: one masked region
          if (vst) __builtin_nontemporal_store(out, reinterpret_cast<V*>(dst));
        } else if (vst) {
          __builtin_nontemporal_store(out, reinterpret_cast<V*>(dst));
        } else if (zin) {
#pragma unroll
          for (int e = 0; e < VZ; ++e)
            if (!zb[e]) dst[e] = out[e];
        }
      }
      // Q plane p+1 into the slot of plane p-2
      qq[SN][r] = ldg<V>(q1 + rowo[r], vo);
    }
    // the edge lanes, one masked region: the other half of the edge values of
    // plane p+1, and their own values of both new planes for the neighbours.
    // Stage 2 reads intermediate-1 on tile rows 1 .. TYE-2, stage 3 reads
    // intermediate-2 on rows 2 .. TYE-3: `cls` = which of ylo (1) / yhi (2) a
    // row of the wave needs to be among them.
    if (ledge) {
#pragma unroll
      for (int h = RY / 2; h < RY; ++h) ev[h] = ldg<T>(t1 + rowo[h], voe);
      auto share = [&](auto cls) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < RY; ++r) {
          if ((r < 1 ? 1 : 0) + (r > RY - 2 ? 2 : 0) == decltype(cls)::value)
            zedge1[ZP * SB + r * ZR + zo] = l63 ? i1[SB][r][VZ - 1] : i1[SB][r][0];
          if ((r < 2 ? 1 : 0) + (r > RY - 3 ? 2 : 0) == decltype(cls)::value)
            zedge2[ZP * SA + r * ZR + zo] = l63 ? i2[SA][r][VZ - 1] : i2[SA][r][0];
        }
      };
      share(std::integral_constant<int, 0>{});
      if (ylo) share(std::integral_constant<int, 1>{});
      if (yhi) share(std::integral_constant<int, 2>{});
      if (ylo && yhi) share(std::integral_constant<int, 3>{});
    }
    __syncthreads();

    // the plane pointers of position p+1
    t1 = t2;
    if (p + 3 <= n0 - 1) t2 += s0b;
    if (p + 2 <= n0 - 1) q1 += s0b;
    oo += s0b;
  };

  // the last output plane xe-1 is formed at position xe+1
  for (int p = p0;;) {
    position(std::integral_constant<int, 0>{}, p);
    if (p == xe + 1) break;
    ++p;
    position(std::integral_constant<int, 1>{}, p);
    if (p == xe + 1) break;
    ++p;
    position(std::integral_constant<int, 2>{}, p);
    if (p == xe + 1) break;
    ++p;
  }
}

// The same march with Q parked in LDS. A Q value is used three times - by
// stage 1 at position p, stage 2 at p+1 and stage 3 at p+2 - and only by the
// lane that loaded it. So the lane keeps in registers only the plane stage 1
// reads, stores each value after stage 1 into a slot of its own (qslot[plane
// parity][tile row][thread]) and reads it back for stages 2 and 3: no barrier,
// nothing shared. T's values beyond a wave's rows and segment travel through
// LDS as those of the intermediate fields do. The registers that frees buy a
// taller tile (RY = 5 at 16 bytes per lane); RY may be odd.
template <typename T, int BY, int RY, int VZ, int BZ>
__device__ __forceinline__ void body_qlds(const K2Args<T>& a) {
  using V = typename Vec2<T, VZ>::type;
  constexpr int WS = 64 * VZ;  // points of one wave's row segment
  constexpr int W = WS * BZ;
  constexpr int TYE = BY * RY, TYS = TYE - 4;
  constexpr uint32_t ES = sizeof(T);
  static_assert(TYE > 4, "a tile writes TYE - 4 rows");
  static_assert(BY >= 2, "the row buffers hold the rows between waves");
  // The parts of T (0) and of the two intermediate fields (1, 2) shared between
  // waves. rowsN is [3][BY - 1][2][W]: per pair of neighbouring waves the last
  // row of the lower and the first row of the upper one (rowsN[RP * slot + lb +
  // k * W], k = 0..3: the last row of the wave below, this wave's first and
  // last row, the first row of the wave above; the first / last wave along y
  // has no k = 0, 1 / k = 2, 3 and never touches them: the tile's outer rows
  // take part in stage 1 only). zedgeN is [3][TYE][BZ + 1][2]: per row the
  // values left ([0]) and right ([1]) of every segment boundary. T's parts are
  // written one position ahead, from the registers that hold plane p+1, so of
  // T around the wave's rows and segment only the row beyond the tile is loaded
  // (yo).
  constexpr int RP = (BY - 1) * 2 * W;
  constexpr int ZR = (BZ + 1) * 2, ZP = TYE * ZR;
  // The parked Q values, [2][TYE - 2][W]: plane parity, tile row 1 .. TYE-2 (the
  // rows stages 2 and 3 run on), the thread's vector. Plane p overwrites plane
  // p-2 row by row, each row behind the read of its stage-3 operand.
  constexpr int QP = (TYE - 2) * W;
  // One array, the small parts first, so that one address register per kind of
  // index reaches most of them through the instructions' offsets.
  constexpr int ZB = (9 * ZP + VZ - 1) / VZ * VZ;
  __shared__ __attribute__((aligned(16))) T pool[ZB + 9 * RP + 2 * QP];
  T* const zedge0 = pool;
  T* const zedge1 = pool + 3 * ZP;
  T* const zedge2 = pool + 6 * ZP;
  T* const rows1 = pool + ZB;
  T* const rows2 = pool + ZB + 3 * RP;
  T* const rows0 = pool + ZB + 6 * RP;
  T* const qslot = pool + ZB + 9 * RP;

  // Indices and in-plane byte offsets are 32-bit (diffusion3d_threestep_ok: a
  // plane is below 2 GiB); only plane pointers are 64-bit, and wave-uniform.
  const int b = static_cast<int>(xcd_remap(blockIdx.x, a.nblk));
  const int nty = static_cast<int>(a.nty);
  const int ty = b % nty;
  const int cx = b / nty;

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // Wave wid takes rows wy * RY .. of the tile and segment wz of the row; the
  // odd wy take their segments rotated by BZ/2. Waves s and s + 4 usually share
  // a SIMD, and the workgroup moves at the pace of its slowest SIMD (one barrier
  // per position): so a wave that holds an end of the row, the only kind that
  // selects (`wplain` below), shares its SIMD with one that holds none.
  const int wy = wid / BZ, wz = (wid + (wy & 1) * (BZ / 2)) % BZ;
  const int n0 = static_cast<int>(a.n0), n1 = static_cast<int>(a.n1), n2 = static_cast<int>(a.n2);
  const uint32_t s1b = n2 * ES, s0b = n1 * s1b;  // row / plane stride in bytes
  const int zw = wz * WS;                        // segment origin (wave-uniform)
  const int ye0 = ty * TYS - 1;                  // first ring row of the tile: rows ye0+2 .. ye0+TYE-3 are written
  const int xs = 1 + cx * static_cast<int>(a.ch);
  const int xe = min(xs + static_cast<int>(a.ch), n0 - 1);
  const int p0 = max(xs - 2, 0);  // first march position

  // Lanes past the row alias its last vector (loads stay in bounds, nothing
  // stored).
  const int z0 = zw + lane * VZ;
  const int zc = min(z0, n2 - VZ);
  const bool zin = z0 < n2;
  // The z neighbours of the wave's edge lanes come from zedgeN, where i63
  // selects the lane's side (beyond an end of the row: whatever is there; it
  // only enters a z-boundary point, which keeps T's value).
  const bool l63 = lane == 63, ledge = ((lane + 1) & 63) < 2;  // ledge: lane 0 or 63, one compare
  const int i63 = l63 ? 1 : 0;
  const int zx = wy * RY * ZR + (wz + i63) * 2 + i63;  // read here, written at zx + 1 - 2 * i63
  const uint32_t vo = zc * ES;
  const int lb = (wy * 2 - 2) * W + wz * WS + lane * VZ;  // the lane's place in the LDS rows
  // the lane's Q slot of its row 0 at parity 0 (tile row wy * RY is slot row wy * RY - 1)
  const int qb = (wy * RY - 1) * W + wz * WS + lane * VZ;
  const bool vst = zin && (!twostep::zany_of(z0, n2, VZ) || a.halo_z);  // the lane stores whole vectors
  const bool wvst = __ballot(zin && !vst) == 0;  // ... and so does every lane of the wave that stores at all
  bool zb[VZ];  // boundary point along z: both intermediate values are T's
#pragma unroll
  for (int e = 0; e < VZ; ++e) zb[e] = z0 + e == 0 || z0 + e >= n2 - 1;

  // Rows outside the array alias row 0 / n1-1 (boundary rows: never written).
  uint32_t rowo[RY];  // wave-uniform row offsets (bytes)
  uint32_t rbnd = 0, rout = 0;  // bit r: row r is a boundary row / is written
#pragma unroll
  for (int r = 0; r < RY; ++r) {
    const int yr = ye0 + wy * RY + r;
    const int lr = wy * RY + r;
    rowo[r] = min(max(yr, 0), n1 - 1) * s1b;
    rbnd |= (yr <= 0 || yr >= n1 - 1 ? 1u : 0u) << r;
    rout |= (lr >= 2 && lr <= TYE - 3 && yr <= n1 - 2 ? 1u : 0u) << r;
  }
  // Stage 2 (intermediate-2) is wanted on tile rows 1 .. TYE-2, stage 3 on rows
  // 2 .. TYE-3: row 0 of the first wave along y and row RY-1 of the last are
  // formed in stage 1 alone, and nothing of them is shared.
  const bool ylo = wy != 0, yhi = wy != BY - 1;
  // The plain class of waves: no lane holds an end of the row (z = 0 or n2-1)
  // and no row is a boundary row, so on an inner plane no point of the wave
  // keeps T's value. Lanes past the row do not count: no value of theirs
  // reaches a stored point.
  uint64_t zbm[VZ], zanym = 0;  // zb as lane masks: what the selects take
#pragma unroll
  for (int e = 0; e < VZ; ++e) zanym |= zbm[e] = __ballot(zb[e]);
  const bool wplain = (zanym & __ballot(zin)) == 0 && rbnd == 0;
  const uint32_t rowm = min(max(ye0 + wy * RY - 1, 0), n1 - 1) * s1b;
  const uint32_t rowp = min(max(ye0 + wy * RY + RY, 0), n1 - 1) * s1b;

  const char* const tb0 = reinterpret_cast<const char*>(a.t);
  const char* const qb0 = reinterpret_cast<const char*>(a.cp);
  const T rdx2 = a.rdx2, rdy2 = a.rdy2, rdz2 = a.rdz2;

  // March state, slot = (plane - p0) % 3: tt = T planes p-1, p, p+1; i1 =
  // intermediate-1 planes p-2, p-1, p; i2 = intermediate-2 planes p-3, p-2,
  // p-1. qq = Q of plane p (p+1 row by row behind stage 2); planes p-1 and p-2
  // are in qslot, at parity offsets QP - qo and qo, qo = (p & 1) * QP. yo = T of
  // plane p in the row beyond the tile (the first and the last wave along y
  // have one), reloaded for plane p+1 behind its use.
  V tt[3][RY], qq[RY], i1[3][RY], i2[3][RY];
  int qo = (p0 & 1) * QP;  // wave-uniform
  V yo;
  // Plane pointers of the next position's loads, clamped at the last plane
  // (what is loaded there is unused): T planes p+1 and p+2, Q plane p+1; oo =
  // byte offset of output plane p-2.
  const char *t1, *t2, *q1;
  int64_t oo;
  {
    const int64_t pl = s0b;
    const char* tm = tb0 + max(p0 - 1, 0) * pl;
    const char* tc = tb0 + p0 * pl;
    const char* qc = qb0 + p0 * pl;
    t1 = tc + pl;  // p0 + 1 <= n0 - 1
    t2 = tb0 + min(p0 + 2, n0 - 1) * pl;
    q1 = qc + pl;
    oo = (p0 - 2) * pl;
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      tt[2][r] = ldg<V>(tm + rowo[r], vo);
      tt[0][r] = ldg<V>(tc + rowo[r], vo);
      tt[1][r] = ldg<V>(t1 + rowo[r], vo);
      qq[r] = ldg<V>(qc + rowo[r], vo);
      // planes before the chunk: never used by a value that is stored (of Q:
      // whatever qslot holds; every stored value's Q was parked by this march)
      i1[1][r] = i1[2][r] = tt[0][r];
      i2[0][r] = i2[1][r] = i2[2][r] = tt[0][r];
    }
    yo = ldg<V>(tc + (ylo ? rowp : rowm), vo);
    // the shared parts of T's first plane
    if (ylo) *reinterpret_cast<V*>(&rows0[lb + W]) = tt[0][0];
    if (yhi) *reinterpret_cast<V*>(&rows0[lb + 2 * W]) = tt[0][RY - 1];
    if (ledge) {
#pragma unroll
      for (int r = 0; r < RY; ++r) zedge0[r * ZR + zx + 1 - 2 * i63] = l63 ? tt[0][r][VZ - 1] : tt[0][r][0];
    }
    __syncthreads();
  }

  // One stencil update of row r of a plane held in registers `cc` (its x
  // neighbours xm / xp), whose parts beyond the wave come from `yv` / `yn`
  // (rows) and `zl` (the edge lanes' z neighbour). A point on the boundary keeps
  // c: a z-boundary point by a select on its lane mask, a boundary plane or row
  // (`keep`, wave-uniform) as a whole. A `plain` update (wave-uniform) holds no
  // such point and skips both: one scalar branch where the selects were. The
  // empty asm statements cannot be speculated, which keeps the compiler from
  // folding the branches back into selects that every wave would execute.
  auto update = [&](bool plain, const V& c, const V& xm, const V& xp, const V& yv, const V& yn, T zl, const V& q,
                    bool keep) __attribute__((always_inline)) {
    const T prev = lane_shift_keep<0x138>(zl, c[VZ - 1]);  // wave_shr:1, lane 0 keeps zl
    const T next = lane_shift_keep<0x130>(zl, c[0]);       // wave_shl:1, lane 63 keeps zl
    V out;
#pragma unroll
    for (int e = 0; e < VZ; ++e) {
      const T zm = e == 0 ? prev : c[e > 0 ? e - 1 : 0];
      const T zp = e == VZ - 1 ? next : c[e + 1 < VZ ? e + 1 : e];
      out[e] = diffusion_point_q(c[e], xm[e], xp[e], yv[e], yn[e], zm, zp, q[e], rdx2, rdy2, rdz2);
    }
    if (!plain) {  // wave-uniform
      asm volatile("");
#pragma unroll
      for (int e = 0; e < VZ; ++e) out[e] = __builtin_amdgcn_inverse_ballot_w64(zbm[e]) ? c[e] : out[e];
      if (keep) {  // rare
        asm volatile("");
        out = c;
      }
    }
    return out;
  };

  // One march position at phase PH = (p - p0) % 3.
  auto position = [&](auto phase, const int p) __attribute__((always_inline)) {
    constexpr int PH = decltype(phase)::value;
    const bool plain = wplain && p > 1 && p < n0 - 1;  // neither stage 1 nor stage 2 is on a boundary plane
    constexpr int SA = (PH + 2) % 3, SB = PH, SN = (PH + 1) % 3;  // slots of planes p-1 (and p-4), p (p-3), p+1 (p-2)
    const bool pb1 = p <= 0 || p >= n0 - 1;      // boundary plane: the intermediate value is T's
    const bool pb2 = p - 1 <= 0 || p >= n0;
    const bool st = p - 2 >= xs;                 // output plane p-2 belongs to the chunk
    char* const ob = reinterpret_cast<char*>(a.t2) + oo;
    // the edge lane's place in zedgeN to write, formed here from zx
    const int zo = static_cast<int>(here(static_cast<uint32_t>(zx))) + 1 - 2 * i63;

#pragma unroll
    for (int r = 0; r < RY; ++r) {
      // stages 2 and 3 run on this row (at most): not one of the tile's outer rows (wave-uniform)
      const bool mid = (r > 0 || ylo) && (r < RY - 1 || yhi);
      // the row's Q of planes p-1 and p-2 come out of the lane's slots, each one
      // row update ahead of its use: p-1 here, p-2 behind stage 1
      V q2, q3;
      if (mid) q2 = *reinterpret_cast<const V*>(&qslot[QP - qo + qb + r * W]);
      // 1. intermediate-1 plane p, then T plane p+2 into the slot of plane p-1
      {
        // T beyond the wave's rows: the neighbouring wave's row out of rows0, or yo beyond the tile
        V yv0 = yo, yn0 = yo;
        if (r == 0 && ylo) yv0 = *reinterpret_cast<const V*>(&rows0[RP * SB + lb]);
        if (r == RY - 1 && yhi) yn0 = *reinterpret_cast<const V*>(&rows0[RP * SB + lb + 3 * W]);
        const V& yv = (r == 0) ? yv0 : tt[SB][r > 0 ? r - 1 : 0];
        const V& yn = (r == RY - 1) ? yn0 : tt[SB][r + 1 < RY ? r + 1 : r];
        const T zl = zedge0[ZP * SB + r * ZR + zx];
        i1[SB][r] = update(plain, tt[SB][r], tt[SA][r], tt[SN][r], yv, yn, zl, qq[r], (pb1 | ((rbnd >> r) & 1)) != 0);
        tt[SA][r] = ldg<V>(t2 + rowo[r], vo);
        // T of plane p+1 beyond the tile, behind the use of plane p's, and the
        // wave's own outer rows of plane p+1 for the waves beside it
        if (r == 0 && !ylo) yo = ldg<V>(t1 + rowm, vo);
        if (r == RY - 1 && !yhi) yo = ldg<V>(t1 + rowp, vo);
        if (r == 0 && ylo) *reinterpret_cast<V*>(&rows0[RP * SN + lb + W]) = tt[SN][r];
        if (r == RY - 1 && yhi) *reinterpret_cast<V*>(&rows0[RP * SN + lb + 2 * W]) = tt[SN][r];
      }
      // 2. intermediate-2 plane p-1 from intermediate-1 planes p-2, p-1, p; not
      // for the tile's outer rows (wave-uniform), whose intermediate-1 values
      // no other wave reads either
      if (mid) {
        // Q of plane p-2, then Q of plane p, which stage 1 is done with, into its place
        q3 = *reinterpret_cast<const V*>(&qslot[qo + qb + r * W]);
        *reinterpret_cast<V*>(&qslot[qo + qb + r * W]) = qq[r];
        if (r == 0) *reinterpret_cast<V*>(&rows1[RP * SB + lb + W]) = i1[SB][r];
        if (r == RY - 1) *reinterpret_cast<V*>(&rows1[RP * SB + lb + 2 * W]) = i1[SB][r];
        V yv, yn;
        if (r == 0) yv = *reinterpret_cast<const V*>(&rows1[RP * SA + lb]);
        else yv = i1[SA][r > 0 ? r - 1 : 0];
        if (r == RY - 1) yn = *reinterpret_cast<const V*>(&rows1[RP * SA + lb + 3 * W]);
        else yn = i1[SA][r + 1 < RY ? r + 1 : r];
        const T zl = zedge1[ZP * SA + r * ZR + zx];  // every lane reads; the edge lanes use it
        i2[SA][r] = update(plain, i1[SA][r], i1[SN][r], i1[SB][r], yv, yn, zl, q2, (pb2 | ((rbnd >> r) & 1)) != 0);
        if (r == 0) *reinterpret_cast<V*>(&rows2[RP * SA + lb + W]) = i2[SA][r];
        if (r == RY - 1) *reinterpret_cast<V*>(&rows2[RP * SA + lb + 2 * W]) = i2[SA][r];
      }
      // Q plane p+1 into the registers of plane p, behind stage 1 and the store
      qq[r] = ldg<V>(q1 + rowo[r], vo);
      // 3. output plane p-2 from intermediate-2 planes p-3, p-2, p-1
      if (st && ((rout >> r) & 1) != 0) {  // wave-uniform
        V yv, yn;
        if (r == 0) yv = *reinterpret_cast<const V*>(&rows2[RP * SN + lb]);
        else yv = i2[SN][r > 0 ? r - 1 : 0];
        if (r == RY - 1) yn = *reinterpret_cast<const V*>(&rows2[RP * SN + lb + 3 * W]);
        else yn = i2[SN][r + 1 < RY ? r + 1 : r];
        const T zl = zedge2[ZP * SN + r * ZR + zx];
        // z boundary: T's value (written only with halo_z)
        const V out = update(plain, i2[SN][r], i2[SB][r], i2[SA][r], yv, yn, zl, q3, false);
        T* dst = reinterpret_cast<T*>(ob + rowo[r] + here(vo));
        if (wvst) {  // wave-uniform: one masked region
          if (vst) __builtin_nontemporal_store(out, reinterpret_cast<V*>(dst));
        } else if (vst) {
          __builtin_nontemporal_store(out, reinterpret_cast<V*>(dst));
        } else if (zin) {
#pragma unroll
          for (int e = 0; e < VZ; ++e)
            if (!zb[e]) dst[e] = out[e];
        }
      }
    }
    // the edge lanes, one masked region: their own values of T's plane p+1 and
    // of both new planes for the neighbours.
    // Stage 2 reads intermediate-1 on tile rows 1 .. TYE-2, stage 3 reads
    // intermediate-2 on rows 2 .. TYE-3: `cls` = which of ylo (1) / yhi (2) a
    // row of the wave needs to be among them.
    if (ledge) {
#pragma unroll
      for (int r = 0; r < RY; ++r) zedge0[ZP * SN + r * ZR + zo] = l63 ? tt[SN][r][VZ - 1] : tt[SN][r][0];
      auto share = [&](auto cls) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < RY; ++r) {
          if ((r < 1 ? 1 : 0) + (r > RY - 2 ? 2 : 0) == decltype(cls)::value)
            zedge1[ZP * SB + r * ZR + zo] = l63 ? i1[SB][r][VZ - 1] : i1[SB][r][0];
          if ((r < 2 ? 1 : 0) + (r > RY - 3 ? 2 : 0) == decltype(cls)::value)
            zedge2[ZP * SA + r * ZR + zo] = l63 ? i2[SA][r][VZ - 1] : i2[SA][r][0];
        }
      };
      share(std::integral_constant<int, 0>{});
      if (ylo) share(std::integral_constant<int, 1>{});
      if (yhi) share(std::integral_constant<int, 2>{});
      if (ylo && yhi) share(std::integral_constant<int, 3>{});
    }
    __syncthreads();

    // the plane pointers of position p+1
    t1 = t2;
    if (p + 3 <= n0 - 1) t2 += s0b;
    if (p + 2 <= n0 - 1) q1 += s0b;
    oo += s0b;
    qo = QP - qo;
  };

  // the last output plane xe-1 is formed at position xe+1
  for (int p = p0;;) {
    position(std::integral_constant<int, 0>{}, p);
    if (p == xe + 1) break;
    ++p;
    position(std::integral_constant<int, 1>{}, p);
    if (p == xe + 1) break;
    ++p;
    position(std::integral_constant<int, 2>{}, p);
    if (p == xe + 1) break;
    ++p;
  }
}

// The launch plan of an (n0, n1, .) field with tiles that write `tys` rows, for
// a grid of about `target` workgroups: tiles along dim 1, the length of an x
// chunk and the workgroups (tiles x chunks). Equal x chunks so that the grid
// is about the target; a chunk pays a four-position lead-in, so it is at least
// MIN_CHUNK planes long (or the whole inner range, where that is shorter).
inline ThreestepPlan plan(int64_t n0, int64_t n1, int tys, int64_t target) {
  ThreestepPlan pl;
  pl.tiles = (n1 - 2 + tys - 1) / tys;
  const int64_t len0 = n0 - 2;
  target = std::max<int64_t>(target, 1);
  const int64_t ch_min = std::max<int64_t>(std::min<int64_t>(MIN_CHUNK, len0), (len0 * pl.tiles + target - 1) / target);
  const int64_t nch = std::max<int64_t>(1, len0 / ch_min);
  pl.chunk = (len0 + nch - 1) / nch;
  pl.workgroups = pl.tiles * ((len0 + pl.chunk - 1) / pl.chunk);
  return pl;
}

template <typename T, int BY, int RY, int BZ, typename Kern>
void launch_form(Kern kern, const DiffusionArgs& a, hipStream_t stream) {
  constexpr int TYS = BY * RY - 4, BLOCK = 64 * BY * BZ;
  K2Args<T> k;
  k.t2 = reinterpret_cast<T*>(a.t2);
  k.t = reinterpret_cast<const T*>(a.t);
  k.cp = reinterpret_cast<const T*>(a.q);
  k.n0 = a.n[0]; k.n1 = a.n[1]; k.n2 = a.n[2];
  k.rdx2 = static_cast<T>(a.rd2[0]);
  k.rdy2 = static_cast<T>(a.rd2[1]);
  k.rdz2 = static_cast<T>(a.rd2[2]);
  k.dtlam = static_cast<T>(a.dt_lam);
  k.halo_z = a.halo_z ? 1 : 0;
  k.ntz = 1;
  // a grid of about `rounds` residency rounds
  const ThreestepPlan pl = plan(k.n0, k.n1, TYS, diffusion3d_target_blocks(reinterpret_cast<const void*>(kern), BLOCK, a.rounds));
  k.nty = pl.tiles;
  k.ch = pl.chunk;
  k.nblk = pl.workgroups;
  if (k.nblk > 0x7fffffffLL) fail("diffusion3d_threestep: grid too large");
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(k.nblk)), dim3(BLOCK), 0, stream, k);
  IGG_HIP_CHECK(hipGetLastError());
}

}  // namespace threestep
}  // namespace igg
