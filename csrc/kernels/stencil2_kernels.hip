// Two diffusion time steps in one pass over memory (temporal blocking) for
// gfx950: t2 = step(step(t)) on the whole inner box of a rank without
// neighbours, bitwise what two launch_diffusion3d calls leave (every point goes
// through diffusion_point_q, devmath.hpp; the boundary planes keep t's values
// in the intermediate field, as they do in the ping-pong loop).
//
// The single-step loop moves 3 arrays per step (read T, read Cp, write T2);
// here the intermediate field never reaches memory: about 1 write + (1 + ring)
// reads of T and Cp per TWO steps.
//
// Shape: a 2.5-D march along dim 0 like diffusion3d_vkernel. A workgroup of
// BY x BZ waves owns TYE = BY*RY rows x W = 64*VZ*BZ points of the (dim 1,
// dim 2) plane: the outer rows are the 1-wide ring of the intermediate field,
// the TYE-2 inner rows are written. Tiles advance by TYE-2 rows (rows have no
// alignment to keep) and by W points (vector accesses stay aligned). At march
// position p a lane
//   1. forms the intermediate plane p at its own points from T planes p-1, p,
//      p+1 (registers; y neighbours beyond the wave's rows and the two z
//      segment-edge values are loaded, as in the single-step kernel);
//   2. issues the loads of the next position (T plane p+2, Cp plane p+1);
//   3. forms output plane p-1 from intermediate planes p-2, p-1, p: x
//      neighbours and the wave's own rows are registers, z neighbours lane
//      neighbours; the first/last row of every wave and the wave-edge z values
//      of intermediate plane p-1 come from LDS (double-buffered, one barrier
//      per position);
//   4. puts those parts of plane p into the other LDS buffer.
// dtlam/Cp is divided once per point and kept for the second use. Where a tile
// does not span the row, the intermediate values at z = zt-1 and zt+W (the z
// ring) are formed by 2*TYE "edge" threads with scalar loads. An x chunk
// [xs, xe) starts with the two-position lead-in p = xs-1, xs.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "igg/devmath.hpp"
#include "igg/stencil.hpp"
#include "igg/xcd.hpp"

namespace igg {
namespace {

template <typename T>
struct K2Args {
  T* __restrict__ t2;
  const T* __restrict__ t;
  const T* __restrict__ cp;
  int64_t n0, n1, n2;
  T rdx2, rdy2, rdz2, dtlam;
  int halo_z;
  int64_t ntz, nty, ch, nblk;
};

template <typename T, int VZ>
struct Vec2 {
  typedef T type __attribute__((ext_vector_type(VZ)));
};

template <typename T, int BY, int RY, int VZ, int BZ>
__global__ void __launch_bounds__(64 * BY * BZ)
diffusion3d_twostep_kernel(const K2Args<T> a) {
  using V = typename Vec2<T, VZ>::type;
  constexpr int WS = 64 * VZ;  // points of one wave's row segment
  constexpr int W = WS * BZ;
  constexpr int TYE = BY * RY, TYS = TYE - 2;
  static_assert(2 * TYE <= 64, "edge threads live in wave 0");
  // intermediate plane parts shared between waves, [position parity]:
  // first / last row of every wave, and per row the values left ([0], z =
  // segment origin - 1) and right ([1], z = segment origin) of every segment
  // boundary j = 0..BZ
  __shared__ __attribute__((aligned(16))) T rows[2][BY][2][W];
  __shared__ T zedge[2][TYE][BZ + 1][2];

  int64_t b = xcd_remap(blockIdx.x, a.nblk);
  const int64_t tz = b % a.ntz;
  b /= a.ntz;
  const int64_t ty = b % a.nty;
  const int64_t cx = b / a.nty;

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wz = wid % BZ, wy = wid / BZ;
  const int64_t n0 = a.n0, n1 = a.n1, n2 = a.n2;
  const int64_t s1 = n2, s0 = n1 * n2;
  const int64_t zt = tz * W;          // tile origin
  const int64_t zw = zt + wz * WS;    // segment origin (wave-uniform)
  const int64_t ye0 = ty * TYS;       // first (ring) row of the tile
  const int64_t xs = 1 + cx * a.ch;
  const int64_t xe = min(xs + a.ch, n0 - 1);

  // Lanes past the row alias its last vector (loads stay in bounds, nothing stored).
  const int64_t z0 = zw + lane * VZ;
  const int64_t zlast = n2 - VZ;
  const int64_t zc = min(z0, zlast);
  const bool zin = z0 < n2;
  const int zl = static_cast<int>(zc - zw);
  const bool load_prev = lane == 0;
  const bool load_next = lane == 63 || z0 + VZ > zlast;
  const int zpi = static_cast<int>(max<int64_t>(zc - 1, 0) - zw);
  const int zni = static_cast<int>(min<int64_t>(zc + VZ, n2 - 1) - zw);
  bool zb[VZ];  // boundary point along z: the intermediate value is T's
  bool zany = false;
#pragma unroll
  for (int e = 0; e < VZ; ++e) {
    zb[e] = z0 + e == 0 || z0 + e >= n2 - 1;
    zany = zany || zb[e];
  }

  // Rows past the array alias row n1-1 (a boundary row: never written).
  int64_t rowb[RY];  // wave-uniform row bases
  bool rbnd[RY], rout[RY];
#pragma unroll
  for (int r = 0; r < RY; ++r) {
    const int64_t yr = ye0 + wy * RY + r;
    const int lr = wy * RY + r;
    rowb[r] = min(yr, n1 - 1) * s1 + zw;
    rbnd[r] = yr == 0 || yr >= n1 - 1;
    rout[r] = lr >= 1 && lr <= TYE - 2 && yr <= n1 - 2;
  }
  const int64_t rowm = min(max<int64_t>(ye0 + wy * RY - 1, 0), n1 - 1) * s1 + zw;
  const int64_t rowp = min(ye0 + wy * RY + RY, n1 - 1) * s1 + zw;

  // z-ring ("edge") threads: thread s*TYE + el forms the intermediate value
  // of tile row el at z = zt-1 (s = 0) or zt+W (s = 1) where that point exists
  const int et = static_cast<int>(threadIdx.x);
  const int es = et / TYE, el = et % TYE;
  const int64_t ez = es == 0 ? zt - 1 : zt + W;
  const bool eact = et < 2 * TYE && (es == 0 ? zt > 0 : zt + W < n2);
  const int64_t eyr = ye0 + el;
  const bool ebnd = eyr == 0 || eyr >= n1 - 1 || ez >= n2 - 1;
  int64_t eo = 0, eom = 0, eop = 0, eozm = 0, eozp = 0;
  if (eact) {
    const int64_t y = min(eyr, n1 - 1);
    eo = y * s1 + ez;
    eom = max<int64_t>(y - 1, 0) * s1 + ez;
    eop = min(y + 1, n1 - 1) * s1 + ez;
    eozm = eo - 1;                              // ez >= W - 1 > 0
    eozp = y * s1 + min(ez + 1, n2 - 1);
  }

  const T* __restrict__ t = a.t;
  const T* __restrict__ cpp = a.cp;
  const T rdx2 = a.rdx2, rdy2 = a.rdy2, rdz2 = a.rdz2, dtlam = a.dtlam;

  // March state at position p: ta/tb/tn = T planes p-1/p/p+1, cpv = Cp plane
  // p, ym/yp/em/ep = T plane p around the wave's rows and segment; im/ic =
  // intermediate planes p-2/p-1, q0 = dtlam/Cp of plane p-1.
  V ta[RY], tb[RY], tn[RY], cpv[RY], im[RY], ic[RY], q0[RY];
  V ym, yp;
  T em[RY], ep[RY];
  T eta = T(0), etb = T(0);
  {
    const int64_t p = xs - 1;  // >= 0; p+1 = xs <= n0-2
    const int64_t om = max<int64_t>(p - 1, 0) * s0, oc = p * s0, on = (p + 1) * s0;
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      ta[r] = *reinterpret_cast<const V*>(t + om + rowb[r] + zl);
      tb[r] = *reinterpret_cast<const V*>(t + oc + rowb[r] + zl);
      tn[r] = *reinterpret_cast<const V*>(t + on + rowb[r] + zl);
      cpv[r] = *reinterpret_cast<const V*>(cpp + oc + rowb[r] + zl);
      em[r] = load_prev ? t[oc + rowb[r] + zpi] : T(0);
      ep[r] = load_next ? t[oc + rowb[r] + zni] : T(0);
      im[r] = tb[r];
      ic[r] = tb[r];
      q0[r] = tb[r];
    }
    ym = *reinterpret_cast<const V*>(t + oc + rowm + zl);
    yp = *reinterpret_cast<const V*>(t + oc + rowp + zl);
    if (eact) {
      eta = t[om + eo];
      etb = t[oc + eo];
    }
  }

  for (int64_t p = xs - 1; p <= xe; ++p) {
    const bool pb = p == 0 || p == n0 - 1;  // boundary plane: intermediate = T
    const int bn = static_cast<int>(p & 1), bc = bn ^ 1;

    // 1. intermediate plane p
    V in[RY], q1[RY];
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      const V& c = tb[r];
      const V& yv = (r == 0) ? ym : tb[r > 0 ? r - 1 : 0];
      const V& yn = (r == RY - 1) ? yp : tb[r + 1 < RY ? r + 1 : r];
      T prev = __shfl_up(c[VZ - 1], 1);
      T next = __shfl_down(c[0], 1);
      if (load_prev) prev = em[r];
      if (load_next) next = ep[r];
#pragma unroll
      for (int e = 0; e < VZ; ++e) {
        const T zm = e == 0 ? prev : c[e > 0 ? e - 1 : 0];
        const T zp = e == VZ - 1 ? next : c[e + 1 < VZ ? e + 1 : e];
        q1[r][e] = dtlam / cpv[r][e];
        const T v = diffusion_point_q(c[e], ta[r][e], tn[r][e], yv[e], yn[e], zm, zp, q1[r][e], rdx2, rdy2, rdz2);
        in[r][e] = (pb || rbnd[r] || zb[e]) ? c[e] : v;
      }
    }
    T ein = T(0);
    if (eact) {
      const int64_t oc = p * s0;
      const T etn = t[min(p + 1, n0 - 1) * s0 + eo];
      const T v = diffusion_point_q(etb, eta, etn, t[oc + eom], t[oc + eop], t[oc + eozm], t[oc + eozp],
                                    dtlam / cpp[oc + eo], rdx2, rdy2, rdz2);
      ein = (pb || ebnd) ? etb : v;
      eta = etb;
      etb = etn;
    }

    // 2. loads of position p+1 (clamped at the last plane: then unused)
    V tn2[RY], cpn[RY];
    V ymn, ypn;
    T emn[RY], epn[RY];
    {
      const int64_t o1 = min(p + 1, n0 - 1) * s0, o2 = min(p + 2, n0 - 1) * s0;
#pragma unroll
      for (int r = 0; r < RY; ++r) {
        tn2[r] = *reinterpret_cast<const V*>(t + o2 + rowb[r] + zl);
        cpn[r] = *reinterpret_cast<const V*>(cpp + o1 + rowb[r] + zl);
        emn[r] = load_prev ? t[o1 + rowb[r] + zpi] : T(0);
        epn[r] = load_next ? t[o1 + rowb[r] + zni] : T(0);
      }
      ymn = *reinterpret_cast<const V*>(t + o1 + rowm + zl);
      ypn = *reinterpret_cast<const V*>(t + o1 + rowp + zl);
    }

    // 3. output plane x = p-1 from intermediate planes p-2 (im), p-1 (ic), p (in)
    if (p - 1 >= xs) {
      const int64_t off = (p - 1) * s0;
#pragma unroll
      for (int r = 0; r < RY; ++r) {
        const int lr = wy * RY + r;
        if (!rout[r]) continue;  // wave-uniform
        const V& c = ic[r];
        V yv, yn;
        if (r == 0) yv = *reinterpret_cast<const V*>(&rows[bc][wy > 0 ? wy - 1 : 0][1][wz * WS + lane * VZ]);
        else yv = ic[r > 0 ? r - 1 : 0];
        if (r == RY - 1) yn = *reinterpret_cast<const V*>(&rows[bc][wy + 1 < BY ? wy + 1 : wy][0][wz * WS + lane * VZ]);
        else yn = ic[r + 1 < RY ? r + 1 : r];
        T prev = __shfl_up(c[VZ - 1], 1);
        T next = __shfl_down(c[0], 1);
        if (lane == 0) prev = zedge[bc][lr][wz][0];
        if (lane == 63) next = zedge[bc][lr][wz + 1][1];
        V out;
#pragma unroll
        for (int e = 0; e < VZ; ++e) {
          const T zm = e == 0 ? prev : c[e > 0 ? e - 1 : 0];
          const T zp = e == VZ - 1 ? next : c[e + 1 < VZ ? e + 1 : e];
          const T v = diffusion_point_q(c[e], im[r][e], in[r][e], yv[e], yn[e], zm, zp, q0[r][e], rdx2, rdy2, rdz2);
          out[e] = zb[e] ? c[e] : v;  // z boundary: T's value (written only with halo_z)
        }
        if (zin) {
          T* dst = a.t2 + off + rowb[r] + zl;
          if (!zany || a.halo_z) {
            __builtin_nontemporal_store(out, reinterpret_cast<V*>(dst));
          } else {
#pragma unroll
            for (int e = 0; e < VZ; ++e)
              if (!zb[e]) dst[e] = out[e];
          }
        }
      }
    }

    // 4. the shared parts of intermediate plane p
#pragma unroll
    for (int r = 0; r < RY; ++r) {
      const int lr = wy * RY + r;
      if (r == 0) *reinterpret_cast<V*>(&rows[bn][wy][0][wz * WS + lane * VZ]) = in[r];
      if (r == RY - 1) *reinterpret_cast<V*>(&rows[bn][wy][1][wz * WS + lane * VZ]) = in[r];
      if (lane == 0) zedge[bn][lr][wz][1] = in[r][0];
      if (lane == 63) zedge[bn][lr][wz + 1][0] = in[r][VZ - 1];
    }
    if (eact) zedge[bn][el][es == 0 ? 0 : BZ][es == 0 ? 0 : 1] = ein;
    __syncthreads();

#pragma unroll
    for (int r = 0; r < RY; ++r) {
      ta[r] = tb[r];
      tb[r] = tn[r];
      tn[r] = tn2[r];
      cpv[r] = cpn[r];
      em[r] = emn[r];
      ep[r] = epn[r];
      im[r] = ic[r];
      ic[r] = in[r];
      q0[r] = q1[r];
    }
    ym = ymn;
    yp = ypn;
  }
}

struct Form {
  const char* name;
  int by, ry, bz;
};

// Lanes hold 16 bytes (VZ = 2 f64 / 4 f32), so a tile is 128*BZ f64 or 256*BZ
// f32 points wide: form 0 spans a 512-point f64 / 1024-point f32 row (no z
// ring). RY = 4 is the most the register file holds without scratch at two
// waves per SIMD (RY = 5 and 6 spill).
constexpr Form FORMS[] = {
    {"t2_by2_ry4_bz4", 2, 4, 4},  // 0: 8 rows x 512 (f64) tile, 512 threads
    {"t2_by4_ry4_bz2", 4, 4, 2},  // 1: 16 rows x 256, 512 threads
    {"t2_by4_ry4_bz1", 4, 4, 1},  // 2: 16 rows x 128, 256 threads (two workgroups per CU)
};
constexpr int NFORMS = sizeof(FORMS) / sizeof(FORMS[0]);

template <typename T, int BY, int RY, int BZ>
void launch_form(const DiffusionArgs& a, hipStream_t stream) {
  constexpr int VZ = 16 / static_cast<int>(sizeof(T));
  constexpr int W = 64 * VZ * BZ, TYS = BY * RY - 2, BLOCK = 64 * BY * BZ;
  auto kern = &diffusion3d_twostep_kernel<T, BY, RY, VZ, BZ>;
  K2Args<T> k;
  k.t2 = reinterpret_cast<T*>(a.t2);
  k.t = reinterpret_cast<const T*>(a.t);
  k.cp = reinterpret_cast<const T*>(a.cp);
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

template <typename T>
void dispatch2(const DiffusionArgs& a, hipStream_t s) {
  switch (a.form) {
    case 0: launch_form<T, 2, 4, 4>(a, s); break;
    case 1: launch_form<T, 4, 4, 2>(a, s); break;
    case 2: launch_form<T, 4, 4, 1>(a, s); break;
    default: fail("diffusion3d_twostep: no form ", a.form);
  }
}

}  // namespace

int diffusion3d_twostep_num_forms() { return NFORMS; }
const char* diffusion3d_twostep_form_name(int form) {
  return (form >= 0 && form < NFORMS) ? FORMS[form].name : "invalid";
}

bool diffusion3d_twostep_ok(const DiffusionArgs& a) {
  if (a.form < 0 || a.form >= NFORMS) return false;
  if (a.elem_bytes != 4 && a.elem_bytes != 8) return false;
  const int vz = 16 / a.elem_bytes;
  if (a.n[0] < 3 || a.n[1] < 3 || a.n[2] < 3) return false;
  return a.n[2] % vz == 0;  // aligned 16-byte vectors along every row
}

void launch_diffusion3d_twostep(const DiffusionArgs& a, hipStream_t stream) {
  if (!diffusion3d_twostep_ok(a))
    fail("diffusion3d_twostep: form ", a.form, " cannot run this shape (", a.n[0], ", ", a.n[1], ", ", a.n[2],
         ") at ", a.elem_bytes, " bytes per element; run two single steps");
  if (a.elem_bytes == 8) dispatch2<double>(a, stream);
  else dispatch2<float>(a, stream);
}

}  // namespace igg
