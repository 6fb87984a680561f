"""The z edge of the fused diffusion kernels at every lane position.

The fused kernels (csrc/include/igg/fused_impl.hpp) keep the z-face values of a
wave's rows one per lane; where they sit depends on zh (the lane of the high z
edge), nv (the rows the wave really has) and on whether one wave holds both
edges (csrc/include/igg/zedge.hpp; tests/test_fused_zedge_cpu.py enumerates the
rule on the host). Here the kernels themselves run at the zh values next to
every threshold of that rule: 0, 1, RY - 1, RY, 31, 32, 32 + RY - 1, 32 + RY,
63, a wave with both edges, and for fused variant 48 (DPP row shifts) every zh
of 7..15 plus the 16k + 7 and the readlane fall-backs around them.

Reference: the plain step + update_halo_, bitwise, after sync_halo(), with
check(). Shapes: n0 = 6, n1 = 2 + RY + 3 (a full wave and one with nv = 3),
n2 = 64 * VZ * k + VZ * (zh + 1); fields distinct at every point; 4 steps per
send form, and the send forms 0, 1, 8, 64 (z unpack), 4 (direct z) cycled on
the same pair. One test per (variant, dtype); it collects every failure.

The model asks n2 % 4 == 0 of a fusable grid because it does not know the
variant's VZ; the kernels ask n2 % VZ == 0 (launch_hx). The VZ = 2 tilings
reach an even zh only with n2 % 4 == 2, so the fused model here is a subclass
whose can_fuse states the kernel's own condition.
"""
import time

import pytest
import torch

import igg
from igg.models.diffusion3d import Diffusion3D
from igg.ops import stencil

native = stencil.native
FUSED = stencil.compiled_fused_variants()
MODES = (0, 1, 8, 64, 4)
STEPS = 4
ZP, XYZP = (0, 0, 1), (1, 1, 1)
F32_VARIANTS = (0, 40, 9, 14)  # one of each tiling family


class _KernelFusable(Diffusion3D):
    """Fusable wherever the fused kernel of its variant is (n2 a multiple of VZ)."""
    _vz = 4

    @property
    def can_fuse(self):
        n2 = int(self.T.shape[2])
        return self.device.type == "cuda" and n2 % self._vz == 0 and n2 >= 2 * self._vz


def _n2(vz, k, zh):
    return 64 * vz * k + vz * (zh + 1)


def _cases(variant, dtype):
    """(n2, periods, zh, both edges in one wave, DPP form expected) of a test."""
    by, ry, vz, bz, dpp = native.diffusion3d_fused_tile(variant)
    out = []

    def add(n2, periods, zh, one_wave=False):
        # coverage from host arithmetic, the launch's own predicates
        assert n2 % vz == 0 and n2 >= 2 * vz
        assert native.fused_zedge_zh(n2, vz) == zh, (n2, vz, zh)
        assert native.fused_zedge_one_wave(n2, vz) == one_wave, (n2, vz)
        out.append((n2, periods, zh, one_wave, dpp and native.fused_zedge_dpp_ok(n2, vz, ry)))

    if dpp:
        assert (ry, vz) == (8, 4)
        dagger = (7, 8, 13, 23, 63)
        for zh in (6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 22, 23, 31, 39, 47, 55, 63):
            add(_n2(vz, 1, zh), ZP, zh)
            if zh in dagger:
                add(_n2(vz, 1, zh), XYZP, zh)
        add(_n2(vz, 2, 7), ZP, 7)
        # 6, 16 and 22 take the readlane fall-back; 7..15 and every 16k + 7 the DPP form
        assert {c[2] for c in out if not c[4]} == {6, 16, 22}
        assert {c[2] for c in out if c[4]} >= set(range(7, 16)) | {23, 39, 55}
        return ry, vz, out
    if dtype == torch.float64:
        dagger = (ry - 1, 32, 63)
        for zh in (0, 1, ry - 1, ry, 31, 32, 32 + ry - 1, 32 + ry, 63):
            # zh = 0 is n2 = 65 * VZ: lane 0 of the second wave, and the limit up to which the
            # launch guards still count a wave with both edges
            add(_n2(vz, 1, zh), ZP, zh, one_wave=zh == 0)
            if zh in dagger:
                add(_n2(vz, 1, zh), XYZP, zh)
        add(_n2(vz, 2, ry - 1), ZP, ry - 1)
        for n2 in (2 * vz, vz * (ry + 1), 33 * vz, 64 * vz):  # one wave holds both edges (65 * VZ: zh = 0 above)
            add(n2, ZP, n2 // vz - 1, one_wave=True)
        add(64 * vz, XYZP, 63, one_wave=True)
        assert not native.fused_zedge_one_wave(66 * vz, vz)  # 65 * VZ is the limit
    else:
        for zh in (ry - 1, 32, 63):
            add(_n2(vz, 1, zh), ZP, zh)
        add(64 * vz, ZP, 63, one_wave=True)
    return ry, vz, out


_fields = {}


def _inputs(shape, dtype, gpu):
    """(T, Cp) distinct at every point, computed once per shape, never written."""
    key = (shape, dtype)
    if key not in _fields:
        g = torch.Generator().manual_seed(29)
        n = shape[0] * shape[1] * shape[2]
        assert n < 1 << 22  # i / n + 0.5 stays distinct in f32
        T = (torch.randperm(n, generator=g).to(torch.float64) / n + 0.5).reshape(shape)
        Cp = 1 + 5 * torch.rand(shape, generator=g, dtype=torch.float64)
        _fields[key] = (T.to(dtype).to(gpu), Cp.to(dtype).to(gpu))
    return _fields[key]


def _pair(shape, periods, dtype, variant, vz, gpu):
    igg.init_global_grid(*shape, periodx=periods[0], periody=periods[1], periodz=periods[2], quiet=True,
                         init_MPI=False)
    plain = variant if variant in stencil.compiled_variants() else 0
    a = Diffusion3D(dtype=dtype, variant=plain)
    b = _KernelFusable(dtype=dtype, variant=plain)
    b._vz = vz
    T, Cp = _inputs(shape, dtype, gpu)
    for m in (a, b):
        m.T.copy_(T)
        m.T2.copy_(T)
        m.Cp.copy_(Cp)
    b.fused_variant, b.fused_mode = variant, MODES[0]
    assert b.set_fused(True)
    assert b.fused_variant == variant, f"fused variant {variant} is not compiled in this build"
    return a, b


def _where(a, b, n2):
    """Where two fields differ, per z side: the side and its first (x, y) rows."""
    d = (a != b).nonzero()
    out = []
    for side, sel in ((0, d[:, 2] < n2 // 2), (n2 - 1, d[:, 2] >= n2 // 2)):
        rows = torch.unique(d[sel][:, :2], dim=0)[:6].tolist()
        if rows:
            out.append((f"z side {side}", [tuple(r) for r in rows]))
    return out


def _sweep(variant, dtype, gpu):
    ry, vz, cases = _cases(variant, dtype)
    failures = []
    for n2, periods, zh, one_wave, dpp_form in cases:
        shape = (6, 2 + ry + 3, n2)
        a, b = _pair(shape, periods, dtype, variant, vz, gpu)
        for mode in MODES:
            b.fused_mode = mode  # another receive form re-primes from the field
            a.run(STEPS)
            b.run(STEPS)
            assert b.fused_mode == mode, f"variant {variant}: send mode {mode} unavailable"
            b.sync_halo()
            torch.cuda.synchronize()
            b.check()
            if not torch.equal(a.T, b.T):
                failures.append((f"n2 {n2}", f"zh {zh}", f"mode {mode}", f"periods {periods}",
                                 "DPP" if dpp_form else "readlane", *_where(a.T, b.T, n2)))
                # later forms start from the reference's state, not from the wrong one
                b.T.copy_(a.T)
                b.T2.copy_(a.T2)
                b.mark_modified()
        b.close()
        igg.finalize_global_grid(finalize_MPI=False)
    return len(cases), failures


def _ids():
    return [(v, dt) for v in FUSED for dt in (torch.float64, torch.float32)
            if dt == torch.float64 or v in F32_VARIANTS or native.diffusion3d_fused_tile(v)[4]]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,dtype", _ids(), ids=lambda p: str(p).replace("torch.", ""))
def test_fused_z_edge_sweep(gpu, variant, dtype):
    t0 = time.perf_counter()
    n, failures = _sweep(variant, dtype, gpu)
    print(f"fused variant {variant} {dtype}: {n} shapes x {len(MODES)} send forms in "
          f"{time.perf_counter() - t0:.2f} s, {len(failures)} differ")
    assert not failures, "\n".join(map(str, failures))
