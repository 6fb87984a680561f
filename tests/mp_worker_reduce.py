"""Per-rank scenario of the global-reduction tests (ops/reduce.py), launched by
tests/test_reduce_cpu.py and tests/test_gpu_reduce.py, one process per rank.

Every local cell holds an integer function of its GLOBAL index (overlapping
cells of neighbouring ranks hold the same value), so the reductions over the
implicit global grid must equal, bitwise, the same reduction of the global
array built directly - on every rank."""
import math
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import igg  # noqa: E402

ONE = ("sum", "sumsq", "max", "min", "maxabs")
TWO = ("dot", "sumsq_diff", "maxabs_diff")


def _device(kind):
    if kind == "gpu":  # every rank on device 0
        torch.cuda.set_device(0)
        return torch.device("cuda", 0)
    return torch.device("cpu")


def _values(g):
    """Two integer functions of the global index grids ``g`` (|x| <= 1024):
    F positive, its unique maximum and minimum are set by the caller."""
    gx, gy, gz = g
    F = 1 + (7 * gx + 13 * gy + 29 * gz) % 1000
    G = ((5 * gx + 3 * gy + 11 * gz) % 601) - 300
    return F.to(torch.float64), G.to(torch.float64)


def _global_shape(gg, shape):
    out = []
    for d in range(3):
        n, o = int(gg.nxyz[d]), int(gg.overlaps[d])
        ol = o + shape[d] - n
        out.append(int(gg.dims[d]) * (n - o) + (0 if int(gg.periods[d]) else ol))
    return out


def _global_arrays(gg, shape):
    ng = _global_shape(gg, shape)
    g = torch.meshgrid(*(torch.arange(k, dtype=torch.int64) for k in ng), indexing="ij")
    F, G = _values(g)
    n0, o0 = int(gg.nxyz[0]), int(gg.overlaps[0])
    # the unique maximum in a cell two ranks hold (the x overlap of ranks 0 and 1), the minimum in a corner
    F[n0 - o0, ng[1] // 2, ng[2] // 2] = 1024.0
    F[0, 0, 0] = -1000.0
    return F, G


def _local(gg, shape, Fg):
    idx = []
    for d in range(3):
        n, o = int(gg.nxyz[d]), int(gg.overlaps[d])
        i = int(gg.coords[d]) * (n - o) + torch.arange(shape[d], dtype=torch.int64)
        idx.append(i % Fg.shape[d] if int(gg.periods[d]) else i)
    return Fg[idx[0].view(-1, 1, 1), idx[1].view(1, -1, 1), idx[2].view(1, 1, -1)].contiguous()


def _expected(op, F, G):
    if op == "sum":
        return F.sum()
    if op == "sumsq":
        return (F * F).sum()
    if op == "max":
        return F.max()
    if op == "min":
        return F.min()
    if op == "maxabs":
        return F.abs().max()
    if op == "dot":
        return (F * G).sum()
    if op == "sumsq_diff":
        return ((F - G) * (F - G)).sum()
    return (F - G).abs().max()


def _bits(t):
    return struct.pack("<d", float(t)).hex()


def scenario_reduce(dev, dtype, dimx, dimy, dimz, periodic, overlap, halowidth):
    device = _device(dev)
    dt = getattr(torch, dtype)
    per, o, w = int(periodic), int(overlap), int(halowidth)
    n = (9, 8, 10)
    me, dims, nprocs, coords, comm = igg.init_global_grid(
        *n, dimx=int(dimx), dimy=int(dimy), dimz=int(dimz), periodx=per & 1, periody=(per >> 1) & 1,
        periodz=(per >> 2) & 1, overlapx=o, overlapy=o, overlapz=o, halowidthx=w, halowidthy=w, halowidthz=w,
        quiet=True, select_device=False, device_type="none" if dev == "cpu" else "AMDGPU")
    gg = igg.get_global_grid()
    bits = []
    for shape in (n, (n[0] + 1, n[1], n[2]), (n[0], n[1] - 1, n[2])):  # the grid's size, two staggered ones
        Fg, Gg = _global_arrays(gg, shape)
        A = _local(gg, shape, Fg).to(dt).to(device)
        B = _local(gg, shape, Gg).to(dt).to(device)
        cells = igg.ops.reduce.global_cells(A)
        assert cells == Fg.numel(), (cells, tuple(Fg.shape))

        def check(tag):
            for op in ONE + TWO:
                r = igg.reduce_g(op, A, other=B if op in TWO else None)
                assert r.dtype == torch.float64 and r.dim() == 0 and r.device == A.device
                want = _expected(op, Fg, Gg)
                if _bits(r) != _bits(want):
                    raise AssertionError(f"rank {me} {tag} {shape} {op}: got {float(r)!r}, want {float(want)!r}")
                bits.append(_bits(r))
            m = igg.mean_g(A)
            assert _bits(m) == _bits(Fg.sum() / Fg.numel()), (tag, float(m))
            bits.append(_bits(m))

        check("plain")
        # a NaN in a plane nobody owns changes nothing
        rng = igg.owned_ranges(A)
        A0, B0 = A.clone(), B.clone()
        if int(coords[0]) == 1 and rng[0][0] > 0:
            A[0, :, :] = math.nan
            B[0, :, :] = math.nan
        if rng[2][1] < shape[2]:
            A[:, :, -1] = math.nan
        check("nan outside")
        # a NaN owned by rank 1 reaches every rank, for every op
        A.copy_(A0)
        B.copy_(B0)
        if me == 1:
            A[rng[0][0], rng[1][0], rng[2][1] - 1] = math.nan
        for op in ONE + TWO:
            r = igg.reduce_g(op, A, other=B if op in TWO else None)
            assert math.isnan(float(r)), f"rank {me} {shape} {op}: NaN owned by rank 1 gave {float(r)!r}"
        assert math.isnan(float(igg.mean_g(A)))
        # several fields in one call, and a local reduction next to the global one
        A.copy_(A0)
        r3 = igg.reduce_g("sum", A, B, A)
        assert r3.shape == (3,) and _bits(r3[0]) == _bits(Fg.sum()) and _bits(r3[1]) == _bits(Gg.sum())
        loc = igg.reduce_g("sum", A, local=True)
        assert _bits(loc) == _bits(igg.owned_view(A).double().sum())
    igg.finalize_global_grid()
    print(f"rank {me} reduce OK BITS={','.join(bits)}")


if __name__ == "__main__":
    name, *args = sys.argv[1:]
    globals()[f"scenario_{name}"](*args)
