"""Per-rank scenarios of the gather_g tests (parallel/gather_g.py), launched by
tests/test_gather_g_cpu.py and tests/test_gpu_gather_g.py, one process per rank.

Every local cell holds an integer function of its GLOBAL index (|x| <= 1024:
exact in f32 and f64), the global index comes from ``coords_g`` - not from the
code under test - and every plane a rank does not own is NaN. The result on
the root must equal, bitwise, the global array built directly."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import igg  # noqa: E402

N = (9, 8, 10)


def _device(kind):
    if kind == "mgpu":  # one rank per device
        r = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(r)
        return torch.device("cuda", r)
    if kind == "gpu":  # every rank on device 0
        torch.cuda.set_device(0)
        return torch.device("cuda", 0)
    return torch.device("cpu")


def _extents(gg, shape):
    out = []
    for d in range(len(shape)):
        n, o = int(gg.nxyz[d]), int(gg.overlaps[d])
        out.append(int(gg.dims[d]) * (n - o) + (0 if int(gg.periods[d]) else o + shape[d] - n))
    return out


def _global_array(ext):
    g = torch.meshgrid(*(torch.arange(k, dtype=torch.int64) for k in ext), indexing="ij")
    F = torch.zeros(ext, dtype=torch.int64)
    for d, w in enumerate((7, 13, 29)[:len(ext)]):
        F = F + w * g[d]
    return (F % 2039) - 1015  # |x| <= 1023


def _indices_from_coords(gg, d, A):
    """Global indices of axis ``d`` of ``A`` from ``coords_g`` with spacing 1:
    a periodic axis is ordered by the wrapped coordinate (its floor); on a
    non-periodic axis the coordinate is the index plus the field's stagger
    offset ``0.5*(n - m)``."""
    x = igg.coords_g(d, 1.0, A, device="cpu")
    if not int(gg.periods[d]):
        x = x - 0.5 * (int(gg.nxyz[d]) - A.shape[d])
    return torch.floor(x).to(torch.int64)


def _local(gg, shape, Fg, dtype, device):
    probe = torch.empty(shape, device="meta")
    idx = [_indices_from_coords(gg, d, probe) for d in range(len(shape))]
    view = [[-1 if e == d else 1 for e in range(len(shape))] for d in range(len(shape))]
    A = Fg[tuple(i.view(v) for i, v in zip(idx, view))].to(dtype).contiguous()
    if dtype.is_floating_point:  # NaN in every plane this rank does not own
        rng = igg.owned_ranges(probe)
        for d, (a, b) in enumerate(rng):
            sl = [slice(None)] * len(shape)
            sl[d] = slice(0, a)
            A[tuple(sl)] = math.nan
            sl[d] = slice(b, shape[d])
            A[tuple(sl)] = math.nan
    return A.to(device)


def _slices(sel_shape, ext, box, step):
    nd = len(ext)
    box = box if box is not None else (None,) * nd
    step = (step,) * nd if isinstance(step, int) else step
    out = []
    for d in range(nd):
        b = box[d]
        lo, hi = (0, ext[d]) if b is None else (b, b + 1) if isinstance(b, int) else b
        out.append(slice(lo, hi, step[d]))
    return tuple(out)


def _check(me, gg, A, Fg, ext, *, root=0, box=None, step=1, dtype=None, cpu_out=False, tag=""):
    out_dtype = A.dtype if dtype is None else dtype
    shape = igg.selection_shape_g(A, box, step)
    want = Fg[_slices(shape, ext, box, step)].to(out_dtype)
    assert tuple(want.shape) == shape, (tag, tuple(want.shape), shape)
    G = None
    if me == root:
        G = torch.full(shape, -7, dtype=out_dtype, device="cpu" if cpu_out else A.device)
    igg.gather_g(A, G, root=root, box=box, step=step, dtype=dtype)
    if me == root:
        got = G.cpu()
        if not torch.equal(got, want):
            bad = (got != want).nonzero()[:5].tolist()
            raise AssertionError(f"rank {me} {tag} {tuple(A.shape)} box={box} step={step} dtype={dtype}: differs at "
                                 f"{bad}: got {[got[tuple(b)].item() for b in bad]}, "
                                 f"want {[want[tuple(b)].item() for b in bad]}")


def scenario_gather(dev, dtype, dimx, dimy, dimz, periodic, overlap, halowidth):
    device = _device(dev)
    dt = getattr(torch, dtype)
    per, o, w = int(periodic), int(overlap), int(halowidth)
    me, dims, nprocs, coords, comm = igg.init_global_grid(
        *N, dimx=int(dimx), dimy=int(dimy), dimz=int(dimz), periodx=per & 1, periody=(per >> 1) & 1,
        periodz=(per >> 2) & 1, overlapx=o, overlapy=o, overlapz=o, halowidthx=w, halowidthy=w, halowidthz=w,
        quiet=True, select_device=False, device_type="none" if dev == "cpu" else "AMDGPU")
    gg = igg.get_global_grid()
    last = nprocs - 1
    for shape in (N, (N[0] + 1, N[1], N[2]), (N[0], N[1] - 1, N[2])):  # the grid's size, two staggered ones
        ext = _extents(gg, shape)
        Fg = _global_array(ext)
        A = _local(gg, shape, Fg, dt, device)
        kw = dict(me=me, gg=gg, A=A, Fg=Fg, ext=ext)
        # first, a box the last rank in x owns nothing of: it sends nothing, yet must not leave the others waiting
        _check(**kw, box=((2, 4), None, None), tag="box that misses ranks")
        _check(**kw, tag="whole")
        _check(**kw, box=(N[0] - o, None, None), tag="x-plane two ranks hold")
        _check(**kw, box=(None, ext[1] // 2, None), root=last, tag="y-plane, last root")
        _check(**kw, box=((1, ext[0] - 1), None, (2, ext[2])), step=(2, 3, 1), tag="box with steps")
        _check(**kw, step=3, root=last, tag="step 3")
        if dt == torch.float64:
            _check(**kw, dtype=torch.float32, tag="f32 whole")
            _check(**kw, box=((1, ext[0] - 1), None, (2, ext[2])), step=(2, 3, 1), dtype=torch.float32, root=last,
                   tag="f32 box with steps")
        if dev != "cpu":
            _check(**kw, cpu_out=True, tag="A_global on the CPU")
            _check(**kw, box=(None, ext[1] // 2, None), dtype=torch.float32 if dt == torch.float64 else None,
                   cpu_out=True, tag="plane, A_global on the CPU")
    # other same-dtype paths, and fields of fewer dimensions
    Fg = _global_array(_extents(gg, N))
    for other in (torch.float32, torch.int32):
        A = _local(gg, N, Fg, other, device)
        _check(me, gg, A, Fg, _extents(gg, N), tag=str(other))
        _check(me, gg, A, Fg, _extents(gg, N), box=(None, None, 3), step=(2, 1, 1), root=last, tag=str(other))
    for shape in (N[:2], N[:1], (N[0] + 1,)):
        ext = _extents(gg, shape)
        Fg2 = _global_array(ext)
        A = _local(gg, shape, Fg2, dt, device)
        _check(me, gg, A, Fg2, ext, tag="low-dimensional")
        _check(me, gg, A, Fg2, ext, box=((1, ext[0] - 1),) + (None,) * (len(shape) - 1), step=2, root=last,
               dtype=torch.float32 if dt == torch.float64 else None, tag="low-dimensional box")
    igg.finalize_global_grid()
    print(f"rank {me} gather_g OK")


def scenario_fused(nx, ny, nz, steps):
    """A fused Diffusion3D after ``steps`` steps WITHOUT sync_halo(): its
    halos are stale, gather_g reads owned cells only and must give the global
    field of the same model run with update_halo_."""
    from igg.models.diffusion3d import Diffusion3D

    device = _device("gpu")
    me, dims, nprocs, coords, comm = igg.init_global_grid(int(nx), int(ny), int(nz), quiet=True, select_device=False)
    steps = int(steps)
    a = Diffusion3D(dtype=torch.float64, device=device, variant=0)
    f = Diffusion3D(dtype=torch.float64, device=device, variant=0)
    assert f.set_fused(True), "fused mode unavailable"
    a.run(steps)
    f.run(steps)
    shape = igg.selection_shape_g(a.T)
    Ga = torch.zeros(shape, dtype=torch.float64, device=device) if me == 0 else None
    Gf = torch.full(shape, -1.0, dtype=torch.float64, device=device) if me == 0 else None
    igg.gather_g(a.T, Ga)
    igg.gather_g(f.T, Gf)
    plane = (None, shape[1] // 2, None)
    Pf = torch.full(igg.selection_shape_g(f.T, plane), -1.0, dtype=torch.float32, device=device) if me == 0 else None
    igg.gather_g(f.T, Pf, box=plane, dtype=torch.float32)
    torch.cuda.synchronize()
    if me == 0:
        assert shape == tuple(int(v) for v in igg.get_global_grid().nxyz_g)
        assert torch.equal(Ga, Gf), "the fused model's global field differs"
        assert torch.equal(Pf, Ga[:, shape[1] // 2:shape[1] // 2 + 1, :].float())
        assert Ga.max().item() > 1.0
    f.sync_halo()
    torch.cuda.synchronize()
    f.close()
    igg.finalize_global_grid()
    print(f"rank {me} gather_g OK")


if __name__ == "__main__":
    name, *args = sys.argv[1:]
    globals()[f"scenario_{name}"](*args)
