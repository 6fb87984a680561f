"""Per-rank scenarios of the wide-halo tests (halo widths above 1), launched
by tests/test_wide_halo_cpu.py and tests/test_gpu_wide_halo.py, one process
per rank."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import igg  # noqa: E402


def _device(kind):
    """cpu | gpu (every rank on device 0) | mgpu (one rank per device: LOCAL_RANK)."""
    if kind == "mgpu":
        r = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(r)
        return torch.device("cuda", r)
    if kind == "gpu":
        torch.cuda.set_device(0)
        return torch.device("cuda", 0)
    return torch.device("cpu")


def _global_code(gg, shape):
    """1 + linear global coordinate of every local cell (overlapping cells of
    neighbouring ranks get the same code; periodic dimensions wrap)."""
    idx = []
    for d in range(3):
        n, o = int(gg.nxyz[d]), int(gg.overlaps[d])
        g = int(gg.coords[d]) * (n - o) + torch.arange(shape[d], dtype=torch.int64)
        if int(gg.periods[d]):
            g = g % int(gg.nxyz_g[d])
        idx.append(g)
    ng = [int(v) + 1 for v in gg.nxyz_g]  # room for a staggered field's extra plane
    return 1 + (idx[0].view(-1, 1, 1) * ng[1] + idx[1].view(1, -1, 1)) * ng[2] + idx[2].view(1, 1, -1)


def _halo_masks(gg, shape, w):
    """(in a halo plane of any dimension, in one with no neighbour behind it)."""
    any_halo = torch.zeros(shape, dtype=torch.bool)
    dead = torch.zeros(shape, dtype=torch.bool)
    for d in range(3):
        for side in range(2):
            sl = [slice(None)] * 3
            sl[d] = slice(0, w) if side == 0 else slice(shape[d] - w, shape[d])
            any_halo[tuple(sl)] = True
            if int(gg.neighbors[side, d]) < 0:
                dead[tuple(sl)] = True
    return any_halo, dead


def scenario_halo(dev, periodic, dimx, dimy, dimz):
    """Every cell holds its global coordinate, the halo planes are zeroed,
    update_halo_ runs: a halo cell with a neighbour behind it (in every
    dimension whose halo it lies in) holds its own global coordinate again,
    one on a physical boundary is still zero. Sequential and one-phase
    schedules with width 2; the one-phase message count is printed for width
    2 and for width 1 on the same grid."""
    from igg.parallel import halo as H

    device = _device(dev)
    per = int(periodic)
    n = (12, 11, 13)
    counts = {}
    first = True
    for w in (2, 1):
        igg.init_global_grid(*n, periodx=per, periody=per, periodz=per, dimx=int(dimx), dimy=int(dimy),
                             dimz=int(dimz), overlapx=4, overlapy=4, overlapz=4, halowidthx=w, halowidthy=w,
                             halowidthz=w, quiet=True, select_device=False, init_MPI=first,
                             device_type="none" if dev == "cpu" else "AMDGPU")
        first = False
        gg = igg.get_global_grid()
        for mode in ("sequential", "onephase"):
            H.set_halo_mode(mode)
            for shape in (n, (n[0] + 1, n[1], n[2])):
                code = _global_code(gg, shape).to(torch.float64)
                halo, dead = _halo_masks(gg, shape, w)
                # staggered field: its overlap is one more, the halo is still w planes
                exp = torch.where(dead, torch.zeros_like(code), code)
                X = torch.where(halo, torch.zeros_like(code), code).to(device)
                igg.update_halo_(X)
                got = X.cpu()
                if not torch.equal(got, exp):
                    bad = (got != exp).nonzero()[:5].tolist()
                    raise AssertionError(f"rank {gg.me} w={w} {mode} shape {shape}: mismatch at {bad}")
            if mode == "onephase":
                counts[w] = H.engine().last_message_count
        igg.finalize_global_grid(finalize_MPI=(w == 1))
    print(f"rank {gg.me} wide halo OK MSGS2={counts[2]} MSGS1={counts[1]}")


def scenario_model(dev, nx, ny, nz, steps, graph, dimx, dimy, dimz):
    """Diffusion3D on a grid with overlap 4 and halo width 2: the two-step
    pass (one exchange of two planes per two steps) against single steps,
    bitwise per rank; the single-step model against the same physics on the
    global grid in one array; the automatic choice is the same on every rank."""
    from igg.models.diffusion3d import Diffusion3D
    from igg.ops import stencil

    device = _device(dev)
    nx, ny, nz, steps, graph = int(nx), int(ny), int(nz), int(steps), int(graph)
    me, dims, nprocs, coords, comm = igg.init_global_grid(
        nx, ny, nz, dimx=int(dimx), dimy=int(dimy), dimz=int(dimz), overlapx=4, overlapy=4, overlapz=4,
        halowidthx=2, halowidthy=2, halowidthz=2, quiet=True, select_device=False, device_type="AMDGPU")
    gg = igg.get_global_grid()
    models = {}
    for name, env in (("single", "0"), ("pass", "1"), ("auto", "auto")):
        os.environ["IGG_STENCIL_TWOSTEP"] = env
        models[name] = Diffusion3D(dtype=torch.float64, device=device, variant=0)
    a, b, c = models["single"], models["pass"], models["auto"]
    assert not a._two_step_now() and b._two_step_now(), "forced choices ignored"
    assert not b.fused_available()
    a.run(steps)
    if graph:
        b.capture(graph)  # performs the eager first step (and its exchange) itself
        b.run(steps - 1)
    else:
        b.run(steps)
    torch.cuda.synchronize()
    if not torch.equal(a.T, b.T):
        bad = (a.T != b.T).nonzero()[:5].tolist()
        raise AssertionError(f"rank {me}: the two-step model differs from single steps at {bad}")
    loc = a.T.cpu()
    ng = [int(v) for v in gg.nxyz_g]
    lx = ly = lz = 10.0
    dx, dy, dz = lx / (ng[0] - 1), ly / (ng[1] - 1), lz / (ng[2] - 1)
    x = (torch.arange(ng[0], dtype=torch.float64) * dx).view(-1, 1, 1)
    y = (torch.arange(ng[1], dtype=torch.float64) * dy).view(1, -1, 1)
    z = (torch.arange(ng[2], dtype=torch.float64) * dz).view(1, 1, -1)
    Cp = 1 + 5 * torch.exp(-(x - lx / 1.5) ** 2 - (y - ly / 2) ** 2 - (z - lz / 1.5) ** 2) + \
        5 * torch.exp(-(x - lx / 3.0) ** 2 - (y - ly / 2) ** 2 - (z - lz / 1.5) ** 2)
    T = 100 * torch.exp(-((x - lx / 2) / 2) ** 2 - ((y - ly / 2) / 2) ** 2 - ((z - lz / 3.0) / 2) ** 2) + \
        50 * torch.exp(-((x - lx / 2) / 2) ** 2 - ((y - ly / 2) / 2) ** 2 - ((z - lz / 1.5) / 2) ** 2)
    for _ in range(steps):
        T = stencil.diffusion3d_reference(T, Cp, lam=a.lam, dt=a.dt, dx=a.dx, dy=a.dy, dz=a.dz)
    o = [int(coords[d]) * (int(gg.nxyz[d]) - int(gg.overlaps[d])) for d in range(3)]
    blk = T[o[0]:o[0] + nx, o[1]:o[1] + ny, o[2]:o[2] + nz]
    err = (loc - blk).abs().max().item()
    print(f"rank {me}: err {err:.3e}")
    assert err < 1e-10, f"rank {me}: diffusion mismatch {err}"
    two = int(c.two_step)
    igg.finalize_global_grid()
    print(f"rank {me} wide model OK TWO={two}")


if __name__ == "__main__":
    name, *args = sys.argv[1:]
    globals()[f"scenario_{name}"](*args)
