"""Per-rank scenario of the ``Acoustic2D.adjoint_run`` tests, launched by
tests/test_acoustic_adjoint_cpu.py and tests/test_gpu_acoustic_adjoint.py, one
process per rank - and the helpers both files share.

The model is dyadic (``dt = 1/4``, ``K = rho = 1``, ``dx = dy = 1/2``) and the
fields are integers in [-8, 8], so three steps, forward or transposed, are
exact in float32 and float64 in any order of summation:

(a) ``sum <g, run(3) x> == sum <adjoint_run(3, g), x>`` over the three fields
    and the ranks (``comm.allreduce``), with independent ``x`` and ``g`` per rank;
(b) seeded from one global ``g`` per field placed on owned cells only, the
    ranks' ``adjoint_run(3)``, every local cell added to its global cell
    (``indices_g``) and summed over the ranks, equals the same of a single
    rank on the global grid, bit for bit.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import igg  # noqa: E402
from tests.mp_worker_sample_g import _device, extents, global_values  # noqa: E402

N_LOCAL = (6, 7)  # local (nx, ny) of every rank
DKW = dict(dt=0.25, K=1.0, rho=0.5, dx=0.5, dy=0.25)  # a = 1/4, b = 1/2, 1/dx = 2, 1/dy = 4 (the operator tests)
MKW = dict(dt=0.25, K=1.0, rho=1.0, dx=0.5, dy=0.5)   # the dyadic model


def single_rank_size(dims, overlap=2):
    """Local size of the one rank whose grid is the ranks' global grid."""
    return tuple(d * (n - overlap) + overlap for d, n in zip(dims, N_LOCAL))


def dyadic_model(device, dtype, **kw):
    from igg.models.acoustic2d import Acoustic2D

    m = Acoustic2D(dtype=dtype, device=device, **kw)
    m.dt, m.K, m.rho, m.dx, m.dy = (MKW[k] for k in ("dt", "K", "rho", "dx", "dy"))
    return m


def int_fields(m, seed):
    """Integer fields in [-8, 8] of the model's shapes, dtype and device,
    different on every rank."""
    gen = torch.Generator().manual_seed(1000 * seed + int(igg.get_global_grid().me))
    return [torch.randint(-8, 9, tuple(F.shape), generator=gen).to(m.dtype).to(m.device) for F in (m.P, m.Vx, m.Vy)]


def set_fields(m, x):
    for dst, src in zip((m.P, m.Vx, m.Vy), x):
        dst.copy_(src)
    m.mark_modified()


def inner(a, b):
    return sum((s.double() * t.double()).sum().item() for s, t in zip(a, b))


def identity_sides(m, nt, seed=0):
    """(sum <g, run(nt) x>, sum <adjoint_run(nt, g), x>) of this rank."""
    x, g = int_fields(m, seed + 1), int_fields(m, seed + 2)
    res = m.adjoint_run(nt, *g)
    set_fields(m, x)
    m.run(nt)
    return inner(g, (m.P, m.Vx, m.Vy)), inner(res, x)


def global_adjoint(m, nt):
    """``adjoint_run(nt)`` from one global seed per field, placed on owned
    cells only; every local cell of the result is added to its global cell and
    the ranks are summed: the three global arrays (float64, CPU, on every rank)."""
    gg = igg.get_global_grid()
    me, comm = int(gg.me), gg.comm
    seeds, Es = [], []
    for k, F in enumerate((m.P, m.Vx, m.Vy)):
        E = extents(gg, tuple(F.shape))
        Es.append(E)
        G = (torch.remainder((global_values(E, 20 + k) * 64).round(), 17.0) - 8.0) if me == 0 else None
        loc = torch.zeros(tuple(F.shape), dtype=torch.float64, device=m.device)
        igg.scatter_g(G, loc)
        g = torch.zeros_like(loc)
        own = tuple(slice(a, b) for a, b in igg.owned_ranges(loc))
        g[own] = loc[own]
        seeds.append(g.to(m.dtype))
    names = ("P", "Vx", "Vy", "P2", "Vx2", "Vy2")
    before = [getattr(m, k).clone() for k in names]
    res = m.adjoint_run(nt, *seeds)
    assert all(torch.equal(getattr(m, k), b) for k, b in zip(names, before)), "adjoint_run touched the model's fields"
    out = []
    for r, E in zip(res, Es):
        r = r.double().cpu()
        ix, iy = igg.indices_g(0, r), igg.indices_g(1, r)
        G = torch.zeros(E[0] * E[1], dtype=torch.float64)
        G.index_add_(0, (ix.view(-1, 1) * E[1] + iy.view(1, -1)).flatten(), r.flatten())
        out.append(comm.allreduce_(G, "sum").view(E))  # (CPU tensor: the host group, also for a GPU model)
    return out


def scenario_adjoint_run(dev, dimx, dimy, periodic, nt, ref_path, dtype="f64"):
    device = _device(dev)
    per, nt = int(periodic), int(nt)
    me, dims, nprocs, coords, comm = igg.init_global_grid(
        *N_LOCAL, 1, dimx=int(dimx), dimy=int(dimy), dimz=1, periodx=per, periody=per, quiet=True,
        select_device=False, device_type="none" if dev == "cpu" else "AMDGPU")
    m = dyadic_model(device, torch.float64 if dtype == "f64" else torch.float32)
    # (a)
    lhs, rhs = identity_sides(m, nt)
    lhs, rhs = comm.allreduce(lhs), comm.allreduce(rhs)
    assert lhs == rhs and lhs != 0, (lhs, rhs)
    # (b)
    got = global_adjoint(m, nt)
    ref = np.load(ref_path)
    for k, G in zip(("P", "Vx", "Vy"), got):
        want = torch.from_numpy(ref[k])
        assert G.shape == want.shape, (k, G.shape, want.shape)
        assert torch.equal(G, want), f"{k}: {int((G != want).sum())} cells differ from the single-rank run"
    igg.finalize_global_grid()
    print(f"rank {me} acoustic adjoint OK")


def run_ranks(nprocs: int, *args, timeout: float = 150.0, env_extra=None) -> list:
    """``tests/mp_worker_acoustic_adjoint.py adjoint_run ...`` on ``nprocs``
    local ranks: the first rank that fails stops the others, a timeout fails
    the test with every rank's output."""
    import subprocess
    import tempfile
    import time

    from tests._mp import MAX_TIMEOUT, free_port

    port = free_port()
    procs, logs = [], []
    for r in range(nprocs):
        env = dict(os.environ)
        env.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(r),
                    "WORLD_SIZE": str(nprocs), "LOCAL_RANK": str(r), "LOCAL_WORLD_SIZE": str(nprocs),
                    "OMP_NUM_THREADS": "1", "IGG_HOST_THREADS": "2",
                    "PYTHONPATH": ROOT + os.pathsep + env.get("PYTHONPATH", "")})
        env.update(env_extra or {})
        log = tempfile.TemporaryFile(mode="w+")
        logs.append(log)
        procs.append(subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "adjoint_run", *map(str, args)],
            env=env, stdout=log, stderr=subprocess.STDOUT, text=True, cwd=ROOT))
    deadline = time.monotonic() + min(timeout, MAX_TIMEOUT)
    try:
        while True:
            codes = [p.poll() for p in procs]
            if any(c not in (None, 0) for c in codes) or all(c == 0 for c in codes) or time.monotonic() > deadline:
                break
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    outs = []
    for log in logs:
        log.seek(0)
        outs.append(log.read())
        log.close()
    codes = [p.returncode for p in procs]
    if any(c != 0 for c in codes):
        msg = "\n".join(f"--- rank {r} rc={c}\n{o[-2500:]}" for r, (c, o) in enumerate(zip(codes, outs)))
        raise AssertionError(f"acoustic adjoint ranks {args} failed or timed out:\n{msg}")
    for r, o in enumerate(outs):
        assert f"rank {r} acoustic adjoint OK" in o, o[-1500:]
    return outs


if __name__ == "__main__":
    name, *args = sys.argv[1:]
    globals()[f"scenario_{name}"](*args)
