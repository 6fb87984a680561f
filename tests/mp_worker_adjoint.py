"""Per-rank scenario of the ``Diffusion3D.adjoint_run`` tests, launched by
tests/test_diffusion_adjoint_cpu.py and tests/test_gpu_diffusion_adjoint.py,
one process per rank - and the helpers both files share: dyadic global fields
built from global indices, and the adjoint run of a model on whatever grid is
initialised, brought home to the global grid.

Everything is dyadic (``g`` multiples of 1/64, ``Cp`` in {1, 2, 4},
``dt*lam = 1/8``, ``1/d^2 = 1, 4, 16``), so three adjoint steps are exact in
float64 in any order of summation and the ranks' result must equal the
single-rank run on the global grid bit for bit.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import igg  # noqa: E402
from tests.mp_worker_sample_g import _device, extents, global_values, local_of_global  # noqa: E402

N_LOCAL = (6, 5, 7)  # local size of every rank
KW = dict(lam=1.0, dt=0.125, dx=1.0, dy=0.5, dz=0.25)


def single_rank_size(dims, overlap=2):
    """Local size of the one rank whose grid is the ranks' global grid."""
    return tuple(d * (n - overlap) + overlap for d, n in zip(dims, N_LOCAL))


def global_cp(E) -> torch.Tensor:
    """1, 2 or 4 at every global cell."""
    return torch.pow(2.0, torch.remainder((global_values(E, 5) * 64).abs().round(), 3.0))


def make_model(device):
    """A float64 ``Diffusion3D`` on the initialised grid with the dyadic
    constants, ``Cp`` from the global cells, and the seed ``g``: a functional of the
    global field, ``sum over the global cells of g * T``."""
    from igg.models.diffusion3d import Diffusion3D

    gg = igg.get_global_grid()
    m = Diffusion3D(dtype=torch.float64, device=device, variant=0)
    shape = tuple(m.T.shape)
    E = extents(gg, shape)
    m.lam, m.dt, m.dx, m.dy, m.dz = KW["lam"], KW["dt"], KW["dx"], KW["dy"], KW["dz"]
    m.Cp.copy_(local_of_global(global_cp(E), shape))
    # the seed counts every global cell once: its value in the owned cells, 0 in the other copies
    g = torch.zeros(shape, dtype=torch.float64)
    own = tuple(slice(a, b) for a, b in igg.owned_ranges(g))
    g[own] = local_of_global(global_values(E, 9), shape)[own]
    return m, g.to(device), E


def adjoint_global(m, g, nt, E):
    """``adjoint_run`` then one more ``accumulate_halo_``: the gradient with
    respect to the global initial field, gathered on rank 0 (None elsewhere)."""
    T0, T20 = m.T.clone(), m.T2.clone()
    g0 = g.clone()
    res = m.adjoint_run(nt, g)
    assert res is not g and res.shape == g.shape and torch.equal(g, g0), "g was modified"
    out = torch.full_like(g, 3.0)
    assert m.adjoint_run(nt, g, out=out) is out and torch.equal(out, res)
    assert torch.equal(m.T, T0) and torch.equal(m.T2, T20), "adjoint_run touched T or T2"
    igg.accumulate_halo_(res)
    me = int(igg.get_global_grid().me)
    G = torch.empty(E, dtype=res.dtype, device=res.device) if me == 0 else None
    igg.gather_g(res, G)
    return G


def scenario_adjoint_run(dev, dimx, dimy, dimz, periodic, nt, ref_path):
    device = _device(dev)
    per = int(periodic)
    me, dims, nprocs, coords, comm = igg.init_global_grid(
        *N_LOCAL, dimx=int(dimx), dimy=int(dimy), dimz=int(dimz), periodx=per, periody=per, periodz=per,
        quiet=True, select_device=False, device_type="none" if dev == "cpu" else "AMDGPU")
    m, g, E = make_model(device)
    G = adjoint_global(m, g, int(nt), E)
    if me == 0:
        want = torch.from_numpy(np.load(ref_path))
        got = G.cpu()
        assert got.shape == want.shape, (got.shape, want.shape)
        assert torch.equal(got, want), f"{int((got != want).sum())} cells differ from the single-rank run"
    igg.finalize_global_grid()
    print(f"rank {me} adjoint OK")


def run_adjoint_ranks(nprocs: int, scenario: str, *args, timeout: float = 150.0, env_extra=None) -> list:
    """``tests/mp_worker_adjoint.py <scenario> ...`` on ``nprocs`` local ranks
    (the launcher of tests/test_accumulate_halo_cpu.py): the first rank that
    fails stops the others, a timeout fails the test with every rank's output."""
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
            [sys.executable, os.path.join(ROOT, "tests", "mp_worker_adjoint.py"), scenario, *map(str, args)],
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
        raise AssertionError(f"adjoint scenario {scenario} {args} failed or timed out:\n{msg}")
    for r, o in enumerate(outs):
        assert f"rank {r} adjoint OK" in o, o[-1500:]
    return outs


if __name__ == "__main__":
    name, *args = sys.argv[1:]
    globals()[f"scenario_{name}"](*args)
