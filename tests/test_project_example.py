"""examples/diffusion3D_profiles.py runs end to end on two CPU ranks at a tiny
size, and what it writes is what the global field says."""
import os
import subprocess
import sys

import numpy as np

from tests._mp import MAX_TIMEOUT, ROOT, free_port


def test_profiles_example_on_two_cpu_ranks(tmp_path):
    out = str(tmp_path / "p")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "examples", "diffusion3D_profiles.py"),
           "--nx", "16", "--ny", "12", "--nz", "10", "--nt", "20", "--every", "10", "--device", "cpu", "--out", out]
    env = dict(os.environ, OMP_NUM_THREADS="1", IGG_HOST_THREADS="2")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=MAX_TIMEOUT, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "wrote 3 z-maximum maps of 30x12 cells and 3 profiles of 30 cells of the 30x12x10 global grid" in r.stdout
    prof = np.load(out + "_mean_x.npy")
    assert prof.shape == (3, 30) and prof.dtype == np.float64 and np.isfinite(prof).all()
    maps = [np.load(f"{out}_zmax_{it:06d}.npy") for it in (0, 10, 20)]
    assert all(m.shape == (30, 12) and np.isfinite(m).all() for m in maps)
    # a column's maximum is at least its plane's mean; diffusion flattens the field and, with fixed boundary
    # values, never raises its maximum
    for p, m in zip(prof, maps):
        assert (m.max(axis=1) >= p - 1e-12).all()
    assert maps[2].max() <= maps[0].max() + 1e-12
    assert not np.array_equal(prof[0], prof[2])
