#!/usr/bin/env python3
"""3-D heat diffusion with in-situ PROFILES of the global field.

Every ``--every`` steps ``project_g`` reduces the true global temperature
field over some of its axes and keeps the others: the plane-mean profile
``T(x)`` (the mean over y and z, printed by rank 0) and the maximum over z as a
map over x and y (written with ``np.save``). No volume is gathered and no
rank reduces another rank's cells: every rank reduces the cells it owns, one
all-reduce of the profile (or the map) combines the ranks, and every rank
holds the result. Only owned cells are read, so no ``sync_halo()`` is needed
on a fused model. Pass ``--device cpu`` for host fields.

    torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 8 \\
        examples/diffusion3D_profiles.py --nx 128 --nt 2000 --every 200
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import igg  # noqa: E402
from igg.models.diffusion3d import Diffusion3D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=128)
    ap.add_argument("--ny", type=int, default=None, help="default: --nx")
    ap.add_argument("--nz", type=int, default=None, help="default: --nx")
    ap.add_argument("--nt", type=int, default=2000)
    ap.add_argument("--every", type=int, default=200)
    ap.add_argument("--device", choices=("auto", "cpu"), default="auto")
    ap.add_argument("--out", default="diffusion3D_profiles", help="prefix of the .npy files")
    a = ap.parse_args()
    import numpy as np
    import torch

    cpu = a.device == "cpu"
    nx, ny, nz = a.nx, a.ny or a.nx, a.nz or a.nx
    me, dims, nprocs, coords, comm = igg.init_global_grid(nx, ny, nz, device_type="none" if cpu else "auto")
    model = Diffusion3D(dtype=torch.float64, device="cpu" if cpu else None)
    gshape = igg.selection_shape_g(model.T)
    profile = torch.zeros(gshape[0], dtype=torch.float64, device=model.T.device)
    zmax = torch.zeros(gshape[:2], dtype=torch.float64, device=model.T.device)
    profiles, written = [], 0
    for it in range(a.nt + 1):
        if it % a.every == 0:
            igg.project_g("mean", model.T, 0, out=profile)   # T(x): the mean over the global y-z planes
            igg.project_g("max", model.T, (0, 1), out=zmax)  # the maximum over z of every global column
            if me == 0:
                p = profile.cpu().numpy()
                profiles.append(p.copy())
                np.save(f"{a.out}_zmax_{it:06d}.npy", zmax.cpu().numpy())
                written += 1
                k = max(1, len(p) // 8)
                print(f"step {it:6d}: mean T(x) = [{' '.join(f'{v:.4f}' for v in p[::k])}], max T = {zmax.max().item():.4f}")
        if it < a.nt:
            model.step()
    if me == 0:
        np.save(f"{a.out}_mean_x.npy", np.stack(profiles))
        print(f"wrote {written} z-maximum maps of {gshape[0]}x{gshape[1]} cells and {len(profiles)} profiles of "
              f"{gshape[0]} cells of the {igg.nx_g()}x{igg.ny_g()}x{igg.nz_g()} global grid")
    igg.finalize_global_grid()


if __name__ == "__main__":
    main()
