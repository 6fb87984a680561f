#!/usr/bin/env python3
"""3-D heat diffusion with in-situ visualisation of ONE plane of the global field.

Every ``--vis-every`` steps ``gather_g`` assembles the y-mid plane of the true
global temperature field on rank 0 - only that plane's owned cells travel,
converted to float32 at the senders - and appends it to an animated GIF
(utils/vis.py). Unlike examples/diffusion3D_multigpu.py there is no halo-free
copy of the field, no gather of the whole volume and no volume-sized array on
the root, the outermost global cells are part of the picture, and the result
is the global field for every overlap, periodicity and fused mode. Pass
``--cpu`` for host fields.

    torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 8 \\
        examples/diffusion3D_slices.py --nx 128 --nt 2000 --vis-every 100
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import igg  # noqa: E402
from igg.models.diffusion3d import Diffusion3D  # noqa: E402
from igg.utils.vis import Animation  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=128)
    ap.add_argument("--nt", type=int, default=2000)
    ap.add_argument("--vis-every", type=int, default=100)
    ap.add_argument("--out", default="diffusion3D_slices.gif")
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    import torch

    nx = a.nx
    me, dims, nprocs, coords, comm = igg.init_global_grid(nx, nx, nx, device_type="none" if a.cpu else "auto")
    model = Diffusion3D(dtype=torch.float64, device="cpu" if a.cpu else None)
    plane = (None, igg.ny_g() // 2, None)  # the y-mid plane of the global grid
    shape = igg.selection_shape_g(model.T, plane)
    T_v = torch.zeros(shape, dtype=torch.float32, device=model.T.device) if me == 0 else None
    anim = Animation()
    for it in range(a.nt):
        if it % a.vis_every == 0:
            igg.gather_g(model.T, T_v, box=plane, dtype=torch.float32)  # owned cells only: no sync_halo() needed
            if me == 0:
                anim.frame(T_v[:, 0, :].T, scale=max(1, 256 // shape[0]))
        model.step()
    if me == 0:
        anim.save_gif(a.out, fps=15)
        print(f"wrote {a.out} ({len(anim.frames)} frames of the {shape[0]}x{shape[2]} y-mid plane of the "
              f"{igg.nx_g()}x{igg.ny_g()}x{igg.nz_g()} global grid)")
    igg.finalize_global_grid()


if __name__ == "__main__":
    main()
