#!/usr/bin/env python3
"""3-D heat diffusion restarted on a DIFFERENT decomposition.

``--save F.npz`` runs ``--nt`` steps and writes the true global fields of ``T``
and ``Cp`` (``gather_g``, on rank 0) with the number of steps taken so far.
``--init F.npz`` starts from such a file instead of the analytic initial
condition: rank 0 reads the global arrays, ``scatter_g`` fills ``model.T`` and
``model.Cp`` of every rank - halo cells included, so no ``update_halo_``
follows - and the run continues. The file knows nothing of the ranks that
wrote it: the local sizes only have to give the same global grid. Both options
combine. Pass ``--cpu`` for host fields.

    torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 2 \\
        examples/diffusion3D_regrid.py --nx 128 --nt 1000 --save T.npz
    python examples/diffusion3D_regrid.py --nx 254 --ny 128 --nz 128 --nt 1000 --init T.npz
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
    ap.add_argument("--nt", type=int, default=1000)
    ap.add_argument("--init", default=None, metavar="F.npz", help="start from the global fields of this file")
    ap.add_argument("--save", default=None, metavar="F.npz", help="write the global fields after the run")
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch

    nx, ny, nz = a.nx, a.ny or a.nx, a.nz or a.nx
    me, dims, nprocs, coords, comm = igg.init_global_grid(nx, ny, nz, device_type="none" if a.cpu else "auto")
    model = Diffusion3D(dtype=torch.float64, device="cpu" if a.cpu else None)
    size_g = igg.selection_shape_g(model.T)
    steps = 0
    if a.init:
        T_g = Cp_g = None
        if me == 0:
            with np.load(a.init) as f:
                T_g, Cp_g, steps = torch.from_numpy(f["T"]), torch.from_numpy(f["Cp"]), int(f["steps"])
            if tuple(T_g.shape) != size_g:
                comm.abort(f"{a.init} holds a {tuple(T_g.shape)} global grid, this run has {size_g}")
        steps = int(comm.broadcast_object(steps, 0))
        igg.scatter_g(T_g, model.T)  # a CPU array on the root: every local cell, halos included
        igg.scatter_g(Cp_g, model.Cp)
        model.T2.copy_(model.T)
        model.mark_cp_modified()
        model.mark_modified()
    model.run(a.nt)
    steps += a.nt
    if a.save:
        T_g, Cp_g = (torch.zeros(size_g, dtype=torch.float64) if me == 0 else None for _ in range(2))
        igg.gather_g(model.T, T_g)
        igg.gather_g(model.Cp, Cp_g)
        if me == 0:
            np.savez(a.save, T=T_g.numpy(), Cp=Cp_g.numpy(), steps=steps)
    if me == 0:
        print(f"{'x'.join(map(str, size_g))} global grid on {nprocs} ranks: {a.nt} steps, {steps} in all"
              + (f", wrote {a.save}" if a.save else ""))
    igg.finalize_global_grid()


if __name__ == "__main__":
    main()
