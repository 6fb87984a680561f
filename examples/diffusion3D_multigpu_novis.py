#!/usr/bin/env python3
"""3-D heat diffusion on multiple MI355X GPUs, no visualisation.

Counterpart of the reference's examples/diffusion3D_multigpu_CuArrays_novis.jl
(same physics, initial conditions and time step), written against this
framework: the per-step update is ONE fused HIP stencil kernel instead of five
broadcasts, followed by update_halo_(T).

    torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 8 \\
        examples/diffusion3D_multigpu_novis.py --nx 256 --nt 1000
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import igg  # noqa: E402
from igg.models.diffusion3d import Diffusion3D, t_eff_gbs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=256)
    ap.add_argument("--nt", type=int, default=1000)
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--fused", action="store_true",
                    help="exchange halos from inside the stencil kernel (peer stores over xGMI) instead of update_halo_")
    a = ap.parse_args()
    import torch

    me, dims, nprocs, coords, comm = igg.init_global_grid(a.nx, a.nx, a.nx)  # Initialize the implicit global grid
    model = Diffusion3D(dtype=getattr(torch, a.dtype))                       # lam=1, cp_min=1, l=10, Gaussian ICs
    if a.fused:
        model.set_fused(True)                                                # collective; no-op without neighbours
    model.run(10)                                                            # warm-up (kernel variant, buffers)
    model.capture()                                                          # hipGraph of GRAPH_STEPS steps
    igg.tic()
    model.run(a.nt)
    t = igg.toc()
    model.sync_halo()                                                        # halos of T valid again (fused mode)
    model.close()
    t_max = igg.max_g(model.T)                                               # global max (HIP reduction + RCCL)
    t_mean = igg.mean_g(model.T)                                             # every global cell counted once
    if me == 0:
        t_it = t / a.nt
        print(f"{nprocs} process(es) {dims.tolist()}, local {a.nx}^3, global {igg.nx_g()}x{igg.ny_g()}x{igg.nz_g()}: "
              f"{t:.3f} s, {t_it * 1e3:.4f} ms/step, T_eff = {t_eff_gbs(model, t_it):.1f} GB/s per GPU, "
              f"global T_max = {float(t_max):.6f}, global T_mean = {float(t_mean):.6f}")
    igg.finalize_global_grid()                                               # Finalize the implicit global grid


if __name__ == "__main__":
    main()
