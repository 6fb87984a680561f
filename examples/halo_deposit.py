#!/usr/bin/env python3
"""Deposit into halo cells and bring the contributions home.

Every rank adds a contribution to ALL of its local cells, halo cells included -
as a particle-to-grid deposit or a flux assembly does when a particle or a face
sits in the overlap. A cell of the global grid that several ranks hold then has
one partial sum per copy. ``accumulate_halo_`` adds the halo copies into the
cells of the ranks that own them (and zeroes the halos); ``update_halo_``
copies the totals back out. With ``overlap == 2*halowidth`` every copy of a
cell then holds the total of all contributions to that cell.

The check: each rank deposits 1 into every cell, so the total of a cell is the
number of copies the grid holds of it - 2 per dimension in which the cell lies
in an overlap shared with a neighbour - and ``sum_g``, which counts every
global cell once, returns the number of local cells of all ranks.

    python examples/halo_deposit.py [--cpu]
    torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 2 examples/halo_deposit.py
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import igg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=12)
    ap.add_argument("--ny", type=int, default=10)
    ap.add_argument("--nz", type=int, default=8)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    import torch

    n = (a.nx, a.ny, a.nz)
    me, dims, nprocs, coords, comm = igg.init_global_grid(*n, periodx=1, periody=1, periodz=1, quiet=True,
                                                          device_type="none" if a.cpu else "auto")
    gg = igg.get_global_grid()
    device = "cpu" if a.cpu or not gg.amdgpu_enabled else "cuda"
    rho = torch.zeros(n, dtype=torch.float64, device=device)
    rho += 1.0                      # the deposit: every local cell, halos included
    igg.accumulate_halo_(rho)       # halo contributions go to the owners; halos become zero
    total = igg.sum_g(rho)          # every global cell once
    igg.update_halo_(rho)           # the totals go back out to every copy
    copies = torch.ones(n, dtype=torch.float64, device=device)
    for d in range(3):
        shared = torch.zeros(n[d], dtype=torch.bool, device=device)
        shared[:2] = shared[-2:] = True  # overlap 2: the two planes at each end have a copy on the neighbour
        shape = [1, 1, 1]
        shape[d] = n[d]
        copies = copies * torch.where(shared, 2.0, 1.0).view(shape)
    ok = torch.equal(rho, copies) and float(total) == float(nprocs * n[0] * n[1] * n[2])
    if not ok:
        raise SystemExit(f"rank {me}: the deposit does not add up (sum_g = {float(total)})")
    if me == 0:
        print(f"deposit on {nprocs} rank(s), dims {list(map(int, dims))}: sum_g = {float(total):.0f} = "
              f"{nprocs} x {n[0] * n[1] * n[2]} local cells; every copy of a cell holds the total")
    igg.finalize_global_grid()


if __name__ == "__main__":
    main()
