#!/usr/bin/env python3
"""Sensitivity of a temperature probe to the initial field, by the adjoint.

After ``nt`` steps of ``Diffusion3D`` the temperature at one cell of the global
grid is a linear function of the initial field. Its gradient - how much each
initial cell contributes - takes ONE backward sweep: seed ``g`` with 1 at the
probe's owner, ``model.adjoint_run(nt, g)`` applies the transpose of the ``nt``
steps, and one more ``accumulate_halo_`` brings the halo cells' share home, so
the owned cells hold the gradient with respect to the global initial field.
Three of its cells are then checked against finite differences of
``model.run`` (two forward runs per cell).

    python examples/diffusion3D_adjoint.py --nx 12 --nt 6
    torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 2 \\
        examples/diffusion3D_adjoint.py --nx 12 --nt 6
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import igg  # noqa: E402
from igg.models.diffusion3d import Diffusion3D  # noqa: E402


def local_copies(A, cell):
    """Index tensors of every local copy of the global cell ``cell`` (halo and
    overlap copies included), or None if this rank holds none."""
    idx = [(igg.indices_g(d, A) == cell[d]).nonzero().flatten() for d in range(3)]
    if any(i.numel() == 0 for i in idx):
        return None
    return idx[0].view(-1, 1, 1), idx[1].view(1, -1, 1), idx[2].view(1, 1, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=12)
    ap.add_argument("--nt", type=int, default=6)
    a = ap.parse_args()
    me, dims, nprocs, coords, comm = igg.init_global_grid(a.nx, a.nx, a.nx, device_type="none", quiet=True)
    model = Diffusion3D(dtype=torch.float64, device="cpu")
    T0 = model.T.clone()
    probe = (igg.nx_g() // 2, igg.ny_g() // 2, igg.nz_g() // 2)
    P = torch.tensor([probe], dtype=torch.float64)

    def probe_after_run(T_init):
        model.T.copy_(T_init)
        model.T2.copy_(T_init)
        model.mark_modified()
        model.run(a.nt)
        return float(igg.sample_g(model.T, P)[0])

    # backward: one adjoint sweep from the probe
    g = torch.zeros_like(T0)
    igg.spread_g(g, P, torch.ones(1, dtype=torch.float64), copies="owner")  # the transpose of the probe's sample_g
    grad = model.adjoint_run(a.nt, g)
    igg.accumulate_halo_(grad)  # overlap == 2 * halowidth: the owned cells now hold the global gradient
    total = float(igg.sum_g(grad))

    # forward: finite differences of model.run at three cells (the map is linear: any step size is exact)
    cells = [probe, (probe[0] - 1, probe[1], probe[2] + 1), (probe[0] + 2, probe[1] - 1, probe[2])]
    worst = 0.0
    for c in cells:
        fd = []
        for sign in (1.0, -1.0):
            Tp = T0.clone()
            idx = local_copies(Tp, c)
            if idx is not None:
                Tp[idx] += sign
            fd.append(probe_after_run(Tp))
        fd = 0.5 * (fd[0] - fd[1])
        ad = float(igg.sample_g(grad, torch.tensor([c], dtype=torch.float64))[0])
        worst = max(worst, abs(fd - ad))
        if me == 0:
            print(f"dT_probe/dT0{c}: adjoint {ad:.12e}, finite differences {fd:.12e}")
    ok = worst <= 1e-10
    if me == 0:
        print(f"{nprocs} process(es) {dims.tolist()}: probe {probe}, {a.nt} steps, sum of the gradient {total:.6f}, "
              f"largest difference {worst:.2e}: {'adjoint check OK' if ok else 'MISMATCH'}")
    igg.finalize_global_grid()
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
