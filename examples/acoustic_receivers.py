#!/usr/bin/env python3
"""Seismograms: the pressure of a 2-D acoustic wave at a line of receivers.

The receivers sit on a line that follows no grid line. ``igg.index_g`` turns
their physical coordinates into positions in the global index space of ``P``;
an ``igg.Recorder`` samples ``P`` there after every step - one launch and one
counter increment per step, no collective and no host synchronisation - and
``result()`` combines the ranks once at the end. Whichever rank owns a
receiver's cell interpolates it, so the traces do not depend on the number of
ranks, bit for bit.

Two of the receivers are moved onto grid nodes. The check: their last samples
equal the cells of the global pressure field that ``gather_g`` assembles, bit
for bit.

    python examples/acoustic_receivers.py [--cpu]
    torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 2 examples/acoustic_receivers.py [--cpu]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import igg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=48)
    ap.add_argument("--ny", type=int, default=40)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--receivers", type=int, default=16)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    import torch

    from igg.models.acoustic2d import Acoustic2D

    me, dims, nprocs, coords, comm = igg.init_global_grid(a.nx, a.ny, 1, quiet=True,
                                                          device_type="none" if a.cpu else "auto")
    m = Acoustic2D(dtype=torch.float64)
    lx, ly = m.dx * (igg.nx_g() - 1), m.dy * (igg.ny_g() - 1)
    # a slanted line of receivers, in physical coordinates, then in the index space of P
    s = torch.linspace(0.0, 1.0, a.receivers, dtype=torch.float64)
    X = torch.stack([igg.index_g(0, (0.15 + 0.7 * s) * lx, m.dx, m.P),
                     igg.index_g(1, (0.30 + 0.4 * s) * ly, m.dy, m.P)], dim=1)
    nodes = [2, a.receivers - 3]
    X[nodes] = X[nodes].round()  # two receivers exactly on grid nodes
    X = X.to(m.device)
    rec = igg.Recorder(m.P, X, a.steps)
    for _ in range(a.steps):
        m.step()
        m.sync_halo()
        rec.record(m.P)
    traces = rec.result()  # (steps, receivers), the same bits on every rank
    G = torch.empty(igg.selection_shape_g(m.P), dtype=m.P.dtype, device=m.device) if me == 0 else None
    igg.gather_g(m.P, G)
    if me == 0:
        ij = X[nodes].long()
        want = G[ij[:, 0], ij[:, 1]].double()
        got = traces[-1, nodes]
        if not torch.equal(got.view(torch.int64), want.view(torch.int64)):
            raise SystemExit(f"the node receivers' last samples {got.tolist()} differ from the global field "
                             f"{want.tolist()}")
        peak = traces.abs().max(dim=0).values
        print(f"{a.receivers} receivers, {a.steps} steps on {nprocs} rank(s), dims {list(map(int, dims))}: peak |P| "
              f"from {float(peak.min()):.4f} to {float(peak.max()):.4f}; the node receivers equal gather_g's cells "
              "bit for bit")
    m.close()
    igg.finalize_global_grid()


if __name__ == "__main__":
    main()
