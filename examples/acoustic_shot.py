#!/usr/bin/env python3
"""A shot: a Ricker wavelet injected into the pressure of a 2-D acoustic wave,
recorded at a line of receivers.

The medium starts at rest. The source sits at a physical position that is no
grid node; ``igg.index_g`` turns it into a position in the global index space
of ``P`` and an ``igg.Source`` adds one sample of the wavelet there after every
step (``model.step()`` then ``inject``): one launch and one counter increment
per step, no collective and no host synchronisation. With ``copies="all"``
every rank that holds a copy of one of the source's four cells - halo and
overlap copies included - adds the same value, so ``P`` stays halo-consistent
without an exchange and the wave does not depend on the number of ranks. An
``igg.Recorder`` samples ``P`` at the receivers; ``result()`` combines the
ranks once at the end.

The check: after the last step ``update_halo_`` changes no bit of a copy of
``P``. ``--out`` saves the seismogram (steps x receivers) from rank 0.

    python examples/acoustic_shot.py [--cpu]
    torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 2 examples/acoustic_shot.py [--cpu]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import igg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=48)
    ap.add_argument("--ny", type=int, default=40)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--receivers", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    import torch

    from igg.models.acoustic2d import Acoustic2D

    me, dims, nprocs, coords, comm = igg.init_global_grid(a.nx, a.ny, 1, quiet=True,
                                                          device_type="none" if a.cpu else "auto")
    m = Acoustic2D(dtype=torch.float64)
    m.P.zero_()  # at rest: the shot is the only source of energy
    lx, ly = m.dx * (igg.nx_g() - 1), m.dy * (igg.ny_g() - 1)
    # the shot position, in physical coordinates, then in the index space of P
    shot = torch.tensor([[float(igg.index_g(0, 0.5 * lx + 0.3 * m.dx, m.dx, m.P)),
                          float(igg.index_g(1, 0.4 * ly + 0.6 * m.dy, m.dy, m.P))]], dtype=torch.float64)
    # a Ricker wavelet with about 12 cells per dominant wavelength, delayed so that it starts near zero
    f0 = math.sqrt(m.K / m.rho) / (12.0 * max(m.dx, m.dy))
    t = (torch.arange(a.steps, dtype=torch.float64) + 1.0) * m.dt - 1.2 / f0
    arg = (math.pi * f0 * t) ** 2
    W = ((1.0 - 2.0 * arg) * torch.exp(-arg) * m.dt).view(-1, 1).to(m.device)
    src = igg.Source(m.P, shot.to(m.device), W)
    s = torch.linspace(0.0, 1.0, a.receivers, dtype=torch.float64)
    X = torch.stack([igg.index_g(0, (0.1 + 0.8 * s) * lx, m.dx, m.P),
                     igg.index_g(1, (0.8 + 0.05 * s) * ly, m.dy, m.P)], dim=1).to(m.device)
    rec = igg.Recorder(m.P, X, a.steps)
    for _ in range(a.steps):
        m.step()
        src.inject(m.P)
        rec.record(m.P)
    traces = rec.result()  # (steps, receivers), the same bits on every rank
    Q = m.P.clone()
    igg.update_halo_(Q)
    same = torch.equal(Q.view(torch.int64), m.P.view(torch.int64))
    if not same:
        raise SystemExit(f"rank {me}: update_halo_ changed P after the shot: a copy of a source cell was missed")
    if me == 0:
        if a.out:
            torch.save(traces.cpu(), a.out)
        peak = traces.abs().max(dim=0).values
        print(f"1 shot, {a.receivers} receivers, {a.steps} steps on {nprocs} rank(s), dims {list(map(int, dims))}: "
              f"peak |P| at the receivers from {float(peak.min()):.3e} to {float(peak.max()):.3e}; the field stayed "
              "halo-consistent")
    m.close()
    igg.finalize_global_grid()


if __name__ == "__main__":
    main()
