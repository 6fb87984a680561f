#!/usr/bin/env python3
"""Sensitivity of one receiver sample to the initial pressure, by the adjoint.

After ``nt`` steps of ``Acoustic2D`` the pressure at one node of the global
grid - one sample of a receiver's trace - is a linear function of the initial
fields. Its gradient with respect to the initial pressure takes ONE backward
sweep: seed ``gP`` with 1 at the node's owner (``gVx = gVy = 0``),
``model.adjoint_run(nt, gP, gVx, gVy)`` applies the transpose of the ``nt``
steps, one ``accumulate_halo_(gP)`` brings the halo cells' share home and
``gather_g`` assembles the global gradient.

Check: the step is linear, so bumping three global cells of the initial
pressure by ``h`` - on every copy, via ``scatter_g`` - changes the sample by
``h * (sum of the gradient at the three cells)``, up to the rounding of two
forward runs and one backward sweep.

    python examples/acoustic_adjoint.py [--cpu] --nx 48 --nt 40
    torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 2 examples/acoustic_adjoint.py [--cpu]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import igg  # noqa: E402
from igg.models.acoustic2d import Acoustic2D  # noqa: E402


def owned_copy(A, cell):
    """Local index of the global cell ``cell`` if this rank owns it, else None."""
    at = []
    for d, (a, b) in enumerate(igg.owned_ranges(A)):
        hit = (igg.indices_g(d, A)[a:b] == cell[d]).nonzero().flatten()
        if hit.numel() == 0:
            return None
        at.append(a + int(hit[0]))
    return tuple(at)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=48)
    ap.add_argument("--nt", type=int, default=40)
    ap.add_argument("--f32", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    me, dims, nprocs, coords, comm = igg.init_global_grid(a.nx, a.nx, 1, quiet=True,
                                                          device_type="none" if a.cpu else "auto")
    dtype = torch.float32 if a.f32 else torch.float64
    m = Acoustic2D(dtype=dtype)
    P0 = m.P.clone()
    E = igg.selection_shape_g(m.P)
    rec = (E[0] // 2 + 2, E[1] // 3)
    X = torch.tensor([rec], dtype=torch.float64, device=m.device)

    def sample_after_run(P_init):
        m.P.copy_(P_init)
        m.Vx.zero_()
        m.Vy.zero_()
        m.mark_modified()
        m.run(a.nt)
        return float(igg.sample_g(m.P, X)[0]), float(igg.max_g(m.P.abs()))

    # backward: one adjoint sweep from the receiver sample
    gP, gVx, gVy = torch.zeros_like(m.P), torch.zeros_like(m.Vx), torch.zeros_like(m.Vy)
    at = owned_copy(gP, rec)
    if at is not None:
        gP[at] = 1.0
    grad = m.adjoint_run(a.nt, gP, gVx, gVy)[0]
    igg.accumulate_halo_(grad)  # overlap == 2 * halowidth: the owned cells now hold the global gradient
    G = torch.empty(E, dtype=dtype, device=m.device) if me == 0 else None
    igg.gather_g(grad, G)

    # forward: the sample of the model's own initial pressure, and of the bumped one
    h = 0.5
    cells = [rec, (rec[0] - 3, rec[1] + 2), (2, E[1] - 3)]
    B = None
    if me == 0:
        B = torch.zeros(E, dtype=dtype, device=m.device)
        for c in cells:
            B[c] = h
    bump = torch.zeros_like(P0)
    igg.scatter_g(B, bump)
    s0, p0 = sample_after_run(P0)
    s1, p1 = sample_after_run(P0 + bump)
    pmax = float(igg.max_g(P0.abs()))
    ok = True
    if me == 0:
        gsum = sum(float(G[c]) for c in cells)
        gabs = float(G.abs().max())
        # Rounding: every step rounds a field value a few times relative to the fields' size, and the
        # scheme is stable, so nt steps leave at most ~16*nt*eps*size in a sample - twice forward (sizes
        # pmax and pmax + h) and once backward (size: the largest gradient entry, times h, per cell).
        eps = torch.finfo(dtype).eps
        tol = 16 * a.nt * eps * ((pmax + max(p0, abs(s0))) + (pmax + h + max(p1, abs(s1))) + len(cells) * h * gabs)
        diff = abs((s1 - s0) - h * gsum)
        ok = diff <= tol
        print(f"sample {s0:.12e} -> {s1:.12e} after the bump of {h} at {cells}; h * gradient = {h * gsum:.12e}; "
              f"max|P0| {pmax:.3f}, max|P| after the runs {p0:.3f} / {p1:.3f}, max|gradient| {gabs:.3e}")
        print(f"{nprocs} process(es) {list(map(int, dims))}: receiver {rec}, {a.nt} steps, {str(dtype)[6:]}, "
              f"difference {diff:.2e} (tolerance {tol:.2e}): {'adjoint check OK' if ok else 'MISMATCH'}")
    ok = bool(comm.allreduce(0.0 if ok else 1.0, "max") == 0.0) if nprocs > 1 else ok
    m.close()
    igg.finalize_global_grid()
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
