#!/usr/bin/env python3
"""spread_g: the apply launch, the plan build, and the torch formulation.

One 512^3 float64 field on one process; point sets: 10^4 and 10^6 random points
and 10^6 points sorted by memory order. Three things per set:

* ``apply``: ``SpreadPlan.apply`` - the per-step launch (one lane per touched
  cell, a fixed order of additions);
* ``plan``: ``spread_plan`` - the count and fill kernels around a torch
  ``cumsum``, stable ``sort`` and ``unique_consecutive``, with its one host
  synchronisation;
* ``torch``: what a user writes today - ``floor`` and 8
  ``index_put_(accumulate=True)`` calls on the same data. It adds with float
  atomics in whatever order the hardware takes them: two runs can differ in
  the last bits wherever two points share a cell, which is why it is the thing
  compared against and not the implementation.

And the cost of one lane folding a long segment alone: 1000 points in one cell
against 1000 points in 1000 cells.

Interleaved rounds (utils/timing.py), medians, warm-up first, events on the
stream; the two forms are compared first (to rounding: the orders differ).

    python benchmarks/spread_g.py [--quick]

One JSON line at the end.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import igg  # noqa: E402
from igg.utils.timing import interleaved_medians  # noqa: E402

med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731


def torch_spread(A, P, V):
    """The same operator in torch (non-periodic, one rank), atomics inside."""
    E = torch.tensor(A.shape, dtype=torch.float64, device=P.device)
    g = torch.minimum(P.floor(), E - 2.0)
    t = P - g
    i, j, k = g.long().unbind(1)
    f = [(1.0 - t, t)[c].unbind(1) for c in (0, 1)]
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                A.index_put_((i + a, j + b, k + c), ((f[a][0] * f[b][1]) * f[c][2]) * V, accumulate=True)


def timed(cands, run, steps, rounds):
    per = [[] for _ in cands]
    for r in range(rounds):
        for t, ms in zip(per, interleaved_medians(cands, run, steps=steps, rounds=1, warm=2 if r == 0 else 0)):
            t.append(ms)
    return {c: [round(min(t) * 1e3, 1), round(med(t) * 1e3, 1), round(max(t) * 1e3, 1)] for c, t in zip(cands, per)}


def case(A, P, steps, rounds, label):
    V = torch.randn(P.shape[0], dtype=torch.float64, device=P.device)
    plan = igg.spread_plan(A, P)
    ref = torch.zeros_like(A)
    torch_spread(ref, P, V)
    got = torch.zeros_like(A)
    plan.apply(V, got)
    err = float((got - ref).abs().max())
    assert err < 1e-9, f"{label}: the two forms differ by {err}"
    del ref, got
    cands = ["apply", "plan", "torch"]

    def run(cand, k):
        for _ in range(k):
            if cand == "apply":
                plan.apply(V, A)
            elif cand == "plan":
                igg.spread_plan(A, P)
            else:
                torch_spread(A, P, V)

    us = timed(cands, run, steps, rounds)
    seg = (plan.start[1:] - plan.start[:-1])
    res = {"us_min_med_max": us, "ncells": plan.ncells, "nentries": plan.nentries,
           "longest_segment": int(seg.max()), "torch_over_apply": round(us["torch"][1] / us["apply"][1], 1)}
    print(f"{label:34s} | apply {us['apply'][1]:9.1f} us   plan {us['plan'][1]:10.1f} us   torch "
          f"{us['torch'][1]:9.1f} us   torch/apply x{res['torch_over_apply']:<6} {plan.ncells} cells, "
          f"{plan.nentries} entries, longest segment {res['longest_segment']}", flush=True)
    return res


def long_segment(A, n, steps, rounds):
    """1000 points in one cell against 1000 points in 1000 cells of one plane."""
    dev = A.device
    one = torch.tensor([[7.0, 9.0, 11.0]], dtype=torch.float64, device=dev).repeat(1000, 1)
    k = torch.arange(1000, dtype=torch.float64, device=dev)
    many = torch.stack([torch.full_like(k, 7.0), (k // 40) * 3.0, (k % 40) * 5.0], dim=1)
    V = torch.randn(1000, dtype=torch.float64, device=dev)
    plans = {"1000 points in 1 cell": igg.spread_plan(A, one), "1000 points in 1000 cells": igg.spread_plan(A, many)}
    assert [p.ncells for p in plans.values()] == [1, 1000]
    us = timed(list(plans), lambda c, k: [plans[c].apply(V, A) for _ in range(k)], steps, rounds)
    for c, t in us.items():
        print(f"{c:34s} | apply {t[1]:9.1f} us (min {t[0]:.1f}, max {t[2]:.1f})", flush=True)
    return us


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="a 128^3 field and fewer points: a check of the script")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 128 if a.quick else 512
    big, small = (10 ** 5, 10 ** 3) if a.quick else (10 ** 6, 10 ** 4)
    igg.init_global_grid(n, n, n, quiet=True)
    A = torch.randn(n, n, n, dtype=torch.float64, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    R = torch.rand(big, 3, generator=g, dtype=torch.float64, device=dev) * (n - 1.0)
    cell = R.floor().long()
    S = R[torch.argsort((cell[:, 0] * n + cell[:, 1]) * n + cell[:, 2])].contiguous()
    sets = {f"{small:.0e} random": R[:small].contiguous(), f"{big:.0e} random": R, f"{big:.0e} sorted": S}
    results = {}
    for name, P in sets.items():
        label = f"{n}^3 float64, {name}"
        results[label] = case(A, P, a.steps, a.rounds, label)
    results["long segment, us_min_med_max"] = long_segment(A, n, a.steps, a.rounds)
    igg.finalize_global_grid()
    print(json.dumps({"spread_g": results}))


if __name__ == "__main__":
    main()
