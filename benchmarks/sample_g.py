#!/usr/bin/env python3
"""sample_g against the plain torch formulation on the same device and buffers.

What a user writes today for the values of a field at arbitrary points: floor,
``2^nd`` advanced-index gathers and lerps in torch - dozens of launches and
temporaries. ``sample_g`` is one launch. Fields: 512^3 float64 and 1024^3
float32 on one process; point sets: 10^6 points, random and sorted by memory
order, and 10^4 points (the receiver-count regime, where launch cost
dominates); 1 and 3 fields per call. Interleaved rounds (utils/timing.py),
medians, warm-up first, events on the stream; the two forms are compared first.

The bar: in every case the kernel's slowest round is faster than the torch
formulation's fastest round. ``line_GBs`` is the rate of fetched 128-B lines
the kernel sustains if every point touches four of them per field (the two
corners along the innermost axis share a line but for one point in 16 or 32).

    python benchmarks/sample_g.py [--quick]

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


def torch_sample(fields, P):
    """The same interpolation in torch (non-periodic, one rank)."""
    A0 = fields[0]
    E = torch.tensor(A0.shape, dtype=torch.float64, device=P.device)
    g = torch.minimum(P.floor(), E - 2.0)
    t = P - g
    i, j, k = g.long().unbind(1)
    t0, t1, t2 = t.unbind(1)
    out = []
    for A in fields:
        c = [[[A[i + a, j + b, k + c].double() for c in (0, 1)] for b in (0, 1)] for a in (0, 1)]
        v = [[(1.0 - t2) * c[a][b][0] + t2 * c[a][b][1] for b in (0, 1)] for a in (0, 1)]
        w = [(1.0 - t1) * v[a][0] + t1 * v[a][1] for a in (0, 1)]
        out.append((1.0 - t0) * w[0] + t0 * w[1])
    return torch.stack(out)


def case(fields, P, steps, rounds, label):
    cands = ["sample_g", "torch"]
    out = torch.empty(len(fields), P.shape[0], dtype=torch.float64, device=P.device)
    ref = torch_sample(fields, P)
    igg.sample_g(tuple(fields), P, out=out)
    err = float((out - ref).abs().max())
    assert err < 1e-9, f"{label}: the two forms differ by {err}"
    del ref

    def run(cand, k):
        for _ in range(k):
            if cand == "sample_g":
                igg.sample_g(tuple(fields), P, out=out)
            else:
                torch_sample(fields, P)

    per = [[] for _ in cands]
    for r in range(rounds):
        for t, ms in zip(per, interleaved_medians(cands, run, steps=steps, rounds=1, warm=3 if r == 0 else 0)):
            t.append(ms)
    us = {c: [round(min(t) * 1e3, 1), round(med(t) * 1e3, 1), round(max(t) * 1e3, 1)] for c, t in zip(cands, per)}
    res = {"us_min_med_max": us, "speedup": round(med(per[1]) / med(per[0]), 1),
           "bar_met": max(per[0]) < min(per[1]),
           "line_GBs": round(P.shape[0] * len(fields) * 4 * 128 / (med(per[0]) * 1e-3) / 1e9, 1)}
    print(f"{label:44s} | sample_g {us['sample_g'][1]:9.1f} us (max {us['sample_g'][2]:9.1f})   torch "
          f"{us['torch'][1]:9.1f} us (min {us['torch'][0]:9.1f})   x{res['speedup']:<6} "
          f"{'bar met' if res['bar_met'] else 'BAR MISSED'}   {res['line_GBs']:7.1f} GB/s of lines", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="128^3 fields and fewer points: a check of the script")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    results = {}
    sizes = [(128, torch.float64), (160, torch.float32)] if a.quick else [(512, torch.float64), (1024, torch.float32)]
    big, small = (10 ** 5, 10 ** 3) if a.quick else (10 ** 6, 10 ** 4)
    for n, dtype in sizes:
        igg.init_global_grid(n, n, n, quiet=True)
        fields = [torch.randn(n, n, n, dtype=dtype, device=dev) for _ in range(3)]
        g = torch.Generator(device=dev).manual_seed(1)
        R = torch.rand(big, 3, generator=g, dtype=torch.float64, device=dev) * (n - 1.0)
        cell = R.floor().long()
        S = R[torch.argsort((cell[:, 0] * n + cell[:, 1]) * n + cell[:, 2])].contiguous()
        sets = {f"{big:.0e} random": R, f"{big:.0e} sorted": S, f"{small:.0e} random": R[:small].contiguous()}
        for (name, P), nf in ((s, nf) for s in sets.items() for nf in (1, 3)):
            label = f"{n}^3 {str(dtype)[6:]}, {name}, {nf} field{'s' if nf > 1 else ''}"
            results[label] = case(fields[:nf], P, a.steps, a.rounds, label)
        del fields
        igg.finalize_global_grid()
        torch.cuda.empty_cache()
    results["every_bar_met"] = all(r["bar_met"] for r in results.values())
    print(json.dumps({"sample_g": results}))


if __name__ == "__main__":
    main()
