#!/usr/bin/env python3
"""accumulate_halo_ against update_halo_ on the same field (one process).

A float64 field of ``n^3`` on a single-process grid that is periodic in x, y
and z, and in each of the three alone: the exchange and its transpose are then
one launch per periodic dimension, the exchange reading one slab and writing
one per side, the transpose reading and clearing one and reading and writing
another. Interleaved rounds (utils/timing.py), medians, warm-up first, events
on the stream; both results are checked first (<Hx,y> == <x,H'y> in the
field's own arithmetic is not exact, so the check is the CPU's result on a
small field of the same layout).

    python benchmarks/accumulate_halo.py --nx 512

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


def check(dev):
    igg.init_global_grid(40, 36, 70, periodx=1, periody=1, periodz=1, quiet=True)
    c = torch.randn(40, 36, 70, dtype=torch.float64)
    g = c.to(dev)
    igg.accumulate_halo_(c)
    igg.accumulate_halo_(g)
    assert torch.equal(g.cpu(), c), "the GPU result differs from the CPU's"
    igg.finalize_global_grid()


def one(n, periods, steps, rounds, dev, dtype):
    igg.init_global_grid(n, n, n, periodx=periods[0], periody=periods[1], periodz=periods[2], quiet=True)
    A = torch.randn(n, n, n, dtype=dtype, device=dev)
    cands = ["update_halo_", "accumulate_halo_"]

    def run(cand, k):
        f = igg.update_halo_ if cand == cands[0] else igg.accumulate_halo_
        for _ in range(k):
            f(A)

    per = [[] for _ in cands]
    for r in range(rounds):
        for t, ms in zip(per, interleaved_medians(cands, run, steps=steps, rounds=1, warm=3 if r == 0 else 0)):
            t.append(ms)
    igg.finalize_global_grid()
    res = {c: {"us": round(med(t) * 1e3, 1), "min_max_us": [round(min(t) * 1e3, 1), round(max(t) * 1e3, 1)]}
           for c, t in zip(cands, per)}
    res["ratio"] = round(med(per[1]) / med(per[0]), 3)
    name = "".join(d for d, p in zip("xyz", periods) if p)
    print(f"{n}^3 {str(dtype)[6:]} periodic in {name:3s} | update_halo_ {res[cands[0]]['us']:8.1f} us   "
          f"accumulate_halo_ {res[cands[1]]['us']:8.1f} us   ratio {res['ratio']:.2f}", flush=True)
    return name, res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--nx", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--dtype", choices=("float64", "float32"), default="float64")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    check(dev)
    out = {"n": a.nx, "dtype": a.dtype}
    for periods in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        name, res = one(a.nx, periods, a.steps, a.rounds, dev, getattr(torch, a.dtype))
        out[name] = res
    print(json.dumps({"accumulate_halo": out}))


if __name__ == "__main__":
    main()
