#!/usr/bin/env python3
"""Global reductions (ops/reduce.py) against what a user writes in torch today
and against the read roof.

For ``sumsq`` (one input) and ``maxabs_diff`` (two inputs), at 512^3 float64
and 1024^3 float32, on the owned box ``[1, n-1)^3`` of a periodic rank (the
rows path) and on a whole array (the flat path), interleaved rounds of

  new    ``igg.reduce_g(op, A, other=B, out=r)``: the HIP kernels, two launches;
  torch  the same reduction in torch on the same view, e.g.
         ``(A[1:-1,1:-1,1:-1] - B[1:-1,1:-1,1:-1]).abs().max()`` (every way
         listed in TORCH_FORMS; the fastest one is the competitor);
  roof   the read probe ``native.stream_probe`` kind 5 over the same bytes (the
         fastest of a few grid sizes).

Per case: ms and GB/s of each side (bytes = the box's elements x element size x
inputs), the new path's share of the roof, and the verdict on "faster than
torch": established when the slowest new round is ahead of the fastest torch
round by more than the spread (max - min over the rounds) of either side.
Last, the cost of the two launches at a tiny size. One JSON line at the end.

    python benchmarks/global_reduce.py [--sizes 512:float64,1024:float32] [--rounds 7] [--steps 10]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import igg  # noqa: E402
from igg._native import native  # noqa: E402
from igg.utils.timing import interleaved_medians  # noqa: E402

TORCH_FORMS = {
    "sumsq": {"square().sum()": lambda v, w: v.square().sum(),
              "vector_norm()**2": lambda v, w: torch.linalg.vector_norm(v) ** 2},
    "maxabs_diff": {"(v-w).abs().max()": lambda v, w: (v - w).abs().max()},
}
PROBE_BLOCKS = (1024, 2048, 4096, 8192)


def rounds_of(cands, run, steps, rounds, warm):
    """Per-round ms per step of each candidate: ``rounds`` interleaved visits."""
    out = [[] for _ in cands]
    for r in range(rounds):
        for t, ms in zip(out, interleaved_medians(cands, run, steps=steps, rounds=1, warm=warm if r == 0 else 0)):
            t.append(ms)
    return out


def case(op, A, B, inner, steps, rounds):
    n, es = A.shape[0], A.element_size()
    two = op == "maxabs_diff"
    sl = (slice(1, -1),) * 3 if inner else (slice(None),) * 3
    v, w = A[sl], B[sl]
    nbytes = v.numel() * es * (2 if two else 1)
    r = torch.zeros((), dtype=torch.float64, device=A.device)
    scratch = torch.empty(max(PROBE_BLOCKS) * 256, dtype=torch.float64, device=A.device)
    s = torch.cuda.current_stream().cuda_stream
    # the probe reads two streams of 8-byte words: the two inputs, or the two halves of one
    words = nbytes // 16
    pa = A.data_ptr()
    pb = B.data_ptr() if two else A.data_ptr() + words * 8
    cands = [("new", None)] + [("torch", k) for k in TORCH_FORMS[op]] + [("roof", b) for b in PROBE_BLOCKS]

    def run(c, k):
        kind, arg = c
        for _ in range(k):
            if kind == "new":
                igg.reduce_g(op, A, other=B if two else None, out=r)
            elif kind == "torch":
                TORCH_FORMS[op][arg](v, w)
            else:
                native.stream_probe(5, scratch.data_ptr(), pa, pb, words, arg, s)

    # same answer first (the torch forms accumulate in the input type)
    igg.reduce_g(op, A, other=B if two else None, out=r)
    ref = TORCH_FORMS[op][next(iter(TORCH_FORMS[op]))](v.double() if n <= 512 else v, w.double() if n <= 512 else w)
    rel = abs(r.item() - float(ref)) / max(abs(float(ref)), 1e-300)
    assert rel < (1e-12 if n <= 512 else 1e-3), (op, r.item(), float(ref))
    t = rounds_of(cands, run, steps, rounds, warm=3)
    new = t[0]
    torch_best = min((x for c, x in zip(cands, t) if c[0] == "torch"), key=lambda x: sorted(x)[len(x) // 2])
    torch_name = next(c[1] for c, x in zip(cands, t) if x is torch_best)
    roof = min((x for c, x in zip(cands, t) if c[0] == "roof"), key=lambda x: sorted(x)[len(x) // 2])
    roof_blocks = next(c[1] for c, x in zip(cands, t) if x is roof)
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    spread = max(max(new) - min(new), max(torch_best) - min(torch_best))
    lead = min(torch_best) - max(new)
    res = {
        "op": op, "n": n, "dtype": str(A.dtype).replace("torch.", ""), "box": "inner" if inner else "whole",
        "path": native.reduce_plan(list(A.shape), list(A.stride()), [1 if inner else 0] * 3,
                                   [n - 1 if inner else n] * 3, es, A.data_ptr())["path"],
        "MiB": round(nbytes / 2 ** 20, 1),
        "new_ms": round(med(new), 4), "new_min_max": [round(min(new), 4), round(max(new), 4)],
        "new_GBs": round(nbytes / med(new) / 1e6, 1),
        "torch_form": torch_name, "torch_ms": round(med(torch_best), 4),
        "torch_min_max": [round(min(torch_best), 4), round(max(torch_best), 4)],
        "torch_GBs": round(nbytes / med(torch_best) / 1e6, 1),
        "roof_ms": round(med(roof), 4), "roof_GBs": round(nbytes / med(roof) / 1e6, 1), "roof_blocks": roof_blocks,
        "share_of_roof": round(med(roof) / med(new), 3),
        "speedup_vs_torch": round(med(torch_best) / med(new), 2),
        "faster_than_torch": "established" if lead > spread else "not established",
    }
    print(f"{res['op']:12s} {n}^3 {res['dtype']:8s} {res['box']:6s} {res['path']:5s} {res['MiB']:8.1f} MiB | "
          f"new {res['new_ms']:8.4f} ms {res['new_GBs']:7.1f} GB/s | torch [{torch_name}] {res['torch_ms']:8.4f} ms "
          f"{res['torch_GBs']:7.1f} GB/s | roof {res['roof_ms']:8.4f} ms {res['roof_GBs']:7.1f} GB/s @{roof_blocks} | "
          f"share {res['share_of_roof']:.3f} | x{res['speedup_vs_torch']:.2f} vs torch: {res['faster_than_torch']}",
          flush=True)
    return res


def tiny(device):
    """The two launches at a size where nothing else counts (8^3 f64)."""
    A = torch.ones(8, 8, 8, dtype=torch.float64, device=device)
    r = torch.zeros((), dtype=torch.float64, device=device)
    s = torch.cuda.current_stream().cuda_stream
    job = [(A.data_ptr(), 0, [8, 8, 8], [64, 8, 1], [], [1, 1, 1], [7, 7, 7])]
    g = torch.cuda.CUDAGraph()
    igg.reduce_g("sumsq", A, out=r)
    with torch.cuda.graph(g):
        for _ in range(20):
            igg.reduce_g("sumsq", A, out=r)
    cands = ["reduce_g", "native.reduce", "graph of 20", "torch square().sum()"]

    def run(c, k):
        for _ in range(k):
            if c == "reduce_g":
                igg.reduce_g("sumsq", A, out=r)
            elif c == "native.reduce":
                native.reduce(1, job, 8, r.data_ptr(), 0, s)
            elif c == "graph of 20":
                g.replay()
            else:
                A[1:-1, 1:-1, 1:-1].square().sum()

    ms = interleaved_medians(cands, run, steps=200, rounds=5, warm=20)
    out = {c: round(x * 1e3 / (20 if c == "graph of 20" else 1), 2) for c, x in zip(cands, ms)}
    print("tiny (8^3 f64, us per reduction: enqueue-bound eager, device-bound in a graph):", out, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="512:float64,1024:float32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    results = []
    for spec in a.sizes.split(","):
        n, dt = spec.split(":")
        n, dtype = int(n), getattr(torch, dt)
        for inner in (True, False):
            # a periodic rank owns [1, n-1)^3, a non-periodic single rank the whole array
            per = 1 if inner else 0
            igg.init_global_grid(n, n, n, periodx=per, periody=per, periodz=per, quiet=True)
            dev = torch.device("cuda", torch.cuda.current_device())
            g = torch.Generator(device=dev).manual_seed(1)
            A = torch.randn(n, n, n, dtype=dtype, device=dev, generator=g)
            B = torch.randn(n, n, n, dtype=dtype, device=dev, generator=g)
            for op in ("sumsq", "maxabs_diff"):
                results.append(case(op, A, B, inner, a.steps, a.rounds))
            if n == int(a.sizes.split(",")[0].split(":")[0]) and inner:
                tiny_us = tiny(dev)
            del A, B
            igg.finalize_global_grid()
    print(json.dumps({"global_reduce": results, "tiny_us": tiny_us}))


if __name__ == "__main__":
    main()
