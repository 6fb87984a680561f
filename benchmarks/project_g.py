#!/usr/bin/env python3
"""``project_g`` (ops/reduce.py) against what a user writes in torch today and
against the read roof.

For ``sum`` (one input) and ``maxabs_diff`` (two inputs), for the six keep-sets
of a 3-D field, at 512^3 float64 and 1024^3 float32 on the owned box
``[1, n-1)^3`` of a periodic rank, interleaved rounds of

  new    ``igg.project_g(op, A, keep, other=B, out=r)``: the HIP kernels, two launches;
  torch  the same reduction in torch on ``owned_view``, e.g.
         ``(v - w).abs().amax(dim=red)`` (every way listed in TORCH_FORMS; the
         fastest one is the competitor);
  roof   the read probe ``native.stream_probe`` kind 5 over the same bytes (the
         fastest of a few grid sizes).

Per case: the plan (family, pattern, slices, blocks), ms and GB/s of each side
(bytes = the box's elements x element size x inputs), the new path's share of
the roof, and the verdict on "faster than torch": established when the slowest
new round is ahead of the fastest torch round by more than the spread (max -
min over the rounds) of either side. One JSON line at the end.

    python benchmarks/project_g.py [--sizes 512:float64,1024:float32] [--rounds 7] [--steps 10]
"""
import argparse
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import igg  # noqa: E402
from igg._native import native  # noqa: E402
from igg.utils.timing import interleaved_medians  # noqa: E402

TORCH_FORMS = {
    "sum": {"sum(dim)": lambda v, w, red: v.sum(dim=red),
            "sum(dim, dtype=f64)": lambda v, w, red: v.sum(dim=red, dtype=torch.float64)},
    "maxabs_diff": {"(v-w).abs().amax(dim)": lambda v, w, red: (v - w).abs().amax(dim=red)},
}
PROBE_BLOCKS = (2048, 4096, 8192)
KEEPS = [k for r in (1, 2) for k in itertools.combinations(range(3), r)]


def rounds_of(cands, run, steps, rounds, warm):
    """Per-round ms per step of each candidate: ``rounds`` interleaved visits."""
    out = [[] for _ in cands]
    for r in range(rounds):
        for t, ms in zip(out, interleaved_medians(cands, run, steps=steps, rounds=1, warm=warm if r == 0 else 0)):
            t.append(ms)
    return out


def case(op, A, B, keep, steps, rounds):
    n, es = A.shape[0], A.element_size()
    two = op == "maxabs_diff"
    red = tuple(d for d in range(3) if d not in keep)
    v, w = igg.owned_view(A), igg.owned_view(B)
    nbytes = v.numel() * es * (2 if two else 1)
    r = torch.zeros([igg.selection_shape_g(A)[d] for d in keep], dtype=torch.float64, device=A.device)
    scratch = torch.empty(max(PROBE_BLOCKS) * 256, dtype=torch.float64, device=A.device)
    s = torch.cuda.current_stream().cuda_stream
    # the probe reads two streams of 8-byte words: the two inputs, or the two halves of one
    words = nbytes // 16
    pa = A.data_ptr()
    pb = B.data_ptr() if two else A.data_ptr() + words * 8
    forms = dict(TORCH_FORMS[op])
    if A.dtype == torch.float64:
        forms.pop("sum(dim, dtype=f64)", None)
    cands = [("new", None)] + [("torch", k) for k in forms] + [("roof", b) for b in PROBE_BLOCKS]

    def run(c, k):
        kind, arg = c
        for _ in range(k):
            if kind == "new":
                igg.project_g(op, A, keep, other=B if two else None, out=r)
            elif kind == "torch":
                forms[arg](v, w, red)
            else:
                native.stream_probe(5, scratch.data_ptr(), pa, pb, words, arg, s)

    # same answer first (a single periodic rank: the owned box is the global grid)
    igg.project_g(op, A, keep, other=B if two else None, out=r)
    ref = (v.double() - w.double()).abs().amax(dim=red) if two else v.sum(dim=red, dtype=torch.float64)
    err = ((r - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()
    assert err < 1e-9, (op, keep, err)
    t = rounds_of(cands, run, steps, rounds, warm=3)
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    new = t[0]
    torch_best = min((x for c, x in zip(cands, t) if c[0] == "torch"), key=med)
    torch_name = next(c[1] for c, x in zip(cands, t) if x is torch_best)
    roof = min((x for c, x in zip(cands, t) if c[0] == "roof"), key=med)
    roof_blocks = next(c[1] for c, x in zip(cands, t) if x is roof)
    spread = max(max(new) - min(new), max(torch_best) - min(torch_best))
    lead = min(torch_best) - max(new)
    rng = igg.owned_ranges(A)
    p = native.project_plan(list(A.shape), list(A.stride()), [a for a, _ in rng], [b for _, b in rng], list(keep), es,
                            A.data_ptr(), **(dict(strides_b=list(B.stride()), base_b=B.data_ptr()) if two else {}))
    res = {
        "op": op, "n": n, "dtype": str(A.dtype).replace("torch.", ""), "keep": list(keep),
        "family": p["family"], "pattern": p["pattern"], "path": p["path"], "slices": p["slices"],
        "blocks": p["blocks"], "lanes": p["lanes"], "index_bits": p["index_bits"],
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
    print(f"{op:12s} {n}^3 {res['dtype']:8s} keep {str(keep):7s} {p['pattern']:3s} f{p['family']} "
          f"slices {p['slices']:3d} blocks {p['blocks']:4d} | new {res['new_ms']:8.4f} ms {res['new_GBs']:7.1f} GB/s "
          f"[{res['new_min_max'][0]:.4f}, {res['new_min_max'][1]:.4f}] | torch [{torch_name}] {res['torch_ms']:8.4f} ms "
          f"[{res['torch_min_max'][0]:.4f}, {res['torch_min_max'][1]:.4f}] | roof {res['roof_ms']:8.4f} ms "
          f"{res['roof_GBs']:7.1f} GB/s @{roof_blocks} | share {res['share_of_roof']:.3f} | "
          f"x{res['speedup_vs_torch']:.2f} vs torch: {res['faster_than_torch']}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="512:float64,1024:float32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ops", default="sum,maxabs_diff")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    results = []
    for spec in a.sizes.split(","):
        n, dt = spec.split(":")
        n, dtype = int(n), getattr(torch, dt)
        igg.init_global_grid(n, n, n, periodx=1, periody=1, periodz=1, quiet=True)
        dev = torch.device("cuda", torch.cuda.current_device())
        g = torch.Generator(device=dev).manual_seed(1)
        A = torch.randn(n, n, n, dtype=dtype, device=dev, generator=g)
        B = torch.randn(n, n, n, dtype=dtype, device=dev, generator=g)
        for op in a.ops.split(","):
            for keep in KEEPS:
                results.append(case(op, A, B, keep, a.steps, a.rounds))
        del A, B
        igg.finalize_global_grid()
    print(json.dumps({"project_g": results}))


if __name__ == "__main__":
    main()
