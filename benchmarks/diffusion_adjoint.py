#!/usr/bin/env python3
"""The adjoint diffusion kernels against the forward single-step kernel.

``adjoint_t`` (gT = S^T g) moves the forward step's three arrays - read g,
read Cp or Q, write gT - so its yardstick is the forward kernel the autotune
picks for the same shape, not a fixed time. Both run on the same buffers:
512^3 float64 and 1024^3 float32 on one process, interleaved rounds
(utils/timing.py), medians, warm-up first, events on the stream. ``adjoint_cp``
(four arrays: read T, Cp and g, write gCp; five accumulated) is timed in the
same rounds. The device results are compared with a plain torch formulation of
the transpose on a small field first.

    python benchmarks/diffusion_adjoint.py [--quick] [--only f64|f32]

One JSON line at the end: per case the ms of every form and the ratios to the
forward kernel.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import igg  # noqa: F401, E402
from igg.ops import stencil  # noqa: E402
from igg.utils.timing import interleaved_medians  # noqa: E402

KW = dict(lam=1.0, dt=0.01, dx=0.3, dy=0.25, dz=0.2)


def torch_adjoint_t(g, Cp):
    """S^T g in plain torch: the ten passes a user would write today."""
    rd2 = [1.0 / KW[k] ** 2 for k in ("dx", "dy", "dz")]
    u = torch.zeros_like(g)
    u[1:-1, 1:-1, 1:-1] = KW["dt"] * KW["lam"] / Cp[1:-1, 1:-1, 1:-1] * g[1:-1, 1:-1, 1:-1]
    out = g - 2.0 * sum(rd2) * u
    for d in range(3):
        out.narrow(d, 1, g.shape[d] - 1).add_(u.narrow(d, 0, g.shape[d] - 1), alpha=rd2[d])
        out.narrow(d, 0, g.shape[d] - 1).add_(u.narrow(d, 1, g.shape[d] - 1), alpha=rd2[d])
    return out


def check(dtype, dev):
    g = torch.rand(40, 33, 72, dtype=dtype, device=dev) - 0.5
    Cp = 1 + torch.rand_like(g)
    out = torch.empty_like(g)
    stencil.diffusion3d_adjoint_(out, g, Cp, **KW)
    err = float((out - torch_adjoint_t(g, Cp)).abs().max())
    assert err < (1e-5 if dtype == torch.float32 else 1e-13), err
    return err


def case(n, dtype, steps, rounds, dev):
    shape = (n, n, n)
    es = torch.empty(0, dtype=dtype).element_size()
    T = torch.rand(shape, dtype=dtype, device=dev)
    Cp = 1 + torch.rand(shape, dtype=dtype, device=dev)
    g = torch.rand(shape, dtype=dtype, device=dev) - 0.5
    Q = torch.empty_like(Cp)
    stencil.quotient_(Q, Cp, lam=KW["lam"], dt=KW["dt"])
    out = T.clone()
    rd2 = [1.0 / KW[k] ** 2 for k in ("dx", "dy", "dz")]
    boxes = [(list(b[0]), list(b[1])) for b in [stencil.inner_box(shape)]]
    short = [v for v in stencil.SHORTLIST if v in stencil.compiled_variants()]
    tv = stencil.time_variants(out, T, Cp, rd2, KW["dt"] * KW["lam"], boxes, candidates=short, reps=steps)
    best = min(tv, key=tv.get)

    forms = {
        "forward": lambda: stencil.diffusion3d_(out, T, Cp, variant=best, **KW),
        "adjoint_t": lambda: stencil.diffusion3d_adjoint_(out, g, Cp, **KW),
        "adjoint_t_q": lambda: stencil.diffusion3d_adjoint_(out, g, Cp, Q=Q, **KW),
        "adjoint_cp": lambda: stencil.diffusion3d_adjoint_(None, g, Cp, T=T, gCp=out, **KW),
        "adjoint_cp_acc": lambda: stencil.diffusion3d_adjoint_(None, g, Cp, T=T, gCp=out, accumulate=True, **KW),
    }
    names = list(forms)

    def run(c, k):
        for _ in range(k):
            forms[c]()

    ms = dict(zip(names, interleaved_medians(names, run, steps, rounds, warm=2)))
    cells = n ** 3
    res = {"n": n, "dtype": str(dtype).split(".")[-1], "forward_variant": stencil.variants()[best],
           "ms": {k: round(v, 4) for k, v in ms.items()},
           "ratio_to_forward": {k: round(ms[k] / ms["forward"], 3) for k in names if k != "forward"},
           "GBs": {k: round(cells * es * a / ms[k] / 1e6, 1)
                   for k, a in (("forward", 3), ("adjoint_t", 3), ("adjoint_t_q", 3), ("adjoint_cp", 4),
                                ("adjoint_cp_acc", 5))}}
    print(f"{n}^3 {res['dtype']}: forward {res['forward_variant']} {ms['forward']:.4f} ms; " +
          ", ".join(f"{k} {ms[k]:.4f} ms ({res['ratio_to_forward'][k]:.3f}x)" for k in names[1:]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--quick", action="store_true", help="256^3 / 512^3, fewer rounds")
    ap.add_argument("--only", choices=["f64", "f32"], default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    errs = {"f64": check(torch.float64, dev), "f32": check(torch.float32, dev)}
    steps, rounds = (5, 3) if a.quick else (10, 7)
    cases = []
    if a.only != "f32":
        cases.append(case(256 if a.quick else 512, torch.float64, steps, rounds, dev))
    if a.only != "f64":
        cases.append(case(512 if a.quick else 1024, torch.float32, steps, rounds, dev))
    print(json.dumps({"bench": "diffusion_adjoint", "check_err": errs, "cases": cases}))


if __name__ == "__main__":
    main()
