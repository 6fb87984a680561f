#!/usr/bin/env python3
"""The adjoint acoustic kernel against the forward single-step kernel.

The transpose of the staggered step moves the forward step's six array passes
- read gP2, gVx2, gVy2, write gP, gVx, gVy - with the same data flow, so its
yardstick is the forward vector-march kernel (``native.acoustic2d``, variant 2,
its default chunk) on buffers of the same placement: 8192^2 float32 and 4096^2
float64 in one process, interleaved rounds (utils/timing.py), medians, warm-up
first, events on the stream. The adjoint is timed with 2, 4, 8, 12 and 16 rows
of x per wave and with its default. The device result is compared with a plain
torch formulation of the transpose on a small field first.

    python benchmarks/acoustic_adjoint.py [--quick] [--only f64|f32]

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
from igg._native import native  # noqa: E402
from igg.ops import stencil  # noqa: E402
from igg.utils.timing import interleaved_medians  # noqa: E402

KW = dict(dt=0.01, K=1.3, rho=0.8, dx=0.1, dy=0.07)
CHUNKS = (2, 4, 8, 12, 16)


def torch_adjoint(gP2, gVx2, gVy2):
    """S^T in plain torch: the dozen passes a user would write today."""
    a, b, rdx, rdy = KW["dt"] * KW["K"], KW["dt"] / KW["rho"], 1.0 / KW["dx"], 1.0 / KW["dy"]
    wx, wy = torch.zeros_like(gVx2), torch.zeros_like(gVy2)
    wx[1:-1] = b * gVx2[1:-1] * rdx
    wy[:, 1:-1] = b * gVy2[:, 1:-1] * rdy
    r = gP2 + (wx[1:] - wx[:-1]) + (wy[:, 1:] - wy[:, :-1])
    gVx, gVy = gVx2.clone(), gVy2.clone()
    gVx[:-1] += a * r * rdx
    gVx[1:] -= a * r * rdx
    gVy[:, :-1] += a * r * rdy
    gVy[:, 1:] -= a * r * rdy
    return r, gVx, gVy


def fields(nx, ny, dtype, dev):
    return [torch.rand(s, dtype=dtype, device=dev) - 0.5 for s in ((nx, ny), (nx + 1, ny), (nx, ny + 1))]


def check(dtype, dev):
    errs = []
    for nx, ny in ((37, 53), (41, 504)):
        gin = fields(nx, ny, dtype, dev)
        out = [torch.empty_like(t) for t in gin]
        stencil.acoustic2d_adjoint_(*out, *gin, **KW)
        errs.append(max(float((o - w).abs().max()) for o, w in zip(out, torch_adjoint(*gin))))
    err = max(errs)
    assert err < (1e-5 if dtype == torch.float32 else 1e-13), err
    return err


def case(n, dtype, steps, rounds, dev):
    es = torch.empty(0, dtype=dtype).element_size()
    src, dst = fields(n, n, dtype, dev), fields(n, n, dtype, dev)
    coef = (n, n, KW["dt"] * KW["K"], KW["dt"] / KW["rho"], 1.0 / KW["dx"], 1.0 / KW["dy"], es)
    ptrs = [t.data_ptr() for t in dst + src]
    s = torch.cuda.current_stream().cuda_stream
    native.acoustic2d_set_variant(2)
    native.acoustic2d_set_chunk(0)
    forms = {"forward": lambda: native.acoustic2d(*ptrs, *coef, True, s),
             "adjoint": lambda: native.acoustic2d_adjoint(*ptrs, *coef, True, s, 0)}
    for c in CHUNKS:
        forms[f"adjoint_c{c}"] = lambda c=c: native.acoustic2d_adjoint(*ptrs, *coef, True, s, c)
    names = list(forms)

    def run(c, k):
        for _ in range(k):
            forms[c]()

    ms = dict(zip(names, interleaved_medians(names, run, steps, rounds, warm=2)))
    nbytes = 2 * sum(t.numel() for t in src) * es
    res = {"n": n, "dtype": str(dtype).split(".")[-1], "default_chunk": int(native.acoustic2d_adjoint_chunk()),
           "ms": {k: round(v, 4) for k, v in ms.items()},
           "ratio_to_forward": {k: round(ms[k] / ms["forward"], 3) for k in names if k != "forward"},
           "GBs": {k: round(nbytes / ms[k] / 1e6, 1) for k in names}}
    print(f"{n}^2 {res['dtype']}: forward {ms['forward']:.4f} ms; " +
          ", ".join(f"{k} {ms[k]:.4f} ms ({res['ratio_to_forward'][k]:.3f}x)" for k in names[1:]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--quick", action="store_true", help="4096^2 / 2048^2, fewer rounds")
    ap.add_argument("--only", choices=["f64", "f32"], default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    errs = {"f64": check(torch.float64, dev), "f32": check(torch.float32, dev)}
    steps, rounds = (5, 3) if a.quick else (10, 7)
    cases = []
    if a.only != "f64":
        cases.append(case(4096 if a.quick else 8192, torch.float32, steps, rounds, dev))
    if a.only != "f32":
        cases.append(case(2048 if a.quick else 4096, torch.float64, steps, rounds, dev))
    print(json.dumps({"bench": "acoustic_adjoint", "check_err": errs, "cases": cases}))


if __name__ == "__main__":
    main()
