#!/usr/bin/env python3
"""Single-step acoustic ping-pong against the two-step pass, per chunk length.

At --n^2 cells (default 8192) and --dtype, both forms run the time loop's
ping-pong between two field triples; interleaved rounds, medians, ms per STEP.
Before any timing the end states of 4 single steps and of 2 passes are compared
bitwise for every chunk; no number is printed if one differs."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import igg  # noqa: E402,F401
from igg._native import native  # noqa: E402
from igg.ops import stencil  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--dtype", default="float32", choices=["float32", "float64"])
ap.add_argument("--chunks", default="0,4,8,16,32,64,128", help="rows of x per wave, comma separated (0: the default)")
ap.add_argument("--steps", type=int, default=20, help="steps per timed interval (a multiple of 4)")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--once", type=int, default=0, metavar="K",
                help="no timing: after the bitwise check, one copy of P (calibration), K single steps and K "
                     "passes per chunk, for a `rocprofv3 --pmc` pass")
args = ap.parse_args()
if args.steps < 4 or args.steps % 4:
    ap.error("--steps must be a multiple of 4")

n, dt = args.n, getattr(torch, args.dtype)
chunks = [int(c) for c in args.chunks.split(",")]
g = torch.Generator(device="cuda").manual_seed(3)
shapes = [(n, n), (n + 1, n), (n, n + 1)]
init = [torch.rand(s, dtype=dt, device="cuda", generator=g) for s in shapes]
a = tuple(t.clone() for t in init)
b = tuple(torch.empty_like(t) for t in init)
if not stencil.acoustic2d_twostep_ok(a[0]):
    sys.exit(f"the two-step pass cannot run {n}^2 {args.dtype}")
s = torch.cuda.current_stream().cuda_stream
dx = 10.0 / (n - 1)
coef = (n, n, dx / 4.1, dx / 4.1, 1.0 / dx, 1.0 / dx, a[0].element_size())  # K = rho = 1, dt = dx / 4.1


def single(dst, src):
    native.acoustic2d(*(t.data_ptr() for t in dst + src), *coef, True, s)


def twostep(dst, src, chunk):
    native.acoustic2d_twostep(*(t.data_ptr() for t in dst + src), *coef, chunk, s)


def reset():
    for t, t0 in zip(a, init):
        t.copy_(t0)


native.acoustic2d_set_variant(2)
for k in range(4):
    single(*((b, a) if k % 2 == 0 else (a, b)))
ref = [t.clone() for t in a]
for c in chunks:
    reset()
    twostep(b, a, c)
    twostep(a, b, c)
    torch.cuda.synchronize()
    if not all(torch.equal(x, y) for x, y in zip(a, ref)):
        sys.exit(f"chunk {c}: 2 passes differ from 4 single steps - nothing timed")
reset()
if args.once:
    b[0].copy_(a[0])
    for k in range(args.once):
        single(*((b, a) if k % 2 == 0 else (a, b)))
    for c in chunks:
        for k in range(args.once):
            twostep(*((b, a) if k % 2 == 0 else (a, b)), c)
    torch.cuda.synchronize()
    print(json.dumps({"n": n, "dtype": args.dtype, "bitwise": "ok", "launches_per_form": args.once,
                      "chunks": chunks}))
    sys.exit(0)
t1, t2 = stencil.time_acoustic_twostep_pingpong(a, b, single, twostep, chunks, steps=args.steps, rounds=args.rounds)
nbytes = 2 * sum(t.numel() for t in a) * a[0].element_size()  # 6 arrays per step
res = {"n": n, "dtype": args.dtype, "bitwise": "ok", "ms_per_step": {"single": round(t1, 5)},
       "a_eff_GBs": {"single": round(nbytes / t1 / 1e6, 1)}}
for c, t in t2.items():
    res["ms_per_step"][f"c{c}"] = round(t, 5)
    res["a_eff_GBs"][f"c{c}"] = round(nbytes / t / 1e6, 1)
print(json.dumps(res))
