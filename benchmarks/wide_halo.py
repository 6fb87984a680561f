#!/usr/bin/env python3
"""Wide halos on one GPU: what the slab copy kernel and the two-step pass on
a rank with neighbours cost (profiles/wide_halo/NOTES.md).

Part 1 (``--part copy``): the z pack + unpack pair of an n x n x w slab of a
C-ordered n^3 field (one side: what one z neighbour costs), timed with events
in two forms in the same process, alternated:
  slab    one 3-extent copy through the slab kernel (a lane moves a row's w
          elements; one vector access where w * element size is 4, 8 or 16);
  planes  w one-plane copies through the 2-D kernel, batched in one launch
          (what the exchange would do without the slab kernel).

Part 2 (``--part step``): the per-rank step of Diffusion3D in the one-sided
loopback shapes x+, xy+, xyz+ of benchmarks/rank_shapes.py (n^3, graph form),
alternated rounds of
  single  overlap 2, halo width 1, the model's best single step with one
          exchange per step (what a rank with neighbours ran before);
  pass    overlap 4, halo width 2, the two-step pass with one exchange of two
          planes per two steps;
and the N = 1 two-step step (no neighbours) of the same job. Everything is on
one GPU through the loopback emulation: no xGMI transfer is in these numbers.

Usage: python benchmarks/wide_halo.py [--part copy|step|all] [--n 512] [--dtype float64]
                                      [--shapes x+,xy+,xyz+] [--steps 200] [--rounds 3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import igg  # noqa: E402
from igg._native import native  # noqa: E402

SHAPES = {"x+": ((False, True), False, False), "xy+": ((False, True), (False, True), False),
          "xyz+": ((False, True),) * 3}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def part_copy(n, dt, w, reps, rounds):
    T = torch.rand(n, n, n, dtype=torch.float64, device="cuda").to(dt)
    eb = T.element_size()
    buf = torch.empty(w * n * n, dtype=dt, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    base, bp = T.data_ptr(), buf.data_ptr()
    o = 2 * w
    send, recv = n - o, n - w  # right side: planes [n-o, n-o+w) out, [n-w, n) in
    box_p = [(n, n, w, n * n, n, 1, n * w, w, 1)]
    box_u = [(n, n, w, n * w, w, 1, n * n, n, 1)]
    slab_pack = lambda: native.copy3d(box_p, [(base + send * eb, bp)], eb, True, s)  # noqa: E731
    slab_unpack = lambda: native.copy3d(box_u, [(bp, base + recv * eb)], eb, True, s)  # noqa: E731
    # the same bytes as w planes: plane k of the slab is a strided n x n face,
    # packed plane after plane (any packed order costs the 2-D kernel the same)
    pl_p = [(base + (send + k) * eb, bp + k * n * n * eb, n, n, n * n, n, n, 1) for k in range(w)]
    pl_u = [(bp + k * n * n * eb, base + (recv + k) * eb, n, n, n, 1, n * n, n) for k in range(w)]
    planes_pack = lambda: native.copy2d(pl_p, eb, True, s)  # noqa: E731
    planes_unpack = lambda: native.copy2d(pl_u, eb, True, s)  # noqa: E731
    # both forms move the same planes
    ref = T.clone()
    ref[:, :, recv:recv + w] = ref[:, :, send:send + w]
    for pack, unpack in ((slab_pack, slab_unpack), (planes_pack, planes_unpack)):
        X = T.clone()
        T[:, :, recv:] = 0
        pack(), unpack()
        torch.cuda.synchronize()
        assert torch.equal(T, ref), "round trip mismatch"
        T.copy_(X)
    out = {k: [] for k in ("slab_pack", "slab_unpack", "planes_pack", "planes_unpack")}
    for _ in range(rounds):
        for k, fn in (("slab_pack", slab_pack), ("planes_pack", planes_pack), ("slab_unpack", slab_unpack),
                      ("planes_unpack", planes_unpack)):
            out[k].append(round(timed(fn, reps), 3))
    med = {k: sorted(v)[len(v) // 2] for k, v in out.items()}
    res = {"part": "copy", "n": n, "w": w, "dtype": str(dt), "us": med, "all_us": out,
           "slab_pair_us": round(med["slab_pack"] + med["slab_unpack"], 3),
           "planes_pair_us": round(med["planes_pack"] + med["planes_unpack"], 3)}
    print(json.dumps(res), flush=True)
    return res


def _model_step_ms(m, steps, graph_steps):
    m.capture(graph_steps)
    m.run(graph_steps)  # realign + first replay
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    m.run(steps)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def part_step(n, dt, shapes, steps, rounds):
    from igg.models.diffusion3d import Diffusion3D
    from igg.parallel import halo as H

    from igg.parallel import comm as _comm

    if not _comm.runtime_initialized():
        _comm.init_runtime()  # once: the grids below come and go (init_MPI=False)
    graph_steps = 8
    res = {"part": "step", "n": n, "dtype": str(dt), "steps": steps, "shapes": {}}

    def grid(wide, sides):
        kw = dict(overlapx=4, overlapy=4, overlapz=4, halowidthx=2, halowidthy=2, halowidthz=2) if wide else {}
        igg.init_global_grid(n, n, n, quiet=True, init_MPI=False, **kw)
        if sides is not None:
            H.enable_loopback(sides)

    # N = 1: no neighbours, the two-step pass as selected by the model
    ts = []
    for _ in range(rounds):
        grid(False, None)
        m = Diffusion3D(dtype=dt)
        ts.append(_model_step_ms(m, steps, graph_steps))
        two = m._two_step_now()
        del m
        igg.finalize_global_grid(finalize_MPI=False)
    res["n1"] = {"ms": [round(t, 4) for t in ts], "two_step": bool(two)}
    print(json.dumps({"n1": res["n1"]}), flush=True)
    n1 = sorted(ts)[len(ts) // 2]
    for name in shapes:
        rec = {"single": [], "pass": []}
        info = {}
        for _ in range(rounds):
            for form in ("single", "pass"):
                os.environ["IGG_STENCIL_TWOSTEP"] = "0" if form == "single" else "1"
                grid(form == "pass", SHAPES[name])
                m = Diffusion3D(dtype=dt)
                rec[form].append(round(_model_step_ms(m, steps, graph_steps), 4))
                info[form] = {"two_step_now": bool(m._two_step_now()), "variant": m.variant,
                              "transport": H.transport_name(), "mode": H.plan_mode(m.T)}
                del m
                igg.finalize_global_grid(finalize_MPI=False)
        os.environ.pop("IGG_STENCIL_TWOSTEP", None)
        med = {k: sorted(v)[len(v) // 2] for k, v in rec.items()}
        res["shapes"][name] = {"ms": rec, "median_ms": med, "info": info,
                               "pass_over_single": round(med["pass"] / med["single"], 4),
                               "n1_over_pass": round(n1 / med["pass"], 4),
                               "n1_over_single": round(n1 / med["single"], 4)}
        print(json.dumps({name: res["shapes"][name]}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("copy", "step", "all"))
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--w", type=int, default=2)
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="x+,xy+,xyz+")
    ap.add_argument("--out", default=None, help="also write the results as JSON to this file")
    a = ap.parse_args()
    dt = getattr(torch, a.dtype)
    out = []
    if a.part in ("copy", "all"):
        out.append(part_copy(a.n, dt, a.w, a.reps, max(3, a.rounds)))
    if a.part in ("step", "all"):
        out.append(part_step(a.n, dt, [s for s in a.shapes.split(",") if s], a.steps, a.rounds))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
