#!/usr/bin/env python3
"""gather_g (parallel/gather_g.py): the converting pack against the byte mover,
and one plane of the global field against what examples/diffusion3D_multigpu.py
does for a frame today.

pack   the owned box ``[1, n-1)^3`` of an ``n^3`` float64 field packed into a
       compact buffer: ``native.select_convert`` (f64 read, f32 written: 12
       bytes per element) against ``native.copy3d`` (f64 both ways: 16 bytes per
       element). One process, interleaved rounds (utils/timing.py), medians,
       warm-up first, device-synchronised. us and GB/s of the bytes each moves.
plane  the y-mid plane for a GIF frame: ``gather_g(T, P, box=(None, ny_g//2,
       None), dtype=float32)`` against today's form - ``contiguous()`` of the
       halo-free interior, ``gather_`` of the whole volume, indexing the plane.
       Collective: run it alone (one rank) or under ``torch.distributed.run``
       (``--share-gpu``: every rank on device 0). ms per frame between
       ``tic()``/``toc()`` (device drained, barrier) and the bytes the root
       allocates for each form (``--only-new``: ``gather_g`` alone).

    python benchmarks/gather_g.py --part pack --nx 512
    python benchmarks/gather_g.py --part plane --nx 512
    python -m torch.distributed.run --nproc-per-node 8 benchmarks/gather_g.py --part plane --nx 256 --share-gpu

One JSON line at the end (rank 0).
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


def pack(n, steps, rounds):
    dev = torch.device("cuda", torch.cuda.current_device())
    A = torch.randn(n, n, n, dtype=torch.float64, device=dev)
    m = n - 2
    c = [m, m, m]
    S, T = [n * n, n, 1], [m * m, m, 1]
    off = 8 * (n * n + n + 1)
    out32 = torch.empty(m * m * m, dtype=torch.float32, device=dev)
    out64 = torch.empty(m * m * m, dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    job = [(A.data_ptr() + off, out32.data_ptr(), c, S, T)]
    box, ptrs = [c + S + T], [(A.data_ptr() + off, out64.data_ptr())]
    cands = ["select_convert f64->f32", "copy3d f64"]

    def run(cand, k):
        for _ in range(k):
            if cand == cands[0]:
                native.select_convert(job, s)
            else:
                native.copy3d(box, ptrs, 8, True, s)

    run(cands[0], 1)
    run(cands[1], 1)
    torch.cuda.synchronize()
    inner = A[1:-1, 1:-1, 1:-1]
    assert torch.equal(out64.view(m, m, m), inner) and torch.equal(out32.view(m, m, m), inner.float())
    per = [[] for _ in cands]
    for r in range(rounds):
        for t, ms in zip(per, interleaved_medians(cands, run, steps=steps, rounds=1, warm=3 if r == 0 else 0)):
            t.append(ms)
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    elems = m ** 3
    res = {"n": n, "plan": native.select_plan(c, S, T), "copy3d_plan": native.copy3d_plan(c + S + T, ptrs[0], 8)["path"]}
    for name, t, bpe in zip(cands, per, (12, 16)):
        res[name] = {"us": round(med(t) * 1e3, 1), "min_max_us": [round(min(t) * 1e3, 1), round(max(t) * 1e3, 1)],
                     "bytes": elems * bpe, "GBs": round(elems * bpe / med(t) / 1e6, 1)}
        print(f"pack {n}^3 owned box | {name:24s} {res[name]['us']:9.1f} us  [{res[name]['min_max_us'][0]}, "
              f"{res[name]['min_max_us'][1]}]  {res[name]['GBs']:7.1f} GB/s of {bpe} B/element", flush=True)
    res["convert_over_copy"] = round(med(per[0]) / med(per[1]), 3)
    return res


def plane(n, steps, rounds, share_gpu, only_new=False):
    if share_gpu:
        torch.cuda.set_device(0)
    me, dims, nprocs, coords, comm = igg.init_global_grid(n, n, n, quiet=True, select_device=not share_gpu)
    dev = torch.device("cuda", torch.cuda.current_device())
    T = torch.randn(n, n, n, dtype=torch.float64, device=dev)
    igg.update_halo_(T)
    sel = (None, igg.ny_g() // 2, None)
    shape = igg.selection_shape_g(T, sel)
    P = torch.zeros(shape, dtype=torch.float32, device=dev) if me == 0 else None
    v = [(n - 2) * int(d) for d in dims]
    T_v = torch.zeros(v, dtype=torch.float64, device=dev) if me == 0 and not only_new else None

    def new():
        igg.gather_g(T, P, box=sel, dtype=torch.float32)
        return P[:, 0, :] if me == 0 else None

    def today():
        T_nohalo = T[1:-1, 1:-1, 1:-1].contiguous()
        igg.gather_(T_nohalo, T_v)
        return T_v[:, v[1] // 2, :] if me == 0 else None

    forms = {"gather_g plane f32": new, "contiguous + gather_ + index": today}
    if only_new:
        del forms["contiguous + gather_ + index"]
    for f in forms.values():  # warm-up: buffers, transports, code objects
        for _ in range(3):
            f()
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            igg.tic()
            for _ in range(steps):
                f()
            times[k].append(igg.toc() / steps * 1e3)
    # today's picture is the new one without the outermost global cells (overlap 2, not periodic)
    Pg = torch.zeros(shape, dtype=torch.float32, device=dev) if me == 0 else None
    igg.gather_g(T, Pg, box=(None, v[1] // 2 + 1, None), dtype=torch.float32)
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    res = None
    if me == 0:
        if not only_new:
            assert torch.equal(Pg[1:-1, 0, 1:-1], today().float()), "the two forms disagree on the shared cells"
        alloc = {"gather_g plane f32": P.numel() * 4,
                 "contiguous + gather_ + index": (v[0] * v[1] * v[2] + (n - 2) ** 3) * 8}
        res = {"n": n, "nprocs": nprocs, "dims": [int(d) for d in dims], "share_gpu": bool(share_gpu),
               "plane_shape": list(shape)}
        for k in forms:
            res[k] = {"ms_per_frame": round(med(times[k]), 3),
                      "min_max_ms": [round(min(times[k]), 3), round(max(times[k]), 3)], "root_bytes": alloc[k]}
            print(f"plane {n}^3 x {nprocs} ranks | {k:30s} {res[k]['ms_per_frame']:9.3f} ms/frame "
                  f"[{res[k]['min_max_ms'][0]}, {res[k]['min_max_ms'][1]}]  root allocates "
                  f"{alloc[k] / 2 ** 20:9.1f} MiB", flush=True)
        if only_new:
            res["contiguous + gather_ + index"] = {"root_bytes": alloc["contiguous + gather_ + index"]}
        else:
            res["speedup"] = round(med(times["contiguous + gather_ + index"]) / med(times["gather_g plane f32"]), 2)
    igg.finalize_global_grid()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=("pack", "plane"), required=True)
    ap.add_argument("--nx", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--share-gpu", action="store_true", help="plane: every rank on device 0")
    ap.add_argument("--only-new", action="store_true", help="plane: time gather_g alone")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = pack(a.nx, a.steps, a.rounds) if a.part == "pack" else plane(a.nx, a.steps, a.rounds, a.share_gpu, a.only_new)
    if res is not None:
        print(json.dumps({f"gather_g_{a.part}": res}))


if __name__ == "__main__":
    main()
