#!/usr/bin/env python3
"""scatter_g (parallel/scatter_g.py): the widening placement against the byte
mover, and a whole field from a root against what a user does today.

unpack  the interior box ``[1, n-1)^3`` of an ``n^3`` float64 field filled from
        a compact buffer: ``native.select_widen`` (f32 read, f64 written: 12
        bytes per element) against ``native.copy3d`` (f64 both ways: 16 bytes
        per element). One process, interleaved rounds (utils/timing.py),
        medians, warm-up first, device-synchronised, both results checked
        first. us and GB/s of the bytes each moves.
field   ``scatter_g(G, A)`` of a whole float64 field against today's form -
        ``comm.bcast_`` of the global array to every rank, indexing it with
        ``indices_g``, ``update_halo_``. Collective: run it alone (one rank)
        or under ``torch.distributed.run`` (``--share-gpu``: every rank on
        device 0; the broadcast then goes through the host, as RCCL refuses
        ranks that share a GPU). ms per call between ``tic()``/``toc()``
        (device drained, barrier) and the bytes each form allocates per rank.

    python benchmarks/scatter_g.py --part unpack --nx 512
    python benchmarks/scatter_g.py --part field --nx 512
    python -m torch.distributed.run --nproc-per-node 8 benchmarks/scatter_g.py --part field --nx 256 --share-gpu

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
from igg.parallel import gather_g as GG  # noqa: E402
from igg.utils.timing import interleaved_medians  # noqa: E402

med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731


def unpack(n, steps, rounds):
    dev = torch.device("cuda", torch.cuda.current_device())
    m = n - 2
    c = [m, m, m]
    S, T = [m * m, m, 1], [n * n, n, 1]
    off = 8 * (n * n + n + 1)
    in32 = torch.randn(m * m * m, dtype=torch.float32, device=dev)
    in64 = in32.double()
    A32 = torch.zeros(n, n, n, dtype=torch.float64, device=dev)
    A64 = torch.zeros(n, n, n, dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    job = [(in32.data_ptr(), A32.data_ptr() + off, c, S, T)]
    box, ptrs = [c + S + T], [(in64.data_ptr(), A64.data_ptr() + off)]
    cands = ["select_widen f32->f64", "copy3d f64"]

    def run(cand, k):
        for _ in range(k):
            if cand == cands[0]:
                native.select_widen(job, s)
            else:
                native.copy3d(box, ptrs, 8, True, s)

    run(cands[0], 1)
    run(cands[1], 1)
    torch.cuda.synchronize()
    want = torch.zeros(n, n, n, dtype=torch.float64, device=dev)
    want[1:-1, 1:-1, 1:-1] = in64.view(m, m, m)
    assert torch.equal(A32, want) and torch.equal(A64, want)
    del want
    per = [[] for _ in cands]
    for r in range(rounds):
        for t, ms in zip(per, interleaved_medians(cands, run, steps=steps, rounds=1, warm=3 if r == 0 else 0)):
            t.append(ms)
    elems = m ** 3
    res = {"n": n, "plan": native.select_plan(c, S, T), "copy3d_plan": native.copy3d_plan(c + S + T, ptrs[0], 8)["path"]}
    for name, t, bpe in zip(cands, per, (12, 16)):
        res[name] = {"us": round(med(t) * 1e3, 1), "min_max_us": [round(min(t) * 1e3, 1), round(max(t) * 1e3, 1)],
                     "bytes": elems * bpe, "GBs": round(elems * bpe / med(t) / 1e6, 1)}
        print(f"unpack {n}^3 interior box | {name:24s} {res[name]['us']:9.1f} us  [{res[name]['min_max_us'][0]}, "
              f"{res[name]['min_max_us'][1]}]  {res[name]['GBs']:7.1f} GB/s of {bpe} B/element", flush=True)
    res["widen_over_copy"] = round(med(per[0]) / med(per[1]), 3)
    return res


def field(n, steps, rounds, share_gpu):
    if share_gpu:
        torch.cuda.set_device(0)
    me, dims, nprocs, coords, comm = igg.init_global_grid(n, n, n, quiet=True, select_device=not share_gpu)
    dev = torch.device("cuda", torch.cuda.current_device())
    A = torch.zeros(n, n, n, dtype=torch.float64, device=dev)
    B = torch.zeros(n, n, n, dtype=torch.float64, device=dev)
    ext = igg.selection_shape_g(A)
    G = torch.randn(ext, dtype=torch.float64, device=dev) if me == 0 else None
    ix = [igg.indices_g(d, A).to(dev) for d in range(3)]
    held = {}

    def new():
        igg.scatter_g(G, A)

    def today():
        if share_gpu:  # RCCL refuses ranks that share a GPU: the broadcast goes through the host
            Gh = G.cpu() if me == 0 else torch.empty(ext, dtype=torch.float64)
            comm.bcast_(Gh, 0)
            Gb = Gh.to(dev)
        else:
            Gb = G if me == 0 else torch.empty(ext, dtype=torch.float64, device=dev)
            comm.bcast_(Gb, 0)
        B.copy_(Gb[ix[0].view(-1, 1, 1), ix[1].view(1, -1, 1), ix[2].view(1, 1, -1)])
        igg.update_halo_(B)
        held["bytes"] = 0 if me == 0 and not share_gpu else Gb.numel() * 8

    forms = {"scatter_g": new, "bcast_ + index + update_halo_": today}
    for f in forms.values():  # warm-up: buffers, transports, code objects
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    assert torch.equal(A, B), "the two forms disagree"
    staged = sum(b.numel() for b in GG._bufs.values())
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            igg.tic()
            for _ in range(steps):
                f()
            times[k].append(igg.toc() / steps * 1e3)
    alloc = comm.all_gather_object((staged, held["bytes"] + n ** 3 * 8))  # (today's indexing makes one field-sized temporary)
    res = None
    if me == 0:
        res = {"n": n, "nprocs": nprocs, "dims": [int(d) for d in dims], "share_gpu": bool(share_gpu),
               "global_shape": list(ext)}
        for j, k in enumerate(forms):
            per_rank = [a[j] for a in alloc]
            res[k] = {"ms_per_call": round(med(times[k]), 3),
                      "min_max_ms": [round(min(times[k]), 3), round(max(times[k]), 3)],
                      "bytes_root": per_rank[0], "bytes_other_rank_max": max(per_rank[1:], default=0)}
            print(f"field {n}^3 x {nprocs} ranks | {k:30s} {res[k]['ms_per_call']:9.3f} ms/call "
                  f"[{res[k]['min_max_ms'][0]}, {res[k]['min_max_ms'][1]}]  allocates {per_rank[0] / 2 ** 20:9.1f} MiB "
                  f"on the root, up to {res[k]['bytes_other_rank_max'] / 2 ** 20:9.1f} MiB elsewhere", flush=True)
        res["speedup"] = round(med(times["bcast_ + index + update_halo_"]) / med(times["scatter_g"]), 2)
    igg.finalize_global_grid()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=("unpack", "field"), required=True)
    ap.add_argument("--nx", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--share-gpu", action="store_true", help="field: every rank on device 0")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = unpack(a.nx, a.steps, a.rounds) if a.part == "unpack" else field(a.nx, a.steps, a.rounds, a.share_gpu)
    if res is not None:
        print(json.dumps({f"scatter_g_{a.part}": res}))


if __name__ == "__main__":
    main()
