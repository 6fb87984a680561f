"""Per-rank scenario of the ``project_g`` tests (ops/reduce.py), launched by
tests/test_project_cpu.py and tests/test_gpu_project.py, one process per rank.

Every local cell holds an integer function of its GLOBAL index (``indices_g``;
overlapping cells of neighbouring ranks hold the same value), so a projection
over the implicit global grid must equal, bitwise, the same torch reduction of
the global array built directly - on every rank."""
import hashlib
import itertools
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import igg  # noqa: E402

ONE = ("sum", "sumsq", "max", "min", "maxabs")
TWO = ("dot", "sumsq_diff", "maxabs_diff")


def keep_sets(nd):
    return [k for r in range(1, nd) for k in itertools.combinations(range(nd), r)]


def expected(op, F, G, red):
    """The torch reduction of the global arrays over the axes ``red``."""
    if op == "sum":
        return F.sum(dim=red)
    if op == "mean":
        return F.sum(dim=red) / torch.full((), float(math.prod(F.shape[d] for d in red)), dtype=torch.float64)
    if op == "sumsq":
        return (F * F).sum(dim=red)
    if op == "max":
        return F.amax(dim=red)
    if op == "min":
        return F.amin(dim=red)
    if op == "maxabs":
        return F.abs().amax(dim=red)
    if op == "dot":
        return (F * G).sum(dim=red)
    if op == "sumsq_diff":
        return ((F - G) * (F - G)).sum(dim=red)
    return (F - G).abs().amax(dim=red)


def global_arrays(gshape):
    """Two integer functions of the global index (|x| <= 1024), float64."""
    g = torch.meshgrid(*(torch.arange(k, dtype=torch.int64) for k in gshape), indexing="ij")
    g = list(g) + [torch.zeros_like(g[0])] * (3 - len(g))
    F = ((7 * g[0] + 13 * g[1] + 29 * g[2]) % 1000) - 400
    G = ((5 * g[0] + 3 * g[1] + 11 * g[2]) % 601) - 300
    return F.to(torch.float64), G.to(torch.float64)


def local_of(Fg, A_shape):
    """This rank's local array: cell i of axis d holds global cell ``indices_g(d)[i]``."""
    probe = torch.empty(A_shape, device="meta")
    idx = [igg.indices_g(d, probe) for d in range(len(A_shape))]
    return Fg[tuple(torch.meshgrid(*idx, indexing="ij"))].contiguous()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int64), b.view(torch.int64))


def scenario_project(dev, dtype, dimx, dimy, dimz, periodic, overlap, halowidth):
    if dev == "gpu":  # every rank on device 0
        torch.cuda.set_device(0)
        device = torch.device("cuda", 0)
    else:
        device = torch.device("cpu")
    dt = getattr(torch, dtype)
    per, o, w = int(periodic), int(overlap), int(halowidth)
    n = (9, 8, 10)
    me, dims, nprocs, coords, comm = igg.init_global_grid(
        *n, dimx=int(dimx), dimy=int(dimy), dimz=int(dimz), periodx=per & 1, periody=(per >> 1) & 1,
        periodz=(per >> 2) & 1, overlapx=o, overlapy=o, overlapz=o, halowidthx=w, halowidthy=w, halowidthz=w,
        quiet=True, select_device=False, device_type="none" if dev == "cpu" else "AMDGPU")
    h = hashlib.sha256()
    for shape in (n, (n[0] + 1, n[1], n[2]), n[:2]):  # the grid's size, a staggered one, a 2-D field
        nd = len(shape)
        gshape = igg.selection_shape_g(torch.empty(shape, device="meta"))
        Fg, Gg = global_arrays(gshape)
        A = local_of(Fg, shape).to(dt).to(device)
        B = local_of(Gg, shape).to(dt).to(device)
        # the identity with gather_g: the same torch reduction of the array gather_g assembles
        Gath = torch.zeros(gshape, dtype=dt, device=device) if me == 0 else None
        igg.gather_g(A, Gath)
        if me == 0:
            assert torch.equal(Gath.cpu().double(), Fg), shape
        rng = igg.owned_ranges(A)
        for keep in keep_sets(nd):
            red = tuple(d for d in range(nd) if d not in keep)
            for op in ONE + TWO + ("mean",):
                r = igg.project_g(op, A, keep if len(keep) > 1 else keep[0], other=B if op in TWO else None)
                assert r.dtype == torch.float64 and r.device == A.device and r.is_contiguous()
                want = expected(op, Fg, Gg, red)
                if not same(r.cpu(), want):
                    raise AssertionError(f"rank {me} {shape} keep {keep} {op}: got {r.cpu()}, want {want}")
                if me == 0 and op in ("sum", "max"):
                    assert same(r.cpu(), expected(op, Gath.cpu().double(), None, red)), (shape, keep, op)
                h.update(r.cpu().numpy().tobytes())
            # a NaN owned by rank 1 turns NaN exactly the cells whose line or plane holds it, on every rank
            A0 = A.clone()
            at = tuple(r0 for r0, _r1 in rng)
            where = torch.zeros(1 + nd, dtype=torch.int64)  # (owned by rank 1?, its global index)
            if me == 1 and all(int(coords[d]) == 0 for d in range(nd, 3)):
                A[at] = math.nan
                where[0] = 1
                where[1:] = torch.tensor([int(igg.indices_g(d, A)[at[d]]) for d in range(nd)])
            comm.allreduce_(where, "sum")
            for op in ONE + TWO + ("mean",):
                r = igg.project_g(op, A, keep, other=B if op in TWO else None).cpu()
                want = expected(op, Fg, Gg, red)
                if int(where[0]):
                    want[tuple(int(where[1 + d]) for d in keep)] = math.nan
                bad = torch.isnan(r) != torch.isnan(want)
                assert not bad.any() and torch.equal(torch.nan_to_num(r, nan=7.0), torch.nan_to_num(want, nan=7.0)), \
                    f"rank {me} {shape} keep {keep} {op}: the NaN owned by rank 1"
                h.update(r.numpy().tobytes())
            A.copy_(A0)
            # this rank's own contribution: the owned cells at their global indices, the identity elsewhere
            loc = igg.project_g("sum", A, keep, local=True)
            tot = loc.cpu().clone()
            comm.allreduce_(tot, "sum")
            assert same(tot, expected("sum", Fg, Gg, red)), (shape, keep)
    igg.finalize_global_grid()
    print(f"rank {me} project OK BITS={h.hexdigest()}")


if __name__ == "__main__":
    name, *args = sys.argv[1:]
    globals()[f"scenario_{name}"](*args)
