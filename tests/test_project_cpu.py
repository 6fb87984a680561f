"""``project_g`` on the host (ops/reduce.py): the host-side plan of the
projection kernels, the placement of a rank's contribution on simulated
topologies, every op on CPU tensors and multi-rank gloo runs.

Oracle: the same torch / numpy reduction, over the reduced axes, of the global
array built directly. Data are integers of [-1024, 1024], so every f64 sum is
exact whatever its order and every comparison is bitwise.
"""
import itertools
import math
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest
import torch

import igg
from igg._native import native
from igg.parallel import grid as G
from tests._mp import MAX_TIMEOUT, ROOT, free_port
from tests.mp_worker_project import ONE, TWO, expected, global_arrays, keep_sets, same

KW = dict(quiet=True, init_MPI=False, device_type="none")
BASE = 1 << 20


def run_project_ranks(nprocs: int, *args, timeout: float = 150.0) -> list:
    """``tests/mp_worker_project.py project ...`` on ``nprocs`` local ranks;
    the first rank that fails stops the others, a timeout fails the test with
    every rank's output."""
    port = free_port()
    procs, logs = [], []
    for r in range(nprocs):
        env = dict(os.environ)
        env.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(r),
                    "WORLD_SIZE": str(nprocs), "LOCAL_RANK": str(r), "LOCAL_WORLD_SIZE": str(nprocs),
                    "OMP_NUM_THREADS": "1", "IGG_HOST_THREADS": "2",
                    "PYTHONPATH": ROOT + os.pathsep + env.get("PYTHONPATH", "")})
        log = tempfile.TemporaryFile(mode="w+")
        logs.append(log)
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tests", "mp_worker_project.py"), "project", *map(str, args)],
            env=env, stdout=log, stderr=subprocess.STDOUT, text=True, cwd=ROOT))
    deadline = time.monotonic() + min(timeout, MAX_TIMEOUT)
    try:
        while True:
            codes = [p.poll() for p in procs]
            if any(c not in (None, 0) for c in codes) or all(c == 0 for c in codes) or time.monotonic() > deadline:
                break
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    outs = []
    for log in logs:
        log.seek(0)
        outs.append(log.read())
        log.close()
    codes = [p.returncode for p in procs]
    if any(c != 0 for c in codes):
        msg = "\n".join(f"--- rank {r} rc={c}\n{o[-2500:]}" for r, (c, o) in enumerate(zip(codes, outs)))
        raise AssertionError(f"project scenario {args} failed or timed out:\n{msg}")
    return outs


def check_rank_outputs(outs) -> None:
    """Every rank passed and received the same result bits."""
    bits = []
    for r, o in enumerate(outs):
        m = re.search(rf"rank {r} project OK BITS=(\S+)", o)
        assert m, o[-1500:]
        bits.append(m.group(1))
    assert len(set(bits)) == 1, "the ranks received different bits"


def _place(dims, coords, periods=None):
    """Pretend to be rank ``coords`` of a ``dims`` grid (the grid's arrays are mutable)."""
    gg = G.global_grid()
    gg.dims[:] = dims
    gg.coords[:] = coords
    if periods is not None:
        gg.periods[:] = periods
    gg.nxyz_g[:] = gg.dims * (gg.nxyz - gg.overlaps) + gg.overlaps * (gg.periods == 0)
    return gg


# ----------------------------------------------------------------------- plan
def _perm_strides(shape, order):
    """Dense strides of ``shape`` whose axes lie in memory in ``order`` (outer .. inner)."""
    s, acc = [0] * len(shape), 1
    for d in reversed(order):
        s[d] = acc
        acc *= shape[d]
    return s


def _plan(shape, lo, hi, keep, es=8, strides=None, base=BASE, **kw):
    if strides is None:
        strides = _perm_strides(shape, range(len(shape)))
    return native.project_plan(list(shape), list(strides), list(lo), list(hi), list(keep), es, base, **kw)


@pytest.mark.parametrize("es", [4, 8])
def test_plan_family_and_path_for_every_keep_set_and_layout(es):
    for shape, vector in (((8, 12, 16), True), ((5, 7, 9), False)):  # every pitch a multiple of 16 B, or none
        nd = len(shape)
        lo, hi = (1,) * nd, tuple(n - 1 for n in shape)
        for order in itertools.permutations(range(nd)):
            strides = _perm_strides(shape, order)
            for keep in keep_sets(nd):
                p = _plan(shape, lo, hi, keep, es=es, strides=strides)
                want = "".join("K" if d in keep else "R" for d in order)  # an interior box: nothing merges
                assert p["pattern"] == want, (order, keep, p)
                assert p["family"] == (1 if order[-1] in keep else 2), (order, keep, p)
                assert p["path"] == ("vector" if vector else "element"), (order, keep, p)
                assert p["vec"] == (16 // es if vector else 1) and p["total"] == math.prod(h - 1 for h in hi)
                assert p["outputs"] == math.prod(hi[d] - lo[d] for d in keep)
    for shape in ((8, 16), (7, 9)):  # 2-D
        for order in itertools.permutations(range(2)):
            for keep in ((0,), (1,)):
                p = _plan(shape, (1, 1), (shape[0] - 1, shape[1] - 1), keep, es=es, strides=_perm_strides(shape, order))
                assert p["family"] == (1 if order[-1] in keep else 2)
                assert p["pattern"] == "".join("K" if d in keep else "R" for d in order)
                assert p["path"] == ("vector" if shape == (8, 16) else "element")


def test_plan_merges_and_drops():
    p = _plan((8, 8, 8), (0, 0, 0), (8, 8, 8), (0,))  # a fully owned dense array: rows of 64 per output
    assert p["pattern"] == "KR" and p["family"] == 2 and p["box"] == (1, 8, 1, 64) and p["outputs"] == 8
    p = _plan((8, 8, 8), (0, 0, 0), (8, 8, 8), (2,))
    assert p["pattern"] == "RK" and p["family"] == 1 and p["box"] == (1, 1, 64, 8) and p["strides"][2:] == (8, 1)
    p = _plan((8, 8, 8), (0, 0, 0), (8, 8, 8), (1, 2))
    assert p["pattern"] == "RK" and p["box"] == (1, 1, 8, 64) and p["partial_strides"] == (8, 1)
    p = _plan((8, 8, 8), (1, 1, 0), (7, 7, 8), (0,))  # whole rows: the two reduced axes are one run per plane
    assert p["pattern"] == "KR" and p["box"] == (1, 6, 1, 48) and p["offset"] == 72
    p = _plan((8, 8, 8), (1, 1, 1), (7, 7, 7), (0, 2))
    assert p["pattern"] == "KRK" and p["box"] == (6, 1, 6, 6) and p["head"] == 1 and p["loads_per_row"] == 4
    p = _plan((8, 8, 8), (1, 3, 1), (7, 4, 7), (0, 2))  # one reduced cell: the extent of one drops out
    assert p["pattern"] == "KK" and p["family"] == 1 and p["reduced"] == 1 and p["slices"] == 1
    p = _plan((8, 8, 8), (3, 1, 1), (4, 7, 7), (0,))  # one output cell
    assert p["pattern"] == "RR" and p["family"] == 2 and p["outputs"] == 1
    p = _plan((8, 8, 8), (3, 3, 3), (4, 4, 4), (1,))  # a single element
    assert p["total"] == 1 and p["outputs"] == 1 and p["blocks"] == 1
    p = _plan((8, 8, 8), (3, 3, 3), (4, 3, 4), (1,))  # an empty box: no first stage
    assert p["total"] == 0 and p["blocks"] == 0 and p["outputs"] == 0
    # a permuted layout: the partials follow the memory order, the strides map the field's kept axes into it
    p = _plan((6, 7, 9), (1, 1, 1), (5, 6, 8), (0, 2), strides=(1, 6, 42))
    assert p["pattern"] == "KRK" and p["path"] == "vector" and p["partial_strides"] == (1, 4)
    # with a second input both must be contiguous for a merge, and share the head residue for vector loads
    p = _plan((8, 8), (0, 0), (8, 8), (0,), strides_b=[8, 1], base_b=BASE)
    assert p["path"] == "vector" and p["pattern"] == "KR"
    p = _plan((8, 8), (0, 0), (8, 8), (0,), strides_b=[1, 8], base_b=BASE)
    assert p["path"] == "element"
    p = _plan((8, 8), (0, 1), (8, 7), (0,), strides_b=[8, 1], base_b=BASE + 8)
    assert p["path"] == "element"


@pytest.mark.parametrize("es", [4, 8])
def test_plan_vector_loads_need_aligned_base_and_pitches(es):
    vec = 16 // es
    for pitch in range(8, 8 + 2 * vec + 1):
        for off in range(0, 2 * vec + 1):
            for keep in ((0,), (2,), (0, 2)):
                p = _plan((4, 5, 6), (0, 1, 1), (4, 4, 5), keep, es=es, strides=(5 * pitch + es * 16, pitch, 1),
                          base=BASE + off * es)
                aligned = (off * es) % 16 == 0 and (pitch * es) % 16 == 0 and ((5 * pitch + es * 16) * es) % 16 == 0
                assert (p["path"] == "vector") == aligned, (pitch, off, p)
                if not aligned:
                    assert p["vec"] == 1 and p["head"] == 0 and p["index_bits"] == 64


def test_plan_depends_on_the_box_and_the_keep_set_only():
    cap, smax = native.PROJECT_MAX_BLOCKS, native.PROJECT_MAX_SLICES
    for shape, lo, hi in [((70, 33, 9), (1, 1, 1), (69, 32, 8)), ((192, 40, 64), (0, 0, 0), (192, 40, 64)),
                          ((512, 512, 512), (1, 1, 1), (511, 511, 511)), ((1024, 1024, 1024), (1,) * 3, (1023,) * 3)]:
        for keep in keep_sets(3):
            plans = [_plan(shape, lo, hi, keep, es=4, base=b) for b in (BASE, 7 * BASE, 1 << 40)]
            assert all(p == plans[0] for p in plans)
            p = plans[0]
            assert 1 <= p["slices"] <= min(smax, p["reduced"]) and p["units"] == p["slices"] * (
                p["box"][0] if p["family"] == 1 else p["outputs"])
            assert p["blocks"] == min(p["block_units"], cap) and 1 <= p["blocks"] <= cap
    # 1024^3 f32: element offsets fit 32 bits; a box whose span does not takes 64-bit offsets
    assert _plan((1024,) * 3, (1,) * 3, (1023,) * 3, (1,), es=4)["index_bits"] == 32
    assert _plan((2048, 1024, 1024), (1,) * 3, (2047, 1023, 1023), (1,), es=4)["index_bits"] == 64
    assert _plan((512,) * 3, (1,) * 3, (511,) * 3, (0, 1))["blocks"] == cap
    assert _plan((512,) * 3, (1,) * 3, (511,) * 3, (2,))["slices"] == smax


def _visits(p, size):
    """Replay the first stage's index arithmetic from the plan alone: the
    (partial index, element offset from the field's base) pairs of every load
    element that counts, and the slice each belongs to."""
    n, s = p["box"], p["strides"]
    vec, head, nv, lanes, cx = p["vec"], p["head"], p["loads_per_row"], p["lanes"], p["chunks_per_row"]
    out = []
    for unit in range(p["units"]):
        if p["family"] == 1:  # slots [KO, R0, R1, KI]
            ko, sl = divmod(unit, p["slices"])
            rb, re_ = sl * p["reduced"] // p["slices"], (sl + 1) * p["reduced"] // p["slices"]
            for j in range(nv):
                for e in range(vec):
                    pos = j * vec - head + e
                    if not 0 <= pos < n[3]:
                        continue
                    for r in range(rb, re_):
                        r0, r1 = divmod(r, n[2])
                        out.append((sl, ko * n[3] + pos, p["offset"] + ko * s[0] + r0 * s[1] + r1 * s[2] + pos * s[3]))
        else:  # slots [K0, K1, RO, RI]
            sl, o = divmod(unit, p["outputs"])
            k0, k1 = divmod(o, n[1])
            tb, te = sl * p["reduced"] // p["slices"], (sl + 1) * p["reduced"] // p["slices"]
            for t in range(tb, te):
                ro, c = divmod(t, cx)
                for lane in range(lanes):
                    j = c * lanes + lane
                    if j >= nv:
                        continue
                    for e in range(vec):
                        pos = j * vec - head + e
                        if 0 <= pos < n[3]:
                            out.append((sl, o, p["offset"] + k0 * s[0] + k1 * s[1] + ro * s[2] + pos * s[3]))
    assert all(0 <= off < size for _sl, _o, off in out)
    return out


@pytest.mark.parametrize("es", [4, 8])
def test_plan_brute_force_every_element_once_by_its_output(es):
    shapes = [((6, 8, 12), (1, 1, 1), (5, 7, 11)), ((6, 8, 12), (0, 0, 0), (6, 8, 12)), ((5, 7, 9), (1, 0, 2), (4, 7, 8)),
              ((3, 4, 300), (0, 1, 3), (3, 3, 297)), ((40, 3, 5), (1, 1, 1), (39, 2, 4)), ((6, 10), (1, 1), (5, 9))]
    for shape, lo, hi in shapes:
        nd = len(shape)
        for order in itertools.permutations(range(nd)):
            strides = _perm_strides(shape, order)
            for keep in keep_sets(nd):
                p = _plan(shape, lo, hi, keep, es=es, strides=strides)
                size = math.prod(shape)
                count = np.zeros(size, dtype=np.int64)
                owner = np.full(size, -1, dtype=np.int64)
                for sl, o, off in _visits(p, size):
                    assert 0 <= sl < p["slices"] and 0 <= o < p["outputs"]
                    count[off] += 1
                    owner[off] = o
                # the box, and the output every element belongs to: the kept indices through partial_strides
                want_count = np.zeros(shape, dtype=np.int64)
                want_owner = np.full(shape, -1, dtype=np.int64)
                box = tuple(slice(a, b) for a, b in zip(lo, hi))
                want_count[box] = 1
                idx = np.meshgrid(*(np.arange(b - a) for a, b in zip(lo, hi)), indexing="ij")
                want_owner[box] = sum(idx[d] * ps for d, ps in zip(keep, p["partial_strides"]))
                flat = np.lib.stride_tricks.as_strided(count, shape, [st * 8 for st in strides])
                assert (flat == want_count).all(), (shape, order, keep, p)
                flat = np.lib.stride_tricks.as_strided(owner, shape, [st * 8 for st in strides])
                assert (flat == want_owner).all(), (shape, order, keep, p)


def test_plan_errors():
    for call in (lambda: _plan((4, 4), (0, 0), (5, 4), (0,)),          # box outside
                 lambda: _plan((4,), (0,), (4,), (0,)),                 # one dimension
                 lambda: _plan((4, 4), (0, 0), (4, 4), ()),             # nothing kept
                 lambda: _plan((4, 4), (0, 0), (4, 4), (0, 1)),         # everything kept
                 lambda: _plan((4, 4, 4), (0,) * 3, (4,) * 3, (2, 0)),  # not increasing
                 lambda: _plan((4, 4, 4), (0,) * 3, (4,) * 3, (3,)),    # no such axis
                 lambda: _plan((4, 4), (0, 0), (4, 4), (0,), es=2)):
        with pytest.raises(igg.IGGError):
            call()


# ------------------------------------------------------------------ placement
def _local(Fg, shape):
    idx = [igg.indices_g(d, torch.empty(shape, device="meta")) for d in range(len(shape))]
    return Fg[tuple(torch.meshgrid(*idx, indexing="ij"))].contiguous()


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 1, 1), (3, 2, 1), (2, 2, 2)])
@pytest.mark.parametrize("periods", [(0, 0, 0), (1, 1, 1), (1, 0, 1)])
@pytest.mark.parametrize("overlap", [2, 3, 4])
def test_placement_on_simulated_topologies(dims, periods, overlap):
    """Summed over all ranks, every global output cell receives the
    contributions of each global cell once; a rank's own part sits at its
    global indices (two segments where a periodic range wraps), zero elsewhere."""
    n = (9, 8, 10)
    igg.init_global_grid(*n, overlapx=overlap, overlapy=overlap, overlapz=overlap, **KW)
    for shape in (n, (n[0] + 1, n[1], n[2]), (n[0], n[1] - 1, n[2] + 1), n[:2]):
        nd = len(shape)
        _place(dims, [0, 0, 0], periods)
        gshape = igg.selection_shape_g(torch.empty(shape, device="meta"))
        Fg, _ = global_arrays(gshape)
        for keep in keep_sets(nd):
            red = tuple(d for d in range(nd) if d not in keep)
            total = torch.zeros([gshape[d] for d in keep], dtype=torch.float64)
            covered = torch.zeros_like(total)
            for coords in itertools.product(*(range(D) for D in dims)):
                _place(dims, coords, periods)
                A = _local(Fg, shape)
                loc = igg.project_g("sum", A, keep, local=True)
                assert loc.shape == total.shape and loc.dtype == torch.float64
                total += loc
                ones = igg.project_g("sum", torch.ones(shape, dtype=torch.float64), keep, local=True)
                covered += ones
                # the max-type identity outside of the rank's own cells
                mx = igg.project_g("max", A, keep, local=True)
                mn = igg.project_g("min", A, keep, local=True)
                assert ((ones > 0) | ((mx == -math.inf) & (mn == math.inf))).all()
                assert (torch.isfinite(mx) == (ones > 0)).all()
            assert same(total, Fg.sum(dim=red)), (shape, keep)
            assert same(covered, torch.full_like(covered, float(math.prod(gshape[d] for d in red))))
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------------------ CPU tensors
def _ints(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1024, 1025, shape, generator=g).to(dtype)


def _single_rank_global(A):
    """The global array of a single rank's field: owned cells at their global indices."""
    rng = igg.owned_ranges(A)
    gshape = igg.selection_shape_g(A)
    Gl = torch.zeros(gshape, dtype=torch.float64)
    idx = [igg.indices_g(d, A)[a:b] for d, (a, b) in enumerate(rng)]
    Gl[tuple(torch.meshgrid(*idx, indexing="ij"))] = igg.owned_view(A).double()
    return Gl


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.float16, torch.int32])
def test_every_op_on_cpu_tensors(dtype):
    igg.init_global_grid(9, 8, 7, periodx=1, periodz=1, overlapz=3, **KW)
    for shape in [(9, 8, 7), (10, 8, 7), (9, 7, 8), (9, 8)]:
        A, B = _ints(shape, dtype, 1), _ints(shape, dtype, 2)  # (f16 holds every integer up to 2048)
        Fg, Gg = _single_rank_global(A), _single_rank_global(B)
        for keep in keep_sets(len(shape)):
            red = tuple(d for d in range(len(shape)) if d not in keep)
            for op in ONE + TWO + ("mean",):
                r = igg.project_g(op, A, keep, other=B if op in TWO else None)
                assert r.dtype == torch.float64 and r.device.type == "cpu" and r.is_contiguous()
                assert tuple(r.shape) == tuple(igg.selection_shape_g(A)[d] for d in keep)
                assert same(r, expected(op, Fg, Gg, red)), (shape, keep, op)
            assert same(igg.project_g("sum", A, keep[0] if len(keep) == 1 else list(keep)),
                        expected("sum", Fg, Gg, red))  # an int, a list
    # permuted and sliced layouts
    A = _ints((7, 8, 9), torch.float64, 3).permute(2, 1, 0)
    assert same(igg.project_g("max", A, (0, 2)), expected("max", _single_rank_global(A), None, (1,)))
    igg.finalize_global_grid(finalize_MPI=False)


def test_out_local_and_mean_on_cpu():
    igg.init_global_grid(9, 8, 7, periody=1, **KW)
    A, B = _ints((9, 8, 7), torch.float64, 3), _ints((9, 8, 7), torch.float64, 4)
    Fg = _single_rank_global(A)
    out = torch.full((9, 7), -1.0, dtype=torch.float64)
    assert igg.project_g("sum", A, (0, 2), out=out) is out and same(out, Fg.sum(dim=1))
    assert igg.project_g("min", A, (0, 2), out=out) is out and same(out, Fg.amin(dim=1))
    assert igg.project_g("maxabs_diff", A, 1, other=B).shape == (6,)  # periodic y: 1*(8 - 2) cells
    assert same(igg.project_g("mean", A, 0), Fg.sum(dim=(1, 2)) / torch.full((9,), 42.0, dtype=torch.float64))
    assert same(igg.project_g("sum", A, 0, local=True), igg.project_g("sum", A, 0))  # one rank: local is global
    igg.finalize_global_grid(finalize_MPI=False)
    # a rank of a larger grid: its own cells at their global indices, the identity elsewhere
    igg.init_global_grid(9, 8, 7, periody=1, overlapy=4, **KW)
    _place([3, 2, 2], [1, 1, 0], [0, 1, 0])
    loc = igg.project_g("max", A, (0, 1), local=True)
    assert loc.shape == (3 * 7 + 2, 2 * 4)
    rng = igg.owned_ranges(A)
    gx = igg.indices_g(0, A)[rng[0][0]:rng[0][1]]
    gy = igg.indices_g(1, A)[rng[1][0]:rng[1][1]]
    want = torch.full(loc.shape, -math.inf, dtype=torch.float64)
    want[gx.view(-1, 1), gy.view(1, -1)] = igg.owned_view(A).amax(dim=2)
    assert gy[-1] < gy[0]  # this rank's y range wraps: two segments
    assert same(loc, want)
    igg.finalize_global_grid(finalize_MPI=False)


def test_nan_rule_on_cpu():
    igg.init_global_grid(9, 8, 7, periodx=1, periody=1, periodz=1, **KW)
    A, B = _ints((9, 8, 7), torch.float64, 6), _ints((9, 8, 7), torch.float64, 7)
    Fg, Gg = _single_rank_global(A), _single_rank_global(B)
    for X in (A, B):  # every plane nobody owns
        X[0], X[-1], X[:, 0], X[:, -1], X[:, :, 0], X[:, :, -1] = (math.nan,) * 6
    for keep in keep_sets(3):
        red = tuple(d for d in range(3) if d not in keep)
        for op in ONE + TWO + ("mean",):
            assert same(igg.project_g(op, A, keep, other=B if op in TWO else None), expected(op, Fg, Gg, red)), op
    keepv = A[1, 4, 5].clone()
    A[1, 4, 5] = math.nan  # an owned cell: global index (0, 3, 4)
    for keep in keep_sets(3):
        red = tuple(d for d in range(3) if d not in keep)
        for op in ONE + TWO + ("mean",):
            r = igg.project_g(op, A, keep, other=B if op in TWO else None)
            want = expected(op, Fg, Gg, red)
            hit = torch.zeros(want.shape, dtype=torch.bool)
            hit[tuple((0, 3, 4)[d] for d in keep)] = True
            assert (torch.isnan(r) == hit).all(), (keep, op)  # only the line or plane that holds it
            assert torch.equal(r[~hit], want[~hit]), (keep, op)
    A[1, 4, 5] = keepv
    A[2, 2, 2], B[2, 2, 2] = math.inf, math.inf  # inf alone is a value, inf - inf is a NaN term
    assert igg.project_g("max", A, 0)[1].item() == math.inf
    r = igg.project_g("maxabs_diff", A, 0, other=B)
    assert math.isnan(r[1].item()) and int(torch.isnan(r).sum()) == 1
    igg.finalize_global_grid(finalize_MPI=False)


def test_errors():
    A = torch.zeros(9, 8, 7, dtype=torch.float64)
    with pytest.raises(igg.IGGError, match="init_global_grid"):
        igg.project_g("sum", A, 0)
    igg.init_global_grid(9, 8, 7, **KW)
    with pytest.raises(igg.IGGError, match="reduce_g"):
        igg.project_g("sum", A, ())
    with pytest.raises(igg.IGGError, match="gather_g"):
        igg.project_g("sum", A, (0, 1, 2))
    with pytest.raises(igg.IGGError, match="gather_g"):
        igg.project_g("sum", torch.zeros(9), 0)
    with pytest.raises(igg.IGGError, match="strictly increasing"):
        igg.project_g("sum", A, (1, 0))
    with pytest.raises(igg.IGGError, match="strictly increasing"):
        igg.project_g("sum", A, (0, 0))
    with pytest.raises(igg.IGGError, match="strictly increasing"):
        igg.project_g("sum", A, 3)
    with pytest.raises(igg.IGGError, match="strictly increasing"):
        igg.project_g("sum", A, -1)
    with pytest.raises(igg.IGGError, match="axis or a tuple of axes"):
        igg.project_g("sum", A, "x")
    with pytest.raises(igg.IGGError, match="axis or a tuple of axes"):
        igg.project_g("sum", A, (0, True))
    with pytest.raises(igg.IGGError, match="op must be one of"):
        igg.project_g("median", A, 0)
    for call in (lambda: igg.project_g("dot", A, 0),                                   # no other
                 lambda: igg.project_g("dot", A, 0, other=torch.zeros(9, 8, 6)),       # other's shape
                 lambda: igg.project_g("dot", A, 0, other=A.float()),                  # other's dtype
                 lambda: igg.project_g("sum", A, 0, other=A),                          # other without a use
                 lambda: igg.project_g("mean", A, 0, other=A),
                 lambda: igg.project_g("sum", A, 0, out=torch.zeros(8, dtype=torch.float64)),   # out's shape
                 lambda: igg.project_g("sum", A, 0, out=torch.zeros(9)),               # out's dtype
                 lambda: igg.project_g("sum", A, (0, 1), out=torch.zeros(8, 9, dtype=torch.float64).t()),
                 lambda: igg.project_g("sum", A, 0, out=torch.zeros(9, dtype=torch.float64, device="meta")),
                 lambda: igg.project_g("sum", torch.zeros(2, 2, 2, 2), 0),             # four dimensions
                 lambda: igg.project_g("mean", A, 0, local=True)):
        with pytest.raises(igg.IGGError):
            call()
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------------------ multi-rank
@pytest.mark.parametrize("nprocs,args", [
    (2, (2, 1, 1, 0, 2, 1)),
    (4, (2, 2, 1, 3, 3, 1)),   # periodic x and y, overlap 3
    (8, (2, 2, 2, 4, 2, 1)),   # periodic z; the 2-D field on dimz = 2 is counted once
])
def test_multi_rank_gloo(nprocs, args):
    check_rank_outputs(run_project_ranks(nprocs, "cpu", "float64", *args))
