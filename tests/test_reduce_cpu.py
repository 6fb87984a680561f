"""Global reductions on the host (ops/reduce.py): ownership (table, partition,
no received plane), the host-side plan of the reduction kernels, every op on
CPU tensors, multi-rank gloo runs and the convergence-controlled time loop.

Oracle: the same reduction of ``A.double()`` over ``owned_ranges(A)`` in
numpy. Sum-type ops are compared bitwise on integer-valued data (every product
and partial sum is exact in f64 whatever the order); for random real data the
bound is ``n * 2**-53 * sum|term|`` for the accumulation plus ``2**-53 *
sum|term|`` for f64 products, which round once, against ``math.fsum``.
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
from igg.ops import reduce as R
from igg.parallel import grid as G
from igg.parallel import halo as H
from tests._mp import MAX_TIMEOUT, ROOT, free_port

KW = dict(quiet=True, init_MPI=False, device_type="none")
ONE = ("sum", "sumsq", "max", "min", "maxabs")
TWO = ("dot", "sumsq_diff", "maxabs_diff")
U53 = 2.0 ** -53


def run_reduce_ranks(nprocs: int, *args, timeout: float = 150.0, env_extra=None) -> list:
    """``tests/mp_worker_reduce.py reduce ...`` on ``nprocs`` local ranks; the
    first rank that fails stops the others, a timeout fails the test with
    every rank's output."""
    port = free_port()
    procs, logs = [], []
    for r in range(nprocs):
        env = dict(os.environ)
        env.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(r),
                    "WORLD_SIZE": str(nprocs), "LOCAL_RANK": str(r), "LOCAL_WORLD_SIZE": str(nprocs),
                    "OMP_NUM_THREADS": "1", "IGG_HOST_THREADS": "2",
                    "PYTHONPATH": ROOT + os.pathsep + env.get("PYTHONPATH", "")})
        env.update(env_extra or {})
        log = tempfile.TemporaryFile(mode="w+")
        logs.append(log)
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tests", "mp_worker_reduce.py"), "reduce", *map(str, args)],
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
        raise AssertionError(f"reduce scenario {args} failed or timed out:\n{msg}")
    return outs


def check_rank_outputs(outs) -> None:
    """Every rank passed and printed the same result bits."""
    bits = []
    for r, o in enumerate(outs):
        m = re.search(rf"rank {r} reduce OK BITS=(\S+)", o)
        assert m, o[-1500:]
        bits.append(m.group(1))
    assert len(set(bits)) == 1, "the ranks received different bits"


def _place(dims, coords, periods=None):
    """Pretend to be rank ``coords`` of a ``dims`` grid (the grid's arrays are
    mutable, as in the reference's tests)."""
    gg = G.global_grid()
    gg.dims[:] = dims
    gg.coords[:] = coords
    if periods is not None:
        gg.periods[:] = periods
    gg.nxyz_g[:] = gg.dims * (gg.nxyz - gg.overlaps) + gg.overlaps * (gg.periods == 0)
    return gg


# ------------------------------------------------------------------ ownership
# (grid overlap, field size m with n = 12) -> the interior rank's owned range,
# worked out by hand from o = overlap + m - n, lo = o // 2, [lo, m - (o - lo))
N = 12
INTERIOR = {
    (2, 11): (0, 10), (2, 12): (1, 11), (2, 13): (1, 11),
    (3, 11): (1, 10), (3, 12): (1, 10), (3, 13): (2, 11),
    (4, 11): (1, 9), (4, 12): (2, 10), (4, 13): (2, 10),
}


@pytest.mark.parametrize("overlap", [2, 3, 4])
@pytest.mark.parametrize("m", [N - 1, N, N + 1])
def test_owned_ranges_table(overlap, m):
    w = 2 if overlap == 4 else 1  # a halo width of 2 needs an overlap of 4
    igg.init_global_grid(N, N, N, overlapx=overlap, overlapy=overlap, overlapz=overlap, halowidthx=w, halowidthy=w,
                         halowidthz=w, **KW)
    lo, hi = INTERIOR[(overlap, m)]
    for d in range(3):
        shape = [N, N, N]
        shape[d] = m
        A = torch.zeros(shape)
        other = (overlap // 2, N - (overlap - overlap // 2))
        for D, c, per, want in [
            (3, 1, 0, (lo, hi)),      # interior
            (3, 0, 0, (0, hi)),       # first: the lower bound goes to 0
            (3, 2, 0, (lo, m)),       # last: the upper bound goes to m
            (3, 0, 1, (lo, hi)),      # periodic: every rank like an interior one
            (3, 2, 1, (lo, hi)),
            (1, 0, 0, (0, m)),        # a single non-periodic rank owns everything
            (1, 0, 1, (lo, hi)),      # a single periodic rank does not own its halo
        ]:
            dims, coords, periods = [3, 3, 3], [1, 1, 1], [0, 0, 0]
            dims[d], coords[d], periods[d] = D, c, per
            _place(dims, coords, periods)
            got = igg.owned_ranges(A)
            assert got[d] == want, (overlap, m, d, D, c, per, got)
            assert all(got[e] == other for e in range(3) if e != d)
            assert igg.owned_view(A).shape[d] == want[1] - want[0]
    # 1-D and 2-D fields: the dimensions a field does not have are skipped
    _place([3, 3, 3], [1, 0, 2], [0, 0, 0])
    assert igg.owned_ranges(torch.zeros(m)) == ((lo, hi),)
    A2 = torch.zeros(m, N)
    assert igg.owned_ranges(A2) == ((lo, hi), (0, N - (overlap - overlap // 2)))
    assert igg.owned_view(A2).shape == (hi - lo, N - (overlap - overlap // 2))
    igg.finalize_global_grid(finalize_MPI=False)


def test_ownership_ignores_loopback_table():
    """Ownership does not read the neighbour table (what enable_loopback edits)."""
    igg.init_global_grid(8, 8, 8, **KW)
    A = torch.zeros(8, 8, 8)
    before = igg.owned_ranges(A)
    G.global_grid().neighbors[:] = 0
    assert igg.owned_ranges(A) == before == ((0, 8),) * 3
    igg.finalize_global_grid(finalize_MPI=False)


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 1, 1), (3, 2, 1), (2, 2, 2)])
@pytest.mark.parametrize("periods", [(0, 0, 0), (1, 1, 1), (1, 0, 1)])
@pytest.mark.parametrize("overlap", [2, 3, 4])
def test_partition_brute_force(dims, periods, overlap):
    n = (9, 8, 10)
    igg.init_global_grid(*n, overlapx=overlap, overlapy=overlap, overlapz=overlap, **KW)
    for shape in (n, (n[0] + 1, n[1], n[2]), (n[0], n[1] - 1, n[2] + 1), (n[0] - 1, n[1], n[2])):
        A = torch.zeros(shape)
        step = [n[d] - overlap for d in range(3)]
        ol = [overlap + shape[d] - n[d] for d in range(3)]
        ng = [dims[d] * step[d] + (0 if periods[d] else ol[d]) for d in range(3)]
        count = np.zeros(ng, dtype=np.int64)
        for coords in itertools.product(*(range(D) for D in dims)):
            _place(dims, coords, periods)
            rng = igg.owned_ranges(A)
            idx = []
            for d in range(3):
                a, b = rng[d]
                assert 0 <= a < b <= shape[d]
                g = coords[d] * step[d] + np.arange(a, b)
                idx.append(g % ng[d] if periods[d] else g)
                # rank c ends where rank c + 1 begins
                if coords[d] + 1 < dims[d] or periods[d]:
                    assert coords[d] * step[d] + b == (coords[d] + 1) * step[d] + ol[d] // 2
            count[np.ix_(*idx)] += 1
        assert (count == 1).all(), (shape, int(count.min()), int(count.max()))
        _place(dims, [0, 0, 0], periods)
        assert R.global_cells(A) == count.size
    igg.finalize_global_grid(finalize_MPI=False)


@pytest.mark.parametrize("overlap,w", [(2, 1), (3, 1), (4, 2), (4, 1), (5, 2)])
def test_no_owned_plane_is_received(overlap, w):
    n = (12, 11, 13)
    igg.init_global_grid(*n, overlapx=overlap, overlapy=overlap, overlapz=overlap, halowidthx=w, halowidthy=w,
                         halowidthz=w, **KW)
    for shape in (n, (n[0] + 1, n[1], n[2]), (n[0], n[1] + 1, n[2] + 1)):
        A = torch.zeros(shape)
        for D, c, per in [(3, 0, 0), (3, 1, 0), (3, 2, 0), (3, 0, 1), (1, 0, 1), (2, 1, 1)]:
            _place([D] * 3, [c] * 3, [per] * 3)
            rng = igg.owned_ranges(A)
            for d in range(3):
                assert G.ol(d + 1, A) >= 2 * w
                owned = set(range(*rng[d]))
                for side in (1, 2):
                    behind = per or (c > 0 if side == 1 else c < D - 1)  # a rank sends into this side
                    if behind:
                        recv = {i - 1 for i in H.recvranges(side, d + 1, A)[d]}
                        assert not (recv & owned), (shape, D, c, per, d, side)
    igg.finalize_global_grid(finalize_MPI=False)


# ----------------------------------------------------------------------- plan
BASE = 1 << 20


def _plan(shape, lo, hi, es=8, strides=None, base=BASE, **kw):
    if strides is None:
        strides = [int(np.prod(shape[d + 1:])) for d in range(len(shape))]
    return native.reduce_plan(list(shape), list(strides), list(lo), list(hi), es, base, **kw)


def test_plan_merges_contiguous_extents():
    p = _plan((8, 9, 10), (0, 0, 0), (8, 9, 10))
    assert p["path"] == "flat" and p["box"] == (1, 1, 720) and p["head"] == 0 and p["vec"] == 2
    p = _plan((16, 16, 16), (1, 0, 0), (15, 16, 16))  # whole planes: one run
    assert p["path"] == "flat" and p["box"] == (1, 1, 14 * 256) and p["offset"] == 256
    p = _plan((16, 16, 16), (1, 1, 0), (15, 15, 16))  # whole rows: rows of 14 * 16
    assert p["path"] == "rows" and p["box"] == (1, 14, 224) and p["strides"][1:] == (256, 1)
    p = _plan((16, 16, 16), (1, 1, 1), (15, 15, 15))  # nothing merges
    assert p["path"] == "rows" and p["box"] == (14, 14, 14) and p["strides"] == (256, 16, 1)
    assert p["offset"] == 273 and p["head"] == 1 and p["loads_per_row"] == 8 and p["lanes_per_row"] == 8
    p = _plan((16, 16), (2, 0), (3, 16))  # an extent of one drops out
    assert p["path"] == "flat" and p["box"] == (1, 1, 16)
    p = _plan((5,), (2,), (3,))  # a single element
    assert p["path"] == "flat" and p["total"] == 1 and p["blocks"] == 1
    p = _plan((5, 4), (2, 1), (2, 3))  # an empty box
    assert p["total"] == 0 and p["blocks"] == 0
    # with a second input both must be contiguous for a merge
    p = _plan((8, 8), (0, 0), (8, 8), strides_b=[8, 1], base_b=BASE)
    assert p["path"] == "flat"
    p = _plan((8, 8), (0, 0), (8, 8), strides_b=[16, 1], base_b=BASE)
    assert p["path"] == "rows" and p["box"] == (1, 8, 8)


def test_plan_every_path():
    assert _plan((6, 7, 9), (1, 1, 1), (5, 6, 8), es=4, strides=(64 * 8, 64, 1))["path"] == "rows"
    assert _plan((100,), (3,), (97,), es=4)["path"] == "flat"
    assert _plan((100,), (0,), (100,), es=8, base=BASE + 8)["head"] == 1  # flat: any element-aligned base
    for kw in (dict(strides=(1, 6, 42)),                     # permuted, stride0 == 1
               dict(strides=(63, 7, 1), es=4),               # a row pitch of 7 f32
               dict(strides=(64, 8, 1), es=4, base=BASE + 4),  # a base one element off
               dict(strides=(128, 16, 2))):                  # a strided innermost dimension
        p = _plan((6, 7, 5), (1, 1, 1), (5, 6, 4), **kw)
        assert p["path"] == "element" and p["vec"] == 1 and p["head"] == 0, kw
    # two inputs whose head masks differ cannot share vector loads
    p = _plan((64,), (1,), (63,), strides_b=[1], base_b=BASE + 8)
    assert p["path"] == "element"


@pytest.mark.parametrize("es", [4, 8])
def test_plan_rows_need_aligned_base_and_pitch(es):
    vec = 16 // es
    for pitch in range(8, 8 + 2 * vec + 1):
        for off in range(0, 2 * vec + 1):
            p = _plan((4, 5, 6), (0, 1, 1), (4, 4, 5), es=es, strides=(5 * pitch + es * 16, pitch, 1),
                      base=BASE + off * es)
            aligned = (off * es) % 16 == 0 and (pitch * es) % 16 == 0 and ((5 * pitch + es * 16) * es) % 16 == 0
            assert (p["path"] == "rows") == aligned, (pitch, off, p)
            if not aligned:
                assert p["path"] == "element" and p["vec"] == 1


def test_plan_blocks_depend_on_the_box_only():
    cap, unroll = native.REDUCE_MAX_BLOCKS, native.REDUCE_UNROLL
    for shape, lo, hi in [((70, 33, 9), (1, 1, 1), (69, 32, 8)), ((192, 192, 64), (0, 0, 0), (192, 192, 64)),
                          ((512, 512, 512), (1, 1, 1), (511, 511, 511)), ((1 << 22,), (0,), (1 << 22,))]:
        plans = [_plan(shape, lo, hi, es=4, base=b) for b in (BASE, 7 * BASE, 1 << 40)]
        assert all(p == plans[0] for p in plans)
        p = plans[0]
        assert p["blocks"] == min(-(-p["tiles"] // unroll), cap) and 1 <= p["blocks"] <= cap
    assert _plan((512, 512, 512), (1, 1, 1), (511, 511, 511))["blocks"] == cap
    assert _plan((1 << 22,), (0,), (1 << 22,), es=4)["blocks"] == cap


def test_plan_errors():
    with pytest.raises(igg.IGGError):
        _plan((4, 4), (0, 0), (5, 4))
    with pytest.raises(igg.IGGError):
        _plan((4, 4, 4, 4), (0,) * 4, (4,) * 4)
    with pytest.raises(igg.IGGError):
        _plan((4, 4), (0, 0), (4, 4), es=2)


# ------------------------------------------------------------------ CPU tensors
def _oracle(op, A, B=None):
    rng = igg.owned_ranges(A)
    sl = tuple(slice(a, b) for a, b in rng)
    x = A.double().numpy()[sl]
    y = B.double().numpy()[sl] if B is not None else None
    return {"sum": lambda: x.sum(), "sumsq": lambda: (x * x).sum(), "max": lambda: x.max(), "min": lambda: x.min(),
            "maxabs": lambda: np.abs(x).max(), "dot": lambda: (x * y).sum(),
            "sumsq_diff": lambda: ((x - y) * (x - y)).sum(), "maxabs_diff": lambda: np.abs(x - y).max()}[op]()


def _same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _ints(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1024, 1025, shape, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.float16, torch.int32])
def test_every_op_on_cpu_tensors(dtype):
    igg.init_global_grid(9, 8, 7, periodx=1, periodz=1, overlapz=3, **KW)
    _place([2, 2, 1], [1, 0, 0])
    for shape in [(9, 8, 7), (10, 8, 7), (9, 7, 8), (9, 8), (9,)]:
        A, B = _ints(shape, dtype, 1), _ints(shape, dtype, 2)  # (f16 holds every integer up to 2048)
        for op in ONE + TWO:
            r = igg.reduce_g(op, A, other=B if op in TWO else None)
            assert r.dtype == torch.float64 and r.dim() == 0 and r.device.type == "cpu"
            assert _same_bits(r.item(), _oracle(op, A, B)), (shape, op)
        assert _same_bits(igg.sum_g(A).item(), _oracle("sum", A))
        assert _same_bits(igg.max_g(A).item(), _oracle("max", A))
        assert _same_bits(igg.min_g(A).item(), _oracle("min", A))
        assert _same_bits(igg.maxabs_g(A).item(), _oracle("maxabs", A))
        assert _same_bits(igg.dot_g(A, B).item(), _oracle("dot", A, B))
        assert _same_bits(igg.maxabs_diff_g(A, B).item(), _oracle("maxabs_diff", A, B))
        assert _same_bits(igg.norm_g(A).item(), np.sqrt(_oracle("sumsq", A)))
        assert _same_bits(igg.norm_diff_g(A, B).item(), np.sqrt(_oracle("sumsq_diff", A, B)))
    igg.finalize_global_grid(finalize_MPI=False)


def test_batch_out_and_mean_on_cpu():
    igg.init_global_grid(9, 8, 7, periody=1, **KW)
    _place([3, 2, 2], [1, 1, 0])
    A, B, C = _ints((9, 8, 7), torch.float64, 3), _ints((10, 8, 7), torch.float64, 4), _ints((9, 8), torch.float64, 5)
    r = igg.reduce_g("sumsq", A, B, C)
    assert r.shape == (3,) and r.dtype == torch.float64
    for k, X in enumerate((A, B, C)):
        assert _same_bits(r[k].item(), _oracle("sumsq", X))
    r = igg.reduce_g("maxabs_diff", A, B, other=(A + 1, B - 3))
    assert r.tolist() == [1.0, 3.0]
    out = torch.full((3,), -1.0, dtype=torch.float64)
    assert igg.reduce_g("sum", A, B, C, out=out) is out
    assert [_same_bits(out[k].item(), _oracle("sum", X)) for k, X in enumerate((A, B, C))] == [True] * 3
    out0 = torch.zeros((), dtype=torch.float64)
    assert igg.max_g(A, out=out0) is out0 and out0.item() == _oracle("max", A)
    assert igg.norm_g(A, out=out0) is out0 and _same_bits(out0.item(), np.sqrt(_oracle("sumsq", A)))
    # the mean divides by the global cell count of the partition: per dimension D*(n - o) + ol, D*(n - o) periodic
    for X, cells in ((A, (3 * 7 + 2) * (2 * 6) * (2 * 5 + 2)), (B, (3 * 7 + 3) * (2 * 6) * (2 * 5 + 2)),
                     (C, (3 * 7 + 2) * (2 * 6))):
        assert R.global_cells(X) == cells
        assert _same_bits(igg.mean_g(X).item(), _oracle("sum", X) / cells)
    igg.finalize_global_grid(finalize_MPI=False)


def test_nan_rule_on_cpu():
    igg.init_global_grid(9, 8, 7, periodx=1, periody=1, periodz=1, **KW)
    A, B = _ints((9, 8, 7), torch.float64, 6), _ints((9, 8, 7), torch.float64, 7)
    want = {op: _oracle(op, A, B) for op in ONE + TWO}
    for X in (A, B):  # every plane nobody owns
        X[0], X[-1], X[:, 0], X[:, -1], X[:, :, 0], X[:, :, -1] = (math.nan,) * 6
    for op in ONE + TWO:
        assert _same_bits(igg.reduce_g(op, A, other=B if op in TWO else None).item(), want[op]), op
    A[1, 1, 1] = math.nan  # an owned corner
    for op in ONE + TWO:
        assert math.isnan(igg.reduce_g(op, A, other=B if op in TWO else None).item()), op
    assert math.isnan(igg.mean_g(A).item()) and math.isnan(igg.norm_g(A).item())
    A[1, 1, 1] = math.inf  # inf - inf and inf * 0 are NaN terms, inf alone is not
    B[1, 1, 1] = math.inf
    assert igg.max_g(A).item() == math.inf and math.isnan(igg.maxabs_diff_g(A, B).item())
    igg.finalize_global_grid(finalize_MPI=False)


def test_random_data_within_the_derived_bound():
    igg.init_global_grid(17, 16, 15, periodx=1, **KW)
    g = torch.Generator().manual_seed(8)
    for dtype in (torch.float64, torch.float32):
        A = (torch.randn(17, 16, 15, generator=g, dtype=torch.float64) * 100).to(dtype)
        B = torch.randn(17, 16, 15, generator=g, dtype=torch.float64).to(dtype)
        x, y = igg.owned_view(A).double().flatten().tolist(), igg.owned_view(B).double().flatten().tolist()
        n = len(x)
        terms = {"sum": x, "sumsq": [a * a for a in x], "dot": [a * b for a, b in zip(x, y)],
                 "sumsq_diff": [(a - b) * (a - b) for a, b in zip(x, y)]}
        for op, t in terms.items():
            got = igg.reduce_g(op, A, other=B if op in TWO else None).item()
            mag = math.fsum(abs(v) for v in t)
            bound = n * U53 * mag + (U53 * mag if op != "sum" else 0.0)
            assert abs(got - math.fsum(t)) <= bound, (dtype, op, got, math.fsum(t), bound)
    igg.finalize_global_grid(finalize_MPI=False)


def test_errors():
    A = torch.zeros(9, 8, 7, dtype=torch.float64)
    with pytest.raises(igg.IGGError, match="init_global_grid"):
        igg.sum_g(A)
    with pytest.raises(igg.IGGError, match="init_global_grid"):
        igg.owned_ranges(A)
    igg.init_global_grid(9, 8, 7, **KW)
    for call in (lambda: igg.reduce_g("mean", A),                                  # unknown op
                 lambda: igg.reduce_g("sum"),                                      # no field
                 lambda: igg.reduce_g("sum", A, A.float()),                        # mixed dtypes
                 lambda: igg.reduce_g("sum", A, torch.zeros(9, 8, 7, device="meta")),  # mixed devices
                 lambda: igg.reduce_g("dot", A),                                   # no other
                 lambda: igg.reduce_g("dot", A, other=torch.zeros(9, 8, 6)),       # other's shape
                 lambda: igg.reduce_g("dot", A, other=A.float()),                  # other's dtype
                 lambda: igg.reduce_g("dot", A, A, other=(A,)),                    # other's length
                 lambda: igg.reduce_g("sum", A, other=A),                          # other without a use
                 lambda: igg.reduce_g("sum", A, out=torch.zeros(1, dtype=torch.float64)),   # out's shape
                 lambda: igg.reduce_g("sum", A, out=torch.zeros(())),              # out's dtype
                 lambda: igg.reduce_g("sum", A, A, out=torch.zeros(3, dtype=torch.float64)),
                 lambda: igg.reduce_g("sum", A, out=torch.zeros((), dtype=torch.float64, device="meta")),
                 lambda: igg.sum_g(torch.zeros(2, 2, 2, 2)),                       # four dimensions
                 lambda: igg.mean_g(A, local=True)):
        with pytest.raises(igg.IGGError):
            call()
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------------------ multi-rank
@pytest.mark.parametrize("nprocs,args", [
    (2, (2, 1, 1, 0, 2, 1)),
    (4, (2, 2, 1, 0, 2, 1)),
    (8, (2, 2, 2, 0, 2, 1)),
    (3, (3, 1, 1, 1, 3, 1)),   # periodic x, overlap 3
    (4, (2, 2, 1, 0, 4, 2)),   # overlap 4, halo width 2
])
def test_multi_rank_gloo(nprocs, args):
    check_rank_outputs(run_reduce_ranks(nprocs, "cpu", "float64", *args))


# ------------------------------------------------------------------ run_until
class _Stub:
    """A model whose residual halves every step."""

    def __new__(cls, graph_steps=None):
        from igg.models._pingpong import PingPongModel

        class Stub(PingPongModel):
            def __init__(self):
                super().__init__()
                self.calls, self.steps, self.reads = [], 0, 0
                if graph_steps:
                    self.graph, self.graph_steps = object(), graph_steps

            def run(self, nt):
                self.calls.append(("run", nt))
                self.steps += nt

            def step(self):
                self.calls.append(("step",))
                self.steps += 1

            def _residual(self):
                self.reads += 1
                return torch.tensor(2.0 ** -self.steps, dtype=torch.float64)

        return Stub()


def test_run_until_blocks_on_a_stub():
    from igg.models._pingpong import GRAPH_STEPS

    m = _Stub()
    steps, res = m.run_until(2.0 ** -20.5, 1000)  # default block: GRAPH_STEPS + 1 without a graph
    k = GRAPH_STEPS + 1
    assert steps == 2 * k and steps >= 21 and res == 2.0 ** -steps and m.reads == 2
    assert m.calls == [("run", k - 1), ("step",)] * 2
    m = _Stub(graph_steps=6)
    steps, res = m.run_until(0.0, 17)  # never below 0: all of max_steps, the last block shortened
    assert steps == 17 == m.steps and m.reads == 3
    assert m.calls == [("run", 6), ("step",), ("run", 6), ("step",), ("run", 2), ("step",)]
    m = _Stub()
    assert m.run_until(1.0, 5, check_every=1) == (1, 0.5) and m.calls == [("run", 0), ("step",)]
    m = _Stub()
    assert m.run_until(2.0 ** -7, 100, check_every=3) == (9, 2.0 ** -9)  # the first check below tol stops it
    m = _Stub()
    assert m.run_until(0.5, 0) == (0, math.inf) and m.calls == []
    with pytest.raises(ValueError):
        m.run_until(0.5, 10, check_every=0)


def test_run_until_needs_a_steady_state():
    from igg.models.acoustic2d import Acoustic2D

    igg.init_global_grid(16, 16, 1, **KW)
    m = Acoustic2D(dtype=torch.float64, device="cpu")
    p0 = m.P.clone()
    with pytest.raises(NotImplementedError):
        m.run_until(1e-3, 10)
    assert torch.equal(m.P, p0)  # refused before any step ran
    igg.finalize_global_grid(finalize_MPI=False)


def test_run_until_on_cpu_diffusion():
    from igg.models.diffusion3d import Diffusion3D

    igg.init_global_grid(16, 16, 16, **KW)
    a, b, c = (Diffusion3D(dtype=torch.float64, device="cpu") for _ in range(3))
    a.run(23)
    assert b.run_until(0.0, 23) == (23, b.residual().item())
    assert torch.equal(a.T, b.T)
    # the residual is the change over the last single step
    want = (b.T - b.T2).abs().max().item()
    assert b.residual().item() == want and b.residual().dtype == torch.float64
    r1 = (c.run_until(0.0, 1))[1]
    steps, res = c.run_until(r1 / 4, 5000, check_every=7)
    assert steps < 5000 and steps % 7 == 0 and res < r1 / 4
    igg.finalize_global_grid(finalize_MPI=False)
