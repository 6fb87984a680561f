"""spread_g on the host (parallel/spread_g.py): the targets by brute force, the
exact transpose of sample_g, an independent oracle (tests/mp_worker_spread_g.py:
a Python loop over the points into a dict cell -> list, folded in order), the
fixed order of the additions, the rules, several gloo ranks, Source, the
arguments, igg.autograd.sample_g and the example. Every comparison is of bits
unless a bound is stated.
"""
import itertools
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest
import torch

import igg
from igg.parallel.gather_g import _extent, _global_index
from tests._mp import MAX_TIMEOUT, ROOT, free_port
from tests.mp_worker_sample_g import extents, global_values, local_of_global
from tests.mp_worker_spread_g import bits_of, dyadic_points, fold, oracle_global, oracle_owner

KW = dict(quiet=True, init_MPI=False, device_type="none")
F64 = torch.float64


def run_spread_ranks(nprocs: int, scenario: str, *args, timeout: float = 150.0, env_extra=None) -> list:
    """``tests/mp_worker_spread_g.py <scenario> ...`` on ``nprocs`` local
    ranks; the first rank that fails stops the others, a timeout fails the
    test with every rank's output."""
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
            [sys.executable, os.path.join(ROOT, "tests", "mp_worker_spread_g.py"), scenario, *map(str, args)],
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
        raise AssertionError(f"spread_g scenario {scenario} {args} failed or timed out:\n{msg}")
    for r, o in enumerate(outs):
        assert f"rank {r} spread_g OK" in o, o[-1500:]
    return outs


# ------------------------------------------------------------------ the targets
def _targets_by_brute_force(nxyz, overlaps, dims, periods, shape):
    E = tuple(_extent(nxyz[d], overlaps[d], dims[d], periods[d], shape[d]) for d in range(3))
    for c in itertools.product(*[range(D) for D in dims]):
        gidx = [[_global_index(nxyz[d], overlaps[d], dims[d], periods[d], c[d], shape[d], i) for i in range(shape[d])]
                for d in range(3)]
        holders = {}
        for i in itertools.product(*[range(m) for m in shape]):
            holders.setdefault(tuple(gidx[d][i[d]] for d in range(3)), []).append(i)
        for g in itertools.product(*[range(e) for e in E]):
            got = igg.spread_targets(nxyz, overlaps, dims, periods, c, shape, g, "all")
            assert len(set(got)) == len(got) and sorted(got) == sorted(holders.get(g, [])), (c, g, got)
            own = igg.spread_targets(nxyz, overlaps, dims, periods, c, shape, g, "owner")
            cell = all(g[d] < (E[d] if periods[d] else E[d] - 1) for d in range(3))  # g is a cell's lower corner
            if cell:
                lo = igg.sample_owner(nxyz, overlaps, dims, periods, c, shape, g)
                assert own == ([] if lo is None else [lo])
                assert lo is None or lo in got


@pytest.mark.parametrize("dims", [(2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 1, 2)])
@pytest.mark.parametrize("periods", [(0, 0, 0), (1, 0, 1), (1, 1, 1)])
def test_targets_are_exactly_the_local_cells_with_that_global_index(dims, periods):
    nxyz = (6, 5, 7)
    for o, stag in ((2, (0, 0, 0)), (2, (1, 0, -1)), (3, (-1, 1, 0)), (3, (1, 1, 1)), (4, (0, 0, 0)), (4, (0, -1, 1))):
        shape = tuple(nxyz[d] + stag[d] for d in range(3))
        _targets_by_brute_force(nxyz, (o, o, o), dims, periods, shape)


def test_targets_of_a_local_range_longer_than_the_period_and_of_fewer_dimensions():
    # n = 9, o = 4, D = 1, periodic: the period is 5 and the local range holds it in three runs
    nxyz, ov, dims, per = (9, 5, 6), (4, 2, 2), (1, 1, 1), (1, 0, 0)
    _targets_by_brute_force(nxyz, ov, dims, per, nxyz)
    got = igg.spread_targets(nxyz, ov, dims, per, (0, 0, 0), nxyz, (1, 2, 3), "all")
    assert sorted(got) == [(2, 2, 3), (7, 2, 3)]
    assert sorted(igg.spread_targets(nxyz, ov, dims, per, (0, 0, 0), (9,), (4,), "all")) == [(0,), (5,)]
    assert igg.spread_targets(nxyz, ov, dims, per, (0, 0, 0), (9,), (3,), "all") == [(4,)]
    # a 2-D field: the copies at every z coordinate receive, one of them owns
    nxyz, ov, dims, per = (6, 5, 7), (2, 2, 2), (2, 1, 2), (0, 0, 0)
    for cz in (0, 1):
        assert igg.spread_targets(nxyz, ov, dims, per, (0, 0, cz), (6, 5), (1, 1), "all") == [(1, 1)]
    assert igg.spread_targets(nxyz, ov, dims, per, (0, 0, 1), (6, 5), (1, 1), "owner") == []
    assert igg.spread_targets(nxyz, ov, dims, per, (0, 0, 0), (6, 5), (1, 1), "owner") == [(1, 1)]
    with pytest.raises(igg.IGGError, match="overlap"):
        igg.spread_targets(nxyz, ov, dims, per, (0, 0, 0), (4, 5, 7), (1, 1, 1), "owner")
    with pytest.raises(igg.IGGError, match="copies"):
        igg.spread_targets(nxyz, ov, dims, per, (0, 0, 0), (6, 5), (1, 1), "some")


# ------------------------------------------------------------------ one rank
def _init(n, periods=(0, 0, 0), overlap=2):
    n3 = tuple(n) + (1,) * (3 - len(n))
    igg.init_global_grid(*n3, periodx=periods[0], periody=periods[1], periodz=periods[2], overlapx=overlap,
                         overlapy=overlap, overlapz=overlap, **KW)


def _done():
    igg.finalize_global_grid(finalize_MPI=False)


def _layouts(A):
    """C order and other permuted dense layouts of ``A`` (same values)."""
    nd = A.dim()
    yield A
    for perm in list(itertools.permutations(range(nd)))[1:3]:
        inv = [perm.index(d) for d in range(nd)]
        B = A.permute(perm).contiguous().permute(inv)
        assert B.shape == A.shape and torch.equal(A, B)
        yield B


CASES = [((7,), (0, 0, 0)), ((7,), (1, 0, 0)), ((6, 5), (0, 1, 0)), ((5, 6, 4), (0, 0, 0)), ((5, 6, 4), (1, 0, 1))]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,periods", CASES)
def test_owner_is_the_exact_transpose_of_sample_g(n, periods, dtype):
    """The matrix of sample_g from unit fields; spread_g(copies="owner") of a
    unit V into zeros is its row of that point, exactly (dyadic points: every
    weight is a multiple of 4^-nd)."""
    _init(n, periods)
    E = extents(igg.get_global_grid(), n)
    P = torch.cat([dyadic_points(E, periods, 40, 2), torch.tensor([[float(e - 1) for e in E]], dtype=F64)])
    ncell = int(np.prod(n))
    S = torch.empty(P.shape[0], ncell, dtype=F64)
    for j in range(ncell):
        U = torch.zeros(ncell, dtype=dtype)
        U[j] = 1.0
        S[:, j] = igg.sample_g(U.view(n), P)
    assert not torch.isnan(S).any() and (S.sum(dim=1) == 1.0).all()
    V = torch.from_numpy(np.random.default_rng(3).integers(-9, 10, size=P.shape[0]).astype(np.float64))
    for Z0 in _layouts(torch.zeros(n, dtype=dtype)):
        for p in range(P.shape[0]):
            Z = Z0.clone()
            unit = torch.zeros(P.shape[0], dtype=F64)
            unit[p] = 1.0
            igg.spread_g(Z, P, unit, copies="owner")
            assert Z.stride() == Z0.stride() and torch.equal(Z.double().reshape(-1), S[p]), (p, P[p])
        Z = Z0.clone()  # and all points at once: S^T V, exact on small integers
        igg.spread_g(Z, P, V, copies="owner")
        assert torch.equal(Z.double().reshape(-1), S.t() @ V)
    _done()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,periods", CASES)
def test_random_data_against_the_python_oracle_for_both_copies(n, periods, dtype):
    _init(n, periods)
    gg = igg.get_global_grid()
    nd = len(n)
    E = extents(gg, n)
    rng = np.random.default_rng(11)
    lo = [-1.5 * E[d] if periods[d] else 0.0 for d in range(nd)]
    hi = [2.5 * E[d] if periods[d] else E[d] - 1.0 for d in range(nd)]
    P = torch.from_numpy(rng.uniform(lo, hi, size=(150, nd)))
    P = torch.cat([P, P[:50], dyadic_points(E, periods, 30, 4)])  # shared cells, zero factors
    V = torch.from_numpy(rng.standard_normal(P.shape[0]) * 10.0 ** rng.integers(-4, 5, size=P.shape[0]))
    G = torch.from_numpy(rng.standard_normal(E)).to(dtype)
    want_all = local_of_global(oracle_global(G, P, V, periods[:nd]), n)
    A0 = local_of_global(G, n)
    want_own = oracle_owner(A0, P, V, gg)
    assert not torch.equal(bits_of(want_all), bits_of(A0)) and not torch.equal(bits_of(want_own), bits_of(A0))
    for A in _layouts(A0):
        B = A.clone()
        igg.spread_g(B, P, V)
        assert torch.equal(bits_of(B), bits_of(want_all))
        B = A.clone()
        igg.spread_g(B, P.t().contiguous().t(), V, copies="owner")
        assert torch.equal(bits_of(B), bits_of(want_own))
    # a tuple of fields with a (nfields, npts) V, strided
    V2 = torch.stack([V, -2.0 * V, V], dim=1).t()[:2]
    assert not V2.is_contiguous()
    fs = (A0.clone(), A0.clone())
    igg.spread_g(fs, P, V2)
    assert torch.equal(bits_of(fs[0]), bits_of(want_all))
    assert torch.equal(bits_of(fs[1]), bits_of(local_of_global(oracle_global(G, P, -2.0 * V, periods[:nd]), n)))
    _done()


def test_the_order_of_the_additions_is_the_points_order():
    """1000 points in one cell with values 1e16, 1, -1e16, ...: another order
    of the additions gives other bits."""
    _init((6, 5))
    rng = np.random.default_rng(8)
    P = torch.tensor([[2.0, 3.0]], dtype=F64).repeat(1000, 1)
    V = torch.tensor([1e16, 1.0, -1e16, 3.0] * 250, dtype=F64) * torch.from_numpy(rng.integers(1, 4, size=1000) * 1.0)
    want = fold([float(v) for v in V])
    assert want != fold(sorted(float(v) for v in V)) and want != float(V.sum())
    runs = []
    for _ in range(2):
        A = torch.zeros(6, 5, dtype=F64)
        igg.spread_g(A, P, V)
        runs.append(A)
    assert torch.equal(bits_of(runs[0]), bits_of(runs[1]))
    assert runs[0][2, 3].item() == want and int((runs[0] != 0).sum()) == 1
    plan = igg.spread_plan(A, P)
    assert (plan.ncells, plan.nentries) == (1, 1000) and plan.cells.tolist() == [2 * 5 + 3]
    assert plan.start.tolist() == [0, 1000] and plan.point.tolist() == list(range(1000))
    assert (plan.weight == 1.0).all()
    # shuffled points and values: the oracle's bits for the shuffled order; fractional points too
    P = torch.tensor([[2.25, 3.5]], dtype=F64).repeat(1000, 1)
    P[::3] = torch.tensor([2.75, 3.0], dtype=F64)
    perm = torch.from_numpy(rng.permutation(1000))
    G = torch.zeros(6, 5, dtype=F64)
    seen = set()
    for Pk, Vk in ((P, V), (P[perm], V[perm])):
        A = G.clone()
        igg.spread_g(A, Pk, Vk)
        assert torch.equal(bits_of(A), bits_of(oracle_global(G, Pk, Vk, (0, 0))))
        seen.add(tuple(bits_of(A).reshape(-1).tolist()))
    assert len(seen) == 2
    _done()


def test_rules_zero_weights_edges_wrap_invalid_points_nan_and_untouched_cells():
    _init((7, 6), (1, 0, 0))
    E = extents(igg.get_global_grid(), (7, 6))  # (5, 6): periodic in x
    assert E == (5, 6)
    nan = math.nan

    def spread(P, V, A=None, copies="all"):
        G = torch.zeros(E, dtype=F64) if A is None else A
        L = local_of_global(G, (7, 6))
        igg.spread_g(L, torch.tensor(P, dtype=F64), torch.tensor(V, dtype=F64), copies=copies)
        out = torch.empty(E, dtype=F64)
        igg.gather_g(L, out)
        L2 = L.clone()
        igg.update_halo_(L2)
        assert torch.equal(bits_of(L2), bits_of(L))
        return out, L

    # an integer point touches one cell - also when V is NaN and the other corners are sentinels
    S = torch.full(E, 7.5, dtype=F64)
    out, L = spread([[4.0, 3.0]], [nan], S.clone())
    assert math.isnan(out[4, 3].item()) and int(torch.isnan(out).sum()) == 1
    assert torch.equal(bits_of(out[~torch.isnan(out)]), bits_of(S[~torch.isnan(out)]))
    assert int(torch.isnan(L).sum()) == 2  # x is periodic on one rank: global x = 4 has two local copies
    # a zero factor in one dimension: two cells, not four
    out, _ = spread([[2.5, 3.0]], [nan], S.clone())
    assert sorted(torch.isnan(out).nonzero().tolist()) == [[2, 3], [3, 3]]
    # a NaN value with non-zero weights reaches exactly its four corners
    out, _ = spread([[2.5, 3.25]], [nan], S.clone())
    assert sorted(torch.isnan(out).nonzero().tolist()) == [[2, 3], [2, 4], [3, 3], [3, 4]]
    # the non-periodic upper edge u = E - 1: the last cell alone; the periodic wrap: planes E-1 and 0
    out, _ = spread([[1.0, 5.0]], [2.0])
    assert out[1, 5].item() == 2.0 and int((out != 0).sum()) == 1
    out, _ = spread([[4.5, 1.0], [-0.25, 2.0], [5.0, 0.0], [1004.75, 3.0]], [2.0, 4.0, 1.0, 8.0])
    assert (out[4, 1].item(), out[0, 1].item()) == (1.0, 1.0)
    assert (out[4, 2].item(), out[0, 2].item()) == (1.0, 3.0)
    assert out[0, 0].item() == 1.0 and (out[4, 3].item(), out[0, 3].item()) == (2.0, 6.0)
    assert int((out != 0).sum()) == 7
    # invalid and non-finite points add nothing, whatever their value
    bad = [[1.0, -0.001], [1.0, 5.001], [1.0, nan], [nan, 1.0], [math.inf, 1.0], [-math.inf, 1.0], [1.0, math.inf],
           [1.0, 1e300]]
    out, L = spread(bad, [nan, 1.0, 2.0, 3.0, math.inf, 4.0, 5.0, 6.0], S.clone())
    assert torch.equal(bits_of(out), bits_of(S))
    for copies in ("all", "owner"):
        Z = torch.full((7, 6), -0.0, dtype=F64)
        igg.spread_g(Z, torch.tensor(bad, dtype=F64), torch.ones(8, dtype=F64), copies=copies)
        assert (bits_of(Z) == bits_of(torch.tensor([-0.0], dtype=F64))).all()
    # cells no point reaches keep their bits: -0.0 stays -0.0 (an added +0.0 would have made it +0.0)
    G = torch.zeros(E, dtype=F64)
    G[1, 1] = G[3, 4] = G[0, 0] = -0.0
    out, _ = spread([[2.0, 2.0], [2.5, 2.5]], [0.0, 0.0], G.clone())
    minus0 = bits_of(torch.tensor([-0.0], dtype=F64)).item()
    assert [bits_of(out)[i, j].item() for i, j in ((1, 1), (3, 4), (0, 0))] == [minus0] * 3
    # npts == 0
    A = torch.full((7, 6), -0.0, dtype=F64)
    igg.spread_g(A, torch.empty(0, 2, dtype=F64), torch.empty(0, dtype=F64))
    igg.spread_g((A, A.clone()), torch.empty(0, 2, dtype=F64), torch.empty(2, 0, dtype=F64), copies="owner")
    assert (bits_of(A) == minus0).all()
    plan = igg.spread_plan(A, torch.empty(0, 2, dtype=F64))
    assert (plan.ncells, plan.nentries, plan.start.tolist()) == (0, 0, [0])
    plan.apply(torch.empty(0, dtype=F64), A)
    _done()


def test_three_runs_of_a_long_periodic_range_and_the_refusal_of_more():
    igg.init_global_grid(9, 5, 1, periodx=1, overlapx=4, **KW)
    A = torch.zeros(9, 5, dtype=F64)
    ix = igg.indices_g(0, A)
    assert ix.tolist() == [4, 0, 1, 2, 3, 4, 0, 1, 2]
    igg.spread_g(A, torch.tensor([[1.5, 2.0]], dtype=F64), torch.tensor([2.0], dtype=F64))
    assert A[:, 2].tolist() == [0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0]
    B = A.clone()
    igg.update_halo_(B)
    assert torch.equal(A, B)
    A = torch.zeros(24, 5, dtype=F64)  # a field of 24 planes over a period of 5: six runs
    with pytest.raises(igg.IGGError, match="runs"):
        igg.spread_g(A, torch.tensor([[1.5, 2.0]], dtype=F64), torch.tensor([2.0], dtype=F64))
    assert not A.any()
    _done()


# ------------------------------------------------------------------ Source, plan
def test_source_rows_against_repeated_spread_g_and_reset():
    _init((6, 5, 4), (0, 1, 0))
    E = extents(igg.get_global_grid(), (6, 5, 4))
    rng = np.random.default_rng(21)
    P = dyadic_points(E, (0, 1, 0), 30, 6) + 0.125
    P = P[torch.from_numpy((P.numpy()[:, [0, 2]] <= np.array(E)[[0, 2]] - 1).all(axis=1))]
    npts = P.shape[0]
    W = torch.from_numpy(rng.standard_normal((4, 2, npts)))
    A, B = torch.from_numpy(rng.standard_normal((2, 6, 5, 4)))
    B = B.permute(2, 0, 1).contiguous().permute(1, 2, 0)
    for copies in ("all", "owner"):
        src = igg.Source((A, B), P, W, copies=copies)
        f, g = (A.clone(), B.clone()), (A.clone(), B.clone())
        for row in range(4):
            src.inject(*f)
            igg.spread_g(g, P, W[row], copies=copies)
            assert all(torch.equal(bits_of(x), bits_of(y)) for x, y in zip(f, g)), (copies, row)
        kept = [x.clone() for x in f]
        src.inject(*f)  # the rows are used up: nothing is added
        src.inject(*f)
        assert all(torch.equal(bits_of(x), bits_of(y)) for x, y in zip(f, kept))
        src.reset()
        W[0] *= 2.0  # W is used as passed
        src.inject(*f)
        igg.spread_g(g, P, W[0], copies=copies)
        assert all(torch.equal(bits_of(x), bits_of(y)) for x, y in zip(f, g))
        W[0] /= 2.0
    # one field with a (nrows, npts) table; plan.apply equals spread_g
    one = igg.Source(A, P, W[:, 0])
    f, g = A.clone(), A.clone()
    one.inject(f)
    igg.spread_g(g, P, W[0, 0])
    assert torch.equal(bits_of(f), bits_of(g))
    plan = igg.spread_plan(A, P, copies="owner")
    f, g = (A.float(), B.float()), (A.float(), B.float())
    plan.apply(W[1], *f)  # a plan serves fields of any strides and of either dtype
    igg.spread_g(g, P, W[1], copies="owner")
    assert all(torch.equal(bits_of(x), bits_of(y)) for x, y in zip(f, g))
    assert plan.cells.dtype == plan.start.dtype == plan.point.dtype == torch.int64 and plan.weight.dtype == F64
    assert plan.start.numel() == plan.ncells + 1 and int(plan.start[-1]) == plan.nentries == plan.point.numel()
    assert (plan.cells[1:] > plan.cells[:-1]).all()
    for i in range(plan.ncells):
        seg = plan.point[int(plan.start[i]):int(plan.start[i + 1])]
        assert seg.numel() >= 1 and (seg[1:] > seg[:-1]).all()
    for bad in (lambda: igg.Source(A, P, W), lambda: igg.Source((A, B), P, W[:, 0]), lambda: igg.Source(A, P, W.float()),
                lambda: igg.Source(A, P, W[:, 0, :-1]), lambda: igg.Source(A, P, W[:, 0], copies="none"),
                lambda: one.inject(A, B), lambda: one.inject(A.float()), lambda: plan.apply(W[1], A[:5]),
                lambda: plan.apply(W[1, 0], A, B), lambda: plan.apply(W[1].float(), A, B)):
        with pytest.raises(igg.IGGError):
            bad()
    _done()


# --------------------------------------------------------------- the arguments
def test_every_refused_call_leaves_the_fields_untouched():
    _init((6, 5, 4))
    A = global_values((6, 5, 4), 8)
    B = A + 1.0
    P = torch.tensor([[0.5, 1.25, 2.0], [5.0, 4.0, 3.0], [9.0, 0.0, 0.0]], dtype=F64)
    V = torch.tensor([1.0, 2.0, 3.0], dtype=F64)
    before = (A.clone(), B.clone())
    for bad in (lambda: igg.spread_g(A, P.float(), V),
                lambda: igg.spread_g(A, P[:, :2], V),
                lambda: igg.spread_g(A, P[:, 0], V),
                lambda: igg.spread_g(A, P.tolist(), V),
                lambda: igg.spread_g(A, P, V.float()),
                lambda: igg.spread_g(A, P, V[:2]),
                lambda: igg.spread_g(A, P, V.tolist()),
                lambda: igg.spread_g(A, P, torch.stack([V, V])),
                lambda: igg.spread_g((A, B), P, V),
                lambda: igg.spread_g((A, B), P, torch.stack([V, V, V])),
                lambda: igg.spread_g((A, B.float()), P, torch.stack([V, V])),
                lambda: igg.spread_g((A, B[:5]), P, torch.stack([V, V])),
                lambda: igg.spread_g((), P, V),
                lambda: igg.spread_g(A.long(), P, V),
                lambda: igg.spread_g(A.half(), P, V),
                lambda: igg.spread_g(A[None], P, V),
                lambda: igg.spread_g(A, P, V, copies="both"),
                lambda: igg.spread_g(A, P, V, copies=1),
                lambda: igg.spread_plan(A, P.float()),
                lambda: igg.spread_plan(A, P, copies="x")):
        with pytest.raises(igg.IGGError):
            bad()
    assert torch.equal(bits_of(A), bits_of(before[0])) and torch.equal(bits_of(B), bits_of(before[1]))
    igg.spread_g((A,), P, V[None])  # a 1-tuple takes (1, npts)
    assert not torch.equal(A, before[0])
    _done()
    _init((6, 5, 4), (1, 0, 0))
    P = torch.zeros(1, 3, dtype=F64)
    Z = torch.zeros(4, 5, 4, dtype=F64)
    with pytest.raises(igg.IGGError, match="overlap"):  # periodic x, field overlap 2 + 4 - 6 = 0: sample_g's message
        igg.spread_g(Z, P, torch.ones(1, dtype=F64), copies="owner")
    with pytest.raises(igg.IGGError, match="overlap") as e1:
        igg.sample_g(Z, P)
    assert not Z.any() and "upper corner" in str(e1.value)
    with pytest.raises(igg.IGGError, match="extent"):  # E = 1 in y
        igg.spread_g(torch.zeros(6, 1, 4, dtype=F64), P, torch.ones(1, dtype=F64))
    _done()
    _init((6,))
    L = torch.zeros(6, dtype=F64)
    igg.spread_g(L, torch.tensor([0.0, 2.5, 5.0], dtype=F64), torch.tensor([1.0, 2.0, 4.0], dtype=F64))
    assert L.tolist() == [1.0, 0.0, 1.0, 1.0, 0.0, 4.0]
    _done()


# ----------------------------------------------------------------- gloo ranks
RANKS = [
    (2, (2, 1, 1), 0, 2, 3, 0, "float64"),
    (2, (2, 1, 1), 1, 3, 1, 1, "float32"),
    (4, (2, 2, 1), 3, 2, 2, 0, "float64"),
    (4, (2, 2, 1), 2, 3, 3, 1, "float32"),
    (6, (3, 1, 2), 5, 4, 3, 1, "float64"),
    (8, (2, 2, 2), 7, 2, 3, 0, "float64"),
    (8, (2, 2, 2), 0, 3, 3, -1, "float32"),
]


@pytest.mark.parametrize("nprocs,dims,periodic,overlap,nd,stagger,dtype", RANKS)
def test_gloo_ranks_all_copies_equal_the_oracle_on_the_global_array(nprocs, dims, periodic, overlap, nd, stagger, dtype):
    run_spread_ranks(nprocs, "all", "cpu", dtype, *dims, periodic, overlap, nd, stagger)


@pytest.mark.parametrize("nprocs,dims,periodic,overlap,nd,stagger,dtype", RANKS)
def test_gloo_ranks_owner_is_the_transpose_over_the_ranks(nprocs, dims, periodic, overlap, nd, stagger, dtype):
    run_spread_ranks(nprocs, "owner", "cpu", dtype, *dims, periodic, overlap, nd, stagger)


# -------------------------------------------------------------------- autograd
def test_autograd_sample_g_gradcheck_on_one_rank():
    _init((6, 5), (0, 1, 0))
    E = extents(igg.get_global_grid(), (6, 5))
    rng = np.random.default_rng(2)
    P = torch.from_numpy(rng.uniform([0.0, -4.0], [E[0] - 1.0, 9.0], size=(25, 2)))
    A = torch.from_numpy(rng.standard_normal((6, 5))).requires_grad_(True)
    B = torch.from_numpy(rng.standard_normal((5, 6))).t().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a: igg.autograd.sample_g(a, P), (A,))
    assert torch.autograd.gradcheck(lambda a, b: igg.autograd.sample_g((a, b), P), (A, B))
    out = igg.autograd.sample_g((A, B.detach()), P)
    assert torch.equal(bits_of(out), bits_of(igg.sample_g((A.detach(), B.detach()), P)))
    c = torch.from_numpy(rng.standard_normal((2, 25)))
    (out * c).sum().backward()
    want = torch.zeros(6, 5, dtype=F64)
    igg.spread_g(want, P, c[0].contiguous(), copies="owner")
    assert torch.equal(bits_of(A.grad), bits_of(want))
    Af = A.detach().float().requires_grad_(True)  # the gradient has the field's dtype
    igg.autograd.sample_g(Af, P).sum().backward()
    assert Af.grad.dtype == torch.float32 and Af.grad.shape == (6, 5)
    _done()


def test_autograd_sample_g_finite_differences_on_two_ranks_with_update_halo():
    run_spread_ranks(2, "autograd", "cpu", "float64", 2, 1, 1, 2, 2, 2)


# ---------------------------------------------------------------- the example
def _run_example(nprocs, nx, out, extra=()):
    port = free_port()
    procs = []
    for r in range(nprocs):
        e = dict(os.environ)
        e.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(r), "WORLD_SIZE": str(nprocs),
                  "LOCAL_RANK": str(r), "OMP_NUM_THREADS": "1", "IGG_HOST_THREADS": "2",
                  "PYTHONPATH": ROOT + os.pathsep + e.get("PYTHONPATH", "")})
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "examples", "acoustic_shot.py"), "--nx",
                                       str(nx), "--ny", "24", "--steps", "40", "--out", out, *extra], env=e,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT))
    outs = [p.communicate(timeout=MAX_TIMEOUT)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-2000:]
    assert "the field stayed halo-consistent" in outs[0], outs[0][-2000:]
    return torch.load(out)


def test_example_acoustic_shot_on_one_and_two_ranks(tmp_path):
    """The same global grid (46 x 24 cells) on one rank and on two: the
    seismograms are equal, bit for bit as in the acoustic multi-rank tests."""
    one = _run_example(1, 46, str(tmp_path / "one.pt"), ["--cpu"])
    two = _run_example(2, 24, str(tmp_path / "two.pt"), ["--cpu"])
    assert one.shape == two.shape == (40, 12) and float(one.abs().max()) > 0
    assert torch.equal(one, two)
