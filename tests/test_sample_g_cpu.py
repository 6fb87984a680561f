"""sample_g on the host (parallel/sample_g.py): ownership by brute force, the
interpolation rules on one rank, several gloo ranks against the oracle of
tests/mp_worker_sample_g.py (``host_sample`` on the directly built global
array), the arguments, and the example. Every comparison is of bits.
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
from igg._native import native
from igg.parallel.gather_g import _extent, _global_index
from tests._mp import MAX_TIMEOUT, ROOT, free_port
from tests.mp_worker_sample_g import NAN_BITS, bits, extents, global_values, local_of_global, oracle

KW = dict(quiet=True, init_MPI=False, device_type="none")


def run_sample_ranks(nprocs: int, scenario: str, *args, timeout: float = 150.0, env_extra=None) -> list:
    """``tests/mp_worker_sample_g.py <scenario> ...`` on ``nprocs`` local
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
            [sys.executable, os.path.join(ROOT, "tests", "mp_worker_sample_g.py"), scenario, *map(str, args)],
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
        raise AssertionError(f"sample_g scenario {scenario} {args} failed or timed out:\n{msg}")
    for r, o in enumerate(outs):
        assert f"rank {r} sample_g OK" in o, o[-1500:]
    return outs


# ---------------------------------------------------------------- ownership
@pytest.mark.parametrize("dims", [(2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 1, 2)])
@pytest.mark.parametrize("periods", [(0, 0, 0), (1, 0, 1), (1, 1, 1)])
def test_every_cell_has_one_owner_who_holds_its_upper_corners(dims, periods):
    nxyz = (6, 5, 7)
    for o, stag in itertools.product((2, 3, 4), itertools.product((-1, 0, 1), repeat=3)):
        overlaps = (o, o, o)
        shape = tuple(nxyz[d] + stag[d] for d in range(3))
        if stag not in ((0, 0, 0), (1, 0, -1), (-1, 1, 0), (0, -1, 1), (1, 1, 1), (-1, -1, -1)):
            continue
        E = tuple(_extent(nxyz[d], o, dims[d], periods[d], shape[d]) for d in range(3))
        ncells = [E[d] if periods[d] else E[d] - 1 for d in range(3)]  # lower corners of cells
        ranks = list(itertools.product(*[range(D) for D in dims]))
        owners = np.zeros(ncells, dtype=np.int64)
        for c in ranks:
            for g in itertools.product(*[range(k) for k in ncells]):
                i = igg.sample_owner(nxyz, overlaps, dims, periods, c, shape, g)
                if i is None:
                    continue
                owners[g] += 1
                for d in range(3):
                    assert 0 <= i[d] and i[d] + 1 < shape[d], (c, g, i)
                    par = (nxyz[d], o, dims[d], periods[d], c[d], shape[d])
                    assert _global_index(*par, i[d]) == g[d]
                    up = (g[d] + 1) % E[d] if periods[d] else g[d] + 1
                    assert _global_index(*par, i[d] + 1) == up, (c, g, i, d)
        assert (owners == 1).all(), (dims, periods, o, stag, np.argwhere(owners != 1)[:4].tolist())


def test_owner_of_a_field_with_fewer_dimensions_and_the_overlap_refusal():
    nxyz, ov, dims, per = (6, 5, 7), (2, 2, 2), (2, 1, 2), (0, 0, 0)
    assert igg.sample_owner(nxyz, ov, dims, per, (0, 0, 0), (6, 5), (1, 1)) == (1, 1)
    assert igg.sample_owner(nxyz, ov, dims, per, (0, 0, 1), (6, 5), (1, 1)) is None  # a copy at z coordinate 1
    assert igg.sample_owner(nxyz, ov, dims, per, (1, 0, 0), (6, 5), (1, 1)) is None
    with pytest.raises(igg.IGGError, match="overlap"):  # field overlap 0 with a neighbour
        igg.sample_owner(nxyz, ov, dims, per, (0, 0, 0), (4, 5, 7), (1, 1, 1))
    with pytest.raises(igg.IGGError, match="overlap"):  # ... or with a period
        igg.sample_owner(nxyz, ov, (1, 1, 1), (0, 1, 0), (0, 0, 0), (6, 3, 7), (1, 1, 1))
    # overlap 0 without neighbour or period is fine
    assert igg.sample_owner(nxyz, ov, (1, 1, 1), per, (0, 0, 0), (4, 5, 7), (2, 3, 5)) == (2, 3, 5)


# ------------------------------------------------------------------ one rank
def _init(n, periods=(0, 0, 0), overlap=2):
    n3 = tuple(n) + (1,) * (3 - len(n))
    igg.init_global_grid(*n3, periodx=periods[0], periody=periods[1], periodz=periods[2], overlapx=overlap,
                         overlapy=overlap, overlapz=overlap, **KW)


def _done():
    igg.finalize_global_grid(finalize_MPI=False)


def _layouts(A):
    """C order and every other permuted dense layout of ``A`` (same values)."""
    nd = A.dim()
    yield A
    for perm in list(itertools.permutations(range(nd)))[1:3]:
        inv = [perm.index(d) for d in range(nd)]
        B = A.permute(perm).contiguous().permute(inv)
        assert B.shape == A.shape and torch.equal(A, B)
        yield B


def _gathered(A):
    G = torch.empty(igg.selection_shape_g(A), dtype=A.dtype)
    igg.gather_g(A, G)
    return G


def _lattice(E):
    return torch.from_numpy(np.indices(E).reshape(len(E), -1).T.astype(np.float64)).contiguous()


CASES = [((7,), (0, 0, 0)), ((7,), (1, 0, 0)), ((6, 5), (0, 1, 0)), ((5, 6, 4), (0, 0, 0)), ((5, 6, 4), (1, 0, 1))]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,periods", CASES)
def test_integer_points_return_the_global_cells_also_among_nans(n, periods, dtype):
    _init(n, periods)
    gg = igg.get_global_grid()
    E = extents(gg, n)
    A0 = local_of_global(global_values(E, 4, dtype), n)
    P = _lattice(E)
    for A in _layouts(A0):
        G = _gathered(A)
        got = igg.sample_g(A, P)
        assert got.dtype == torch.float64 and got.shape == (P.shape[0],)
        assert torch.equal(bits(got), bits(G.double().reshape(-1)))
        # every other cell NaN: a corner of weight zero never reaches the result
        par = torch.from_numpy(np.indices(E).sum(axis=0) % 2 == 1)
        Gn = torch.where(par, torch.full_like(G, math.nan), G)
        An = local_of_global(Gn, n)
        keep = ~par.reshape(-1)
        gotn = igg.sample_g(An, P)
        assert torch.equal(bits(gotn[keep]), bits(G.double().reshape(-1)[keep]))
        assert (bits(gotn[~keep]) == NAN_BITS).all()
    _done()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,periods", CASES)
def test_multilinear_field_at_dyadic_fractions_is_exact(n, periods, dtype):
    """f = 3 + 2i - 5j + 7k + ij - 2jk + 3ik + ijk with integer coefficients is
    reproduced exactly by multilinear interpolation at multiples of 1/8 inside
    one cell (all terms are small dyadic numbers: nothing rounds). A periodic
    dimension is sampled away from the wrap, where f jumps."""
    _init(n, periods)
    nd = len(n)
    E = extents(igg.get_global_grid(), n)

    def f(x):
        i, j, k = [x[d] if d < nd else 0 * x[0] for d in range(3)]
        return 3 + 2 * i - 5 * j + 7 * k + i * j - 2 * j * k + 3 * i * k + i * j * k

    idx = torch.from_numpy(np.indices(E).astype(np.float64))
    A0 = local_of_global(f(idx).to(dtype), n)
    rng = np.random.default_rng(5)
    P = torch.from_numpy(rng.integers(0, 8 * (np.array(E) - 1) + 1, size=(200, nd)) / 8.0)
    P = torch.cat([P, torch.tensor([[float(e - 1) for e in E]], dtype=torch.float64)])  # the upper edge u = E-1
    want = f(P.t())
    for A in _layouts(A0):
        got = igg.sample_g(A, P)
        assert torch.equal(bits(got), bits(want)), (got - want).abs().max()
    _done()


def test_periodic_wrap_invalid_points_and_negative_zero():
    _init((7, 6), (1, 0, 0))
    gg = igg.get_global_grid()
    E = extents(gg, (7, 6))  # (5, 6): periodic in x
    G = global_values(E, 6)
    G[2, 3] = -0.0
    G[4, 1] = math.inf
    A = local_of_global(G, (7, 6))
    base = torch.tensor([[0.25, 1.5], [4.75, 2.0], [3.0, 0.0], [4.5, 5.0], [0.0, 4.25]], dtype=torch.float64)
    want = igg.sample_g(A, base)
    assert not torch.isnan(want).any()
    for shift in (-3, -1, 1, 2, 1000):  # dyadic coordinates: the wrap is exact
        moved = base + torch.tensor([shift * float(E[0]), 0.0], dtype=torch.float64)
        assert torch.equal(bits(igg.sample_g(A, moved)), bits(want)), shift
    # the wrap cell: between the last and the first plane
    got = igg.sample_g(A, torch.tensor([[4.5, 2.0], [-0.5, 2.0]], dtype=torch.float64))
    assert got[0].item() == got[1].item() == 0.5 * G[4, 2].item() + 0.5 * G[0, 2].item()
    # -0.0 and inf come back as they are
    got = igg.sample_g(A, torch.tensor([[2.0, 3.0], [4.0, 1.0], [7.0, 3.0]], dtype=torch.float64))
    assert bits(got).tolist() == bits(torch.tensor([-0.0, math.inf, -0.0], dtype=torch.float64)).tolist()
    # invalid: out of the non-periodic domain, non-finite anywhere
    bad = torch.tensor([[1.0, -0.001], [1.0, 5.001], [1.0, math.nan], [math.nan, 1.0], [math.inf, 1.0],
                        [-math.inf, 1.0], [1.0, math.inf], [1.0, -math.inf], [1.0, 1e300]], dtype=torch.float64)
    assert (bits(igg.sample_g(A, bad)) == NAN_BITS).all()
    assert not torch.isnan(igg.sample_g(A, torch.tensor([[1e300, 5.0], [-1e17, 0.0]], dtype=torch.float64))).any()
    _done()


def test_half_and_bfloat16_fields_take_the_float64_arithmetic():
    _init((6, 5))
    G = global_values((6, 5), 7)
    P = torch.tensor([[0.5, 0.25], [4.75, 3.5], [5.0, 4.0]], dtype=torch.float64)
    for dt in (torch.float16, torch.bfloat16):
        A = G.to(dt)
        assert torch.equal(bits(igg.sample_g(A, P)), bits(igg.sample_g(A.double(), P)))
    _done()


# --------------------------------------------------------------- the arguments
def test_arguments_out_empty_point_sets_and_tuples():
    _init((6, 5, 4))
    A = global_values((6, 5, 4), 8)
    B, C = A + 1.0, (A * 2.0).to(torch.float64)
    P = torch.tensor([[0.5, 1.25, 2.0], [5.0, 4.0, 3.0], [9.0, 0.0, 0.0]], dtype=torch.float64)
    three = igg.sample_g((A, B, C), P)
    assert three.shape == (3, 3)
    for k, F in enumerate((A, B, C)):
        assert torch.equal(bits(three[k]), bits(igg.sample_g(F, P)))
    assert igg.sample_g((A,), P).shape == (1, 3)
    # (nd, npts) transposed is accepted
    Pt = P.t().contiguous()
    assert torch.equal(bits(igg.sample_g(A, Pt.t())), bits(three[0]))
    # out=
    out = torch.zeros(3, 3, dtype=torch.float64)
    assert igg.sample_g((A, B, C), P, out=out) is out and torch.equal(bits(out), bits(three))
    # npts == 0
    assert igg.sample_g(A, torch.empty(0, 3, dtype=torch.float64)).shape == (0,)
    assert igg.sample_g((A, B), torch.empty(0, 3, dtype=torch.float64)).shape == (2, 0)
    before = A.clone()
    for bad in (lambda: igg.sample_g(A, P.float()),
                lambda: igg.sample_g(A, P[:, :2]),
                lambda: igg.sample_g(A, P[:, 0]),
                lambda: igg.sample_g(A, P.tolist()),
                lambda: igg.sample_g((A, B.float()), P),
                lambda: igg.sample_g((A, B[:5]), P),
                lambda: igg.sample_g((), P),
                lambda: igg.sample_g(A.long(), P),
                lambda: igg.sample_g(A[None], P),
                lambda: igg.sample_g(A, P, out=torch.zeros(3, dtype=torch.float32)),
                lambda: igg.sample_g(A, P, out=torch.zeros(4, dtype=torch.float64)),
                lambda: igg.sample_g((A, B), P, out=torch.zeros(3, 2, dtype=torch.float64).t()),
                lambda: igg.Recorder(A, P, 0),
                lambda: igg.Recorder(A, P.float(), 3)):
        with pytest.raises(igg.IGGError):
            bad()
    rec = igg.Recorder(A, P, 2)
    with pytest.raises(igg.IGGError):
        rec.record(A, B)
    with pytest.raises(igg.IGGError):
        rec.record(A.float())
    assert torch.equal(A, before)
    # a 1-D field takes (npts,) points
    _done()
    _init((6,))
    L = global_values((6,), 9)
    u = torch.tensor([0.0, 2.5, 5.0], dtype=torch.float64)
    assert torch.equal(bits(igg.sample_g(L, u)), bits(igg.sample_g(L, u.view(-1, 1))))
    assert igg.sample_g(L, u)[1].item() == 0.5 * L[2].item() + 0.5 * L[3].item()
    _done()


def test_refusals_of_the_grid():
    _init((6, 5, 4), (1, 0, 0))
    P = torch.zeros(1, 3, dtype=torch.float64)
    with pytest.raises(igg.IGGError, match="overlap"):  # periodic x, field overlap 2 + 4 - 6 = 0
        igg.sample_g(torch.zeros(4, 5, 4, dtype=torch.float64), P)
    with pytest.raises(igg.IGGError, match="extent"):   # E = 1 in y
        igg.sample_g(torch.zeros(6, 1, 4, dtype=torch.float64), P)
    _done()


@pytest.mark.parametrize("periods", [(0, 0, 0), (1, 1, 1)])
def test_index_g_against_coords_g_and_indices_g(periods):
    """For the coordinate of a cell index_g is that cell's global index:
    exactly, with dyadic spacings, for every staggering."""
    _init((8, 7, 6), periods)
    for d, spacing in itertools.product(range(3), (0.5, 0.125, 2.0)):
        for stag in (-1, 0, 1):
            shape = [8, 7, 6]
            shape[d] += stag
            A = torch.zeros(shape)
            x = igg.coords_g(d, spacing, A)
            u = igg.index_g(d, x, spacing, A)
            assert torch.equal(u, igg.indices_g(d, A).double()), (periods, d, spacing, stag, u)
            assert igg.index_g(d, float(x[2]), spacing, A) == float(igg.indices_g(d, A)[2])
    _done()


# ----------------------------------------------------------------- gloo ranks
@pytest.mark.parametrize("nprocs,dims,periodic,overlap,nd,stagger,dtype", [
    (2, (2, 1, 1), 0, 2, 3, 0, "float64"),
    (2, (2, 1, 1), 1, 3, 1, 1, "float32"),
    (4, (2, 2, 1), 3, 2, 2, 0, "float64"),
    (4, (2, 2, 1), 2, 3, 3, 1, "float32"),
    (6, (3, 1, 2), 5, 4, 3, 1, "float64"),
    (8, (2, 2, 2), 7, 2, 3, 0, "float64"),
    (8, (2, 2, 2), 0, 3, 3, -1, "float32"),
])
def test_gloo_ranks_equal_the_oracle_on_the_global_array(nprocs, dims, periodic, overlap, nd, stagger, dtype):
    run_sample_ranks(nprocs, "sample", "cpu", dtype, *dims, periodic, overlap, nd, stagger)


def test_gloo_ranks_after_update_halo():
    run_sample_ranks(4, "sample", "cpu", "float64", 2, 2, 1, 1, 2, 3, 0, 1)


# ---------------------------------------------------------------- the example
@pytest.mark.parametrize("nprocs", [1, 2])
def test_example_acoustic_receivers_cpu(nprocs):
    port = free_port()
    procs = []
    for r in range(nprocs):
        e = dict(os.environ)
        e.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(r), "WORLD_SIZE": str(nprocs),
                  "LOCAL_RANK": str(r), "OMP_NUM_THREADS": "1", "IGG_HOST_THREADS": "2",
                  "PYTHONPATH": ROOT + os.pathsep + e.get("PYTHONPATH", "")})
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "examples", "acoustic_receivers.py"),
                                       "--cpu"], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                                      cwd=ROOT))
    outs = [p.communicate(timeout=MAX_TIMEOUT)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-2000:]
    assert "the node receivers equal gather_g's cells bit for bit" in outs[0], outs[0][-2000:]


def test_host_sample_descriptor_rules():
    """The table straight to native.host_sample: a rank that owns nothing of a
    point writes 0 bits, an invalid point is NaN only with the me0 flag, a
    segment outside of the field is refused."""
    A = global_values((5, 6), 10)
    P = torch.tensor([[0.5, 0.5], [3.5, 4.0], [8.0, 0.0], [2.0, math.nan]], dtype=torch.float64)

    def run(table, me0):
        out = torch.full((4,), 3.0, dtype=torch.float64)
        native.host_sample(table, [(A.data_ptr(), list(A.stride()))], 8, P.data_ptr(), 2, 1, 4, out.data_ptr(), 4, me0)
        return bits(out).tolist()

    full = oracle([A], P, (0, 0))[0]
    left = [(9, 0, 5, [[0, 3, 0]]), (6, 0, 6, [[0, 6, 0]])]  # a rank holding x cells 0..2 of a 9-cell extent
    assert run(left, True) == [bits(full)[0].item(), 0, 0, NAN_BITS]
    assert run(left, False) == [bits(full)[0].item(), 0, 0, 0]
    with pytest.raises(igg.IGGError, match="segment"):
        run([(9, 0, 5, [[0, 6, 0]]), (6, 0, 6, [[0, 6, 0]])], True)
    with pytest.raises(igg.IGGError, match="extent"):
        run([(1, 0, 5, []), (6, 0, 6, [[0, 6, 0]])], True)
