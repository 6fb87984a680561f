"""accumulate_halo_ on the host (parallel/accumulate.py): the transpose of
update_halo_.

One rank: the matrix H of ``update_halo_`` is built column by column from unit
vectors and ``accumulate_halo_(y)`` must be ``Hᵀ y``. Several gloo ranks
(tests/mp_worker_accumulate.py): every rank emulates the definition in plain
numpy on all ranks' inputs and compares its block, and
``Σ<Hx,y> == Σ<x,Hᵀy>`` over all ranks. Every comparison is exact: the values
are integers of magnitude at most 1024, in f64 and f32.
"""
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
from tests._mp import MAX_TIMEOUT, ROOT, free_port
from tests.mp_worker_accumulate import Topology, emulate_accumulate, emulate_exchange, rank_input

KW = dict(quiet=True, init_MPI=False, device_type="none")


def run_accumulate_ranks(nprocs: int, scenario: str, *args, timeout: float = 150.0, env_extra=None) -> list:
    """``tests/mp_worker_accumulate.py <scenario> ...`` on ``nprocs`` local
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
            [sys.executable, os.path.join(ROOT, "tests", "mp_worker_accumulate.py"), scenario, *map(str, args)],
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
        raise AssertionError(f"accumulate scenario {scenario} {args} failed or timed out:\n{msg}")
    for r, o in enumerate(outs):
        assert f"rank {r} accumulate OK" in o, o[-1500:]
    return outs


# ------------------------------------------------------------ one rank: H^T
def _init(n, periods=(1, 1, 1), overlap=2, width=1):
    n3 = tuple(n) + (1,) * (3 - len(n))
    igg.init_global_grid(*n3, periodx=periods[0], periody=periods[1], periodz=periods[2], overlapx=overlap,
                         overlapy=overlap, overlapz=overlap, halowidthx=width, halowidthy=width, halowidthz=width,
                         **KW)


def _matrix(shape, dtype):
    """H of update_halo_ on one field of `shape`, column by column."""
    size = int(np.prod(shape))
    H = torch.zeros(size, size, dtype=torch.float64)
    for j in range(size):
        e = torch.zeros(size, dtype=dtype)
        e[j] = 1
        e = e.view(shape)
        igg.update_halo_(e)
        H[:, j] = e.reshape(-1).double()
    return H


def _values(shape, dtype, seed):
    return torch.from_numpy(rank_input(seed, 0, tuple(shape), np.float64)).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,periods,overlap,width,shape", [
    ((7, 6, 5), (1, 1, 1), 2, 1, None),
    ((9, 8, 9), (1, 1, 1), 4, 2, None),
    ((3, 4, 5), (1, 1, 1), 2, 1, None),     # n = 2*o - 1 in x: the two send slabs are the same plane
    ((6, 7), (1, 1, 0), 2, 1, None),
    ((8,), (1, 0, 0), 2, 1, None),
    ((7, 6, 5), (1, 1, 1), 2, 1, (8, 6, 5)),  # a field of size nx + 1
    ((7, 6, 5), (1, 0, 1), 2, 1, None),     # mixed periods
    ((7, 6, 5), (1, 0, 1), 3, 1, (7, 7, 5)),
])
def test_dense_transpose_on_one_rank(n, periods, overlap, width, shape, dtype):
    _init(n, periods, overlap, width)
    shape = tuple(shape or n)
    H = _matrix(shape, dtype)
    assert (H.sum(1) == 1).all() and ((H == 0) | (H == 1)).all()  # a selection: every cell has one source
    assert not torch.equal(H, torch.eye(H.shape[0], dtype=H.dtype))
    y = _values(shape, dtype, 1)
    got = y.clone()
    igg.accumulate_halo_(got)
    want = (H.t() @ y.reshape(-1).double()).view(shape)
    assert torch.equal(got.double(), want), (got.double() - want).abs().max()
    assert not torch.signbit(got[got == 0]).any()
    # and the emulation the multi-rank tests rely on says the same, both ways
    topo = Topology.of_grid()
    c0 = topo.ranks[0]
    assert np.array_equal(emulate_accumulate(topo, {c0: y.numpy()})[c0], got.numpy())
    hx = y.clone()
    igg.update_halo_(hx)
    assert np.array_equal(emulate_exchange(topo, {c0: y.numpy()})[c0], hx.numpy())
    igg.finalize_global_grid(finalize_MPI=False)


def test_two_fields_in_one_call_and_a_permuted_layout():
    _init((7, 6, 5))
    shapes = [(7, 6, 5), (8, 6, 5)]
    ys = [_values(s, torch.float64, 2 + k) for k, s in enumerate(shapes)]
    want = []
    for s, y in zip(shapes, ys):
        want.append((_matrix(s, torch.float64).t() @ y.reshape(-1)).view(s))
    got = [y.clone() for y in ys]
    igg.accumulate_halo_(*got)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    # the same field stored x-fastest
    p = ys[0].permute(2, 1, 0).contiguous().permute(2, 1, 0)
    assert p.stride() == (1, 7, 42)
    igg.accumulate_halo_(p)
    assert torch.equal(p, want[0])
    igg.finalize_global_grid(finalize_MPI=False)


def test_a_single_rank_without_periods_is_unchanged():
    _init((7, 6, 5), periods=(0, 0, 0))
    y = _values((7, 6, 5), torch.float64, 3)
    got = y.clone()
    igg.accumulate_halo_(got)
    assert torch.equal(got, y)
    igg.finalize_global_grid(finalize_MPI=False)


def test_conservation_on_one_periodic_rank():
    for n, o, w in (((7, 6, 5), 2, 1), ((9, 8, 9), 4, 2)):
        _init(n, overlap=o, width=w)
        y = _values(n, torch.float64, 4)
        total = float(y.sum())
        igg.accumulate_halo_(y)
        assert float(igg.sum_g(y)) == total
        # then the exchange gives every copy of a cell the total of its copies
        z = y.clone()
        igg.update_halo_(z)
        assert torch.equal(igg.owned_view(z), igg.owned_view(y))
        igg.finalize_global_grid(finalize_MPI=False)


@pytest.mark.parametrize("dtype", [torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8, torch.float16,
                                   torch.bfloat16, torch.complex64, torch.complex128])
def test_every_dtype_torch_adds(dtype):
    """The host path adds like torch: the halo of a periodic x dimension, by slices."""
    _init((7, 6, 5), periods=(1, 0, 0))
    g = torch.Generator().manual_seed(5)
    if dtype.is_complex:
        y = torch.complex(torch.randn(7, 6, 5, generator=g), torch.randn(7, 6, 5, generator=g)).to(dtype)
    elif dtype.is_floating_point:
        y = (torch.randn(7, 6, 5, generator=g) * 3).to(dtype)
        y[0, 0, 0], y[5, 0, 0] = 6e4, 6e4          # overflows half
        y[0, 0, 1], y[5, 0, 1] = 3e-7, 2e-7        # subnormal in half
        y[6, 0, 0], y[1, 0, 0] = float("inf"), 1.0
    else:
        info = torch.iinfo(dtype)
        y = torch.randint(info.min, info.max, (7, 6, 5), generator=g, dtype=torch.int64).to(dtype)  # sums wrap
    want = y.clone()
    want[1] = y[1] + y[6]   # the left neighbour's right halo into [ol - w, ol) = [1, 2)
    want[5] = y[5] + y[0]   # the right neighbour's left halo into [n - ol, n - ol + w) = [5, 6)
    want[0] = 0
    want[6] = 0
    got = y.clone()
    igg.accumulate_halo_(got)
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    igg.finalize_global_grid(finalize_MPI=False)


# ----------------------------------------------------------------- the errors
def _raises_and_leaves(match, *fields):
    before = [f.clone() if isinstance(f, torch.Tensor) else f for f in fields]
    with pytest.raises(igg.IGGError, match=match):
        igg.accumulate_halo_(*fields)
    for f, b in zip(fields, before):
        if isinstance(f, torch.Tensor):
            assert torch.equal(f, b)


def test_argument_errors_leave_the_fields_alone():
    _init((7, 6, 5))
    A = _values((7, 6, 5), torch.float64, 6)
    B = _values((7, 6, 5), torch.float64, 7)
    _raises_and_leaves("The field at position 2 has no halo", A, torch.ones(5, 4, 3, dtype=torch.float64))
    _raises_and_leaves("The fields at positions 1 and 3 have no halo", torch.ones(5, 4, 3, dtype=torch.float64), A,
                       torch.ones(5, 4, 3, dtype=torch.float64))
    _raises_and_leaves("position 2 is a duplicate of the one at the position 1", A, A)
    _raises_and_leaves("The pairs of fields with the positions .* are the same", A, A, A)
    _raises_and_leaves("position 2 is of different type than the first field", A, B.float())
    _raises_and_leaves("positions 2 and 3 are of different type", A, B.float(), B.float().clone())
    _raises_and_leaves("position 1 is not a dense array", torch.zeros(7, 6, 10, dtype=torch.float64)[:, :, ::2])
    _raises_and_leaves("bool fields have no addition", torch.ones(7, 6, 5, dtype=torch.bool))
    igg.finalize_global_grid(finalize_MPI=False)
    with pytest.raises(igg.IGGError):
        igg.accumulate_halo_(A)  # no grid
    # the width rule of update_halo_
    igg.init_global_grid(9, 8, 9, periodx=1, overlapx=4, overlapy=4, overlapz=4, halowidthx=2, halowidthy=2,
                         halowidthz=2, **KW)
    _raises_and_leaves(r"ol\(A,dim\)<2\*halowidths\[dim\]", torch.ones(8, 8, 9, dtype=torch.float64))
    igg.finalize_global_grid(finalize_MPI=False)


def test_gpu_only_dtype_error_names_the_types():
    """The dtype rule of GPU fields, on its message (no GPU needed: the meta
    device stands in for one in the check itself)."""
    from igg.parallel import accumulate as AC

    _init((7, 6, 5))

    class OnGpu:  # what check_accumulate reads of a field
        def __init__(self, t):
            self.t, self.dtype, self.is_cuda, self.shape = t, t.dtype, True, t.shape

        def dim(self):
            return self.t.dim()

    for dt in (torch.float16, torch.int32, torch.complex64):
        with pytest.raises(igg.IGGError, match=f"GPU fields must be float32 or float64 \\(got {dt}\\)"):
            AC.check_accumulate(OnGpu(torch.ones(7, 6, 5, dtype=dt)))
    assert AC.check_accumulate(OnGpu(torch.ones(7, 6, 5, dtype=torch.float32))) == "float32"
    igg.finalize_global_grid(finalize_MPI=False)


def test_a_send_slab_that_overlaps_a_halo_is_refused():
    """m < ol + w, which only a non-periodic grid admits: nx = 4 with overlap 4
    and a right neighbour in x (the topology is set by hand, as in
    tests/test_tools.py)."""
    from igg.parallel import accumulate as AC
    from igg.parallel import halo as HL

    from igg.parallel import grid as G

    igg.init_global_grid(4, 6, 5, overlapx=4, **KW)
    gg = G.global_grid()  # the grid itself: its arrays are mutable
    B = _values((4, 6, 5), torch.float64, 9)      # ol = 4, w = 1: 4 < 5
    assert AC.check_accumulate(B) == "float64"    # no neighbour in x: nothing is sent, nothing to refuse
    gg.neighbors[1, 0] = 1
    HL.sync_grid()
    _raises_and_leaves("too small in dimension 1 to accumulate its halo", B)
    with pytest.raises(igg.IGGError, match="a send range would overlap a halo"):  # the engine's own check
        HL.engine().accumulate_set(native.FieldSet([HL.field_tuple(B)]), "float64", 0, None)
    gg.neighbors[1, 0] = igg.PROC_NULL
    HL.sync_grid()
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------------------ autograd
def test_autograd_on_one_rank():
    _init((7, 6, 5))
    c = _values((7, 6, 5), torch.float64, 10)
    A = _values((7, 6, 5), torch.float64, 11).requires_grad_(True)
    out = igg.autograd.update_halo(A)
    ref = A.detach().clone()
    igg.update_halo_(ref)
    assert torch.equal(out.detach(), ref) and out.data_ptr() != A.data_ptr()
    (c * out).sum().backward()
    want = c.clone()
    igg.accumulate_halo_(want)
    assert torch.equal(A.grad, want)
    # a plain sum hands the backward pass an expanded gradient
    A.grad = None
    igg.autograd.update_halo(A).sum().backward()
    ones = torch.ones(7, 6, 5, dtype=torch.float64)
    igg.accumulate_halo_(ones)
    assert torch.equal(A.grad, ones)
    # torch's own check of the Jacobian, on a small field
    igg.finalize_global_grid(finalize_MPI=False)
    _init((4, 3, 3))
    S = torch.randn(4, 3, 3, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(igg.autograd.update_halo, (S,))
    igg.finalize_global_grid(finalize_MPI=False)


def test_autograd_on_two_ranks():
    run_accumulate_ranks(2, "autograd", "cpu", "float64", 2, 1, 1, 0)
    run_accumulate_ranks(2, "autograd", "cpu", "float64", 2, 1, 1, 1)


# ------------------------------------------------------------ several ranks
GRIDS = [(2, (2, 1, 1)), (4, (2, 2, 1)), (8, (2, 2, 2)), (3, (3, 1, 1))]


@pytest.mark.parametrize("overlap,width", [(2, 1), (3, 1), (4, 2)])
@pytest.mark.parametrize("periodic", [0, 7])
@pytest.mark.parametrize("nprocs,dims", GRIDS)
def test_gloo_ranks_against_the_emulation(nprocs, dims, periodic, overlap, width):
    dtype = "float32" if (nprocs + overlap + periodic) % 2 else "float64"
    run_accumulate_ranks(nprocs, "accumulate", "cpu", dtype, *dims, periodic, overlap, width)


def test_two_ranks_whose_send_slabs_are_one_plane():
    """Local n = 2*o - 1 on a periodic 2-rank dimension: both neighbours are
    the same peer and both messages go into plane 1."""
    run_accumulate_ranks(2, "accumulate", "cpu", "float64", 2, 1, 1, 1, 2, 1, "3,8,10")


def test_mixed_periods_on_a_3x1x2_grid():
    run_accumulate_ranks(6, "accumulate", "cpu", "float64", 3, 1, 2, 5, 3, 1)


# ------------------------------------------------------------------- example
@pytest.mark.parametrize("nprocs", [1, 2])
def test_the_deposit_example(nprocs):
    env = dict(os.environ)
    port = free_port()
    procs = []
    for r in range(nprocs):
        e = dict(env)
        e.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(r), "WORLD_SIZE": str(nprocs),
                  "LOCAL_RANK": str(r), "OMP_NUM_THREADS": "1", "IGG_HOST_THREADS": "2",
                  "PYTHONPATH": ROOT + os.pathsep + env.get("PYTHONPATH", "")})
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "examples", "halo_deposit.py"), "--cpu"],
                                      env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT))
    outs = [p.communicate(timeout=MAX_TIMEOUT)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-2000:]
    assert "every copy of a cell holds the total" in outs[0], outs[0][-2000:]
