"""scatter_g on the host (parallel/scatter_g.py): the plan by brute force
against ``indices_g``, one rank in every layout and conversion, every error,
multi-rank gloo runs and the regrid example.

Every comparison is bitwise: the fields hold integers of magnitude at most
1024, exact in f32 and f64. The two properties that pin the semantics: after a
scatter of a whole field ``update_halo_`` changes no bit of it, and ``gather_g``
of it returns the global array that was scattered.
"""
import itertools
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest
import torch

import igg
from igg.parallel import grid as G
from igg.parallel import scatter_g as SG
from tests._mp import MAX_TIMEOUT, ROOT, free_port
from tests.test_gather_g_cpu import KW, N, _init, _place

SENTINEL = -7777


def run_scatter_ranks(nprocs: int, scenario: str, *args, timeout: float = 150.0, env_extra=None) -> list:
    """``tests/mp_worker_scatter_g.py <scenario> ...`` on ``nprocs`` local
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
            [sys.executable, os.path.join(ROOT, "tests", "mp_worker_scatter_g.py"), scenario, *map(str, args)],
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
        raise AssertionError(f"scatter_g scenario {scenario} {args} failed or timed out:\n{msg}")
    for r, o in enumerate(outs):
        assert f"rank {r} scatter_g OK" in o, o[-1500:]
    return outs


# ------------------------------------------------------------------------ plan
def _boxes(ext, overlap):
    return [
        None,                                              # the whole field
        # an x-plane that two ranks hold (one periodic rank: its period is n - o, the plane is its index 0)
        ((N[0] - overlap) % ext[0], None, None),
        ((2, 4), None, (ext[2] - 2, ext[2])),              # a box that misses some ranks entirely
    ]


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 1, 1), (2, 2, 2), (3, 1, 2)])
@pytest.mark.parametrize("periods", [(0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1)])
@pytest.mark.parametrize("overlap", [2, 3, 4])
def test_plan_brute_force(dims, periods, overlap):
    """Over all ranks: every local cell whose indices_g index lies in the box
    is written exactly once, from the cell of that global index; no other
    local cell is written; every global cell of the box is read."""
    _init(overlap)
    gg = G.global_grid()
    for shape in (N, (N[0] + 1, N[1], N[2]), (N[0], N[1] - 1, N[2])):
        A = torch.zeros(shape)
        _place(dims, [0, 0, 0], periods)
        ext = igg.selection_shape_g(A)
        for box in _boxes(ext, overlap):
            sel = SG.normalize_selection(gg.nxyz, gg.overlaps, dims, periods, shape, box)
            lo = [s[0] for s in sel]
            hi = [s[1] for s in sel]
            read = np.zeros(igg.selection_shape_g(A, box), dtype=np.int64)
            empty_ranks = 0
            for coords in itertools.product(*(range(D) for D in dims)):
                pieces = SG.scatter_pieces(gg.nxyz, gg.overlaps, dims, periods, coords, shape, box)
                empty_ranks += not pieces
                _place(dims, coords, periods)
                gidx = [igg.indices_g(d, A).numpy() for d in range(3)]
                inside = [(gidx[d] >= lo[d]) & (gidx[d] < hi[d]) for d in range(3)]
                written = np.zeros(shape, dtype=np.int64)
                for dst, cnt, src in pieces:
                    ix, sx = [], []
                    for d in range(3):
                        assert cnt[d] >= 1
                        k = np.arange(cnt[d])
                        assert dst[d] >= 0 and dst[d] + cnt[d] <= shape[d], (coords, d, dst, cnt)
                        assert (gidx[d][dst[d] + k] == lo[d] + src[d] + k).all(), (coords, d, dst, cnt, src)
                        ix.append(dst[d] + k)
                        sx.append(src[d] + k)
                    written[np.ix_(*ix)] += 1
                    read[np.ix_(*sx)] += 1
                want = inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]
                assert (written == want).all(), (shape, box, coords, int(written.min()), int(written.max()))
                if box is None:
                    assert (written == 1).all()  # halo and overlap cells included
                    if dims == (1, 1, 1) and overlap == 4 and periods[0]:
                        # n=9, o=4, D=1: period 5, global indices 4 | 0 1 2 3 4 | 0 1 2 -> three runs along x
                        if shape[0] == N[0]:
                            assert gidx[0].tolist() == [4, 0, 1, 2, 3, 4, 0, 1, 2]
                        assert len({p[0][0] for p in pieces}) == 3
                        assert len(pieces) == (9 if periods[2] else 3)  # not bounded by 8
            assert (read >= 1).all(), (shape, box, int(read.min()))
            if box is not None and box[0] == (2, 4) and dims[0] > 1 and not periods[0]:
                assert empty_ranks > 0  # the ranks beyond x = 4 hold no cell of the box
    igg.finalize_global_grid(finalize_MPI=False)


def test_three_runs_where_the_local_size_exceeds_the_period():
    assert SG._runs(9, 4, 1, 1, 0, 9) == [(0, 1, 4), (1, 5, 0), (6, 3, 0)]
    assert SG._runs(9, 2, 2, 0, 1, 10) == [(0, 10, 7)]
    assert SG._runs(9, 2, 2, 1, 1, 9) == [(0, 8, 6), (8, 1, 0)]


def test_plan_is_pure_and_low_dimensional():
    _init(2)
    gg = G.global_grid()
    args = (gg.nxyz, gg.overlaps, (2, 2, 2), (0, 0, 0))
    before = (gg.dims.copy(), gg.coords.copy())
    p = SG.scatter_pieces(*args, (1, 1, 0), N)
    assert p == [((0, 0, 0), (9, 8, 10), (7, 6, 0))]  # the last rank in x and y, the first in z: every local cell
    assert (gg.dims == before[0]).all() and (gg.coords == before[1]).all()
    # a 2-D field: the ranks at z coordinate 1 hold copies and receive what those at 0 receive
    assert SG.scatter_pieces(*args, (0, 1, 0), N[:2]) == [((0, 0, 0), (9, 8, 1), (0, 6, 0))]
    assert SG.scatter_pieces(*args, (0, 1, 1), N[:2]) == SG.scatter_pieces(*args, (0, 1, 0), N[:2])
    # relative to the box's lower corner: global 3..11 of x; rank 1 holds 7..15 at local 0..8
    assert SG.scatter_pieces(*args, (1, 0, 0), N[:1], ((3, 12),)) == [((0, 0, 0), (5, 1, 1), (4, 0, 0))]
    assert SG.scatter_pieces(*args, (1, 0, 0), N[:1], ((0, 7),)) == []
    assert "scatter_g" in igg.__all__ and "scatter_pieces" in igg.__all__ and igg.scatter_pieces is SG.scatter_pieces
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------------------ one process
def _expected_local(shape, Gl, box_lo, box_hi, dtype):
    """A sentinel field whose cells inside the box hold the global cell of
    their indices_g index."""
    probe = torch.empty(shape, device="meta")
    nd = len(shape)
    idx = [igg.indices_g(d, probe) for d in range(nd)]
    view = [[-1 if e == d else 1 for e in range(nd)] for d in range(nd)]
    inside = torch.ones(shape, dtype=torch.bool)
    for d in range(nd):
        inside &= ((idx[d] >= box_lo[d]) & (idx[d] < box_hi[d])).view(view[d])
    rel = [(i - box_lo[d]).clamp(0, Gl.shape[d] - 1).view(view[d]) for d, i in enumerate(idx)]
    return torch.where(inside, Gl[tuple(rel)].to(dtype), torch.full(shape, SENTINEL, dtype=dtype))


def one_rank_cases(device, n, rng_seed=1):
    """The one-rank cases (shared with tests/test_gpu_scatter_g.py): fields of
    3, 2 and 1 dimensions, a staggered shape, C and permuted layouts; whole
    field, a plane box and both conversions; then update_halo_ is a no-op and
    gather_g returns A_global."""
    g = torch.Generator().manual_seed(rng_seed)
    for shape in (n, (n[0] + 1, n[1], n[2]), n[:2], n[:1]):
        nd = len(shape)
        ext = igg.selection_shape_g(torch.empty(shape, device="meta"))
        rev = tuple(reversed(range(nd)))
        for permuted, (gdt, dt) in itertools.product((False, True), (
                (torch.float64, torch.float64), (torch.float32, torch.float64), (torch.float64, torch.float32))):
            def field():
                A = torch.full(shape, SENTINEL, dtype=dt, device=device)
                return A.permute(rev).contiguous().permute(rev) if permuted else A

            Gl = torch.randint(-1024, 1025, ext, generator=g).to(gdt)
            A = field()
            assert nd == 1 or A.is_contiguous() != permuted
            Gd = Gl.to(device)
            igg.scatter_g(Gd, A)
            want = _expected_local(shape, Gl, (0,) * nd, ext, dt)
            assert (want != SENTINEL).all()
            assert torch.equal(A.cpu(), want), (shape, gdt, dt, permuted)
            assert torch.equal(Gd.cpu(), Gl)
            igg.update_halo_(A)
            assert torch.equal(A.cpu(), want), (shape, gdt, dt, permuted, "update_halo_ changed the field")
            back = torch.full(ext, SENTINEL, dtype=dt, device=device)
            igg.gather_g(A, back)
            assert torch.equal(back.cpu(), Gl.to(dt)), (shape, gdt, dt, permuted, "round trip")
            # a plane: the cells outside it keep the sentinel
            plane = (None, ext[1] // 2, None)[:nd] if nd > 1 else (ext[0] // 2,)
            lo = [0 if b is None else b for b in plane]
            hi = [ext[d] if b is None else b + 1 for d, b in enumerate(plane)]
            Gp = Gl[tuple(slice(a, b) for a, b in zip(lo, hi))].contiguous()
            assert tuple(Gp.shape) == igg.selection_shape_g(A, plane)
            A = field()
            igg.scatter_g(Gp.to(device), A, box=plane)
            want = _expected_local(shape, Gp, lo, hi, dt)
            assert (want == SENTINEL).any() and (want != SENTINEL).any()
            assert torch.equal(A.cpu(), want), (shape, gdt, dt, permuted, "plane")
            if device.type != "cpu" and not permuted:  # A_global on the CPU
                A = field()
                igg.scatter_g(Gp, A, box=plane)
                assert torch.equal(A.cpu(), want), (shape, gdt, dt, "plane from the CPU")


@pytest.mark.parametrize("periods", [(0, 0, 0), (1, 1, 1), (1, 0, 1)])
def test_one_rank_on_cpu(periods):
    igg.init_global_grid(*N, periodx=periods[0], periody=periods[1], periodz=periods[2], overlapz=3, **KW)
    one_rank_cases(torch.device("cpu"), N)
    igg.finalize_global_grid(finalize_MPI=False)


# ---------------------------------------------------------------------- errors
def test_errors():
    A = torch.full(N, float(SENTINEL), dtype=torch.float64)
    Gl = torch.zeros(N, dtype=torch.float64)
    with pytest.raises(igg.IGGError, match="init_global_grid"):
        igg.scatter_g(Gl, A)
    igg.init_global_grid(*N, **KW)
    Gl = torch.arange(N[0] * N[1] * N[2], dtype=torch.float64).view(N)
    before = (A.clone(), Gl.clone())
    Ai = A.int()
    for call in (
            lambda: igg.scatter_g(Gl, torch.zeros(2, 2, 2, 2)),                       # four dimensions
            lambda: igg.scatter_g(Gl, torch.zeros(())),                               # none
            lambda: igg.scatter_g(Gl, A, box=(None, None)),                           # box of the wrong length
            lambda: igg.scatter_g(Gl, A, box=3),
            lambda: igg.scatter_g(Gl, A, box=((3, 3), None, None)),                   # an empty box
            lambda: igg.scatter_g(Gl, A, box=((4, 2), None, None)),
            lambda: igg.scatter_g(Gl, A, box=((0, N[0] + 1), None, None)),            # out of range
            lambda: igg.scatter_g(Gl, A, box=(None, (-1, 3), None)),                  # no negative indices
            lambda: igg.scatter_g(Gl, A, box=(None, None, N[2])),
            lambda: igg.scatter_g(Gl, A, box=(None, "x", None)),
            lambda: igg.scatter_g(None, A),                                           # A_global missing on the root
            lambda: igg.scatter_g(torch.zeros(N[0], N[1], N[2] + 1, dtype=torch.float64), A),  # wrong shape
            lambda: igg.scatter_g(Gl, A, box=(None, 2, None)),                        # (the axis stays, with length 1)
            lambda: igg.scatter_g(Gl.half(), A),                                      # dtypes outside the table
            lambda: igg.scatter_g(Gl.int(), A),
            lambda: igg.scatter_g(Gl, Ai),
            lambda: igg.scatter_g(Gl.float(), Ai),
            lambda: igg.scatter_g(Gl.float(), A.half()),
            lambda: igg.scatter_g(torch.zeros(N[0], N[1], 2 * N[2], dtype=torch.float64)[:, :, ::2], A),  # not contiguous
            lambda: igg.scatter_g(Gl, A, root=1),                                     # no such rank
            lambda: igg.scatter_g(Gl, A, root=-1),
            lambda: SG.scatter_pieces((9, 8, 10), (2, 2, 2), (1, 1, 1), (0, 0, 0), (0, 0, 0), N, (None,))):
        with pytest.raises(igg.IGGError):
            call()
    with pytest.raises(TypeError):
        igg.scatter_g(Gl, A, step=2)  # there is no step
    with pytest.raises(igg.IGGError, match="scatter_g"):
        igg.scatter_g(Gl, A, box=((3, 3), None, None))
    assert torch.equal(A, before[0]) and torch.equal(Gl, before[1])  # refused before anything was written
    assert (Ai == SENTINEL).all()
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------------------ multi-rank
@pytest.mark.parametrize("nprocs,args", [
    (2, (2, 1, 1, 0, 2, 1)),
    (4, (2, 2, 1, 1, 3, 1)),   # periodic x, overlap 3
    (8, (2, 2, 2, 0, 2, 1)),
    (4, (2, 1, 2, 5, 4, 2)),   # periodic x and z, overlap 4, halo width 2
])
def test_multi_rank_gloo(nprocs, args):
    run_scatter_ranks(nprocs, "scatter", "cpu", "float64", *args)


# --------------------------------------------------------------------- example
def _regrid(nprocs, tmp_path, *args):
    script = os.path.join(ROOT, "examples", "diffusion3D_regrid.py")
    cmd = [sys.executable, script] if nprocs == 1 else [
        sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nprocs}", "--master-addr",
        "127.0.0.1", "--master-port", str(free_port()), script]
    env = dict(os.environ, OMP_NUM_THREADS="1", IGG_HOST_THREADS="2")
    r = subprocess.run(cmd + ["--cpu", "--ny", "16", "--nz", "16", *args], capture_output=True, text=True,
                       timeout=MAX_TIMEOUT, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_regrid_example_restarts_on_another_decomposition(tmp_path):
    """10 steps on 2 ranks, saved, then 10 more on 1 rank from the file, must
    equal 20 uninterrupted steps on 1 rank exactly: the host stencil's per-cell
    expression does not depend on where a cell sits."""
    first, second, straight = (str(tmp_path / f) for f in ("first.npz", "second.npz", "straight.npz"))
    out = _regrid(2, tmp_path, "--nx", "16", "--nt", "10", "--save", first)
    assert "30x16x16 global grid on 2 ranks: 10 steps, 10 in all" in out
    out = _regrid(1, tmp_path, "--nx", "30", "--nt", "10", "--init", first, "--save", second)
    assert "30x16x16 global grid on 1 ranks: 10 steps, 20 in all" in out
    out = _regrid(1, tmp_path, "--nx", "30", "--nt", "20", "--save", straight)
    assert "30x16x16 global grid on 1 ranks: 20 steps, 20 in all" in out
    with np.load(first) as a, np.load(second) as b, np.load(straight) as c:
        assert a["T"].shape == (30, 16, 16) and int(b["steps"]) == 20
        assert not np.array_equal(a["T"], b["T"])  # the second run moved on
        assert np.array_equal(b["Cp"], c["Cp"])
        diff = np.abs(b["T"] - c["T"])
        assert np.array_equal(b["T"], c["T"]), f"max |difference| {diff.max():.3e} at {int((diff > 0).sum())} cells"
