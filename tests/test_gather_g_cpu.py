"""gather_g on the host (parallel/gather_g.py): global indices against
``coords_g``, the selection plan by brute force, multi-rank gloo runs, every
error and the slices example.

Every comparison is bitwise: the fields hold integers of magnitude at most
1024, exact in f32 and f64.

``indices_g`` against ``coords_g``: in a periodic dimension the global array
is ordered by the wrapped coordinate, so ``floor(coords_g(d, 1.0, A))`` IS the
index. In a non-periodic dimension the index is ``c*(n-o) + i`` and the
coordinate carries the field's stagger offset ``0.5*(n-m)`` on top of it, so
the floor is the index plus ``(n-m)//2`` (equal for ``m == n`` and
``m == n - 1``, one less for ``m > n``); the test asserts that relation.
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
from igg.parallel import gather_g as GG
from igg.parallel import grid as G
from tests._mp import MAX_TIMEOUT, ROOT, free_port

KW = dict(quiet=True, init_MPI=False, device_type="none")
N = (9, 8, 10)


def run_gather_ranks(nprocs: int, scenario: str, *args, timeout: float = 150.0, env_extra=None) -> list:
    """``tests/mp_worker_gather_g.py <scenario> ...`` on ``nprocs`` local
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
            [sys.executable, os.path.join(ROOT, "tests", "mp_worker_gather_g.py"), scenario, *map(str, args)],
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
        raise AssertionError(f"gather_g scenario {scenario} {args} failed or timed out:\n{msg}")
    for r, o in enumerate(outs):
        assert f"rank {r} gather_g OK" in o, o[-1500:]
    return outs


def _place(dims, coords, periods=None):
    """Pretend to be rank ``coords`` of a ``dims`` grid (the grid's arrays are
    mutable, as in tests/test_tools.py)."""
    gg = G.global_grid()
    gg.dims[:] = dims
    gg.coords[:] = coords
    if periods is not None:
        gg.periods[:] = periods
    gg.nxyz_g[:] = gg.dims * (gg.nxyz - gg.overlaps) + gg.overlaps * (gg.periods == 0)
    return gg


def _init(overlap, n=N):
    w = 2 if overlap == 4 else 1  # a halo width of 2 needs an overlap of 4
    igg.init_global_grid(*n, overlapx=overlap, overlapy=overlap, overlapz=overlap, halowidthx=w, halowidthy=w,
                         halowidthz=w, **KW)


# ------------------------------------------------------------------- indices_g
@pytest.mark.parametrize("overlap", [2, 3, 4])
def test_indices_g_against_coords_g(overlap):
    _init(overlap)
    size_g = (igg.nx_g, igg.ny_g, igg.nz_g)
    for d, per, D, dm in itertools.product(range(3), (0, 1), (1, 2, 3), (-1, 0, 1, 2)):
        n, m = N[d], N[d] + dm
        shape = list(N)
        shape[d] = m
        A = torch.zeros(shape)
        seen = []
        for c in range(D):
            dims, coords, periods = [2, 2, 2], [1, 0, 1], [0, 1, 0]
            dims[d], coords[d], periods[d] = D, c, per
            _place(dims, coords, periods)
            g = igg.indices_g(d, A)
            assert g.dtype == torch.int64 and g.shape == (m,)
            a, b = igg.owned_ranges(A)[d]
            fl = torch.floor(igg.coords_g(d, 1.0, A)).to(torch.int64)
            ext = igg.selection_shape_g(A)[d]
            if per:
                assert ext == D * (n - overlap)
                assert torch.equal(fl[a:b], g[a:b]), (d, D, c, m, fl.tolist(), g.tolist())
            else:
                assert ext == size_g[d](A) == D * (n - overlap) + overlap + dm
                assert torch.equal(g, c * (n - overlap) + torch.arange(m))
                assert torch.equal(fl, g + (n - m) // 2)  # the coordinate's stagger offset (module docstring)
            assert 0 <= int(g[a:b].min()) and int(g[a:b].max()) < ext
            seen += g[a:b].tolist()
        assert sorted(seen) == list(range(ext)), (d, per, D, m)  # every global index owned exactly once
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------------------------ plan
def _selections(ext, overlap):
    return [
        (None, 1),                                                   # the whole field
        ((N[0] - overlap, None, None), 1),                           # an x-plane that two ranks hold
        (((2, 4), None, (ext[2] - 2, ext[2])), 1),                   # a box that misses some ranks entirely
        (None, (2, 3, 1)),
        (((1, ext[0]), None, (0, ext[2] - 1)), (3, 1, 3)),           # a step of 3 across a wrapping last rank
    ]


@pytest.mark.parametrize("dims", [(2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 1, 2)])
@pytest.mark.parametrize("periods", [(0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1)])
@pytest.mark.parametrize("overlap", [2, 3, 4])
def test_plan_brute_force(dims, periods, overlap):
    _init(overlap)
    gg = G.global_grid()
    wrapped = 0
    for shape in (N, (N[0] + 1, N[1], N[2]), (N[0], N[1] - 1, N[2])):
        A = torch.zeros(shape)
        _place(dims, [0, 0, 0], periods)
        ext = igg.selection_shape_g(A)
        for box, step in _selections(ext, overlap):
            sel = GG.normalize_selection(gg.nxyz, gg.overlaps, dims, periods, shape, box, step)
            out_shape = igg.selection_shape_g(A, box, step)
            count = np.zeros(out_shape, dtype=np.int64)
            empty_ranks = 0
            for coords in itertools.product(*(range(D) for D in dims)):
                pieces = GG.selection_pieces(gg.nxyz, gg.overlaps, dims, periods, coords, shape, box, step)
                assert len(pieces) <= 8
                wrapped += len(pieces) > 1
                empty_ranks += not pieces
                _place(dims, coords, periods)
                owned = igg.owned_ranges(A)
                gidx = [igg.indices_g(d, A).numpy() for d in range(3)]
                for src, cnt, dst in pieces:
                    ix = []
                    for d in range(3):
                        lo, _hi, s = sel[d]
                        assert cnt[d] >= 1
                        k = np.arange(cnt[d])
                        i = src[d] + k * s
                        assert owned[d][0] <= i.min() and i.max() < owned[d][1], (coords, d, src, cnt, owned)
                        assert (gidx[d][i] == lo + (dst[d] + k) * s).all(), (coords, d, src, cnt, dst)
                        ix.append(dst[d] + k)
                    count[np.ix_(*ix)] += 1
            assert (count == 1).all(), (shape, box, step, int(count.min()), int(count.max()))
            if box is not None and box[0] == (2, 4):
                assert empty_ranks > 0
    if overlap == 4 and any(periods):
        assert wrapped > 0  # the last rank's owned range wraps past the global extent
    igg.finalize_global_grid(finalize_MPI=False)


def test_plan_is_pure_and_low_dimensional():
    _init(2)
    gg = G.global_grid()
    args = (gg.nxyz, gg.overlaps, (2, 2, 2), (0, 0, 0))
    before = (gg.dims.copy(), gg.coords.copy())
    p = GG.selection_pieces(*args, (1, 1, 0), N)
    assert p == [((1, 1, 0), (8, 7, 9), (8, 7, 0))]  # the last rank in x and y, the first in z
    assert (gg.dims == before[0]).all() and (gg.coords == before[1]).all()
    # a 2-D field: only the ranks at z coordinate 0 contribute
    assert GG.selection_pieces(*args, (0, 1, 0), N[:2]) == [((0, 1, 0), (8, 7, 1), (0, 7, 0))]
    assert GG.selection_pieces(*args, (0, 1, 1), N[:2]) == []
    # global indices 3, 7, 11: rank 1 owns [8, 16) at local [1, 9), so 11 is its local cell 4, output cell 2
    assert GG.selection_pieces(*args, (1, 0, 0), N[:1], ((3, 12),), 4) == [((4, 0, 0), (1, 1, 1), (2, 0, 0))]
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------------------ one process
def _expected_global(A):
    """The global array of a single rank's field from indices_g and owned_ranges."""
    rng = igg.owned_ranges(A)
    ext = igg.selection_shape_g(A)
    want = torch.full(ext, -9999, dtype=A.dtype)
    ix = [igg.indices_g(d, A)[a:b] for d, (a, b) in enumerate(rng)]
    view = [[-1 if e == d else 1 for e in range(A.dim())] for d in range(A.dim())]
    want[tuple(i.view(v) for i, v in zip(ix, view))] = igg.owned_view(A)
    assert (want != -9999).all()
    return want


@pytest.mark.parametrize("periods", [(0, 0, 0), (1, 1, 1), (1, 0, 1)])
def test_one_rank_on_cpu(periods):
    igg.init_global_grid(*N, periodx=periods[0], periody=periods[1], periodz=periods[2], overlapz=3, **KW)
    g = torch.Generator().manual_seed(1)
    for shape in (N, (N[0] + 1, N[1], N[2]), N[:2], N[:1]):
        C = torch.randint(-1024, 1025, shape, generator=g).to(torch.float64)
        perm = C.permute(*reversed(range(C.dim()))).contiguous().permute(*reversed(range(C.dim())))
        assert torch.equal(perm, C) and (C.dim() == 1 or not perm.is_contiguous())
        for A in (C, perm):
            want = _expected_global(A)
            ext = tuple(want.shape)
            assert ext == tuple(N[d] - (2, 2, 3)[d] if periods[d] else shape[d] for d in range(len(shape)))
            out = torch.zeros(ext, dtype=torch.float64)
            igg.gather_g(A, out)
            assert torch.equal(out, want)
            box = ((1, ext[0]),) + (None,) * (A.dim() - 1)
            out = torch.zeros(igg.selection_shape_g(A, box, 2), dtype=torch.float32)
            igg.gather_g(A, out, box=box, step=2, dtype=torch.float32)
            assert torch.equal(out, want[(slice(1, None, 2),) + (slice(None, None, 2),) * (A.dim() - 1)].float())
    igg.finalize_global_grid(finalize_MPI=False)


def test_buffers_grow_only_and_are_freed():
    from igg.parallel import gather as GA

    igg.init_global_grid(*N, **KW)
    GG._buffer("host", 100, torch.device("cpu"))
    b = GG._buffer("host", 50, torch.device("cpu"))
    assert b.numel() == 100 and GG._buffer("host", 200, torch.device("cpu")).numel() == 200
    GA.free_gather_buffer()
    assert not GG._bufs
    GG._buffer("host", 8, torch.device("cpu"))
    igg.finalize_global_grid(finalize_MPI=False)
    assert not GG._bufs


# ---------------------------------------------------------------------- errors
def test_errors():
    A = torch.zeros(N, dtype=torch.float64)
    out = torch.zeros(N, dtype=torch.float64)
    for call in (lambda: igg.gather_g(A, out), lambda: igg.indices_g(0, A), lambda: igg.selection_shape_g(A)):
        with pytest.raises(igg.IGGError, match="init_global_grid"):
            call()
    igg.init_global_grid(*N, **KW)
    before = out.clone()
    for call in (
            lambda: igg.gather_g(torch.zeros(2, 2, 2, 2), out),                     # four dimensions
            lambda: igg.gather_g(torch.zeros(()), out),                             # none
            lambda: igg.gather_g(A, out, box=(None, None)),                         # box of the wrong length
            lambda: igg.gather_g(A, out, box=3),
            lambda: igg.gather_g(A, out, step=(1, 1)),                              # step of the wrong length
            lambda: igg.gather_g(A, out, step=0),                                   # step < 1
            lambda: igg.gather_g(A, out, step=(1, -2, 1)),
            lambda: igg.gather_g(A, out, step=1.5),
            lambda: igg.gather_g(A, out, box=((3, 3), None, None)),                 # an empty box
            lambda: igg.gather_g(A, out, box=((4, 2), None, None)),
            lambda: igg.gather_g(A, out, box=((0, N[0] + 1), None, None)),          # out of range
            lambda: igg.gather_g(A, out, box=(None, (-1, 3), None)),                # no negative indices
            lambda: igg.gather_g(A, out, box=(None, None, N[2])),
            lambda: igg.gather_g(A, out, box=(None, "x", None)),
            lambda: igg.gather_g(A, out, dtype=torch.float16),                      # unsupported dtype
            lambda: igg.gather_g(A.float(), out, dtype=torch.float64),
            lambda: igg.gather_g(A.int(), out, dtype=torch.float32),
            lambda: igg.gather_g(A, None),                                          # A_global missing on the root
            lambda: igg.gather_g(A, torch.zeros(N[0], N[1], N[2] + 1, dtype=torch.float64)),  # wrong shape
            lambda: igg.gather_g(A, out, box=(None, 2, None)),                      # (the axis stays, with length 1)
            lambda: igg.gather_g(A, out.float()),                                   # wrong dtype
            lambda: igg.gather_g(A, out, dtype=torch.float32),
            lambda: igg.gather_g(A, torch.zeros(N[0], N[1], 2 * N[2], dtype=torch.float64)[:, :, ::2]),  # not contiguous
            lambda: igg.gather_g(A, out, root=1),                                   # no such rank
            lambda: igg.selection_shape_g(A, (None,), 1),
            lambda: igg.selection_shape_g(A, None, 0),
            lambda: igg.indices_g(3, A),
            lambda: igg.indices_g(0, torch.zeros(2, 2, 2, 2))):
        with pytest.raises(igg.IGGError):
            call()
    assert torch.equal(out, before)  # refused before anything was written
    assert igg.selection_shape_g(A, (None, 2, None)) == (N[0], 1, N[2])
    assert igg.selection_shape_g(A, ((1, 8), None, (2, 10)), (2, 3, 1)) == (4, 3, 8)
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------------------ multi-rank
@pytest.mark.parametrize("nprocs,args", [
    (2, (2, 1, 1, 0, 2, 1)),
    (4, (2, 2, 1, 1, 3, 1)),   # periodic x, overlap 3
    (8, (2, 2, 2, 0, 2, 1)),
    (4, (2, 1, 2, 5, 4, 2)),   # periodic x and z, overlap 4, halo width 2: the last rank's owned range wraps
])
def test_multi_rank_gloo(nprocs, args):
    run_gather_ranks(nprocs, "gather", "cpu", "float64", *args)


# --------------------------------------------------------------------- example
def test_slices_example_writes_two_frames(tmp_path):
    from PIL import Image

    gif = str(tmp_path / "s.gif")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "examples", "diffusion3D_slices.py"),
           "--nx", "16", "--nt", "20", "--vis-every", "10", "--cpu", "--out", gif]
    env = dict(os.environ, OMP_NUM_THREADS="1", IGG_HOST_THREADS="2")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=MAX_TIMEOUT, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "2 frames of the 30x16 y-mid plane of the 30x16x16 global grid" in r.stdout
    with Image.open(gif) as im:
        assert im.n_frames == 2
