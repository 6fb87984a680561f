"""The converting lattice copy (csrc/kernels/select_kernels.hip) at descriptor
level and gather_g on the GPU (parallel/gather_g.py).

Kernel tests: the source lattice is carved out of a NaN buffer with NaN
between the selected elements, the destination is a box inside a buffer filled
with a sentinel, and the WHOLE destination allocation is compared byte for byte
with torch's CPU ``.to(torch.float32)`` of the same lattice (for NaN values the
positions are compared): a stray store, a lane one element off or a load that
let a neighbour's NaN in shows up. Integers of magnitude at most 1024 are exact
in f32 and f64, so every comparison is bitwise.
"""
import math

import numpy as np
import pytest
import torch

import igg
from igg._native import native
from igg.parallel import gather_g as GG
from tests.test_gather_g_cpu import N, _expected_global, run_gather_ranks

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 64  # elements around a carved lattice: the buffers' bases stay 256-B aligned
SENTINEL = -777.0


def _span(c, s):
    return sum((n - 1) * k for n, k in zip(c, s)) + 1 if all(c) else 1


def _values(c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1024, 1025, tuple(c), generator=g).to(torch.float64)


class Job:
    """One descriptor with its buffers: the source on the host and the device,
    the destination and what it must hold afterwards."""

    def __init__(self, gpu, c, S, T, src_off=0, dst_off=0, vals=None, seed=1):
        self.c, self.S, self.T = list(c), list(S), list(T)
        vals = _values(c, seed) if vals is None else vals
        src = torch.full((PAD + src_off + _span(c, S) + PAD,), NAN, dtype=torch.float64)
        src.as_strided(self.c, self.S, PAD + src_off).copy_(vals)
        self.want = torch.full((PAD + dst_off + _span(c, T) + PAD,), SENTINEL, dtype=torch.float32)
        self.want.as_strided(self.c, self.T, PAD + dst_off).copy_(vals.to(torch.float32))  # the CPU's conversion
        self.src = src.to(gpu)
        self.dst = torch.full_like(self.want, SENTINEL, device=gpu)
        self.desc = (self.src.data_ptr() + 8 * (PAD + src_off), self.dst.data_ptr() + 4 * (PAD + dst_off), self.c,
                     self.S, self.T)
        self.plan = native.select_plan(self.c, self.S, self.T)

    def check(self, tag=""):
        got = self.dst.cpu()
        gn, wn = torch.isnan(got), torch.isnan(self.want)
        same = torch.equal(gn, wn) and torch.equal(got.view(torch.int32)[~gn], self.want.view(torch.int32)[~wn])
        if not same:
            bad = ((got.view(torch.int32) != self.want.view(torch.int32)) & ~(gn & wn)).nonzero().flatten()[:6]
            raise AssertionError(f"{tag} c={self.c} S={self.S} T={self.T}: {len(bad)}+ differences, first at "
                                 f"{[int(b) - PAD for b in bad]}: got {got[bad].tolist()}, "
                                 f"want {self.want[bad].tolist()}")


def _launch(*jobs):
    native.select_convert([j.desc for j in jobs], torch.cuda.current_stream().cuda_stream)


def _run(gpu, c, S, T, path, **kw):
    j = Job(gpu, c, S, T, **kw)
    assert j.plan["path"] == path and j.plan["index_bits"] == 32, j.plan
    _launch(j)
    j.check(path)
    return j


def _dense(shape):
    return [int(np.prod(shape[d + 1:])) for d in range(len(shape))]


# ------------------------------------------------------------------- rows path
ROW_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 259, 1027)


@pytest.mark.parametrize("n", ROW_LENGTHS)
def test_rows_path_every_head_and_tail(gpu, n):
    """Every source and destination residue of the row start; 3 x 5 rows in
    pitches that are no multiple of 16 B (odd element counts), so the rows of
    one job also start at every residue."""
    ps, pt = (n + 2) | 1, (n + 4) | 1
    assert (ps * 8) % 16 and (pt * 4) % 16
    for rs in (0, 1):
        for rd in (0, 1, 2, 3):
            _run(gpu, (3, 5, n), (5 * ps + 2, ps, 1), (5 * pt + 3, pt, 1), "rows", src_off=rs, dst_off=rd,
                 seed=n + 8 * rs + rd)


def test_rows_path_many_short_rows(gpu):
    """12 000 rows of 7: more rows than one pass of the grid holds waves."""
    j = _run(gpu, (120, 100, 7), (100 * 9 + 1, 9, 1), (100 * 11, 11, 1), "rows", src_off=1, dst_off=3)
    assert j.plan["rows"] == 12000 and j.plan["blocks"] == native.SELECT_MAX_BLOCKS
    assert j.plan["rows"] > 4 * j.plan["blocks"]


def test_steps_along_outer_axes_stay_on_the_rows_path(gpu):
    shape = (9, 14, 70)
    d = _dense(shape)
    c = (5, 5, 70)  # steps (2, 3, 1) of the whole field
    assert native.select_plan(c, [2 * d[0], 3 * d[1], 1], _dense(c))["path"] == "rows"
    _run(gpu, c, (2 * d[0], 3 * d[1], 1), _dense(c), "rows")
    _run(gpu, c, (2 * d[0], 3 * d[1], 1), (5 * 75 + 1, 75, 1), "rows", src_off=1, dst_off=2)


# ---------------------------------------------------------------- element path
@pytest.mark.parametrize("step", [(1, 1, 2), (1, 1, 3), (2, 3, 2)])
def test_element_path_steps(gpu, step):
    shape = (6, 11, 83)
    d = _dense(shape)
    c = [-(-shape[k] // step[k]) for k in range(3)]
    S = [d[k] * step[k] for k in range(3)]
    _run(gpu, c, S, _dense(c), "element", src_off=1)                                   # compact destination
    _run(gpu, c, S, ((c[1] + 2) * (c[2] + 5), c[2] + 5, 1), "element", dst_off=3)      # a box in a larger array


def test_element_path_permuted_and_large(gpu):
    n0, n1, n2 = 7, 9, 13
    _run(gpu, (n0, n1, n2), (1, n0, n0 * n1), _dense((n0, n1, n2)), "element")          # a permuted source
    _run(gpu, (n0, n1, n2), _dense((n0, n1, n2)), (1, n0, n0 * n1), "element")          # a permuted destination
    # more elements than one pass of the grid holds lanes
    c = (70, 90, 100)
    j = _run(gpu, c, (90 * 200, 200, 2), _dense(c), "element")
    assert j.plan["blocks"] == native.SELECT_MAX_BLOCKS and j.plan["total"] > 256 * j.plan["blocks"]


# ----------------------------------------------------------------- the batch
def test_batch_of_eight_jobs_in_one_launch(gpu):
    assert native.SELECT_MAX_JOBS >= 8
    jobs = [
        Job(gpu, (3, 5, 66), (5 * 71, 71, 1), (5 * 69, 69, 1), src_off=1, dst_off=1, seed=1),
        Job(gpu, (1, 1, 1), (0, 0, 1), (0, 0, 1), dst_off=2, seed=2),                     # one element
        Job(gpu, (4, 0, 9), (90, 9, 1), (90, 9, 1), seed=3),                              # empty
        Job(gpu, (2, 7, 31), (7 * 64, 64, 2), (7 * 31, 31, 1), seed=4),                   # element
        Job(gpu, (1, 300, 5), (0, 7, 1), (0, 5, 1), src_off=1, seed=5),
        Job(gpu, (6, 4, 12), (1, 6, 24), (48, 12, 1), seed=6),                            # permuted: element
        Job(gpu, (1, 1, 1027), (0, 0, 1), (0, 0, 1), src_off=1, dst_off=3, seed=7),
        Job(gpu, (9, 2, 4), (2 * 5, 5, 1), (2 * 6, 6, 1), dst_off=1, seed=8),
    ]
    paths = [j.plan["path"] for j in jobs]
    assert paths.count("rows") >= 4 and paths.count("element") >= 2
    assert jobs[2].plan["blocks"] == 0 and jobs[1].plan["total"] == 1
    _launch(*jobs)
    for k, j in enumerate(jobs):
        j.check(f"job {k}")
    # more jobs than one launch takes
    many = [Job(gpu, (2, 3, 5 + k), (3 * 40, 40, 1), (3 * 37, 37, 1), src_off=k & 1, dst_off=k & 3, seed=k)
            for k in range(native.SELECT_MAX_JOBS + 3)]
    _launch(*many)
    for k, j in enumerate(many):
        j.check(f"many {k}")


# ------------------------------------------------------------------ the values
def test_conversion_rounds_to_nearest_even_and_keeps_subnormals(gpu):
    half_max = (2.0 - 2.0 ** -24) * 2.0 ** 127  # halfway from FLT_MAX to 2^128: to even, which is inf
    special = [0.0, -0.0, 1.0, -1024.0, math.inf, -math.inf, NAN,
               1e39, -1e39, 3.5e38,                      # overflow f32 to +-inf
               1e-40, -1e-40, 2.0 ** -149, 2.0 ** -140,  # f32 subnormal images
               2.0 ** -150, 1.5 * 2.0 ** -149,           # ties between subnormals: to even (0 and 2^-148)
               2.0 ** -151,                              # below half the smallest subnormal: 0
               1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24,   # ties: to even (1 and 1 + 2^-22)
               1.0 + 2.0 ** -24 + 2.0 ** -50,            # just above a tie: up
               half_max]
    want = {1e-40: np.float32(1e-40), 2.0 ** -149: np.float32(2.0 ** -149), 2.0 ** -150: np.float32(0.0),
            1.5 * 2.0 ** -149: np.float32(2.0 ** -148), 1.0 + 2.0 ** -24: np.float32(1.0),
            1.0 + 3 * 2.0 ** -24: np.float32(1.0 + 2.0 ** -22), 1e39: np.float32(np.inf),
            1.0 + 2.0 ** -24 + 2.0 ** -50: np.float32(1.0 + 2.0 ** -23), half_max: np.float32(np.inf)}
    assert float(want[1e-40]) != 0.0 and float(want[2.0 ** -149]) != 0.0  # subnormal, not flushed
    n = 67
    vals = _values((2, 3, n), 9)
    flat = vals.view(-1)
    flat[:len(special)] = torch.tensor(special, dtype=torch.float64)
    flat[-len(special):] = torch.tensor(special, dtype=torch.float64)  # in a tail as well
    for c, S, T, path, offs in (((2, 3, n), (3 * 71, 71, 1), (3 * 69, 69, 1), "rows", (1, 1)),
                                ((2, 3, n), (3 * 142, 142, 2), (3 * n, n, 1), "element", (0, 0))):
        j = _run(gpu, c, S, T, path, src_off=offs[0], dst_off=offs[1], vals=vals)
        out = j.dst.cpu().as_strided(list(c), list(T), PAD + offs[1]).reshape(-1)
        for k, v in enumerate(special):
            if v in want:
                assert out[k].numpy().tobytes() == want[v].tobytes(), (path, v, float(out[k]))
        assert math.isnan(out[special.index(1e39) - 1].item())


# -------------------------------------------------------------------- the plan
def test_plan_paths_and_index_widths():
    p = native.select_plan((3, 5, 9), (50, 10, 1), (45, 9, 1))
    assert p["path"] == "rows" and p["index_bits"] == 32 and p["rows"] == 15 and p["total"] == 135
    assert p["blocks"] == 4 and p["src_span"] == 2 * 50 + 4 * 10 + 8 and p["dst_span"] == 134
    assert native.select_plan((3, 5, 9), (100, 20, 2), (45, 9, 1))["path"] == "element"
    assert native.select_plan((3, 5, 9), (50, 10, 1), (90, 18, 2))["path"] == "element"
    assert native.select_plan((3, 5, 9), (1, 3, 15), (45, 9, 1))["path"] == "element"
    assert native.select_plan((3, 0, 9), (50, 10, 1), (45, 9, 1))["blocks"] == 0
    # 64-bit offsets: the plan here; the 64-bit kernel runs in tests/test_gpu_large_offsets.py (a 17 GB field)
    big = native.select_plan((1300, 1300, 1300), (1300 * 1300, 1300, 1), (1300 * 1300, 1300, 1))
    assert big["index_bits"] == 64 and big["path"] == "rows" and big["blocks"] == native.SELECT_MAX_BLOCKS
    assert native.select_plan((2, 2, 2), (1 << 31, 4, 2), (4, 2, 1))["index_bits"] == 64    # the source span alone
    assert native.select_plan((2, 2, 2), (4, 2, 1), (1 << 31, 2, 1))["index_bits"] == 64    # the destination span
    assert native.select_plan((1024, 1024, 1024), (1 << 20, 1 << 10, 1), (1 << 20, 1 << 10, 1))["index_bits"] == 32
    for bad in (((-1, 2, 2), (4, 2, 1), (4, 2, 1)), ((2, 2, 2), (4, -2, 1), (4, 2, 1))):
        with pytest.raises(igg.IGGError):
            native.select_plan(*bad)


# ------------------------------------------------------------- gather_g, 1 rank
def _nan_outside_owned(A):
    rng = igg.owned_ranges(A)
    for d, (a, b) in enumerate(rng):
        sl = [slice(None)] * A.dim()
        sl[d] = slice(0, a)
        A[tuple(sl)] = NAN
        sl[d] = slice(b, None)
        A[tuple(sl)] = NAN


@pytest.mark.parametrize("periods", [(0, 0, 0), (1, 1, 1), (1, 0, 1)])
def test_gather_g_on_one_rank(gpu, periods):
    n = (20, 9, 70)
    igg.init_global_grid(*n, periodx=periods[0], periody=periods[1], periodz=periods[2], overlapz=3, quiet=True,
                         init_MPI=False)
    g = torch.Generator().manual_seed(3)
    for shape in (n, (n[0] + 1, n[1], n[2]), n[:2], n[:1]):
        C = torch.randint(-1024, 1025, shape, generator=g).to(torch.float64)
        _nan_outside_owned(C)
        nd = C.dim()
        want = _expected_global(C)
        ext = tuple(want.shape)
        assert ext == tuple(n[d] - (2, 2, 3)[d] if periods[d] else shape[d] for d in range(nd))
        rev = tuple(reversed(range(nd)))
        for A in (C.to(gpu), C.to(gpu).permute(rev).contiguous().permute(rev)):
            for dtype in (None, torch.float32):
                odt = dtype or torch.float64
                out = torch.full(ext, SENTINEL, dtype=odt, device=gpu)
                igg.gather_g(A, out, dtype=dtype)
                assert torch.equal(out.cpu(), want.to(odt)), (shape, dtype, A.stride())
                plane = (None, ext[1] // 2, None)[:nd] if nd > 1 else (ext[0] // 2,)
                sl = tuple(slice(None) if b is None else slice(b, b + 1) for b in plane)
                out = torch.full(igg.selection_shape_g(A, plane), SENTINEL, dtype=odt, device=gpu)
                igg.gather_g(A, out, box=plane, dtype=dtype)
                assert torch.equal(out.cpu(), want[sl].to(odt)), (shape, dtype, "plane")
                box = ((1, ext[0]),) + (None,) * (nd - 1)
                out = torch.full(igg.selection_shape_g(A, box, 2), SENTINEL, dtype=odt)  # A_global on the CPU
                igg.gather_g(A, out, box=box, step=2, dtype=dtype)
                assert torch.equal(out, want[(slice(1, None, 2),) + (slice(None, None, 2),) * (nd - 1)].to(odt))
    assert GG._bufs == {}  # one rank: no staging, no transport
    igg.finalize_global_grid(finalize_MPI=False)


def test_gather_g_refuses_a_stream_capture(gpu):
    igg.init_global_grid(*N, quiet=True, init_MPI=False)
    A = torch.zeros(N, dtype=torch.float64, device=gpu)
    out = torch.full(N, SENTINEL, dtype=torch.float64, device=gpu)
    igg.gather_g(A, out)
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    mark = torch.zeros(1, device=gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(igg.IGGError, match="captured"):
            igg.gather_g(A, out)
        mark.add_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and mark.item() == 1.0  # refused before doing anything
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------- ranks sharing device 0
@pytest.mark.parametrize("nprocs,dtype,args", [
    (2, "float64", (2, 1, 1, 0, 2, 1)),
    (4, "float32", (2, 1, 2, 5, 4, 2)),   # periodic x and z, overlap 4: wrapping owned ranges
    (4, "float64", (2, 2, 1, 1, 3, 1)),
    (8, "float64", (2, 2, 2, 0, 2, 1)),
])
def test_multi_rank_on_one_device(gpu, nprocs, dtype, args):
    run_gather_ranks(nprocs, "gather", "gpu", dtype, *args, timeout=120)


def test_fused_model_without_sync_halo(gpu):
    # ranks share one GPU here: RCCL cannot, so the plain model's update_halo_ uses 'put' (as tests/test_multiprocess.py)
    run_gather_ranks(2, "fused", 24, 20, 64, 4, timeout=120, env_extra={"IGG_TRANSPORT": "put", "IGG_PUT_TIMEOUT": "20"})


@pytest.mark.multigpu
def test_two_ranks_on_two_devices_over_rccl(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: one rank per device over RCCL")
    run_gather_ranks(2, "gather", "mgpu", "float64", 2, 1, 1, 0, 2, 1, timeout=150)
