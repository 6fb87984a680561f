"""The widening lattice copy (select_widen_kernel, csrc/kernels/select_kernels.hip)
at descriptor level and scatter_g on the GPU (parallel/scatter_g.py).

Kernel tests, in the manner of tests/test_gpu_gather_g.py: the f32 source
lattice is carved out of a NaN buffer with NaN between the selected elements,
the f64 destination is a box inside a buffer filled with a sentinel, and the
WHOLE destination allocation is compared byte for byte with torch's CPU
``.to(torch.float64)`` of the same lattice (for NaN values the positions are
compared): a stray store, a lane one element off or a load that let a
neighbour's NaN in shows up. Widening is exact, so every comparison is bitwise.
"""
import math

import numpy as np
import pytest
import torch

import igg
from igg._native import native
from igg.parallel import gather_g as GG
from tests.test_gather_g_cpu import N
from tests.test_scatter_g_cpu import SENTINEL, one_rank_cases, run_scatter_ranks

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 64  # elements around a carved lattice: the buffers' bases stay 256-B aligned
GIB = 1 << 30


def _span(c, s):
    return sum((n - 1) * k for n, k in zip(c, s)) + 1 if all(c) else 1


def _values(c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1024, 1025, tuple(c), generator=g).to(torch.float32)


class Job:
    """One descriptor with its buffers: the f32 source on the host and the
    device, the f64 destination and what it must hold afterwards."""

    def __init__(self, gpu, c, S, T, src_off=0, dst_off=0, vals=None, seed=1):
        self.c, self.S, self.T = list(c), list(S), list(T)
        vals = _values(c, seed) if vals is None else vals
        src = torch.full((PAD + src_off + _span(c, S) + PAD,), NAN, dtype=torch.float32)
        src.as_strided(self.c, self.S, PAD + src_off).copy_(vals)
        self.want = torch.full((PAD + dst_off + _span(c, T) + PAD,), float(SENTINEL), dtype=torch.float64)
        self.want.as_strided(self.c, self.T, PAD + dst_off).copy_(vals.to(torch.float64))  # the CPU's conversion
        self.src = src.to(gpu)
        self.dst = torch.full_like(self.want, float(SENTINEL), device=gpu)
        self.desc = (self.src.data_ptr() + 4 * (PAD + src_off), self.dst.data_ptr() + 8 * (PAD + dst_off), self.c,
                     self.S, self.T)
        self.plan = native.select_plan(self.c, self.S, self.T)

    def check(self, tag=""):
        got = self.dst.cpu()
        gn, wn = torch.isnan(got), torch.isnan(self.want)
        same = torch.equal(gn, wn) and torch.equal(got.view(torch.int64)[~gn], self.want.view(torch.int64)[~wn])
        if not same:
            bad = ((got.view(torch.int64) != self.want.view(torch.int64)) & ~(gn & wn)).nonzero().flatten()[:6]
            raise AssertionError(f"{tag} c={self.c} S={self.S} T={self.T}: {len(bad)}+ differences, first at "
                                 f"{[int(b) - PAD for b in bad]}: got {got[bad].tolist()}, "
                                 f"want {self.want[bad].tolist()}")


def _launch(*jobs):
    native.select_widen([j.desc for j in jobs], torch.cuda.current_stream().cuda_stream)


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
    """Every source residue (0..3 elements past a 16-B boundary) and
    destination residue (0..1) of the row start; 3 x 5 rows in pitches that
    are no multiple of 16 B (odd element counts), so the rows of one job also
    start at every residue."""
    ps, pt = (n + 2) | 1, (n + 4) | 1
    assert (ps * 4) % 16 and (pt * 8) % 16
    for rs in (0, 1, 2, 3):
        for rd in (0, 1):
            _run(gpu, (3, 5, n), (5 * ps + 2, ps, 1), (5 * pt + 3, pt, 1), "rows", src_off=rs, dst_off=rd,
                 seed=n + 8 * rs + rd)


def test_rows_path_many_short_rows(gpu):
    """12 000 rows of 7: more rows than one pass of the grid holds waves."""
    j = _run(gpu, (120, 100, 7), (100 * 9 + 1, 9, 1), (100 * 11, 11, 1), "rows", src_off=3, dst_off=1)
    assert j.plan["rows"] == 12000 and j.plan["blocks"] == native.SELECT_MAX_BLOCKS
    assert j.plan["rows"] > 4 * j.plan["blocks"]


def test_strides_along_outer_axes_stay_on_the_rows_path(gpu):
    shape = (9, 14, 70)
    d = _dense(shape)
    c = (5, 5, 70)  # every 2nd and 3rd row of the destination field
    assert native.select_plan(c, _dense(c), [2 * d[0], 3 * d[1], 1])["path"] == "rows"
    _run(gpu, c, _dense(c), (2 * d[0], 3 * d[1], 1), "rows")
    _run(gpu, c, (5 * 75 + 1, 75, 1), (2 * d[0], 3 * d[1], 1), "rows", src_off=2, dst_off=1)


# ---------------------------------------------------------------- element path
def test_element_path_permuted_boxed_and_large(gpu):
    n0, n1, n2 = 7, 9, 13
    _run(gpu, (n0, n1, n2), (1, n0, n0 * n1), _dense((n0, n1, n2)), "element")          # a permuted source
    _run(gpu, (n0, n1, n2), _dense((n0, n1, n2)), (1, n0, n0 * n1), "element", src_off=1)  # a permuted destination
    # a box in a larger permuted array
    _run(gpu, (n0, n1, n2), _dense((n0, n1, n2)), (1, n0 + 3, (n0 + 3) * (n1 + 2)), "element", src_off=3, dst_off=1)
    # more elements than one pass of the grid holds lanes
    c = (70, 90, 100)
    j = _run(gpu, c, _dense(c), (90 * 200, 200, 2), "element")
    assert j.plan["blocks"] == native.SELECT_MAX_BLOCKS and j.plan["total"] > 256 * j.plan["blocks"]


# ----------------------------------------------------------------- the batch
def test_batch_of_eight_jobs_in_one_launch(gpu):
    assert native.SELECT_MAX_JOBS >= 8
    jobs = [
        Job(gpu, (3, 5, 66), (5 * 71, 71, 1), (5 * 69, 69, 1), src_off=1, dst_off=1, seed=1),
        Job(gpu, (1, 1, 1), (0, 0, 1), (0, 0, 1), src_off=2, seed=2),                     # one element
        Job(gpu, (4, 0, 9), (90, 9, 1), (90, 9, 1), seed=3),                              # empty
        Job(gpu, (2, 7, 31), (7 * 31, 31, 1), (7 * 64, 64, 2), seed=4),                   # element
        Job(gpu, (1, 300, 5), (0, 5, 1), (0, 7, 1), dst_off=1, seed=5),
        Job(gpu, (6, 4, 12), (48, 12, 1), (1, 6, 24), seed=6),                            # permuted: element
        Job(gpu, (1, 1, 1027), (0, 0, 1), (0, 0, 1), src_off=3, dst_off=1, seed=7),
        Job(gpu, (9, 2, 4), (2 * 5, 5, 1), (2 * 6, 6, 1), src_off=1, seed=8),
    ]
    paths = [j.plan["path"] for j in jobs]
    assert paths.count("rows") >= 4 and paths.count("element") >= 2
    assert jobs[2].plan["blocks"] == 0 and jobs[1].plan["total"] == 1
    _launch(*jobs)
    for k, j in enumerate(jobs):
        j.check(f"job {k}")
    # more jobs than one launch takes
    many = [Job(gpu, (2, 3, 5 + k), (3 * 40, 40, 1), (3 * 37, 37, 1), src_off=k & 3, dst_off=k & 1, seed=k)
            for k in range(native.SELECT_MAX_JOBS + 3)]
    _launch(*many)
    for k, j in enumerate(many):
        j.check(f"many {k}")


def test_alignment_and_null_pointers_are_refused(gpu):
    j = Job(gpu, (2, 3, 9), (27, 9, 1), (27, 9, 1))
    s, d, c, S, T = j.desc
    stream = torch.cuda.current_stream().cuda_stream
    for bad in ((s + 2, d, c, S, T), (s, d + 4, c, S, T), (0, d, c, S, T), (s, 0, c, S, T)):
        with pytest.raises(igg.IGGError):
            native.select_widen([bad], stream)
    torch.cuda.synchronize()
    assert (j.dst == SENTINEL).all()


# ------------------------------------------------------------------ the values
def test_widening_is_exact_for_every_kind_of_value(gpu):
    special = [0.0, -0.0, 1.0, -1024.0, math.inf, -math.inf, NAN,
               2.0 ** -149, -(2.0 ** -149), 1e-40, -1e-40,   # f32 subnormals: normal doubles
               2.0 ** -126, (2.0 - 2.0 ** -23) * 2.0 ** 127,   # the smallest normal, FLT_MAX
               -(2.0 - 2.0 ** -23) * 2.0 ** 127, 1.0 + 2.0 ** -23, 1.0 / 3.0]
    sp32 = torch.tensor(special, dtype=torch.float32)
    assert float(sp32[7]) == 2.0 ** -149 and 0.0 < float(sp32[9]) < 2.0 ** -126  # subnormal, not flushed
    n = 67
    vals = _values((2, 3, n), 9)
    flat = vals.view(-1)
    flat[:len(special)] = sp32
    flat[-len(special):] = sp32  # in a tail as well
    for c, S, T, path, offs in (((2, 3, n), (3 * 71, 71, 1), (3 * 69, 69, 1), "rows", (1, 1)),
                                ((2, 3, n), (3 * n, n, 1), (3 * 142, 142, 2), "element", (0, 0))):
        j = _run(gpu, c, S, T, path, src_off=offs[0], dst_off=offs[1], vals=vals)
        out = j.dst.cpu().as_strided(list(c), list(T), PAD + offs[1]).reshape(-1)
        for block in (out[:len(special)], out[-len(special):]):
            for k, v in enumerate(sp32.tolist()):  # (tolist: the exact double of each float)
                if math.isnan(v):
                    assert math.isnan(block[k].item()), (path, k)
                else:
                    assert np.float64(v).tobytes() == block[k].numpy().tobytes(), (path, v, float(block[k]))
        assert math.copysign(1.0, out[1].item()) == -1.0 and out[1].item() == 0.0  # -0 keeps its sign


# -------------------------------------------------------------- 64-bit offsets
def test_destination_stride_past_2_31_elements(gpu):
    """c = (2, 2, 2) with a destination stride of 2^31 doubles (16 GiB): the
    64-bit kernel, on the rows path and, with a permuted source, on the element
    path. The sentinel is written only around the eight target cells and only
    those neighbourhoods are compared."""
    c, T = (2, 2, 2), (1 << 31, 16, 1)
    n = PAD + 1 + _span(c, T) + PAD
    free = torch.cuda.mem_get_info()[0]
    if free < n * 8 + 4 * GIB:
        pytest.skip(f"needs {n * 8 / GIB:.1f} GiB + 4 GiB of device memory, {free / GIB:.1f} GiB are free")
    dst = torch.empty(n, dtype=torch.float64, device=gpu)
    try:
        base = PAD + 1
        cells = [base + i0 * T[0] + i1 * T[1] + i2 for i0 in range(2) for i1 in range(2) for i2 in range(2)]
        vals = _values(c, 5)
        for S, path in (((4, 2, 1), "rows"), ((1, 2, 4), "element")):
            plan = native.select_plan(c, S, T)
            assert plan["index_bits"] == 64 and plan["path"] == path, plan
            src = torch.full((PAD + 8 + PAD,), NAN, dtype=torch.float32)
            src.as_strided(c, S, PAD).copy_(vals)
            src = src.to(gpu)
            for a in cells:
                dst[a - 8:a + 9] = float(SENTINEL)
            native.select_widen([(src.data_ptr() + 4 * PAD, dst.data_ptr() + 8 * base, list(c), list(S), list(T))],
                                torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            flat = vals.to(torch.float64).reshape(-1)
            for k, a in enumerate(cells):
                want = torch.full((17,), float(SENTINEL), dtype=torch.float64)
                want[8] = flat[k]
                if k % 2 == 0:
                    want[9] = flat[k + 1]  # the row's second cell
                else:
                    want[7] = flat[k - 1]
                assert torch.equal(dst[a - 8:a + 9].cpu(), want), (path, k, dst[a - 8:a + 9].tolist())
    finally:
        del dst
        torch.cuda.empty_cache()


# ------------------------------------------------------------ scatter_g, 1 rank
@pytest.mark.parametrize("periods", [(0, 0, 0), (1, 1, 1), (1, 0, 1)])
def test_scatter_g_on_one_rank(gpu, periods):
    n = (20, 9, 70)
    igg.init_global_grid(*n, periodx=periods[0], periody=periods[1], periodz=periods[2], overlapz=3, quiet=True,
                         init_MPI=False)
    one_rank_cases(torch.device(gpu), n, rng_seed=3)
    assert GG._bufs == {}  # one rank: no staging, no transport
    igg.finalize_global_grid(finalize_MPI=False)


def test_scatter_g_refuses_a_stream_capture(gpu):
    igg.init_global_grid(*N, quiet=True, init_MPI=False)
    A = torch.full(N, float(SENTINEL), dtype=torch.float64, device=gpu)
    Gl = torch.ones(N, dtype=torch.float64, device=gpu)
    igg.scatter_g(Gl, A)
    assert (A == 1.0).all()
    A.fill_(float(SENTINEL))
    torch.cuda.synchronize()
    mark = torch.zeros(1, device=gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(igg.IGGError, match="captured"):
            igg.scatter_g(Gl, A)
        mark.add_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert (A == SENTINEL).all() and mark.item() == 1.0  # refused before doing anything
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------- ranks sharing device 0
@pytest.mark.parametrize("nprocs,dtype,args", [
    (2, "float64", (2, 1, 1, 0, 2, 1)),
    (4, "float32", (2, 1, 2, 5, 4, 2)),   # periodic x and z, overlap 4: local ranges that wrap
    (4, "float64", (2, 2, 1, 1, 3, 1)),
    (8, "float64", (2, 2, 2, 0, 2, 1)),
])
def test_multi_rank_on_one_device(gpu, nprocs, dtype, args):
    # ranks share one GPU: RCCL cannot, scatter_g stages through the host; so does the worker's update_halo_
    run_scatter_ranks(nprocs, "scatter", "gpu", dtype, *args, timeout=120, env_extra={"IGG_TRANSPORT": "staged"})


@pytest.mark.multigpu
def test_two_ranks_on_two_devices_over_rccl(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: one rank per device over RCCL")
    run_scatter_ranks(2, "scatter", "mgpu", "float64", 2, 1, 1, 0, 2, 1, timeout=150,
                      env_extra={"IGG_TRANSPORT": "rccl"})
