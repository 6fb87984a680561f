"""The spread kernels (csrc/kernels/spread_kernels.hip) at descriptor level and
spread_g / SpreadPlan / Source on the GPU (parallel/spread_g.py).

Plan tests: the GPU plan (count kernel, cumsum, fill kernel, stable sort,
unique_consecutive) against ``native.host_spread_plan``, equal as tensors.
Apply tests: every field is carved out of a NaN buffer with odd pitches, and
the WHOLE allocation is compared, bit for bit, with what
``native.host_spread_apply`` leaves in a host copy for the same descriptors - a
stray store or a lane one cell off shows. The multi-rank tests compare with the
Python oracle of tests/mp_worker_spread_g.py.
"""
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import igg
from igg._native import native
from igg.parallel.gather_g import _segments
from igg.parallel.scatter_g import _runs
from igg.parallel.spread_g import SpreadPlan, _build_plan
from tests._mp import MAX_TIMEOUT, ROOT
from tests.mp_worker_sample_g import extents, global_values, local_of_global
from tests.mp_worker_spread_g import bits_of
from tests.test_spread_g_cpu import run_spread_ranks

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 32  # elements around a carved box
DTYPES = {"float64": torch.float64, "float32": torch.float32}
F64 = torch.float64


def _one_rank_table(shape):
    return [(m, 0, m, [[0, m, 0]], [[0, m, 0]]) for m in shape]


def _grid_table(n, o, dims, per, coords):
    table = []
    for d in range(len(n)):
        E = dims[d] * (n[d] - o) + (0 if per[d] else o)
        table.append((E, per[d], n[d], [list(s) for s in _segments(n[d], o, dims[d], per[d], coords[d], n[d])],
                      [list(r) for r in _runs(n[d], o, dims[d], per[d], coords[d], n[d])]))
    return table


def _plans(gpu, shape, table, P, mode, *, transposed=False, max_blocks=0):
    """The host plan and the GPU plan of the same points."""
    nd = len(shape)
    P = P.reshape(-1, nd)
    Ph = P.t().contiguous().t() if transposed else P.contiguous()
    Pd = Ph.t().contiguous().to(gpu).t() if transposed else Ph.to(gpu)
    assert Pd.stride() == Ph.stride()
    pts = lambda Q: (Q, int(Q.shape[0]), int(Q.stride(0)), int(Q.stride(1)))  # noqa: E731
    like = lambda device: torch.empty(1, dtype=F64, device=device).expand(shape)  # noqa: E731 (the shape alone counts)
    host = _build_plan(like("cpu"), table, pts(Ph), mode)
    dev = _build_plan(like(gpu), table, pts(Pd), mode, max_blocks)
    return host, dev


def _assert_same_plan(host: SpreadPlan, dev: SpreadPlan):
    assert (host.ncells, host.nentries) == (dev.ncells, dev.nentries)
    for name in ("cells", "start", "point", "weight"):
        h, d = getattr(host, name), getattr(dev, name)
        assert d.is_cuda and h.dtype == d.dtype and h.shape == d.shape, name
        assert torch.equal(bits_of(h), bits_of(d)), name


def _points(shape, npts, seed, lo=0.0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(npts, len(shape), generator=g, dtype=F64)
    P = lo + u * (scale * torch.tensor([m - 1.0 for m in shape], dtype=F64) - lo)
    P[::5] = (P[::5] * 4).round() / 4  # zero factors
    P[::7] = P[::7].round()
    return P


# ------------------------------------------------------------------- the plan
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("npts", [1, 2, 255, 256, 257, 100003])
def test_plan_kernels_equal_the_host_plan_as_tensors(gpu, npts, mode):
    for shape in ((5, 6, 7), (9, 130), (130,)):
        table = _one_rank_table(shape)
        P = _points(shape, npts, npts + len(shape))
        P[-1] = NAN
        for transposed, max_blocks in ((False, 0), (True, 3)):  # a capped grid: the grid-stride tail runs
            host, dev = _plans(gpu, shape, table, P, mode, transposed=transposed, max_blocks=max_blocks)
            _assert_same_plan(host, dev)
        assert host.nentries > 0 or npts == 1
        if npts == 100003:
            assert npts > 3 * native.SPREAD_BLOCK and host.ncells <= int(np.prod(shape))


@pytest.mark.parametrize("mode", [0, 1])
def test_plan_of_periodic_and_fake_multi_rank_tables(gpu, mode):
    """Tables of ranks that do not exist, a self-periodic rank (two copies of
    a plane) and a local range of three runs."""
    n, o = (9, 8, 7), 2
    pts = torch.cat([_points((30, 8, 12), 400, 11, lo=-3.0),
                     torch.tensor([[NAN, 1.0, 1.0], [1.0, 99.0, 1.0], [1.0, -1.0, 1.0], [math.inf, 0.0, 0.0]],
                                  dtype=F64)])
    sizes = []
    for dims, per, coords in (((1, 1, 1), (1, 0, 1), (0, 0, 0)), ((2, 1, 2), (0, 0, 1), (1, 0, 0)),
                              ((2, 1, 2), (0, 0, 1), (0, 0, 1)), ((3, 1, 1), (1, 0, 0), (2, 0, 0))):
        host, dev = _plans(gpu, n, _grid_table(n, o, dims, per, coords), pts, mode, max_blocks=1)
        _assert_same_plan(host, dev)
        sizes.append(host.nentries)
    assert min(sizes) > 0 and len(set(sizes)) > 1
    table = _grid_table((9, 6), 4, (1, 1), (1, 0), (0, 0))  # period 5 in 9 planes: three runs
    assert len(table[0][4]) == 3
    host, dev = _plans(gpu, (9, 6), table, _points((40, 6), 300, 5, lo=-20.0), mode, transposed=True)
    _assert_same_plan(host, dev)
    if mode == 0:
        single = _build_plan(torch.empty(9, 6, dtype=F64), table, (torch.tensor([[1.5, 2.0]], dtype=F64), 1, 2, 1), 0)
        assert single.cells.tolist() == [2 * 6 + 2, 3 * 6 + 2, 7 * 6 + 2, 8 * 6 + 2]
        assert single.weight.tolist() == [0.5] * 4


def test_bad_descriptors_are_refused(gpu):
    P = torch.zeros(4, 2, dtype=F64, device=gpu)
    cnt = torch.zeros(4, dtype=torch.int64, device=gpu)
    good = _one_rank_table((5, 6))

    def count(table, copies=0, npts=4):
        native.spread_count(table, copies, P.data_ptr(), 2, 1, npts, cnt.data_ptr())

    count(good)
    for bad in (lambda: count([(5, 0, 5, [[0, 6, 0]], [[0, 5, 0]]), good[1]]),  # a segment past the extent
                lambda: count([(9, 0, 5, [[0, 5, 0]], [[1, 5, 0]]), good[1]]),  # a run past the field
                lambda: count([(5, 0, 5, [[0, 5, 0]], [[0, 5, 1]]), good[1]]),  # a run past the extent
                lambda: count([(5, 0, 5, [], [[0, 1, 0]] * 5), good[1]]),       # five runs
                lambda: count([(1, 0, 5, [], []), good[1]]),                    # E < 2
                lambda: count(good, copies=2),
                lambda: count(good, npts=-1),
                lambda: count(good + good)):
        with pytest.raises(igg.IGGError):
            bad()
    A = torch.zeros(5, 6, dtype=F64, device=gpu)
    plan = _build_plan(A, good, (P, 4, 2, 1), 0)
    V = torch.ones(4, dtype=F64, device=gpu)

    def apply(shape=(5, 6), fields=None, elem=8, ncells=None, v_ps=1):
        native.spread_apply(list(shape), fields or [(A.data_ptr(), [6, 1])], elem,
                            plan.ncells if ncells is None else ncells, plan.cells.data_ptr(), plan.start.data_ptr(),
                            plan.point.data_ptr(), plan.weight.data_ptr(), V.data_ptr(), 0, v_ps)

    for bad in (lambda: apply(fields=[(A.data_ptr(), [6, -1])]), lambda: apply(fields=[(A.data_ptr(), [6])]),
                lambda: apply(fields=[(0, [6, 1])]), lambda: apply(elem=2), lambda: apply(ncells=-1),
                lambda: apply(shape=(5, 0)), lambda: apply(shape=(5, 6, 1, 1)), lambda: apply(v_ps=-1)):
        with pytest.raises(igg.IGGError):
            bad()
    torch.cuda.synchronize()
    assert not A.any()
    apply()
    torch.cuda.synchronize()
    assert A[0, 0].item() == 4.0 and int((A != 0).sum()) == 1


# ------------------------------------------------------------------- the apply
def _strides(shape, order, pitch):
    st, run = [0] * len(shape), 1
    for k, ax in enumerate(reversed(order)):
        st[ax] = run
        run = run * shape[ax] + (pitch if k < len(shape) - 1 else 0)
    return st


def _carve(shape, dtype, order, pitch, seed):
    st = _strides(shape, order, pitch)
    span = sum((n - 1) * s for n, s in zip(shape, st)) + 1
    buf = torch.full((PAD + span + PAD,), NAN, dtype=dtype)
    g = torch.Generator().manual_seed(seed)
    v = (torch.randn(tuple(shape), generator=g, dtype=F64) * 8).to(dtype)
    flat = v.view(-1)
    special = [0.0, -0.0, math.inf, -math.inf, torch.finfo(dtype).max, 1.0 / 3.0]
    k = min(len(special), flat.numel())
    flat[:k] = torch.tensor(special[:k], dtype=dtype)
    buf.as_strided(shape, st, PAD).copy_(v)
    return buf, st


def _check_apply(gpu, shape, dtype, P, *, order=None, pitch=3, nf=1, max_blocks=0, seed=1, mode=0, rows=None):
    """native.spread_apply against native.host_spread_apply on the same plan
    and descriptors: the whole allocations, NaN padding included."""
    nd = len(shape)
    dt = DTYPES[dtype]
    eb = torch.empty(0, dtype=dt).element_size()
    order = list(order or range(nd))
    P = P.reshape(-1, nd).contiguous()
    npts = int(P.shape[0])
    plan = _build_plan(torch.empty(shape, dtype=dt), _one_rank_table(shape), (P, npts, nd, 1), mode)
    fields = [_carve(shape, dt, order, pitch + 2 * k, seed + k) for k in range(nf)]
    dev = [buf.to(gpu) for buf, _st in fields]
    g = torch.Generator().manual_seed(seed + 100)
    V = torch.randn(nf, npts, generator=g, dtype=F64) * 3.0
    Vd = V.to(gpu)
    dplan = [t.to(gpu) for t in (plan.cells, plan.start, plan.point, plan.weight)]
    hplan = [plan.cells, plan.start, plan.point, plan.weight]
    row_h = row_d = 0
    extra = ()
    if rows is not None:  # (row, nrows): V is then a table of rows
        V = torch.randn(rows[1], nf, npts, generator=g, dtype=F64)
        Vd = V.to(gpu)
        rh = torch.tensor([rows[0]], dtype=torch.int64)
        rd = rh.to(gpu)
        row_h, row_d, extra = rh.data_ptr(), rd.data_ptr(), (rows[1], nf * npts)
    native.host_spread_apply(list(shape), [(buf.data_ptr() + eb * PAD, st) for buf, st in fields], eb, plan.ncells,
                             *[t.data_ptr() for t in hplan], V.data_ptr(), npts, 1, row_h, *extra)
    native.spread_apply(list(shape), [(d.data_ptr() + eb * PAD, st) for d, (_b, st) in zip(dev, fields)], eb,
                        plan.ncells, *[t.data_ptr() for t in dplan], Vd.data_ptr(), npts, 1, row_d, *extra,
                        stream=torch.cuda.current_stream().cuda_stream, max_blocks=max_blocks)
    torch.cuda.synchronize()
    for k, (d, (h, _st)) in enumerate(zip(dev, fields)):
        got, want = bits_of(d), bits_of(h)
        assert torch.equal(got, want), (f"field {k}: {int((got != want).sum())} of {want.numel()} words differ, first "
                                        f"at {int((got != want).nonzero()[0])} (the field starts at {PAD})")
    return plan


def _lattice(shape):
    return torch.from_numpy(np.indices(shape).reshape(len(shape), -1).T.astype(np.float64)).contiguous()


SHAPES = [(5, 6, 7), (3, 4, 130), (6, 7), (4, 130), (7,), (130,)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_apply_layouts_pitches_and_point_sets(gpu, shape, dtype):
    nd = len(shape)
    orders = [list(range(nd))] + [list(p) for p in list(itertools.permutations(range(nd)))[1:][-2:]]
    sets = {
        "lattice": _lattice(shape),
        "random": _points(shape, 257, 3),
        "one cell": 1.0 + torch.rand(65, nd, generator=torch.Generator().manual_seed(4), dtype=F64),
    }
    for order, (name, P), mode in itertools.product(orders, sets.items(), (0, 1)):
        plan = _check_apply(gpu, shape, dtype, P, order=order, mode=mode)
        if name == "lattice":
            assert plan.ncells == plan.nentries == int(np.prod(shape))
        if name == "one cell":
            assert plan.ncells == 2 ** nd and plan.nentries == 65 * 2 ** nd


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("ncells", [1, 255, 256, 257, 700])
def test_apply_touched_cell_counts_and_the_grid_stride_tail(gpu, ncells, dtype):
    shape = (5, 6, 130)
    P = _lattice(shape)[torch.randperm(5 * 6 * 130, generator=torch.Generator().manual_seed(ncells))[:ncells]]
    plan = _check_apply(gpu, shape, dtype, P)
    assert plan.ncells == ncells
    # a lowered block cap: 2 blocks of 256 lanes walk 700 cells, the last pass is partial
    _check_apply(gpu, shape, dtype, P, max_blocks=2, order=[2, 0, 1])
    _check_apply(gpu, (9, 130), dtype, _lattice((9, 130))[:ncells], max_blocks=1)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_apply_segment_lengths_1_2_and_1000(gpu, dtype):
    shape = (6, 7)
    P = torch.cat([torch.tensor([[1.0, 1.0]], dtype=F64), torch.tensor([[2.0, 3.0]], dtype=F64).repeat(2, 1),
                   torch.tensor([[4.0, 5.0]], dtype=F64).repeat(1000, 1), torch.tensor([[3.5, 0.5]], dtype=F64)])
    P = P[torch.randperm(P.shape[0], generator=torch.Generator().manual_seed(1))]
    plan = _check_apply(gpu, shape, dtype, P, nf=2)
    lens = (plan.start[1:] - plan.start[:-1]).tolist()
    assert sorted(lens) == [1, 1, 1, 1, 1, 2, 1000]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("nf", [1, 2, 5, 8, 9])
def test_apply_several_fields_in_one_call(gpu, nf, dtype):
    for shape in ((5, 6, 7), (6, 7), (130,)):
        _check_apply(gpu, shape, dtype, _points(shape, 300, 7), nf=nf, order=list(range(len(shape)))[::-1])


def test_apply_row_counter(gpu):
    shape = (5, 6, 7)
    P = _points(shape, 100, 9)
    for row in (0, 2, 3, 4, -1):  # rows 3 and beyond of 3, and a negative one: nothing is done
        _check_apply(gpu, shape, "float64", P, nf=2, rows=(row, 3))


def test_offsets_past_2_to_the_31(gpu):
    """A (3, 4, 5) f32 view whose outer stride is 2^31 + 8 elements over an
    unfilled 17 GiB allocation: only the touched cells are written."""
    outer = 2 ** 31 + 8
    need = (2 * outer + 3 * 7 + 5) * 4
    free, _total = torch.cuda.mem_get_info()
    if free < need + (1 << 30):
        pytest.skip(f"the device has {free >> 30} GiB free, the view spans {need >> 30} GiB")
    big = torch.empty(2 * outer + 3 * 7 + 5, dtype=torch.float32, device=gpu)
    view = big.as_strided((3, 4, 5), (outer, 7, 1))
    dense = torch.randn(3, 4, 5, generator=torch.Generator().manual_seed(12), dtype=torch.float32)
    view.copy_(dense.to(gpu))
    P = torch.tensor([[0.0, 0.0, 0.0], [2.0, 3.0, 4.0], [1.5, 2.5, 3.5], [1.0, 0.25, 2.0], [2.0, 3.0, 4.0]], dtype=F64)
    V = torch.tensor([1.0, 2.0, 8.0, 4.0, 0.5], dtype=F64)
    plan = _build_plan(dense, _one_rank_table((3, 4, 5)), (P, 5, 3, 1), 0)
    assert plan.ncells == 11  # 1 + 8 (one of them the twice-hit corner) + 2
    ptrs = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    hp = [plan.cells, plan.start, plan.point, plan.weight]
    native.host_spread_apply([3, 4, 5], [(dense.data_ptr(), list(dense.stride()))], 4, plan.ncells, *ptrs(hp),
                             V.data_ptr(), 0, 1)
    dp = [t.to(gpu) for t in hp]
    Vd = V.to(gpu)
    native.spread_apply([3, 4, 5], [(view.data_ptr(), list(view.stride()))], 4, plan.ncells, *ptrs(dp), Vd.data_ptr(),
                        0, 1, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(bits_of(view), bits_of(dense))
    del big, view


def test_a_shape_of_more_than_2_to_the_31_cells_takes_the_64_bit_split(gpu):
    """A (2^17, 2^17) view with strides (1, 0) over 2^17 elements: 2^34 cells,
    so a cell's linear index needs the 64-bit division; a handful of cells in
    different rows is touched."""
    n = 2 ** 17
    host = torch.zeros(n, dtype=F64)
    dev = host.to(gpu)
    rows = [0, 1, 70000, n - 1, 40001]
    P = torch.tensor([[float(r), float(c)] for r, c in zip(rows, [0, n - 1, 65536, 3, 99999])], dtype=F64)
    V = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0], dtype=F64)
    plan = _build_plan(host.as_strided((n, n), (1, 0)), _one_rank_table((n, n)), (P, 5, 2, 1), 0)
    assert plan.ncells == 5 and int(plan.cells.max()) > 2 ** 33
    ptrs = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    hp = [plan.cells, plan.start, plan.point, plan.weight]
    native.host_spread_apply([n, n], [(host.data_ptr(), [1, 0])], 8, 5, *ptrs(hp), V.data_ptr(), 0, 1)
    dp = [t.to(gpu) for t in hp]
    Vd = V.to(gpu)
    native.spread_apply([n, n], [(dev.data_ptr(), [1, 0])], 8, 5, *ptrs(dp), Vd.data_ptr(), 0, 1,
                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(bits_of(dev), bits_of(host)) and host[rows].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    # the same plan from the plan kernels
    _h, d = _plans(gpu, (n, n), _one_rank_table((n, n)), P, 0)
    assert torch.equal(d.cells.cpu(), plan.cells)


# ------------------------------------------------- spread_g, SpreadPlan, Source
def _periodic_case(gpu, dtype=torch.float64):
    igg.init_global_grid(9, 8, 7, periodx=1, periody=1, periodz=1, quiet=True, init_MPI=False)
    E = extents(igg.get_global_grid(), (9, 8, 7))
    C = [local_of_global(global_values(E, s, dtype), (9, 8, 7)) for s in (1, 2)]
    C[1] = C[1].permute(2, 0, 1).contiguous().permute(1, 2, 0)
    G = [c.to(gpu) for c in C]
    assert G[1].stride() == C[1].stride()
    return E, C, G


def _some_points(E, k, npts=500):
    g = torch.Generator().manual_seed(20 + k)
    u = (torch.rand(npts, 3, generator=g, dtype=F64) * 4 - 1.5) * torch.tensor(E, dtype=F64)
    u[:7] = torch.tensor([[0.0, 0.0, 0.0], [E[0], E[1], E[2]], [-0.5, 1.0, 2.0], [E[0] - 1.0, 0.25, E[2] - 0.5],
                          [NAN, 0.0, 0.0], [0.0, math.inf, 0.0], [3.0, 3.0, 3.0]], dtype=F64)
    k = npts // 5
    u[2 * k:3 * k] = u[k:2 * k]  # cells shared by two points
    return u


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_one_periodic_rank_gpu_against_cpu_bitwise(gpu, dtype):
    E, C, G = _periodic_case(gpu, dtype)
    P = _some_points(E, 0)
    V = torch.randn(2, 500, generator=torch.Generator().manual_seed(3), dtype=F64)
    for copies in ("all", "owner"):
        c = [x.clone() for x in C]
        g = [x.clone() for x in G]
        igg.spread_g(tuple(c), P, V, copies=copies)
        igg.spread_g(tuple(g), P.to(gpu), V.to(gpu), copies=copies)
        for x, y in zip(c, g):
            assert y.stride() == x.stride() and torch.equal(bits_of(x), bits_of(y)), copies
        one = G[1].clone()
        igg.spread_g(one, P.to(gpu).t().contiguous().t(), V[1].to(gpu), copies=copies)
        assert torch.equal(bits_of(one), bits_of(c[1]))
        if copies == "all":
            h = g[0].clone()
            igg.update_halo_(h)
            assert torch.equal(bits_of(h), bits_of(g[0]))
        _assert_same_plan(igg.spread_plan(C[0], P, copies=copies), igg.spread_plan(G[0], P.to(gpu), copies=copies))
    igg.finalize_global_grid(finalize_MPI=False)


def test_plan_apply_and_source_inject_captured(gpu):
    from igg.parallel import halo as HL

    E, C, G = _periodic_case(gpu)
    P = _some_points(E, 5, 200)
    W = torch.randn(4, 2, 200, generator=torch.Generator().manual_seed(8), dtype=F64)
    Wd = W.to(gpu)
    # plan.apply: V is rewritten between the replays
    plan = igg.spread_plan(tuple(G), P.to(gpu))
    V = torch.zeros(2, 200, dtype=F64, device=gpu)
    g = [x.clone() for x in G]
    graph = HL.capture_graph(lambda: plan.apply(V, *g), "SpreadPlan.apply", uses_halo=False)
    for x, y in zip(g, G):
        x.copy_(y)
    c = [x.clone() for x in C]
    for k in range(3):
        V.copy_(Wd[k])
        graph.replay()
        igg.spread_g(tuple(c), P, W[k])
    torch.cuda.synchronize()
    for x, y in zip(c, g):
        assert torch.equal(bits_of(x), bits_of(y))
    # Source.inject: a replay advances the row; W is rewritten between replays; nothing past the last row
    src = igg.Source(tuple(G), P.to(gpu), Wd, copies="owner")
    g = [x.clone() for x in G]
    graph = HL.capture_graph(lambda: src.inject(*g), "Source.inject", uses_halo=False)
    src.reset()
    for x, y in zip(g, G):
        x.copy_(y)
    c = [x.clone() for x in C]
    for k in range(6):
        if k == 2:
            Wd[2].mul_(-3.0)
            W[2].mul_(-3.0)
        graph.replay()
        if k < 4:
            igg.spread_g(tuple(c), P, W[k], copies="owner")
    torch.cuda.synchronize()
    for x, y in zip(c, g):
        assert torch.equal(bits_of(x), bits_of(y))
    assert int(src._count.item()) == 6
    igg.finalize_global_grid(finalize_MPI=False)


def test_spread_g_is_refused_inside_a_capture_and_wrong_devices(gpu):
    igg.init_global_grid(9, 8, 7, quiet=True, init_MPI=False)
    P = torch.zeros(3, 3, dtype=F64, device=gpu)
    V = torch.ones(3, dtype=F64, device=gpu)
    A = torch.ones(9, 8, 7, dtype=F64, device=gpu)
    with pytest.raises(igg.IGGError, match="float32 or float64"):
        igg.spread_g(A.half(), P, V)
    with pytest.raises(igg.IGGError, match="`P`"):
        igg.spread_g(A, P.cpu(), V)
    with pytest.raises(igg.IGGError, match="`V`"):
        igg.spread_g(A, P, V.cpu())
    igg.spread_g(A, P[:0], V[:0])
    seen = []

    def record():
        A.add_(1.0)
        for call in (lambda: igg.spread_g(A, P, V), lambda: igg.spread_plan(A, P), lambda: igg.Source(A, P, V[None])):
            try:
                call()
            except igg.IGGError as e:
                seen.append(str(e))

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        record()
    torch.cuda.synchronize()
    assert len(seen) == 3 and all("capture" in s for s in seen)
    assert (A == 1.0).all()  # nothing ran, neither the capture's add nor a spread
    igg.finalize_global_grid(finalize_MPI=False)


def test_autograd_sample_g_on_the_gpu_equals_the_cpu(gpu):
    E, C, G = _periodic_case(gpu)
    P = _some_points(E, 7, 120)
    P = P[torch.isfinite(P).all(dim=1)]
    c = torch.randn(2, P.shape[0], generator=torch.Generator().manual_seed(4), dtype=F64)
    grads = []
    for fields, dev in ((C, "cpu"), (G, gpu)):
        leaves = [x.clone().requires_grad_(True) for x in fields]
        out = igg.autograd.sample_g(tuple(leaves), P.to(dev))
        (out * c.to(dev)).sum().backward()
        grads.append([x.grad for x in leaves])
    for x, y in zip(*grads):
        assert y.is_cuda and torch.equal(bits_of(x), bits_of(y)) and x.abs().sum() > 0
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------- ranks sharing device 0
@pytest.mark.parametrize("nprocs,scenario,dtype,args", [
    (2, "all", "float64", (2, 1, 1, 0, 2, 3, 0)),
    (4, "all", "float32", (2, 2, 1, 3, 3, 2, 1)),
    (8, "all", "float64", (2, 2, 2, 5, 2, 3, 0)),
    (4, "owner", "float64", (2, 2, 1, 3, 2, 3, 0)),
    (2, "autograd", "float64", (2, 1, 1, 2, 2, 2)),
])
def test_multi_rank_on_one_device(gpu, nprocs, scenario, dtype, args):
    run_spread_ranks(nprocs, scenario, "gpu", dtype, *args, timeout=120, env_extra={"IGG_TRANSPORT": "staged"})


@pytest.mark.multigpu
def test_two_ranks_on_two_devices_over_rccl(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: one rank per device over RCCL")
    run_spread_ranks(2, "all", "mgpu", "float64", 2, 1, 1, 1, 2, 3, 0, timeout=150,
                     env_extra={"IGG_TRANSPORT": "rccl"})


def test_example_acoustic_shot_on_the_gpu(gpu):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "acoustic_shot.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=MAX_TIMEOUT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "the field stayed halo-consistent" in r.stdout
