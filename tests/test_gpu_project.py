"""The projection kernels (csrc/kernels/project_kernels.hip) and ``project_g``
on the GPU (ops/reduce.py).

Fields are carved out of NaN padding and everything outside the box is NaN: a
mask that is off by one lane, a load one element early or late, gives NaN. The
destination is carved from NaN padding too and compared WHOLE. Oracle: the
same reduction of the box's values over the reduced axes in numpy (f64).
Sum-type ops run on integer-valued data (|x| <= 1024: exact in f64 whatever
the order) and are compared bitwise; max and min are always bitwise; for
random real data the bound per output cell is ``n * 2**-53 * sum|term|`` (``n``
the cell's number of terms) plus ``2**-53 * sum|term|`` for f64 products, which
round once, against ``math.fsum``.
"""
import math

import numpy as np
import pytest
import torch

import igg
from igg._native import native
from igg.ops import reduce as R
from tests.mp_worker_project import ONE, TWO, expected, keep_sets, same
from tests.test_gpu_reduce import DTYPES, NAN, PAD, _dense, _field
from tests.test_project_cpu import check_rank_outputs, run_project_ranks

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
IDENT = {"sum": 0.0, "sumsq": 0.0, "dot": 0.0, "sumsq_diff": 0.0, "max": -math.inf, "maxabs": -math.inf,
         "maxabs_diff": -math.inf, "min": math.inf}


@pytest.fixture(scope="module", autouse=True)
def _free_workspace():
    yield
    torch.cuda.synchronize()
    native.project_free_workspace()


def _oracle(op, x, red, y=None):
    return {"sum": lambda: x.sum(axis=red), "sumsq": lambda: (x * x).sum(axis=red), "max": lambda: x.max(axis=red),
            "min": lambda: x.min(axis=red), "maxabs": lambda: np.abs(x).max(axis=red),
            "dot": lambda: (x * y).sum(axis=red), "sumsq_diff": lambda: ((x - y) * (x - y)).sum(axis=red),
            "maxabs_diff": lambda: np.abs(x - y).max(axis=red)}[op]()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _plan(A, lo, hi, keep, B=None):
    kw = dict(strides_b=list(B.stride()), base_b=B.data_ptr()) if B is not None else {}
    return native.project_plan(list(A.shape), list(A.stride()), list(lo), list(hi), list(keep), A.element_size(),
                               A.data_ptr(), **kw)


def _project(op, A, lo, hi, keep, B=None, start=None, extent=None, travel=False):
    """One native projection of the box ``[lo, hi)`` into a destination carved
    from NaN padding: (values, flags or None) on the host; the padding must
    still be NaN afterwards."""
    own = [hi[d] - lo[d] for d in keep]
    extent = own if extent is None else list(extent)
    start = [0] * len(keep) if start is None else list(start)
    cells = int(np.prod(extent))
    n = cells * (2 if travel else 1)
    buf = torch.full((PAD + n + PAD,), NAN, dtype=torch.float64, device=A.device)
    dst = buf.data_ptr() + 8 * PAD
    native.project(R._OPS[op], A.data_ptr(), B.data_ptr() if B is not None else 0, list(A.shape), list(A.stride()),
                   list(B.stride()) if B is not None else [], list(lo), list(hi), list(keep), A.element_size(), dst,
                   dst + 8 * cells if travel else 0, start, extent, _dense(extent),
                   torch.cuda.current_stream().cuda_stream)
    h = buf.cpu().numpy()
    assert np.isnan(h[:PAD]).all() and np.isnan(h[PAD + n:]).all(), "the destination's padding was written"
    v = h[PAD:PAD + cells].reshape(extent)
    return v, (h[PAD + cells:PAD + n].reshape(extent) if travel else None)


def _check(op, A, x, lo, hi, keep, B=None, y=None, tag=""):
    red = tuple(d for d in range(A.dim()) if d not in keep)
    got, _ = _project(op, A, lo, hi, keep, B if op in TWO else None)
    want = _oracle(op, x, red, y)
    assert _bits_equal(got, want), (tag, tuple(A.shape), tuple(A.stride()), A.dtype, lo, hi, keep, op, got, want)


def _layout(inner, n_inner, others, pitch):
    """Shape and strides of a 3-D field whose axis ``inner`` is innermost in
    memory with ``n_inner`` cells in rows of ``pitch``; the other two axes
    (extents ``others``) keep their order."""
    rest = [d for d in range(3) if d != inner]
    shape, strides = [0] * 3, [0] * 3
    shape[inner], strides[inner] = n_inner, 1
    shape[rest[1]], strides[rest[1]] = others[1], pitch
    shape[rest[0]], strides[rest[0]] = others[0], pitch * others[1]
    return shape, strides


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_vector_residues_and_tile_edges(gpu, dtype, aligned):
    """Every keep-set with the inner axis kept and reduced; every residue of
    the 16-B vector at head and tail, rows at the 64-lane and the 256-lane
    edge; in an aligned pitch (vector loads) and an odd one (element loads; 9
    elements for the short rows)."""
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    for n2 in (6, 7, 9, 66, 127, 128, 129, 131, 257, 259):
        pitch = -(-n2 // vec) * vec + vec if aligned else (n2 + 2) | 1
        for inner in range(3):
            shape, strides = _layout(inner, n2, (5, 7), pitch)
            for lo2 in (0, 1, 2):
                lo, hi = [1, 1, 1], [n - 1 for n in shape]
                lo[inner], hi[inner] = lo2, n2 - lo2
                A, x = _field(gpu, shape, dtype, lo, hi, strides=strides, seed=1)
                B, y = _field(gpu, shape, dtype, lo, hi, strides=strides, seed=2)
                for keep in keep_sets(3):
                    p = _plan(A, lo, hi, keep, B)
                    assert p["path"] == ("vector" if aligned else "element"), p
                    assert p["family"] == (1 if inner in keep else 2) and _plan(A, lo, hi, keep)["path"] == p["path"]
                    for op in ("sum", "max", "min", "sumsq_diff"):
                        _check(op, A, x, lo, hi, keep, B, y)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_inputs_with_different_layouts_and_an_odd_base(gpu, dtype):
    lo, hi = (1, 1, 1), (5, 6, 8)
    A, x = _field(gpu, (6, 7, 9), dtype, lo, hi, seed=1)
    B, y = _field(gpu, (6, 7, 9), dtype, lo, hi, seed=2, strides=(1, 6, 42))
    for keep in keep_sets(3):
        assert _plan(A, lo, hi, keep, B)["path"] == "element"
        for op in TWO:
            _check(op, A, x, lo, hi, keep, B, y)
            _check(op, B, y, lo, hi, keep, A, x)  # the first input decides the memory order
    # a base one element off alignment: element loads; the same with both inputs off by one: still element loads
    A, x = _field(gpu, (5, 6, 8), dtype, lo, (4, 5, 7), off=1, seed=3)
    B, y = _field(gpu, (5, 6, 8), dtype, lo, (4, 5, 7), off=1, seed=4)
    for keep in keep_sets(3):
        assert _plan(A, lo, (4, 5, 7), keep)["path"] == "element"
        for op in ("sum", "min", "dot"):
            _check(op, A, x, lo, (4, 5, 7), keep, B, y)
    # a 2-D field, both layouts
    for strides in ((12, 1), (1, 8)):
        A, x = _field(gpu, (7, 11), dtype, (1, 2), (6, 10), strides=strides, seed=5)
        for keep in ((0,), (1,)):
            for op in ("sum", "max"):
                _check(op, A, x, (1, 2), (6, 10), keep)


@pytest.mark.parametrize("dtype", DTYPES)
def test_slicing_and_blocks(gpu, dtype):
    cap, smax = native.PROJECT_MAX_BLOCKS, native.PROJECT_MAX_SLICES
    ops = ("sum", "max", "dot")

    def run(shape, lo, hi, keeps, strides=None, **want):
        A, x = _field(gpu, shape, dtype, lo, hi, strides=strides, seed=1)
        B, y = _field(gpu, shape, dtype, lo, hi, strides=strides, seed=2)
        for keep in keeps:
            p = _plan(A, lo, hi, keep, B)
            for k, v in want.items():
                assert (v(p[k]) if callable(v) else p[k] == v), (k, p)
            for op in ops:
                _check(op, A, x, lo, hi, keep, B, y, tag=str(want))

    # a reduced range longer than one slice, in both families (slices at their cap, several indices each)
    run((1203, 4, 8), (1, 1, 1), (1202, 3, 7), [(2,)], family=1, slices=smax, reduced=lambda r: r > 4 * smax)
    run((6, 1203, 8), (1, 1, 1), (5, 1202, 7), [(0,)], family=2, slices=smax, reduced=lambda r: r > 4 * smax)
    # a reduced range shorter than the slice count the outputs ask for
    run((5, 6, 8), (1, 1, 1), (4, 5, 7), [(0, 2)], family=1, slices=4, reduced=4)
    run((5, 6, 8), (1, 1, 1), (4, 5, 7), [(0,)], family=2, slices=4, reduced=4)
    # more outputs than one workgroup holds: rows of several chunks, many rows
    run((3, 4, 2600), (0, 1, 1), (3, 3, 2599), [(2,), (0, 2), (1, 2)], family=1, chunks_per_row=lambda c: c > 1)
    run((3, 4, 2600), (0, 1, 1), (3, 3, 2599), [(0,), (1,), (0, 1)], family=2, chunks_per_row=lambda c: c > 1)
    run((70, 33, 9), (1, 1, 1), (69, 32, 8), keep_sets(3))
    run((70, 33, 9), (1, 1, 1), (69, 32, 8), keep_sets(3), strides=(33 * 12, 12, 1), path="vector")
    # one output cell; one reduced cell; a single element
    run((8, 9, 10), (3, 1, 1), (4, 8, 9), [(0,)], outputs=1, family=2)
    run((8, 9, 2600), (3, 4, 1), (4, 5, 2599), [(0, 1)], outputs=1, family=2, slices=lambda s: s > 1)
    run((8, 9, 10), (1, 3, 1), (7, 4, 9), [(0, 2)], reduced=1, slices=1, family=1)
    run((8, 9, 10), (1, 1, 3), (7, 8, 4), [(0, 1)], total=42, family=1)
    run((8, 9, 10), (3, 3, 3), (4, 4, 4), keep_sets(3), total=1, outputs=1)
    # plans at the block cap: the workgroups walk their units grid-stride
    run((192, 40, 64), (0, 0, 0), (192, 40, 64), keep_sets(3))
    if dtype == torch.float64:
        run((192, 48, 64), (0, 0, 0), (192, 48, 64), [(0, 1), (0, 2)], blocks=cap, block_units=lambda b: b > cap)
    else:
        run((192, 96, 64), (0, 0, 0), (192, 96, 64), [(0, 1), (0, 2)], blocks=cap, block_units=lambda b: b > cap)
    # a group that spans waves (LDS), one that is a wave, several groups per wave
    for n2, lanes in ((1100, 256), (200, 128 if dtype == torch.float64 else 64), (20, 16 if dtype == torch.float64 else 8)):
        run((6, 7, n2), (1, 1, 1), (5, 6, n2 - 1), [(0,), (1,), (0, 1)], family=2, lanes=lanes)


@pytest.mark.parametrize("dtype", DTYPES)
def test_destination_start_wrap_and_identity(gpu, dtype):
    shape, lo, hi = (8, 9, 12), (1, 2, 1), (7, 8, 11)
    A, x = _field(gpu, shape, dtype, lo, hi, seed=1)
    B, y = _field(gpu, shape, dtype, lo, hi, seed=2)
    for keep, start, extent in [((0,), (9,), (13,)), ((1,), (0,), (6,)), ((2,), (4,), (10,)), ((0, 2), (5, 15), (8, 17)),
                                ((0, 1), (0, 3), (6, 7)), ((1, 2), (2, 0), (9, 30))]:
        red = tuple(d for d in range(3) if d not in keep)
        idx = np.ix_(*((s + np.arange(hi[d] - lo[d])) % e for d, s, e in zip(keep, start, extent)))
        for op in ("sum", "max", "min", "maxabs_diff"):
            o2 = B if op in TWO else None
            want = np.full(extent, IDENT[op])
            want[idx] = _oracle(op, x, red, y)
            got, _ = _project(op, A, lo, hi, keep, o2, start, extent)
            assert _bits_equal(got, want), (keep, start, extent, op)
            if op in R._MAX:  # the travel form: the value with NaN as -inf (min: of -x), a flag
                got, flags = _project(op, A, lo, hi, keep, o2, start, extent, travel=True)
                want = np.full(extent, -math.inf)
                want[idx] = -_oracle(op, x, red, y) if op == "min" else _oracle(op, x, red, y)
                assert _bits_equal(got, want) and _bits_equal(flags, np.zeros(extent)), (keep, op, "travel")
        # nothing owned: the identity everywhere, no first stage
        got, _ = _project("sum", A, lo, (hi[0], lo[1], hi[2]), keep, None, start, extent)
        assert _bits_equal(got, np.zeros(extent))
        got, flags = _project("max", A, lo, (hi[0], lo[1], hi[2]), keep, None, start, extent, travel=True)
        assert _bits_equal(got, np.full(extent, -math.inf)) and _bits_equal(flags, np.zeros(extent))
    # a NaN travels as (-inf, flag) and only in its cell
    A[3, 4, 5] = NAN
    got, flags = _project("maxabs", A, lo, hi, (0,), None, (9,), (13,), travel=True)
    want_f = np.zeros(13)
    want_f[(9 + 2) % 13] = 1.0
    xx = np.abs(x.copy())
    xx[2, 2, 4] = -math.inf
    want = np.full(13, -math.inf)
    want[(9 + np.arange(6)) % 13] = xx.max(axis=(1, 2))
    assert _bits_equal(flags, want_f) and _bits_equal(got, want)
    with pytest.raises(igg.IGGError):  # the box does not fit the destination
        _project("sum", A, lo, hi, (0,), None, (0,), (5,))
    with pytest.raises(igg.IGGError):
        _project("sum", A, lo, hi, (0,), None, (6,), (6,))


@pytest.mark.parametrize("dtype", DTYPES)
def test_reproducible_and_within_the_derived_bound(gpu, dtype):
    shape = (40, 33, 70)
    lo, hi = (1, 1, 1), (39, 32, 69)
    g = torch.Generator().manual_seed(5)
    box = tuple(slice(a, b) for a, b in zip(lo, hi))
    A, _ = _field(gpu, shape, dtype, lo, hi, seed=1)
    B, _ = _field(gpu, shape, dtype, lo, hi, seed=2)
    xv = (torch.randn([b - a for a, b in zip(lo, hi)], generator=g, dtype=torch.float64) * 100).to(dtype)
    yv = (torch.randn([b - a for a, b in zip(lo, hi)], generator=g, dtype=torch.float64) * 100).to(dtype)
    A[box], B[box] = xv.to(gpu), yv.to(gpu)
    x, y = xv.double().numpy(), yv.double().numpy()
    for keep in keep_sets(3):
        red = tuple(d for d in range(3) if d not in keep)
        n = int(np.prod([x.shape[d] for d in red]))
        for op, t in (("sum", x), ("sumsq", x * x), ("dot", x * y)):
            o2 = B if op in TWO else None
            r1, _ = _project(op, A, lo, hi, keep, o2)
            r2, _ = _project(op, A, lo, hi, keep, o2)
            assert _bits_equal(r1, r2), (keep, op)  # run to run
            # (t holds the rounded f64 products; their rounding is the extra 2**-53 * sum|term|)
            rows = np.moveaxis(t, red, tuple(range(-len(red), 0))).reshape(r1.shape + (n,))
            exact = np.array([math.fsum(row) for row in rows.reshape(-1, n)]).reshape(r1.shape)
            mag = np.abs(rows).sum(axis=-1) * (1 + 4 * n * U53)  # (numpy's own sum of the magnitudes rounds)
            f32_exact = dtype == torch.float32 and op != "sum"  # f32 squares and products are exact in f64
            bound = n * U53 * mag + (0.0 if op == "sum" or f32_exact else U53 * mag)
            err = np.abs(r1 - exact)
            print(keep, op, dtype, "max err / bound", float((err / bound).max()))
            assert (err <= bound).all(), (keep, op, float(err.max()), float(bound.min()))
        r1, _ = _project("maxabs_diff", A, lo, hi, keep, B)
        assert _bits_equal(r1, np.abs(x - y).max(axis=red))


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_inf(gpu, dtype):
    shape, lo, hi = (10, 9, 70), (1, 1, 1), (9, 8, 69)
    for strides in (None, (1, 10, 90)):
        A, x = _field(gpu, shape, dtype, lo, hi, strides=strides, seed=7)
        B, y = _field(gpu, shape, dtype, lo, hi, strides=strides, seed=8)
        for where in ((1, 1, 1), (8, 7, 68), (4, 3, 33)):  # owned corners (head and tail lanes) and an inner cell
            saved = A[where].clone()
            A[where] = NAN
            for keep in keep_sets(3):
                red = tuple(d for d in range(3) if d not in keep)
                hit = np.zeros([hi[d] - lo[d] for d in keep], dtype=bool)
                hit[tuple(where[d] - lo[d] for d in keep)] = True
                for op in ONE + TWO:
                    got, _ = _project(op, A, lo, hi, keep, B if op in TWO else None)
                    want = _oracle(op, x, red, y)
                    assert (np.isnan(got) == hit).all(), (where, keep, op)  # exactly the line or plane that holds it
                    assert _bits_equal(got[~hit], want[~hit]), (where, keep, op)
            A[where] = saved
        A[2, 2, 2], B[2, 2, 2] = math.inf, math.inf  # inf alone is a value, inf - inf is a NaN term
        A[3, 3, 3] = -math.inf
        for keep in keep_sets(3):
            c2 = tuple(2 - lo[d] for d in keep)
            c3 = tuple(3 - lo[d] for d in keep)
            got, _ = _project("max", A, lo, hi, keep)
            assert got[c2] == math.inf and np.isfinite(got).sum() == got.size - 1
            got, _ = _project("min", A, lo, hi, keep)
            assert got[c3] == -math.inf and np.isfinite(got).sum() == got.size - 1
            got, _ = _project("sum", A, lo, hi, keep)
            assert got[c2] == math.inf and got[c3] == -math.inf and not np.isnan(got).any()
            for op in ("maxabs_diff", "sumsq_diff"):
                got, _ = _project(op, A, lo, hi, keep, B)
                assert math.isnan(got[c2]) and got[c3] == math.inf and np.isnan(got).sum() == 1


# ------------------------------------------------------------- the public API
def _nan_outside_owned(A):
    for d, (a, b) in enumerate(igg.owned_ranges(A)):
        sl = [slice(None)] * A.dim()
        sl[d] = slice(0, a)
        A[tuple(sl)] = NAN
        sl[d] = slice(b, None)
        A[tuple(sl)] = NAN


def _gathered(A):
    Gl = torch.full(igg.selection_shape_g(A), 777.0, dtype=A.dtype, device=A.device)
    igg.gather_g(A, Gl)
    return Gl.cpu().double()


@pytest.mark.parametrize("periods", [(0, 0, 0), (1, 1, 1), (1, 0, 1)])
def test_project_g_is_the_reduction_of_gather_g_on_one_rank(gpu, periods):
    n = (20, 9, 70)
    igg.init_global_grid(*n, periodx=periods[0], periody=periods[1], periodz=periods[2], overlapz=3, quiet=True,
                         init_MPI=False)
    g = torch.Generator().manual_seed(3)
    for shape, dtype in ((n, torch.float64), ((n[0] + 1, n[1], n[2]), torch.float32), (n[:2], torch.float64)):
        nd = len(shape)
        C = torch.randint(-1024, 1025, shape, generator=g).to(dtype)
        D = torch.randint(-1024, 1025, shape, generator=g).to(dtype)
        _nan_outside_owned(C)
        _nan_outside_owned(D)
        rev = tuple(reversed(range(nd)))
        for A, B in ((C.to(gpu), D.to(gpu)), (C.to(gpu).permute(rev).contiguous().permute(rev), D.to(gpu))):
            Fg, Gg = _gathered(A), _gathered(B)
            for keep in keep_sets(nd):
                red = tuple(d for d in range(nd) if d not in keep)
                for op in ONE + TWO + ("mean",):
                    r = igg.project_g(op, A, keep, other=B if op in TWO else None)
                    assert r.dtype == torch.float64 and r.device == A.device and r.is_contiguous()
                    assert tuple(r.shape) == tuple(Fg.shape[d] for d in keep)
                    assert same(r.cpu(), expected(op, Fg, Gg, red)), (shape, A.stride(), keep, op)
                loc = igg.project_g("min", A, keep, local=True)
                assert same(loc.cpu(), expected("min", Fg, Gg, red))  # one rank: local is global
    igg.finalize_global_grid(finalize_MPI=False)


@pytest.mark.parametrize("dtype", [torch.float16, torch.int32])
def test_other_dtypes_take_the_torch_path(gpu, dtype):
    igg.init_global_grid(10, 9, 12, periodx=1, periody=1, periodz=1, quiet=True, init_MPI=False)
    g = torch.Generator().manual_seed(3)
    A = torch.randint(-1024, 1025, (10, 9, 12), generator=g).to(dtype).to(gpu)
    B = torch.randint(-1024, 1025, (10, 9, 12), generator=g).to(dtype).to(gpu)
    ws = native.project_workspace_bytes()
    Fg, Gg = _gathered(A), _gathered(B)
    if dtype.is_floating_point:
        A[0], A[:, -1] = NAN, NAN  # planes nobody owns
    for keep in keep_sets(3):
        red = tuple(d for d in range(3) if d not in keep)
        for op in ONE + TWO + ("mean",):
            r = igg.project_g(op, A, keep, other=B if op in TWO else None)
            assert r.dtype == torch.float64 and r.is_cuda and same(r.cpu(), expected(op, Fg, Gg, red)), (keep, op)
    if dtype.is_floating_point:
        A[1, 1, 1] = NAN  # global cell (0, 0, 0)
        for op in ONE + TWO:
            r = igg.project_g(op, A, (0, 2), other=B if op in TWO else None).cpu()
            assert math.isnan(r[0, 0].item()) and int(torch.isnan(r).sum()) == 1, op
    assert native.project_workspace_bytes() == ws  # no kernel ran
    igg.finalize_global_grid(finalize_MPI=False)


def test_capture_replays_into_out(gpu):
    igg.init_global_grid(24, 20, 36, periodx=1, periodz=1, quiet=True, init_MPI=False)
    g = torch.Generator().manual_seed(9)
    A = torch.randint(-1024, 1025, (24, 20, 36), generator=g).to(torch.float64).to(gpu)
    _nan_outside_owned(A)
    prof = torch.zeros(22, dtype=torch.float64, device=gpu)
    zmax = torch.zeros(22, 20, dtype=torch.float64, device=gpu)
    igg.project_g("mean", A, 0, out=prof)  # the first calls size the workspace: never inside a capture
    igg.project_g("max", A, (0, 1), out=zmax)
    torch.cuda.synchronize()
    ws = native.project_workspace_bytes()
    assert ws > 0
    count = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]  # noqa: E731  (a host-side counter)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        n0 = count()
        igg.project_g("sum", A, 0, out=prof)
        igg.project_g("max", A, (0, 1), out=zmax)
        n1 = count()
    assert n1 == n0 and native.project_workspace_bytes() == ws  # no allocation, no workspace growth in the capture
    x = igg.owned_view(A).cpu().numpy().copy()
    for scale in (1.0, 2.0, -3.0):
        igg.owned_view(A).copy_(torch.from_numpy(x * scale).to(gpu))
        graph.replay()
        torch.cuda.synchronize()
        assert _bits_equal(prof.cpu().numpy(), (x * scale).sum(axis=(1, 2)))
        assert _bits_equal(zmax.cpu().numpy(), (x * scale).max(axis=2))
    igg.finalize_global_grid(finalize_MPI=False)
    assert native.project_workspace_bytes() == 0  # freed with the grid


def test_growing_the_workspace_inside_a_capture_fails(gpu):
    igg.init_global_grid(24, 20, 36, quiet=True, init_MPI=False)
    A = torch.zeros(24, 20, 36, dtype=torch.float64, device=gpu)
    igg.project_g("sum", A, 0)
    torch.cuda.synchronize()
    ws = native.project_workspace_bytes()
    big = torch.zeros(8, 300, 300, dtype=torch.float64, device=gpu)  # 90000 outputs: more partials than ever before
    out = torch.zeros(300, 300, dtype=torch.float64, device=gpu)
    mark = torch.zeros(1, device=gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(igg.IGGError, match="capture"):
            native.project(0, big.data_ptr(), 0, [8, 300, 300], list(big.stride()), [], [0, 0, 0], [8, 300, 300],
                           [1, 2], 8, out.data_ptr(), 0, [0, 0], [300, 300], [300, 1],
                           torch.cuda.current_stream().cuda_stream)
        mark.add_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert mark.item() == 1.0 and native.project_workspace_bytes() == ws
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------------------ the model
def test_fused_model_without_sync_halo(gpu, monkeypatch):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_VARIANT", "0")
    igg.init_global_grid(32, 32, 32, periodx=1, periody=1, periodz=1, quiet=True, init_MPI=False)
    a, f = Diffusion3D(dtype=torch.float64), Diffusion3D(dtype=torch.float64)
    assert f.set_fused(True)
    for _ in range(3):
        a.step()
        f.step()
    x = igg.owned_view(a.T).cpu().numpy()
    for keep in keep_sets(3):
        red = tuple(d for d in range(3) if d not in keep)
        for op in ("sum", "max", "mean"):
            ra, rf = igg.project_g(op, a.T, keep), igg.project_g(op, f.T, keep)  # the fused model's halos are stale
            assert same(ra.cpu(), rf.cpu()), (keep, op)
        assert _bits_equal(igg.project_g("max", f.T, keep).cpu().numpy(), x.max(axis=red))
    f.sync_halo()
    assert torch.equal(f.T, a.T)
    f.close()
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------- ranks sharing device 0
@pytest.mark.parametrize("nprocs,dtype,args", [
    (2, "float64", (2, 1, 1, 0, 2, 1)),
    (4, "float32", (2, 2, 1, 4, 2, 1)),  # periodic z
])
def test_multi_rank_on_one_device(gpu, nprocs, dtype, args):
    check_rank_outputs(run_project_ranks(nprocs, "gpu", dtype, *args, timeout=120))
