"""The reduction kernels (csrc/kernels/reduce_kernels.hip) and the global
reductions on the GPU (ops/reduce.py).

Fields are carved out of NaN padding and everything outside the reduced box is
NaN: a mask that is off by one lane, a load one element early or late, gives
NaN. Oracle: the same reduction of the box's values in numpy (f64). Sum-type
ops run on integer-valued data (|x| <= 1024: exact in f64 whatever the order)
and are compared bitwise; max, min and maxabs are always bitwise; for random
real data the bound is ``n * 2**-53 * sum|term|`` plus ``2**-53 * sum|term|``
for f64 products (they round once), against ``math.fsum``.
"""
import math

import numpy as np
import pytest
import torch

import igg
from igg._native import native
from igg.ops import reduce as R
from tests.test_reduce_cpu import ONE, TWO, U53, check_rank_outputs, run_reduce_ranks

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 64  # elements of NaN before and after a carved field (a multiple of every vector)
DTYPES = [torch.float32, torch.float64]


def _dense(shape):
    return [int(np.prod(shape[d + 1:])) for d in range(len(shape))]


def _field(gpu, shape, dtype, lo, hi, strides=None, off=0, seed=1):
    """(field, the box's values on the host): a tensor carved from a NaN buffer
    ``off`` elements past an aligned base, NaN everywhere but in ``[lo, hi)``,
    which holds integers of [-1024, 1024]."""
    strides = _dense(shape) if strides is None else list(strides)
    span = sum((n - 1) * s for n, s in zip(shape, strides)) + 1
    buf = torch.full((PAD + off + span + PAD,), NAN, dtype=dtype, device=gpu)
    A = buf.as_strided(list(shape), strides, PAD + off)
    g = torch.Generator().manual_seed(seed)
    vals = torch.randint(-1024, 1025, [h - l for l, h in zip(lo, hi)], generator=g).to(dtype)
    A[tuple(slice(l, h) for l, h in zip(lo, hi))] = vals.to(gpu)
    return A, vals.double().numpy()


def _oracle(op, x, y=None):
    return {"sum": lambda: x.sum(), "sumsq": lambda: (x * x).sum(), "max": lambda: x.max(), "min": lambda: x.min(),
            "maxabs": lambda: np.abs(x).max(), "dot": lambda: (x * y).sum(),
            "sumsq_diff": lambda: ((x - y) * (x - y)).sum(), "maxabs_diff": lambda: np.abs(x - y).max()}[op]()


def _same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _plan(A, lo, hi, B=None):
    kw = dict(strides_b=list(B.stride()), base_b=B.data_ptr()) if B is not None else {}
    return native.reduce_plan(list(A.shape), list(A.stride()), list(lo), list(hi), A.element_size(), A.data_ptr(), **kw)


def _box_reduce(op, A, lo, hi, B=None):
    """One job of the native reduction over the box ``[lo, hi)``."""
    out = torch.full((1,), 777.0, dtype=torch.float64, device=A.device)
    job = (A.data_ptr(), B.data_ptr() if B is not None else 0, list(A.shape), list(A.stride()),
           list(B.stride()) if B is not None else [], list(lo), list(hi))
    native.reduce(R._OPS[op], [job], A.element_size(), out.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()[0]


def _check_box(gpu, shape, dtype, lo, hi, path, ops=ONE + TWO, **kw):
    A, x = _field(gpu, shape, dtype, lo, hi, seed=1, **kw)
    B, y = _field(gpu, shape, dtype, lo, hi, seed=2, **kw)
    assert _plan(A, lo, hi)["path"] == path and _plan(A, lo, hi, B)["path"] == path, (shape, lo, hi, _plan(A, lo, hi))
    for op in ops:
        got = _box_reduce(op, A, lo, hi, B if op in TWO else None)
        want = _oracle(op, x, y)
        print(path, tuple(shape), dtype, lo, hi, op, got, want)
        assert _same_bits(got, want), (path, shape, dtype, lo, hi, op, got, want)


@pytest.fixture(scope="module", autouse=True)
def _free_workspace():
    yield
    torch.cuda.synchronize()
    native.reduce_free_workspace()


# ------------------------------------------------------------------- the paths
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_path_head_and_tail_masks(gpu, dtype):
    """Every residue of the 16-B vector at head and tail, rows at the 64-lane
    pass edge and the 256-lane tile edge; rows in an aligned pitch."""
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    for n2 in (6, 7, 9, 66, 127, 128, 129, 131, 257, 259):
        pitch = -(-n2 // vec) * vec + vec
        for lo2 in (0, 1, 2):
            _check_box(gpu, (5, 7, n2), dtype, (1, 1, lo2), (4, 6, n2 - lo2), "rows",
                       ops=("sum", "max", "min", "sumsq_diff"), strides=(7 * pitch, pitch, 1))
    # long rows: more than four tiles along a row
    n2 = 4 * 256 * vec + 3
    _check_box(gpu, (3, 3, n2), dtype, (1, 0, 1), (3, 2, n2 - 2), "rows", ops=("sum", "maxabs"),
               strides=(3 * (n2 + vec - 3), n2 + vec - 3, 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_path_many_rows_and_block_cap(gpu, dtype):
    es = torch.empty(0, dtype=dtype).element_size()
    # more rows than one pass of the grid; dense, its 9-element pitch is no multiple of 16 B
    _check_box(gpu, (70, 33, 9), dtype, (1, 1, 1), (69, 32, 8), "element")
    _check_box(gpu, (70, 33, 9), dtype, (1, 1, 1), (69, 32, 8), "rows", strides=(33 * 12, 12, 1))
    lo = (1, 1, 1)
    _check_box(gpu, (192, 192, 64), dtype, lo, (191, 191, 63), "rows", ops=("sum", "max", "dot"))
    # past the block cap: 192 x 192 x 64 is with f64; f32 rows are half as many loads, so a taller box
    shape = (192, 192, 64) if dtype == torch.float64 else (400, 192, 64)
    hi = tuple(n - 1 for n in shape)
    p = native.reduce_plan(list(shape), _dense(shape), list(lo), list(hi), es, 1 << 20)
    assert p["path"] == "rows" and p["blocks"] == native.REDUCE_MAX_BLOCKS
    assert p["tiles"] > native.REDUCE_UNROLL * p["blocks"]
    if dtype == torch.float32:
        _check_box(gpu, shape, dtype, lo, hi, "rows", ops=("sum", "max"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_path(gpu, dtype):
    for n in (1, 3, 255, 257, 4099, (1 << 20) + 3):
        _check_box(gpu, (n,), dtype, (0,), (n,), "flat", ops=("sum", "sumsq", "max", "min", "maxabs_diff"))
    _check_box(gpu, (9, 10, 11), dtype, (0, 0, 0), (9, 10, 11), "flat")  # a fully owned dense array
    _check_box(gpu, (9, 10, 11), dtype, (2, 0, 0), (8, 10, 11), "flat")  # whole planes
    for off in (1, 2, 3):  # a flat run starts at any element
        _check_box(gpu, (1031,), dtype, (0,), (1031,), "flat", ops=("sum", "max"), off=off)
        _check_box(gpu, (1031,), dtype, (off,), (1031 - off,), "flat", ops=("sum", "min"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_element_path(gpu, dtype):
    # a permuted tensor with stride0 == 1
    _check_box(gpu, (6, 7, 9), dtype, (1, 1, 1), (5, 6, 8), "element", strides=(1, 6, 42))
    _check_box(gpu, (6, 7, 9), dtype, (0, 0, 0), (6, 7, 9), "element", strides=(1, 6, 42))
    # a row pitch that is no multiple of 16 B
    _check_box(gpu, (5, 6, 7), dtype, (1, 1, 1), (4, 5, 6), "element", strides=(42, 7, 1))
    # a base one element off alignment
    _check_box(gpu, (5, 6, 8), dtype, (1, 1, 1), (4, 5, 7), "element", off=1)
    # a strided innermost dimension, rows longer than a tile
    _check_box(gpu, (3, 700), dtype, (0, 1), (3, 699), "element", strides=(1400, 2), ops=("sum", "max"))


def test_two_inputs_with_different_layouts(gpu):
    lo, hi = (1, 1, 1), (5, 6, 8)
    A, x = _field(gpu, (6, 7, 9), torch.float64, lo, hi, seed=1)
    B, y = _field(gpu, (6, 7, 9), torch.float64, lo, hi, seed=2, strides=(1, 6, 42))
    assert _plan(A, lo, hi, B)["path"] == "element"
    for op in TWO:
        assert _same_bits(_box_reduce(op, A, lo, hi, B), _oracle(op, x, y)), op


# ------------------------------------------------------------- the public API
def _grid_field(gpu, shape, dtype, seed=1, ints=True):
    """A field of the initialised grid carved from NaN padding: values in the
    owned box, NaN in every plane this rank does not own."""
    rng = igg.owned_ranges(torch.empty(shape, device="meta"))
    lo, hi = [r[0] for r in rng], [r[1] for r in rng]
    A, x = _field(gpu, shape, dtype, lo, hi, seed=seed)
    if not ints:
        g = torch.Generator().manual_seed(seed)
        v = (torch.randn(x.shape, generator=g, dtype=torch.float64) * 100).to(dtype)
        A[tuple(slice(l, h) for l, h in zip(lo, hi))] = v.to(gpu)
        x = v.double().numpy()
    return A, x


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_op_and_shape_through_the_api(gpu, dtype):
    igg.init_global_grid(10, 9, 12, periodx=1, periody=1, periodz=1, overlapy=3, quiet=True, init_MPI=False)
    for shape in [(10, 9, 12), (11, 9, 12), (10, 8, 12), (10, 9, 13), (10, 9), (11, 9), (10,), (11,)]:
        A, x = _grid_field(gpu, shape, dtype, 1)
        B, y = _grid_field(gpu, shape, dtype, 2)
        for op in ONE + TWO:
            r = igg.reduce_g(op, A, other=B if op in TWO else None)
            assert r.dtype == torch.float64 and r.dim() == 0 and r.device == A.device
            assert _same_bits(r.item(), _oracle(op, x, y)), (shape, op)
        assert _same_bits(igg.norm_g(A).item(), np.sqrt(_oracle("sumsq", x)))
        assert _same_bits(igg.norm_diff_g(A, B).item(), np.sqrt(_oracle("sumsq_diff", x, y)))
        assert _same_bits(igg.mean_g(A).item(), x.sum() / x.size)  # one periodic rank: the owned cells are the grid
        assert _same_bits(igg.dot_g(A, B).item(), _oracle("dot", x, y))
        assert igg.max_g(A).item() == x.max() and igg.min_g(A).item() == x.min()
        assert igg.maxabs_g(A).item() == np.abs(x).max() and igg.sum_g(A).item() == x.sum()
        assert igg.maxabs_diff_g(A, B).item() == np.abs(x - y).max()
    igg.finalize_global_grid(finalize_MPI=False)


def test_batches(gpu):
    igg.init_global_grid(10, 9, 12, periodx=1, periodz=1, quiet=True, init_MPI=False)
    shapes = [(10, 9, 12), (11, 9, 12), (10, 8, 13)]
    fs = [_grid_field(gpu, s, torch.float32, k) for k, s in enumerate(shapes)]
    gs = [_grid_field(gpu, s, torch.float32, 10 + k) for k, s in enumerate(shapes)]
    for op in ("sum", "max", "sumsq_diff"):
        r = igg.reduce_g(op, *(f[0] for f in fs), other=tuple(g[0] for g in gs) if op in TWO else None)
        assert r.shape == (3,) and r.dtype == torch.float64
        for k in range(3):
            assert _same_bits(r[k].item(), _oracle(op, fs[k][1], gs[k][1])), (op, k)
    # 40 fields: more than one launch; vector and element jobs mixed (a permuted field every seventh)
    many = []
    for k in range(40):
        s = shapes[k % 3]
        if k % 7 == 3:
            rng = igg.owned_ranges(torch.empty(s, device="meta"))
            many.append(_field(gpu, s, torch.float32, [r[0] for r in rng], [r[1] for r in rng], seed=k,
                               strides=(1, s[0], s[0] * s[1])))
        else:
            many.append(_grid_field(gpu, s, torch.float32, k))
    out = torch.full((40,), 777.0, dtype=torch.float64, device=gpu)
    assert igg.reduce_g("sumsq", *(f[0] for f in many), out=out) is out
    want = [_oracle("sumsq", f[1]) for f in many]
    assert out.tolist() == want
    r = igg.reduce_g("min", *(f[0] for f in many))
    assert r.tolist() == [f[1].min() for f in many]
    igg.finalize_global_grid(finalize_MPI=False)


@pytest.mark.parametrize("dtype", [torch.float16, torch.int32])
def test_other_dtypes_take_the_torch_path(gpu, dtype):
    igg.init_global_grid(10, 9, 12, periodx=1, periody=1, periodz=1, quiet=True, init_MPI=False)
    g = torch.Generator().manual_seed(3)
    A = torch.randint(-1024, 1025, (10, 9, 12), generator=g).to(dtype).to(gpu)
    B = torch.randint(-1024, 1025, (10, 9, 12), generator=g).to(dtype).to(gpu)
    x, y = (igg.owned_view(t).cpu().double().numpy() for t in (A, B))
    if dtype.is_floating_point:
        A[0], A[:, -1] = NAN, NAN  # planes nobody owns
    for op in ONE + TWO:
        r = igg.reduce_g(op, A, other=B if op in TWO else None)
        assert r.dtype == torch.float64 and r.is_cuda and _same_bits(r.item(), _oracle(op, x, y)), op
    if dtype.is_floating_point:
        A[1, 1, 1] = NAN
        for op in ONE + TWO:
            assert math.isnan(igg.reduce_g(op, A, other=B if op in TWO else None).item()), op
    igg.finalize_global_grid(finalize_MPI=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reproducible_and_within_the_derived_bound(gpu, dtype):
    igg.init_global_grid(40, 33, 70, periodx=1, periodz=1, quiet=True, init_MPI=False)
    A, x = _grid_field(gpu, (40, 33, 70), dtype, 5, ints=False)
    B, y = _grid_field(gpu, (40, 33, 70), dtype, 6, ints=False)
    xs, ys = x.flatten().tolist(), y.flatten().tolist()
    terms = {"sum": xs, "sumsq": [a * a for a in xs], "dot": [a * b for a, b in zip(xs, ys)],
             "sumsq_diff": [(a - b) * (a - b) for a, b in zip(xs, ys)]}
    for op in ONE + TWO:
        other = B if op in TWO else None
        r1 = igg.reduce_g(op, A, other=other).item()
        r2 = igg.reduce_g(op, A, other=other).item()
        loc = igg.reduce_g(op, A, other=other, local=True).item()
        assert _same_bits(r1, r2) and _same_bits(r1, loc), op  # run to run; one rank: local is global
        if op in terms:
            t = terms[op]
            mag = math.fsum(abs(v) for v in t)
            exact = dtype == torch.float32 and op != "sum"  # f32 squares and products are exact in f64
            bound = len(t) * U53 * mag + (0.0 if op == "sum" or exact else U53 * mag)
            print(op, dtype, "err", abs(r1 - math.fsum(t)), "bound", bound)
            assert abs(r1 - math.fsum(t)) <= bound, (op, r1, math.fsum(t), bound)
        else:
            assert _same_bits(r1, _oracle(op, x, y)), op
    igg.finalize_global_grid(finalize_MPI=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_rule(gpu, dtype):
    igg.init_global_grid(10, 9, 70, periodx=1, periody=1, periodz=1, quiet=True, init_MPI=False)
    A, x = _grid_field(gpu, (10, 9, 70), dtype, 7)  # every plane nobody owns is NaN already
    B, y = _grid_field(gpu, (10, 9, 70), dtype, 8)
    for op in ONE + TWO:
        assert _same_bits(igg.reduce_g(op, A, other=B if op in TWO else None).item(), _oracle(op, x, y)), op
    for where in ((1, 1, 1), (8, 7, 68), (4, 3, 33)):  # owned corners (head and tail lanes) and an inner cell
        keep = A[where].clone()
        A[where] = NAN
        for op in ONE + TWO:
            assert math.isnan(igg.reduce_g(op, A, other=B if op in TWO else None).item()), (op, where)
        assert math.isnan(igg.mean_g(A).item()) and math.isnan(igg.norm_g(A).item())
        A[where] = keep
    A[2, 2, 2], B[2, 2, 2] = math.inf, math.inf  # inf alone is a value, inf - inf is a NaN term
    assert igg.max_g(A).item() == math.inf and math.isnan(igg.maxabs_diff_g(A, B).item())
    assert igg.sum_g(A).item() == math.inf and math.isnan(igg.reduce_g("sumsq_diff", A, other=B).item())
    A[3, 3, 3] = -math.inf
    assert igg.min_g(A).item() == -math.inf and igg.maxabs_g(A).item() == math.inf and math.isnan(igg.sum_g(A).item())
    igg.finalize_global_grid(finalize_MPI=False)


def test_capture_replays_into_out(gpu):
    igg.init_global_grid(24, 20, 36, periodx=1, periodz=1, quiet=True, init_MPI=False)
    A, x = _grid_field(gpu, (24, 20, 36), torch.float64, 9)
    B, y = _grid_field(gpu, (25, 20, 36), torch.float64, 10)
    r = torch.zeros(2, dtype=torch.float64, device=gpu)
    m = torch.zeros((), dtype=torch.float64, device=gpu)
    igg.reduce_g("sumsq", A, B, out=r)  # the first call allocates the workspace: never inside a capture
    torch.cuda.synchronize()
    ws = native.reduce_workspace_bytes()
    assert ws > 0
    count = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]  # noqa: E731  (a host-side counter)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        n0 = count()
        igg.reduce_g("sumsq", A, B, out=r)
        igg.reduce_g("maxabs", A, out=m)
        n1 = count()
    assert n1 == n0 and native.reduce_workspace_bytes() == ws  # no allocation, no workspace growth in the capture
    for scale in (1.0, 2.0, -3.0):
        owned = igg.owned_view(A)
        owned.copy_(torch.from_numpy(x * scale).to(gpu))
        g.replay()
        torch.cuda.synchronize()
        assert r.tolist() == [(x * scale * x * scale).sum(), (y * y).sum()]
        assert m.item() == np.abs(x * scale).max()
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------------------ the model
def _host_residual(m):
    return (igg.owned_view(m.T).cpu().double() - igg.owned_view(m.T2).cpu().double()).abs().max().item()


def test_residual_plain_and_fused(gpu, monkeypatch):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_VARIANT", "0")
    igg.init_global_grid(32, 32, 32, periodx=1, periody=1, periodz=1, quiet=True, init_MPI=False)
    a, f = Diffusion3D(dtype=torch.float64), Diffusion3D(dtype=torch.float64)
    assert f.set_fused(True)
    for _ in range(3):
        a.step()
        f.step()
        ra, rf = a.residual(), f.residual()  # the fused model's halos are stale: not owned, not read
        assert ra.is_cuda and ra.dim() == 0 and ra.dtype == torch.float64
        assert ra.item() == rf.item() == _host_residual(a) and ra.item() > 0
    f.sync_halo()
    assert torch.equal(f.T, a.T)
    f.close()
    igg.finalize_global_grid(finalize_MPI=False)


@pytest.mark.parametrize("mode", ["single", "twostep", "graph", "twostep+graph"])
def test_run_until_is_run_bitwise(gpu, monkeypatch, mode):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_VARIANT", "11")
    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "1" if "twostep" in mode else "0")
    igg.init_global_grid(40, 36, 128, quiet=True, init_MPI=False)
    a, b = Diffusion3D(dtype=torch.float64), Diffusion3D(dtype=torch.float64)
    assert a._two_step_now() == ("twostep" in mode)
    if "graph" in mode:
        a.capture(4)
        b.capture(4)
    a.run(23)
    steps, res = b.run_until(0.0, 23)
    torch.cuda.synchronize()
    assert steps == 23 and torch.equal(a.T, b.T)
    assert res == _host_residual(b) and res > 0  # the change over the last single step
    # stops below tol, at a block end, before max_steps
    steps2, res2 = b.run_until(res * 0.9, 4000, check_every=9)
    assert 0 < steps2 < 4000 and steps2 % 9 == 0 and res2 < res * 0.9 and res2 == _host_residual(b)
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------- ranks sharing device 0
@pytest.mark.parametrize("nprocs,dtype,args", [
    (2, "float64", (2, 1, 1, 0, 2, 1)),
    (4, "float32", (2, 2, 1, 4, 2, 1)),  # periodic z
])
def test_multi_rank_on_one_device(gpu, nprocs, dtype, args):
    check_rank_outputs(run_reduce_ranks(nprocs, "gpu", dtype, *args, timeout=120))
