"""The sampling kernel (sample_kernel, csrc/kernels/sample_kernels.hip) at
descriptor level and sample_g / Recorder on the GPU (parallel/sample_g.py).

Kernel tests: every field is carved out of a NaN buffer with odd pitches (what
lies between the rows is NaN too: a load one element off lets it in), the
output out of a NaN buffer as well, and the WHOLE output allocation is
compared, bit for bit, with what ``native.host_sample`` writes into a host
copy for the same descriptors - a stray store or a lane one point off shows.
The multi-rank tests compare with the oracle of tests/mp_worker_sample_g.py,
``host_sample`` on the directly built global array with the single segment
``[0, E)``: that is the one-rank result for the same global field.
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
from tests._mp import MAX_TIMEOUT, ROOT
from tests.mp_worker_sample_g import NAN_BITS, bits, extents, global_values, local_of_global
from tests.test_sample_g_cpu import run_sample_ranks

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 32  # elements around a carved box
DTYPES = {"float64": torch.float64, "float32": torch.float32}


def _strides(shape, order, pitch):
    """Dense-with-gaps strides: ``order`` lists the axes from the outermost to
    the innermost in memory; each level's extent is padded by ``pitch``."""
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
    v = (torch.randn(tuple(shape), generator=g, dtype=torch.float64) * 8).to(dtype)
    flat = v.view(-1)
    special = [0.0, -0.0, math.inf, -math.inf, torch.finfo(dtype).tiny / 4, torch.finfo(dtype).max, 1.0 / 3.0]
    k = min(len(special), flat.numel())
    flat[:k] = torch.tensor(special[:k], dtype=dtype)
    buf.as_strided(shape, st, PAD).copy_(v)
    return buf, st


def _one_rank_table(shape):
    return [(m, 0, m, [[0, m, 0]]) for m in shape]


def _check(gpu, shape, dtype, P, *, order=None, pitch=3, nf=1, table=None, me0=True, transposed=False,
           max_blocks=0, seed=1):
    """native.sample against native.host_sample on the same descriptors: the
    whole output allocations, NaN padding included. Returns the host's bits."""
    nd = len(shape)
    dt = DTYPES[dtype]
    eb = torch.empty(0, dtype=dt).element_size()
    order = list(order or range(nd))
    table = table or _one_rank_table(shape)
    fields = [_carve(shape, dt, order, pitch + 2 * k, seed + k) for k in range(nf)]
    dev = [buf.to(gpu) for buf, _st in fields]
    P = P.reshape(-1, nd)
    npts = int(P.shape[0])
    Ph = P.t().contiguous().t() if transposed else P.contiguous()
    Pd = Ph.t().contiguous().to(gpu).t() if transposed else Ph.to(gpu)
    hout = torch.full((PAD + nf * npts + PAD,), NAN, dtype=torch.float64)
    dout = hout.to(gpu)
    native.host_sample(table, [(buf.data_ptr() + eb * PAD, st) for buf, st in fields], eb, Ph.data_ptr(),
                       Ph.stride(0), Ph.stride(1), npts, hout.data_ptr() + 8 * PAD, npts, me0)
    native.sample(table, [(d.data_ptr() + eb * PAD, st) for d, (_b, st) in zip(dev, fields)], eb, Pd.data_ptr(),
                  Pd.stride(0), Pd.stride(1), npts, dout.data_ptr() + 8 * PAD, npts, me0,
                  stream=torch.cuda.current_stream().cuda_stream, max_blocks=max_blocks)
    torch.cuda.synchronize()
    got, want = bits(dout), bits(hout)
    assert torch.equal(got, want), (f"{int((got != want).sum())} of {want.numel()} words differ, first at "
                                    f"{int((got != want).nonzero()[0])} (the output starts at {PAD})")
    return want[PAD:PAD + nf * npts].view(nf, npts)


def _random_points(shape, npts, seed, lo=0.0):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(npts, len(shape), generator=g, dtype=torch.float64)
    return lo + u * (torch.tensor([m - 1.0 for m in shape], dtype=torch.float64) - lo)


def _lattice(shape):
    return torch.from_numpy(np.indices(shape).reshape(len(shape), -1).T.astype(np.float64)).contiguous()


SHAPES = [(5, 6, 7), (3, 4, 130), (6, 7), (4, 130), (7,), (130,)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_layouts_pitches_and_point_sets(gpu, shape, dtype):
    nd = len(shape)
    orders = [list(range(nd))] + [list(p) for p in list(itertools.permutations(range(nd)))[1:][-2:]]
    sets = {
        "lattice": _lattice(shape),
        "interior": _random_points(shape, 257, 3),
        "invalid": torch.tensor([[NAN] * nd, [-0.5] * nd, [math.inf] * nd, [1e9] * nd, [-math.inf] * nd],
                                dtype=torch.float64)[:, :nd],
        "one cell": 1.0 + torch.rand(65, nd, generator=torch.Generator().manual_seed(4), dtype=torch.float64),
    }
    for order, (name, P) in itertools.product(orders, sets.items()):
        for transposed in (False, True):
            got = _check(gpu, shape, dtype, P, order=order, transposed=transposed)
            if name == "invalid":
                assert (got == NAN_BITS).all()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("npts", [1, 63, 64, 65, 257, 100003])
def test_point_counts_and_the_grid_stride_tail(gpu, npts, dtype):
    shape = (5, 6, 7)
    P = _random_points(shape, npts, npts)
    _check(gpu, shape, dtype, P)
    assert npts <= native.SAMPLE_MAX_BLOCKS * native.SAMPLE_BLOCK * native.SAMPLE_POINTS
    # a capped grid: every lane walks the grid-stride loop, the last pass is partial
    _check(gpu, shape, dtype, P, max_blocks=3, transposed=True)
    _check(gpu, (9, 130), dtype, _random_points((9, 130), npts, npts + 1), max_blocks=1)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("nf", [1, 2, 5, 9])
def test_several_fields_in_one_call(gpu, nf, dtype):
    for shape in ((5, 6, 7), (6, 7), (130,)):
        got = _check(gpu, shape, dtype, _random_points(shape, 300, 7), nf=nf, order=list(range(len(shape)))[::-1])
        assert got.shape == (nf, 300)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_periodic_and_fake_multi_rank_tables(gpu, dtype):
    """Tables of ranks that do not exist: non-owned points give 0 bits, and
    invalid points NaN only with the me0 flag."""
    n, o = (9, 8, 7), 2
    pts = torch.cat([_random_points((30, 8, 12), 400, 11, lo=-3.0), _lattice((3, 2, 2)) * 4.0,
                     torch.tensor([[NAN, 1.0, 1.0], [1.0, 99.0, 1.0], [1.0, -1.0, 1.0]], dtype=torch.float64)])
    seen = []
    for dims, per, coords in (((1, 1, 1), (1, 0, 1), (0, 0, 0)), ((2, 1, 2), (0, 0, 1), (1, 0, 0)),
                              ((2, 1, 2), (0, 0, 1), (0, 0, 1)), ((3, 1, 1), (1, 0, 0), (2, 0, 0))):
        table = []
        for d in range(3):
            E = dims[d] * (n[d] - o) + (0 if per[d] else o)
            table.append((E, per[d], n[d], [list(s) for s in _segments(n[d], o, dims[d], per[d], coords[d], n[d])]))
        bad = ~torch.isfinite(pts).all(dim=1)
        for d in range(3):
            if not per[d]:
                bad |= (pts[:, d] < 0) | (pts[:, d] > table[d][0] - 1)
        assert 3 <= int(bad.sum()) < 380
        for me0 in (True, False):
            got = _check(gpu, n, dtype, pts, table=table, me0=me0, nf=2)
            assert (got[:, bad] == (NAN_BITS if me0 else 0)).all()
            if me0:
                seen.append(int((got[0] == 0).sum()))
    assert seen[0] <= 3 and min(seen[1:]) > 50  # one rank owns everything; a fake rank leaves many points to others


def test_bad_descriptors_are_refused(gpu):
    A = torch.zeros(5, 6, dtype=torch.float64, device=gpu)
    P = torch.zeros(4, 2, dtype=torch.float64, device=gpu)
    out = torch.zeros(4, dtype=torch.float64, device=gpu)

    def call(table, fields=None, elem=8, npts=4, out_fs=4):
        native.sample(table, fields or [(A.data_ptr(), [6, 1])], elem, P.data_ptr(), 2, 1, npts, out.data_ptr(), out_fs,
                      True)

    good = _one_rank_table((5, 6))
    call(good)
    for bad in (lambda: call([(5, 0, 5, [[0, 6, 0]]), good[1]]),          # a segment past the extent
                lambda: call([(9, 0, 5, [[0, 5, 1]]), good[1]]),          # ... past the field
                lambda: call([(1, 0, 5, []), good[1]]),                   # E < 2
                lambda: call(good, [(A.data_ptr(), [6, -1])]),            # a negative stride
                lambda: call(good, [(A.data_ptr(), [6])]),                # a stride missing
                lambda: call(good, [(0, [6, 1])]),
                lambda: call(good, elem=2),
                lambda: call(good, npts=-1),
                lambda: call(good, [(A.data_ptr(), [6, 1])] * 2, out_fs=2),  # the fields' outputs overlap
                lambda: call(good + good)):
        with pytest.raises(igg.IGGError):
            bad()
    torch.cuda.synchronize()


def test_offsets_past_2_to_the_31(gpu):
    """A (3, 4, 5) f32 view whose outer stride is 2^31 + 8 elements over an
    unfilled 17 GiB allocation: only the 60 touched cells are written."""
    outer = 2 ** 31 + 8
    need = (2 * outer + 3 * 7 + 5) * 4
    free, _total = torch.cuda.mem_get_info()
    if free < need + (1 << 30):
        pytest.skip(f"the device has {free >> 30} GiB free, the view spans {need >> 30} GiB")
    big = torch.empty(2 * outer + 3 * 7 + 5, dtype=torch.float32, device=gpu)
    V = big.as_strided((3, 4, 5), (outer, 7, 1))
    dense = torch.randn(3, 4, 5, generator=torch.Generator().manual_seed(12), dtype=torch.float32)
    V.copy_(dense.to(gpu))
    P = torch.cat([_lattice((3, 4, 5)), _lattice((2, 3, 4)) + 0.5])
    table = _one_rank_table((3, 4, 5))
    want = torch.empty(P.shape[0], dtype=torch.float64)
    native.host_sample(table, [(dense.data_ptr(), list(dense.stride()))], 4, P.data_ptr(), 3, 1, P.shape[0],
                       want.data_ptr(), P.shape[0], True)
    Pd = P.to(gpu)
    got = torch.empty(P.shape[0], dtype=torch.float64, device=gpu)
    native.sample(table, [(V.data_ptr(), list(V.stride()))], 4, Pd.data_ptr(), 3, 1, P.shape[0], got.data_ptr(),
                  P.shape[0], True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(want))
    del big, V


# ------------------------------------------------------------ sample_g, Recorder
def _periodic_case(gpu, dtype=torch.float64):
    igg.init_global_grid(9, 8, 7, periodx=1, periody=1, periodz=1, quiet=True, init_MPI=False)
    E = extents(igg.get_global_grid(), (9, 8, 7))
    C = [local_of_global(global_values(E, s, dtype), (9, 8, 7)) for s in (1, 2)]
    C[1] = C[1].permute(2, 0, 1).contiguous().permute(1, 2, 0)
    G = [c.to(gpu) for c in C]
    assert G[1].stride() == C[1].stride()
    return E, C, G


def _moving_points(E, k):
    g = torch.Generator().manual_seed(20 + k)
    u = (torch.rand(500, 3, generator=g, dtype=torch.float64) * 4 - 1.5) * torch.tensor(E, dtype=torch.float64)
    u[:7] = torch.tensor([[0.0, 0.0, 0.0], [E[0], E[1], E[2]], [-0.5, 1.0, 2.0], [E[0] - 1.0, 0.25, E[2] - 0.5],
                          [NAN, 0.0, 0.0], [0.0, math.inf, 0.0], [3.0, 3.0, 3.0]], dtype=torch.float64)
    return u


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_one_periodic_rank_gpu_against_cpu_bitwise_and_captured(gpu, dtype):
    from igg.parallel import halo as HL

    E, C, G = _periodic_case(gpu, dtype)
    P0 = _moving_points(E, 0)
    assert torch.equal(bits(igg.sample_g(tuple(G), P0.to(gpu))), bits(igg.sample_g(tuple(C), P0)))
    assert torch.equal(bits(igg.sample_g(G[1], P0.to(gpu))), bits(igg.sample_g(C[1], P0)))
    # captured, with P rewritten between three replays: out= is refreshed each time
    P = P0.to(gpu)
    out = torch.zeros(2, 500, dtype=torch.float64, device=gpu)
    graph = HL.capture_graph(lambda: igg.sample_g(tuple(G), P, out=out), "sample_g", uses_halo=False)
    for k in (1, 2, 3):
        Pk = _moving_points(E, k)
        P.copy_(Pk)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(igg.sample_g(tuple(C), Pk))), k
    igg.finalize_global_grid(finalize_MPI=False)


def test_recorder_captured_fills_a_row_per_replay(gpu):
    from igg.parallel import halo as HL

    E, C, G = _periodic_case(gpu)
    P = _moving_points(E, 5).to(gpu)
    rec = igg.Recorder(tuple(G), P, 5)
    eager = igg.Recorder(tuple(G), P, 5)

    def step():
        for A in G:
            A.mul_(1.5)
        igg.update_halo_(*G)

    graph = HL.capture_graph(lambda: rec.record(*G), "Recorder.record", uses_halo=False)
    rec.reset()  # the capture itself wrote nothing that counts
    saved = [A.clone() for A in G]
    for _ in range(5):
        step()
        graph.replay()
    for A, s in zip(G, saved):
        A.copy_(s)
    rows = []
    for _ in range(5):
        step()
        eager.record(*G)
        rows.append(igg.sample_g(tuple(G), P))
    got = rec.result()
    assert got.shape == (5, 2, 500)
    assert torch.equal(bits(got), bits(eager.result())) and torch.equal(bits(got), bits(torch.stack(rows)))
    graph.replay()  # a sixth row does not fit: nothing is written, result() says so
    with pytest.raises(igg.IGGError, match="rows"):
        rec.result()
    assert torch.equal(bits(rec._buf), bits(got))
    igg.finalize_global_grid(finalize_MPI=False)


def test_gpu_dtypes_and_devices_are_refused(gpu):
    igg.init_global_grid(9, 8, 7, quiet=True, init_MPI=False)
    P = torch.zeros(3, 3, dtype=torch.float64, device=gpu)
    A = torch.ones(9, 8, 7, dtype=torch.float64, device=gpu)
    with pytest.raises(igg.IGGError, match="float32 or float64"):
        igg.sample_g(A.half(), P)
    with pytest.raises(igg.IGGError, match="`P`"):
        igg.sample_g(A, P.cpu())
    with pytest.raises(igg.IGGError, match="`out`"):
        igg.sample_g(A, P, out=torch.zeros(3, dtype=torch.float64))
    assert igg.sample_g(A, P[:0]).shape == (0,)
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------- ranks sharing device 0
@pytest.mark.parametrize("nprocs,dtype,args", [
    (2, "float64", (2, 1, 1, 0, 2, 3, 0)),
    (4, "float32", (2, 2, 1, 3, 3, 2, 1)),
    (8, "float64", (2, 2, 2, 5, 2, 3, 0, 1)),  # after update_halo_
])
def test_multi_rank_on_one_device(gpu, nprocs, dtype, args):
    run_sample_ranks(nprocs, "sample", "gpu", dtype, *args, timeout=120, env_extra={"IGG_TRANSPORT": "staged"})


@pytest.mark.multigpu
def test_two_ranks_on_two_devices_over_rccl(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: one rank per device over RCCL")
    run_sample_ranks(2, "sample", "mgpu", "float64", 2, 1, 1, 1, 2, 3, 0, timeout=150,
                     env_extra={"IGG_TRANSPORT": "rccl"})


def test_example_acoustic_receivers_on_the_gpu(gpu):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "acoustic_receivers.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=MAX_TIMEOUT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "the node receivers equal gather_g's cells bit for bit" in r.stdout
