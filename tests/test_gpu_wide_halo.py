"""Wide halos on the GPU: the slab copy kernel through ``update_halo_`` (self-
periodic, loopback over RCCL and the put transport, graph capture) and the
two-step pass of ``Diffusion3D`` on grids that exchange. Every comparison is
bitwise."""
import re

import pytest
import torch

import igg
from igg._native import native
from igg.parallel import halo as H
from tests.copy_oracle import field_slab
from tests.test_wide_halo_cpu import run_wide_ranks

pytestmark = pytest.mark.gpu

KW = dict(quiet=True, init_MPI=False)
# one dtype per element size the copy kernels take: 1, 2, 4, 8, 16 B
DTYPES = [torch.uint8, torch.int16, torch.float32, torch.float64, torch.complex128]


def _data(shape, dtype, order=None):
    g = torch.Generator().manual_seed(11)
    n = 1
    for s in shape:
        n *= s
    if dtype == torch.uint8:
        v = torch.randint(0, 256, (n,), generator=g, dtype=torch.int64).to(dtype)
    elif dtype == torch.int16:
        v = torch.randint(-30000, 30000, (n,), generator=g, dtype=torch.int64).to(dtype)
    elif dtype.is_complex:
        v = torch.complex(torch.rand(n, generator=g, dtype=torch.float64), torch.rand(n, generator=g, dtype=torch.float64))
    else:
        v = torch.rand(n, generator=g, dtype=torch.float64).to(dtype)
    v = v.view(shape)
    if order is not None:  # dense, memory order `order` (slowest first)
        inv = [order.index(d) for d in range(len(shape))]
        v = v.permute(order).contiguous().permute(inv)
    return v


def _wide(w):
    o = max(4, 2 * w)  # width 1 with overlap 4: the planes of a wide grid, moved one at a time
    return dict(overlapx=o, overlapy=o, overlapz=o, halowidthx=w, halowidthy=w, halowidthz=w)


def _host_exchange(fields):
    """The host exchange of the same data on the same grid."""
    out = [f.clone() for f in fields]
    igg.update_halo_(*out)
    return out


# Shapes by what they exercise in the slab kernel: the flat shape everywhere;
# rows just past one wave with an even n2 (aligned pairs); an odd n2 (the
# vector access must fall back) with 67 rows, no multiple of 4*GROWS; the same
# in a permuted layout (the slab dimension is not the unit stride). A periodic
# grid needs n >= 2*overlap-1 = 11 with width 3, so the two small shapes grow
# to the smallest admissible sizes there, keeping what they exercise.
# Width 4 (overlap 8, so n >= 15): the z slab's row is one 16-byte access with
# 4-byte elements, 8 bytes with 2-byte and 4 bytes with 1-byte elements.
SHAPES = {
    "flat": {1: (8, 8, 8), 2: (8, 8, 8), 3: (11, 11, 11), 4: (15, 15, 15)},
    "wave": {1: (9, 10, 70), 2: (9, 10, 70), 3: (11, 12, 70), 4: (15, 16, 72)},
    "odd": {1: (12, 67, 131), 2: (12, 67, 131), 3: (12, 67, 131), 4: (16, 67, 131)},
    "permuted": {1: (12, 67, 131), 2: (12, 67, 131), 3: (12, 67, 131), 4: (16, 67, 131)},
}


@pytest.mark.parametrize("case", list(SHAPES))
@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_slab_exchange_matches_host(gpu, w, case):
    n = SHAPES[case][w]
    igg.init_global_grid(*n, periodx=1, periody=1, periodz=1, **_wide(w), **KW)
    orders = [(1, 2, 0), (2, 0, 1)] if case == "permuted" else [None]
    for dtype in DTYPES:  # width 3 with 8-B elements cannot be one vector access
        for order in orders:
            A = _data(n, dtype, order)
            ref, = _host_exchange([A])
            Ag = A.to(gpu)
            assert Ag.stride() == A.stride()
            if w == 4 and case == "wave":
                # the z slab of this exchange takes the vector rows named above
                mv = field_slab(n, 2, 4, 4)["move"]
                p = Ag.data_ptr()
                eb = Ag.element_size()
                plan = native.copy3d_plan(list(mv["box"]), (p + mv["src_off"] * eb, p + mv["dst_off"] * eb), eb)
                assert (plan["path"], plan["vec_bytes"]) == ("gather", 4 * eb if eb <= 4 else 0), (dtype, plan)
            igg.update_halo_(Ag)
            assert torch.equal(Ag.cpu(), ref), f"{dtype} layout {order}"
    # two staggered fields in one launch
    Vx, Vz = _data((n[0] + 1, n[1], n[2]), torch.float64), _data((n[0], n[1], n[2] + 1), torch.float64)
    rx, rz = _host_exchange([Vx, Vz])
    gx, gz = Vx.to(gpu), Vz.to(gpu)
    igg.update_halo_(gx, gz)
    assert torch.equal(gx.cpu(), rx) and torch.equal(gz.cpu(), rz)
    igg.finalize_global_grid(finalize_MPI=False)


@pytest.mark.parametrize("w", [1, 2, 3])
def test_slab_exchange_lower_dimensional_fields(gpu, w):
    n = (131, 67, 1)
    kw = {k: v for k, v in _wide(w).items() if not k.endswith("z")}
    igg.init_global_grid(*n, periodx=1, periody=1, **kw, **KW)
    for shape in ((131,), (131, 67)):
        for dtype in DTYPES:
            A = _data(shape, dtype)
            ref, = _host_exchange([A])
            Ag = A.to(gpu)
            igg.update_halo_(Ag)
            assert torch.equal(Ag.cpu(), ref), f"{shape} {dtype}"
    igg.finalize_global_grid(finalize_MPI=False)


# ----------------------------------------------------------------- loopback
N_LB = (24, 20, 72)


def _loopback_grid(monkeypatch, transport, mode=None):
    monkeypatch.setenv("IGG_TRANSPORT", transport)
    igg.init_global_grid(*N_LB, periodx=1, periody=1, periodz=1, **_wide(2), **KW)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        fields = [_data(N_LB, dtype), _data((N_LB[0] + 1, N_LB[1], N_LB[2]), dtype)]
        refs[dtype] = (fields, _host_exchange(fields))  # before the loopback: the periodic host exchange
    H.enable_loopback()
    if mode is not None:
        H.set_halo_mode(mode)
    return refs


@pytest.mark.parametrize("mode", ["sequential", "onephase"])
@pytest.mark.parametrize("transport", ["put", "rccl"])
def test_loopback_wide_exchange(gpu, monkeypatch, transport, mode):
    """Every slab, edge and corner through the remote path (pack, transport,
    unpack). The loopback emulation has no host-staged transport; what it
    must reproduce is the periodic exchange, taken here from the host engine."""
    refs = _loopback_grid(monkeypatch, transport, mode)
    for dtype, (fields, want) in refs.items():
        for _ in range(2):  # both arena halves of the put transport
            got = [f.to(gpu) for f in fields]
            igg.update_halo_(*got)
            torch.cuda.synchronize()
            for g, r in zip(got, want):
                assert torch.equal(g.cpu(), r), f"{transport} {mode} {dtype}"
    if mode == "onephase" or transport == "put":
        assert H.engine().last_message_count == 52  # 26 directions x 2 fields, as with width 1
    H.check_transport()
    igg.finalize_global_grid(finalize_MPI=False)


@pytest.mark.parametrize("w", [1, 2, 4])
def test_loopback_put_exchange_every_element_size(gpu, monkeypatch, w):
    """The put transport's system-scope stores with every element size (width
    1: the 2-D kernel; 2 and 4: the slab kernel, scalar and vector rows), into
    both arena halves: the only route to the system stores combined with the
    arena's parity shift."""
    monkeypatch.setenv("IGG_TRANSPORT", "put")
    igg.init_global_grid(*N_LB, periodx=1, periody=1, periodz=1, **_wide(w), **KW)
    refs = {}
    for dtype in DTYPES:
        fields = [_data(N_LB, dtype), _data((N_LB[0] + 1, N_LB[1], N_LB[2]), dtype)]
        refs[dtype] = (fields, _host_exchange(fields))  # before the loopback: the periodic host exchange
    H.enable_loopback()
    for dtype, (fields, want) in refs.items():
        for half in range(2):
            got = [f.to(gpu) for f in fields]
            igg.update_halo_(*got)
            torch.cuda.synchronize()
            for g, r in zip(got, want):
                assert torch.equal(g.cpu(), r), f"put width {w} {dtype} exchange {half}"
    H.check_transport()
    igg.finalize_global_grid(finalize_MPI=False)


def test_loopback_wide_exchange_auto_transport(gpu, monkeypatch):
    refs = _loopback_grid(monkeypatch, "auto")
    assert H.auto_transport()
    for dtype, (fields, want) in refs.items():
        got = [f.to(gpu) for f in fields]
        igg.update_halo_(*got)
        torch.cuda.synchronize()
        for g, r in zip(got, want):
            assert torch.equal(g.cpu(), r), dtype
    log = H.tuned_transports()
    assert len(log) == 2, log  # one record per field-set signature (f64, f32)
    for rec in log:
        assert rec["checked"] == {"rccl": "ok", "put": "ok"}, rec
        assert rec["chosen"] in ("rccl", "put") and rec["chosen"] == min(rec["ms"], key=rec["ms"].get)
    assert H.transport_name() == log[-1]["chosen"]
    H.check_transport()
    igg.finalize_global_grid(finalize_MPI=False)


@pytest.mark.parametrize("transport", ["put", "rccl"])
def test_captured_wide_exchange_replays_like_eager(gpu, monkeypatch, transport):
    monkeypatch.setenv("IGG_TRANSPORT", transport)
    igg.init_global_grid(*N_LB, periodx=1, periody=1, periodz=1, **_wide(2), **KW)
    A0 = _data(N_LB, torch.float64)
    halo = torch.zeros(N_LB, dtype=torch.bool)
    for d in range(3):
        halo.narrow(d, 0, 2).fill_(True)
        halo.narrow(d, N_LB[d] - 2, 2).fill_(True)
    X0 = torch.where(halo, torch.zeros_like(A0), A0)  # halo planes zeroed
    want = [_host_exchange([X0 * k])[0] for k in (1, 2, 3)]  # before the loopback: the periodic host exchange
    H.enable_loopback()
    X0 = X0.to(gpu)
    Ae, Ag = X0.clone(), X0.clone()
    igg.update_halo_(Ag)  # eager first: buffers and arena grow outside the capture
    g = H.capture_graph(lambda: igg.update_halo_(Ag), "test")
    for k in (1, 2, 3):
        Ae.copy_(X0 * k)
        Ag.copy_(X0 * k)
        igg.update_halo_(Ae)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(Ae, Ag), f"replay {k}"
        assert torch.equal(Ag.cpu(), want[k - 1]), f"exchange {k}"
    H.check_transport()
    igg.finalize_global_grid(finalize_MPI=False)


# -------------------------------------------------------------------- model
def _pair(monkeypatch, dtype):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "0")
    a = Diffusion3D(dtype=dtype, variant=0)
    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "1")
    b = Diffusion3D(dtype=dtype, variant=0)
    assert not a._two_step_now() and b._two_step_now()
    assert not b.fused_available() and not b.set_overlap(True)
    return a, b


def _run_pair(a, b):
    """nt = 2, 3, 4, 7 from a common state each time (the models are bitwise
    equal after every run), then a graph of four steps and nine more."""
    for nt in (2, 3, 4, 7):
        a.run(nt)
        b.run(nt)
        torch.cuda.synchronize()
        assert torch.equal(a.T, b.T), f"run({nt}): halos included"
    b.capture(4)
    assert b._graph_two is not None
    a.run(9)
    b.run(9)
    torch.cuda.synchronize()
    assert b.graph is not None
    assert torch.equal(a.T, b.T), "capture(4) + run(9)"


@pytest.mark.parametrize("n,dtype", [((36, 20, 128), torch.float64), ((20, 36, 256), torch.float32)])
def test_model_pass_equals_single_steps_periodic(gpu, monkeypatch, n, dtype):
    igg.init_global_grid(*n, periodx=1, periody=1, periodz=1, **_wide(2), **KW)
    _run_pair(*_pair(monkeypatch, dtype))
    igg.finalize_global_grid(finalize_MPI=False)


@pytest.mark.parametrize("n,dtype", [((36, 20, 128), torch.float64), ((20, 36, 256), torch.float32)])
def test_model_pass_equals_single_steps_loopback_put(gpu, monkeypatch, n, dtype):
    monkeypatch.setenv("IGG_TRANSPORT", "put")
    igg.init_global_grid(*n, periodx=1, periody=1, periodz=1, **_wide(2), **KW)
    H.enable_loopback()
    _run_pair(*_pair(monkeypatch, dtype))
    H.check_transport()
    igg.finalize_global_grid(finalize_MPI=False)


def test_width_one_grid_keeps_single_steps(gpu, monkeypatch):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "1")
    igg.init_global_grid(36, 20, 128, periodx=1, periody=1, periodz=1, **_wide(1), **KW)
    m = Diffusion3D(dtype=torch.float64, variant=0)
    assert not m.two_step and not m._two_step_now()
    igg.finalize_global_grid(finalize_MPI=False)


# --------------------------------------------------------------- multi-rank
def _check_model_ranks(outs):
    two = set()
    for o in outs:
        m = re.search(r"wide model OK TWO=(\d)", o)
        assert m, o[-2000:]
        two.add(m.group(1))
    assert len(two) == 1, f"ranks disagree on the two-step pass: {two}"


@pytest.mark.parametrize("graph", [0, 4])
def test_two_ranks_sharing_the_gpu(gpu, graph):
    outs = run_wide_ranks(2, "model", "gpu", 20, 20, 128, 7, graph, 1, 1, 2, env_extra={"IGG_TRANSPORT": "put"})
    _check_model_ranks(outs)


@pytest.mark.slow
@pytest.mark.parametrize("graph", [0, 4])
def test_eight_ranks_sharing_the_gpu(gpu, graph):
    outs = run_wide_ranks(8, "model", "gpu", 20, 20, 128, 7, graph, 2, 2, 2, env_extra={"IGG_TRANSPORT": "put"})
    _check_model_ranks(outs)


@pytest.mark.multigpu
def test_two_ranks_on_two_devices(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs 2 GPUs (one rank per device), {torch.cuda.device_count()} visible")
    outs = run_wide_ranks(2, "model", "mgpu", 20, 20, 128, 7, 0, 1, 1, 2, env_extra={"IGG_TRANSPORT": "put"})
    _check_model_ranks(outs)
