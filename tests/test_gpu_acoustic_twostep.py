"""The two-step acoustic pass (csrc/kernels/acoustic2_kernels.hip): one kernel
that advances P, Vx, Vy two time steps must leave, bitwise, what two launches
of the single-step vector kernel leave - on shapes picked for where its march,
its chunk edges and its segment edges can go wrong - and the model that uses it
must compute what the single-step model computes."""
import pytest
import torch

import igg
from igg import IGGError
from igg._native import native
from igg.ops import stencil

pytestmark = pytest.mark.gpu

KW = dict(dt=0.004, K=1.7, rho=0.6, dx=0.3, dy=0.25)  # dx != dy, K != rho: a swapped axis or coefficient shows

F32, F64 = torch.float32, torch.float64
# Fewer rows than the pipeline is deep; one segment of 62 vectors exactly (the
# lone lane of column ny falls into the next segment), one vector more, one
# less (OWNV = 248 f32, 124 f64); two segments; many chunks; a long row.
SHAPES = {
    F32: [(1, 8), (2, 8), (3, 12), (5, 8), (9, 248), (9, 252), (7, 244), (6, 500), (70, 64), (17, 1000)],
    F64: [(1, 4), (2, 4), (3, 6), (9, 124), (9, 126), (7, 122), (70, 64), (17, 1000)],
}
# Chunks 1 and 3 put chunk starts 0, 1 and 2 rows from the x boundary and the
# face row nx into a chunk of its own or the last chunk's end; 0 = the default.
# Every shape takes all three but the long row, which pairs 1 and 3 with 0
# across the dtypes.
CASES = []
for _dt, _shapes in SHAPES.items():
    for _k, _s in enumerate(_shapes):
        _chunks = (1, 3, 0) if _s[0] * _s[1] <= 8192 else ((1, 0) if _dt is F32 else (3, 0))
        CASES += [(_s, _dt, _c) for _c in _chunks]
CASES += [((70, 64), F32, 7), ((70, 64), F64, 71)]  # nx+1 = 71: a last chunk of one row; one chunk for everything


def _inputs(nx, ny, dtype, gpu):
    """Values distinct at every element of the three fields, boundary faces
    non-zero."""
    g = torch.Generator().manual_seed(11)
    n = nx * ny + (nx + 1) * ny + nx * (ny + 1)
    v = torch.randperm(n, generator=g).to(torch.float64) / n + 0.5
    P, Vx, Vy = torch.split(v, [nx * ny, (nx + 1) * ny, nx * (ny + 1)])
    f = lambda t, s: t.reshape(s).to(dtype).to(gpu).contiguous()
    return f(P, (nx, ny)), f(Vx, (nx + 1, ny)), f(Vy, (nx, ny + 1))


def _single(dst, src, nx, ny):
    native.acoustic2d(*(t.data_ptr() for t in dst + src), nx, ny, KW["dt"] * KW["K"], KW["dt"] / KW["rho"],
                      1.0 / KW["dx"], 1.0 / KW["dy"], src[0].element_size(), True,
                      torch.cuda.current_stream().cuda_stream)


_refs = {}


def _reference(nx, ny, dtype, gpu):
    """(inputs, the state after two single steps), computed once per shape."""
    key = (nx, ny, dtype)
    if key not in _refs:
        src = _inputs(nx, ny, dtype, gpu)
        tmp = tuple(torch.full_like(t, float("nan")) for t in src)
        ref = tuple(torch.full_like(t, float("nan")) for t in src)
        native.acoustic2d_set_variant(2)
        _single(tmp, src, nx, ny)
        _single(ref, tmp, nx, ny)
        torch.cuda.synchronize()
        _refs[key] = (tuple(t.cpu() for t in src), tuple(t.cpu() for t in ref))
    return _refs[key]


@pytest.mark.parametrize("shape,dtype,chunk", CASES)
def test_pass_equals_two_single_steps_bitwise(gpu, shape, dtype, chunk):
    nx, ny = shape
    src0, ref = _reference(nx, ny, dtype, gpu)
    assert not any(torch.isnan(t).any() for t in ref)
    src = tuple(t.to(gpu) for t in src0)
    assert stencil.acoustic2d_twostep_ok(src[0])
    out = tuple(torch.full_like(t, float("nan")) for t in src)
    stencil.acoustic2d_twostep_(*out, *src, chunk=chunk, **KW)
    torch.cuda.synchronize()
    for name, o, r in zip(("P2", "Vx2", "Vy2"), out, ref):
        bad = o.cpu() != r
        print(shape, dtype, "chunk", chunk, name, "elements differing:", int(bad.sum()))
    for name, o, r in zip(("P2", "Vx2", "Vy2"), out, ref):
        assert not torch.isnan(o).any(), name
        assert torch.equal(o.cpu(), r), (name, (o.cpu() != r).nonzero()[:8].tolist())
    for s, s0 in zip(src, src0):
        assert torch.equal(s.cpu(), s0)
    # boundary faces keep their input values through both steps
    assert torch.equal(out[1][0], src[1][0]) and torch.equal(out[1][-1], src[1][-1])
    assert torch.equal(out[2][:, 0], src[2][:, 0]) and torch.equal(out[2][:, -1], src[2][:, -1])


@pytest.mark.parametrize("shape,dtype,chunk", [((9, 252), F32, 3), ((5, 8), F32, 1), ((9, 126), F64, 0),
                                               ((70, 64), F64, 3)])
def test_pass_on_fields_carved_from_one_allocation(gpu, shape, dtype, chunk):
    """The six fields lie in one NaN-filled allocation with at least one row of
    NaN padding before and after each: nothing is read that matters or written
    outside the arrays."""
    nx, ny = shape
    src0, ref = _reference(nx, ny, dtype, gpu)
    pad = ny + 1 + 3  # more than a row, and odd offsets between the arrays
    sizes = [nx * ny, (nx + 1) * ny, nx * (ny + 1)] * 2
    vj = 16 // src0[0].element_size()
    offs, pos = [], pad
    for n in sizes:
        pos = -(-pos // vj) * vj  # P / Vx rows are read as aligned 16-byte vectors
        offs.append(pos)
        pos += n + pad
    buf = torch.full((pos,), float("nan"), dtype=dtype, device=gpu)
    shapes = [(nx, ny), (nx + 1, ny), (nx, ny + 1)] * 2
    views = [buf[o:o + n].view(s) for o, n, s in zip(offs, sizes, shapes)]
    for v, t in zip(views[:3], src0):
        v.copy_(t)
    stencil.acoustic2d_twostep_(*views[3:], *views[:3], chunk=chunk, **KW)
    torch.cuda.synchronize()
    for v, r in zip(views[3:], ref):
        assert not torch.isnan(v).any()
        assert torch.equal(v.cpu(), r)
    for v, t in zip(views[:3], src0):
        assert torch.equal(v.cpu(), t)
    inside = torch.zeros(pos, dtype=torch.bool, device=gpu)
    for o, n in zip(offs, sizes):
        inside[o:o + n] = True
    assert torch.isnan(buf[~inside]).all()
    assert int((~inside).sum()) >= 7 * pad


def _same_with_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def test_refusals_leave_the_outputs_untouched(gpu):
    # ny is no multiple of the 4-element f32 vector
    src = _inputs(12, 10, F32, gpu)
    out = tuple(torch.full_like(t, float("nan")) for t in src)
    assert not stencil.acoustic2d_twostep_ok(src[0])
    with pytest.raises(IGGError):
        stencil.acoustic2d_twostep_(*out, *src, **KW)
    with pytest.raises(IGGError):  # the native launcher refuses it by itself
        native.acoustic2d_twostep(*(t.data_ptr() for t in out + src), 12, 10, 1e-3, 1e-3, 1.0, 1.0, 4, 0,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in out)
    # an output that is an input
    src = _inputs(12, 16, F32, gpu)
    before = tuple(t.clone() for t in src)
    out = tuple(torch.full_like(t, float("nan")) for t in src)
    for k in range(3):
        o = list(out)
        o[k] = src[k]
        with pytest.raises(IGGError):
            stencil.acoustic2d_twostep_(*o, *src, **KW)
        with pytest.raises(IGGError):
            native.acoustic2d_twostep(*(t.data_ptr() for t in tuple(o) + src), 12, 16, 1e-3, 1e-3, 1.0, 1.0, 4, 0,
                                      torch.cuda.current_stream().cuda_stream)
    # mis-shaped and mixed-dtype fields
    with pytest.raises(IGGError):
        stencil.acoustic2d_twostep_(out[0], out[2], out[1], *src, **KW)
    with pytest.raises(IGGError):
        stencil.acoustic2d_twostep_(out[0].double(), out[1], out[2], *src, **KW)
    with pytest.raises(IGGError):
        stencil.acoustic2d_twostep_(*out, src[0].t().contiguous().t(), src[1], src[2], **KW)
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in out)
    assert all(torch.equal(a, b) for a, b in zip(src, before))


NTS = (1, 2, 3, 7, 20, 45)


def _pair(monkeypatch, dtype, loopback=None, **grid):
    """(two-step model, single-step model) on one grid that stays initialised."""
    from igg.models.acoustic2d import Acoustic2D
    from igg.parallel import halo as H

    igg.init_global_grid(40, 48, 1, quiet=True, init_MPI=False, **grid)
    if loopback is not None:
        H.enable_loopback(loopback)
    monkeypatch.setenv("IGG_ACOUSTIC_TWOSTEP", "1")
    a = Acoustic2D(dtype=dtype)
    monkeypatch.setenv("IGG_ACOUSTIC_TWOSTEP", "0")
    b = Acoustic2D(dtype=dtype)
    return a, b


def _fields_equal(a, b):
    return torch.equal(a.P, b.P) and torch.equal(a.Vx, b.Vx) and torch.equal(a.Vy, b.Vy)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_model_eager_matches_single_step_model(gpu, monkeypatch, dtype):
    a, b = _pair(monkeypatch, dtype)
    assert a.two_step and a._two_step_now()
    assert not b.two_step and not b._two_step_now()
    assert not hasattr(a, "variant")
    for nt in NTS:
        a.run(nt)
        b.run(nt)
        torch.cuda.synchronize()
        assert _fields_equal(a, b), nt
    a.step()  # step() stays a single step
    b.step()
    torch.cuda.synchronize()
    assert _fields_equal(a, b) and torch.equal(a.P2, b.P2)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_model_captured_matches_and_keeps_buffers(gpu, monkeypatch, dtype):
    a, b = _pair(monkeypatch, dtype)
    a.capture()
    b.capture()
    assert a.graph_steps == 20 and a.graph is not None
    for nt in NTS:
        a.run(nt)
        b.run(nt)
        torch.cuda.synchronize()
        assert _fields_equal(a, b), nt
    for steps in (20, 6):  # a replay hands the buffers back in their roles (also with a 4k+2 graph)
        a.capture(steps)
        assert a.graph_steps == steps
        ptr = a.P.data_ptr()
        a.run(steps)
        b.run(steps)
        torch.cuda.synchronize()
        assert a.P.data_ptr() == ptr
        assert _fields_equal(a, b), steps
    # a graph captured with the pass is not replayed once the pass is off
    g = a.graph
    a.two_step = False
    assert not a._two_step_now()
    replays = []
    orig = g.replay
    g.replay = lambda: (replays.append(1), orig())[1]
    a.run(12)
    b.run(12)
    torch.cuda.synchronize()
    assert not replays
    assert _fields_equal(a, b)
    a.two_step = True
    a.run(6)
    b.run(6)
    torch.cuda.synchronize()
    assert replays and _fields_equal(a, b)


@pytest.mark.parametrize("grid", [dict(periodx=1), dict(loopback=(True, True, False), periodx=1, periody=1)],
                         ids=["periodic", "loopback"])
def test_grids_with_neighbours_keep_single_steps(gpu, monkeypatch, grid):
    a, b = _pair(monkeypatch, F32, **grid)
    assert not a.two_step and not a._two_step_now()
    a.two_step = True  # even when asked for by hand
    assert not a._two_step_now()
    a.run(6)
    b.run(6)
    torch.cuda.synchronize()
    assert _fields_equal(a, b)


def test_auto_selection_records_its_times_and_leaves_no_trace(gpu, monkeypatch):
    from igg.models.acoustic2d import Acoustic2D

    igg.init_global_grid(40, 48, 1, quiet=True, init_MPI=False)
    monkeypatch.setenv("IGG_ACOUSTIC_TWOSTEP", "auto")
    m = Acoustic2D()
    monkeypatch.setenv("IGG_ACOUSTIC_TWOSTEP", "0")
    ref = Acoustic2D()
    t = m.two_step_times
    print("two_step_times:", t, "two_step:", m.two_step, "chunk:", m.two_step_chunk)
    assert "single" in t and any(k.startswith("c") and k[1:].isdigit() for k in t)
    assert all(x > 0 for x in t.values())
    assert isinstance(m.two_step, bool)
    assert ref.two_step_times == {} and ref.two_step is False
    for name in ("P", "Vx", "Vy", "P2", "Vx2", "Vy2"):
        assert torch.equal(getattr(m, name), getattr(ref, name)), name
