"""Form 1 of the three-step pass (10-row tile, 6 rows written, Q parked in a
private LDS slot per lane between the stages): on shapes picked for where the
longer tile, the odd row count per wave and the two Q slots can go wrong, the
pass must leave, bitwise, what three single-step launches leave, and touch
nothing else. Q is random at every point, so a Q value taken from another row,
plane or slot changes the result."""
import pytest
import torch

import igg
from igg.ops import stencil

pytestmark = pytest.mark.gpu

FORM = 1
KW = dict(lam=1.3, dt=0.004, dx=0.3, dy=0.25, dz=0.2)  # dx != dy != dz: a swapped axis shows
F64, F32 = torch.float64, torch.float32
BOTH = (F64, F32)
GUARD = 4096  # elements in front of and behind T2 that no store may reach

# Tile rows (tiles advance by 6 rows): one tile with its rows clamped to the
# array (3, 4), exactly one tile (8), a second tile with one written row (9),
# several tiles with a partial last one (14, 33).
ROWS = [((9, n1, 64), 0, dt) for n1 in (3, 4, 8, 9, 14, 33) for dt in BOTH]
# Planes: fewer than the four-position lead-in (3, 4, 5); 9 and 16 run every
# combination of the three register phases with the two Q parities (six
# positions) from a chunk start of either parity.
PLANES = [((n0, 14, 32), 0, dt) for n0 in (3, 4, 5, 9, 16) for dt in BOTH]
# Several x chunks of about the minimum length per tile (rounds 4): see
# test_chunk_seams for what the launch plan makes of it.
CHUNKS = [((70, 20, 64), 4, dt) for dt in BOTH]
# Row length: one partly filled segment (4, 8), lanes past the row in the
# second segment (130; float32 rows are multiples of 4 points: 132), two whole
# segments (f64) or one (f32) and idle waves beside them (256), the full tile.
ROWLEN = [((7, 11, n2), 0, F64) for n2 in (4, 8, 130, 256)] + [((7, 11, n2), 0, F32) for n2 in (4, 8, 132, 256)]
FULL = [((6, 20, 512), 0, F64), ((6, 20, 1024), 0, F32)]
CASES = ROWS + PLANES + CHUNKS + ROWLEN + FULL

_cache = {}


def _inputs(shape, dtype, gpu):
    """(T, Cp, Q, three single steps of T, and copies to compare against) of a
    case: computed once, never written."""
    key = (shape, dtype)
    if key not in _cache:
        g = torch.Generator().manual_seed(47)
        T = (2 * torch.rand(shape, generator=g, dtype=torch.float64) - 1).to(dtype).to(gpu)
        Cp = (1 + 5 * torch.rand(shape, generator=g, dtype=torch.float64)).to(dtype).to(gpu)  # so Q is random per point
        Q = torch.empty_like(Cp)
        stencil.quotient_(Q, Cp, lam=KW["lam"], dt=KW["dt"])
        a, b, ref = T.clone(), T.clone(), T.clone()
        stencil.diffusion3d_(a, T, Cp, variant=1, **KW)
        stencil.diffusion3d_(b, a, Cp, variant=1, **KW)
        stencil.diffusion3d_(ref, b, Cp, variant=1, **KW)
        torch.cuda.synchronize()
        _cache[key] = (T, Cp, Q, ref, T.clone(), Cp.clone(), Q.clone())
    return _cache[key]


def _canary(T):
    """(buffer, T2): T2 a view between two guard bands of the buffer, NaN
    wherever the pass must write and T's values on the boundary, which it must
    leave alone (with halo_z it may rewrite the z boundary with T's values); the
    guard bands hold a finite mark."""
    buf = torch.full((T.numel() + 2 * GUARD,), 7.25, dtype=T.dtype, device=T.device)
    T2 = buf[GUARD:GUARD + T.numel()].view(T.shape)
    T2.fill_(float("nan"))
    for d in range(3):
        for i in (0, -1):
            T2.select(d, i).copy_(T.select(d, i))
    return buf, T2


def _run(gpu, shape, rounds, dtype, halo_z):
    T, Cp, Q, ref, T0, Cp0, Q0 = _inputs(shape, dtype, gpu)
    assert stencil.threestep_ok(T, FORM)
    buf, T2 = _canary(T)
    stencil.diffusion3d_threestep_(T2, T, Cp, Q=Q, form=FORM, rounds=rounds, halo_z=halo_z, **KW)
    torch.cuda.synchronize()
    bad = (T2 != ref)
    print(shape, dtype, "rounds", rounds, "halo_z", halo_z, "points differing:", int(bad.sum()))
    assert not torch.isnan(T2).any()
    assert torch.equal(T2, ref), bad.nonzero()[:8].tolist()  # interior and boundary planes alike
    assert bool((buf[:GUARD] == 7.25).all()) and bool((buf[-GUARD:] == 7.25).all())
    assert torch.equal(T, T0) and torch.equal(Cp, Cp0) and torch.equal(Q, Q0)
    return T2, ref


@pytest.mark.parametrize("halo_z", [False, True])
@pytest.mark.parametrize("shape,rounds,dtype", CASES)
def test_tile10_pass_equals_three_single_steps_bitwise(gpu, shape, rounds, dtype, halo_z):
    _run(gpu, shape, rounds, dtype, halo_z)


@pytest.mark.parametrize("shape,rounds,dtype", CHUNKS)
def test_chunk_seams(gpu, shape, rounds, dtype):
    """The chunk case does run several short x chunks, and the planes on either
    side of every chunk seam are those of three single steps."""
    es = torch.empty(0, dtype=dtype).element_size()
    target = stencil.native.diffusion3d_threestep_target(es, FORM, rounds)
    tiles, ch, nblk = stencil.native.diffusion3d_threestep_plan(list(shape), FORM, target)
    print("target", target, "tiles", tiles, "chunk", ch, "workgroups", nblk)
    assert tiles == 3 and nblk // tiles >= 4 and ch < 2 * 8  # below twice the minimum chunk length
    T2, ref = _run(gpu, shape, rounds, dtype, True)
    for xs in range(1 + ch, shape[0] - 1, ch):  # first plane of every chunk but the first
        assert torch.equal(T2[xs - 1], ref[xs - 1]) and torch.equal(T2[xs], ref[xs]), xs


def _boundary_equal(a, b):
    return all(torch.equal(a.select(d, i), b.select(d, i)) for d in range(3) for i in (0, -1))


def test_model_with_form_1_matches_single_step_model(gpu, monkeypatch):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_VARIANT", "11")
    monkeypatch.setenv("IGG_STENCIL_THREESTEP", "1")
    monkeypatch.delenv("IGG_STENCIL_TWOSTEP", raising=False)
    monkeypatch.delenv("IGG_STENCIL_QUOTIENT", raising=False)
    igg.init_global_grid(20, 26, 64, quiet=True, init_MPI=False)
    a = Diffusion3D(dtype=torch.float64)
    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "0")
    b = Diffusion3D(dtype=torch.float64)
    a.three_step_form = FORM
    assert a.three_step and a._deep_key() == (FORM, a.three_step_rounds)
    assert not b.three_step and not b.two_step
    roles = {a.T.data_ptr(), a.T2.data_ptr()}
    for nt in (5, 7, 1):  # deep + pass, two deep + step, step: 13 steps
        a.run(nt)
    b.run(13)
    torch.cuda.synchronize()
    assert torch.equal(a.T, b.T)
    assert _boundary_equal(a.T2, a.T) and {a.T.data_ptr(), a.T2.data_ptr()} == roles
    a.capture(8)  # two deep passes and two single steps; 13 = a replay, a deep pass and a two-step pass
    b.capture()
    assert a.graph is not None and a.graph_steps == 8 and a._graph_deep == (FORM, a.three_step_rounds)
    a.run(13)
    b.run(13)
    torch.cuda.synchronize()
    assert torch.equal(a.T, b.T)
    assert _boundary_equal(a.T2, a.T) and {a.T.data_ptr(), a.T2.data_ptr()} == roles
