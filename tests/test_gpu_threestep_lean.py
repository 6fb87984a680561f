"""The three-step pass after its march loop was thinned (stage 2 skipped on the
tile's two outer rows, a select-free path for waves that hold no end of the
row, segments of the odd wave rows rotated): on shapes picked for where the new
wave classes can go wrong the pass must still leave, bitwise, what three
single-step launches leave, and touch nothing else."""
import pytest
import torch

import igg
from igg.ops import stencil

pytestmark = pytest.mark.gpu

KW = dict(lam=1.3, dt=0.004, dx=0.3, dy=0.25, dz=0.2)  # dx != dy != dz: a swapped axis shows
F64, F32 = torch.float64, torch.float32

# Row ends relative to the waves' segments (128 f64 / 256 f32 points each): the
# last z point as lane 63 of a wave, as lane 0 of the next, mid-wave, and whole
# waves past the row.
ROW_ENDS = [((7, 11, n2), 0, F64) for n2 in (126, 128, 130, 256, 258, 384, 510, 512)]
ROW_ENDS += [((7, 11, n2), 0, F32) for n2 in (252, 256, 260, 1024)]
# Tile rows (tiles advance by 4 rows): a last tile with 1, 2, 3 or 4 written
# rows, the second row of waves wholly or partly outside the array, and more
# than two tiles, where a wrongly skipped stage-2 row shows between tiles.
TILE_ROWS = [((9, n1, 64), 0, dt) for n1 in (3, 4, 5, 6, 7, 8, 9, 10, 13) for dt in (F64, F32)]
# x chunks: several per tile (rounds 4), so that lead-in positions and the
# first and last planes all occur.
CHUNKS = [((n0, 10, 32), rounds, dt) for n0 in (3, 4, 5, 6, 11, 40) for rounds in (1, 4) for dt in (F64, F32)]
CASES = ROW_ENDS + TILE_ROWS + CHUNKS

_cache = {}


def _inputs(shape, dtype, gpu):
    """(T, Cp, Q, three single steps of T, and copies to compare against) of a
    case: computed once, never written."""
    key = (shape, dtype)
    if key not in _cache:
        g = torch.Generator().manual_seed(29)
        # random T with negative values, random Cp
        T = (2 * torch.rand(shape, generator=g, dtype=torch.float64) - 1).to(dtype).to(gpu)
        Cp = (1 + 5 * torch.rand(shape, generator=g, dtype=torch.float64)).to(dtype).to(gpu)
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
    """NaN wherever the pass must write; T's values on the boundary, which it
    must leave alone (with halo_z it may rewrite the z boundary with T's values)."""
    T2 = torch.full_like(T, float("nan"))
    for d in range(3):
        for i in (0, -1):
            T2.select(d, i).copy_(T.select(d, i))
    return T2


@pytest.mark.parametrize("halo_z", [False, True])
@pytest.mark.parametrize("form", stencil.THREESTEP_FORMS)
@pytest.mark.parametrize("shape,rounds,dtype", CASES)
def test_lean_pass_equals_three_single_steps_bitwise(gpu, form, shape, rounds, dtype, halo_z):
    T, Cp, Q, ref, T0, Cp0, Q0 = _inputs(shape, dtype, gpu)
    assert stencil.threestep_ok(T, form)
    T2 = _canary(T)
    stencil.diffusion3d_threestep_(T2, T, Cp, Q=Q, form=form, rounds=rounds, halo_z=halo_z, **KW)
    torch.cuda.synchronize()
    bad = (T2 != ref)
    print(shape, dtype, "form", form, "rounds", rounds, "halo_z", halo_z, "points differing:", int(bad.sum()))
    assert not torch.isnan(T2).any()
    assert torch.equal(T2, ref), bad.nonzero()[:8].tolist()
    assert torch.equal(T, T0) and torch.equal(Cp, Cp0) and torch.equal(Q, Q0)


def _boundary_equal(a, b):
    return all(torch.equal(a.select(d, i), b.select(d, i)) for d in range(3) for i in (0, -1))


def test_model_eager_and_captured_match_single_step_model(gpu, monkeypatch):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_VARIANT", "11")
    monkeypatch.setenv("IGG_STENCIL_THREESTEP", "1")
    monkeypatch.delenv("IGG_STENCIL_TWOSTEP", raising=False)
    monkeypatch.delenv("IGG_STENCIL_QUOTIENT", raising=False)
    igg.init_global_grid(24, 20, 64, quiet=True, init_MPI=False)
    a = Diffusion3D(dtype=torch.float64)
    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "0")
    b = Diffusion3D(dtype=torch.float64)
    assert a.three_step and a._deep_key() is not None
    assert not b.three_step and not b.two_step
    a.run(45)
    b.run(45)
    torch.cuda.synchronize()
    assert torch.equal(a.T, b.T)
    assert _boundary_equal(a.T2, a.T)
    a.capture(24)  # 45 = a replay of deep passes and 21 eager steps
    b.capture()
    assert a.graph is not None and a.graph_steps == 24
    a.run(45)
    b.run(45)
    torch.cuda.synchronize()
    assert torch.equal(a.T, b.T)
    assert _boundary_equal(a.T2, a.T)
