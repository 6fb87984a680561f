"""The two-step pass (csrc/kernels/stencil2_kernels.hip): one kernel that
advances the field two time steps must leave, bitwise, what two single-step
launches leave - on shapes picked for where its ring logic can go wrong - and
the model that uses it must compute what the single-step model computes."""
import re

import pytest
import torch

import igg
from igg import IGGError
from igg.ops import stencil

pytestmark = pytest.mark.gpu

KW = dict(lam=1.3, dt=0.004, dx=0.3, dy=0.25, dz=0.2)  # dx != dy != dz: a swapped axis shows

# (shape, rounds): every ring point a boundary (inner box 1-2 wide); small;
# one row / one vector past a tile edge (8- and 16-row, 128/256/512-point
# tiles); several x chunks of <= 8 planes with lead-ins (rounds -1: a 4096-block
# target, so chunks of the minimum 4 planes); a row longer than the widest tile.
SHAPES = [((3, 3, 4), 0), ((4, 4, 4), 0), ((5, 6, 8), 0), ((9, 34, 130), 0), ((7, 33, 258), 0),
          ((70, 40, 64), -1), ((6, 20, 516), 0)]
# dtype and halo_z paired across the shapes (not the full product): every form
# meets f32, f64, halo_z on and off, each at several shapes.
FLAGS = [(torch.float64, False), (torch.float32, True), (torch.float64, True), (torch.float32, False)]
CASES = [(s, r, *FLAGS[(i + j) % 4]) for i, (s, r) in enumerate(SHAPES) for j in (0, 1)]
CASES = [c for c in CASES if c[0][2] % (16 // torch.empty(0, dtype=c[2]).element_size()) == 0]
CASES += [((9, 34, 132), 0, torch.float32, True), ((9, 34, 132), 0, torch.float32, False)]


def _inputs(shape, dtype, gpu):
    g = torch.Generator().manual_seed(7)
    n = shape[0] * shape[1] * shape[2]
    # distinct at every point, the boundary planes included
    T = (torch.randperm(n, generator=g).to(torch.float64) / n + 0.5).reshape(shape)
    Cp = 1 + 5 * torch.rand(shape, generator=g, dtype=torch.float64)
    return T.to(dtype).to(gpu), Cp.to(dtype).to(gpu)


def _canary(T):
    T2 = torch.full_like(T, float("nan"))
    for d in range(3):
        for i in (0, -1):
            T2.select(d, i).copy_(T.select(d, i))
    return T2


@pytest.mark.parametrize("form", stencil.TWOSTEP_FORMS)
@pytest.mark.parametrize("shape,rounds,dtype,halo_z", CASES)
def test_pass_equals_two_single_steps_bitwise(gpu, form, shape, rounds, dtype, halo_z):
    T, Cp = _inputs(shape, dtype, gpu)
    T0, Cp0 = T.clone(), Cp.clone()
    assert stencil.twostep_ok(T, form)
    tmp, ref = T.clone(), T.clone()
    stencil.diffusion3d_(tmp, T, Cp, variant=1, **KW)
    stencil.diffusion3d_(ref, tmp, Cp, variant=1, **KW)
    T2 = _canary(T)
    stencil.diffusion3d_twostep_(T2, T, Cp, form=form, rounds=rounds, halo_z=halo_z, **KW)
    torch.cuda.synchronize()
    bad = (T2 != ref)
    print(shape, dtype, "form", form, "halo_z", halo_z, "points differing:", int(bad.sum()))
    assert not torch.isnan(T2).any()
    assert torch.equal(T2, ref), bad.nonzero()[:8].tolist()
    assert torch.equal(T, T0) and torch.equal(Cp, Cp0)


@pytest.mark.parametrize("form", stencil.TWOSTEP_FORMS)
def test_unsupported_row_length_raises_without_launch(gpu, form):
    T, Cp = _inputs((12, 8, 10), torch.float32, gpu)  # 10 is no multiple of the 4-element f32 vector
    T2 = _canary(T)
    before = T2.clone()
    assert not stencil.twostep_ok(T, form)
    with pytest.raises(IGGError):
        stencil.diffusion3d_twostep_(T2, T, Cp, form=form, **KW)
    torch.cuda.synchronize()
    assert torch.equal(torch.isnan(T2), torch.isnan(before))
    assert torch.equal(torch.nan_to_num(T2), torch.nan_to_num(before))


def _boundary_equal(a, b):
    return all(torch.equal(a.select(d, i), b.select(d, i)) for d in range(3) for i in (0, -1))


NTS = (1, 2, 3, 7, 20, 45)


def _pair(monkeypatch, **grid):
    """(two-step model, single-step model) on one grid that stays initialised."""
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_VARIANT", "11")
    igg.init_global_grid(40, 36, 128, quiet=True, init_MPI=False, **grid)
    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "1")
    a = Diffusion3D(dtype=torch.float64)
    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "0")
    b = Diffusion3D(dtype=torch.float64)
    return a, b


def test_model_eager_matches_single_step_model(gpu, monkeypatch):
    a, b = _pair(monkeypatch)
    assert a.two_step and a._two_step_now() and not b.two_step
    for nt in NTS:
        a.run(nt)
        b.run(nt)
        torch.cuda.synchronize()
        assert torch.equal(a.T, b.T), nt
        assert _boundary_equal(a.T2, a.T), nt


def test_model_captured_matches_and_keeps_buffers(gpu, monkeypatch):
    a, b = _pair(monkeypatch)
    a.capture()
    b.capture()
    assert a.graph_steps == 20 and a.graph is not None
    for nt in NTS:
        a.run(nt)
        b.run(nt)
        torch.cuda.synchronize()
        assert torch.equal(a.T, b.T), nt
        assert _boundary_equal(a.T2, a.T), nt
    # a replay hands the buffers back in their roles (also with a 4k+2 graph)
    for steps in (20, 6):
        a.capture(steps)
        assert a.graph_steps == steps
        ptr = a.T.data_ptr()
        a.run(steps)
        b.run(steps)
        torch.cuda.synchronize()
        assert a.T.data_ptr() == ptr
        assert torch.equal(a.T, b.T), steps


def test_variant_assignment_switches_the_pass(gpu, monkeypatch):
    a, b = _pair(monkeypatch)
    v = a.variant
    assert a.two_step
    a.variant = 2
    assert not a.two_step and not a._two_step_now()
    a.run(4)  # single steps with the other kernel: same values
    b.run(4)
    torch.cuda.synchronize()
    assert torch.equal(a.T, b.T)
    a.variant = v
    assert a.two_step and a._two_step_now()


def test_periodic_grid_keeps_single_steps(gpu, monkeypatch):
    a, b = _pair(monkeypatch, periodx=1)
    assert not a.two_step and not a._two_step_now()
    a.run(6)
    b.run(6)
    torch.cuda.synchronize()
    assert torch.equal(a.T, b.T)


def test_auto_selection_records_its_times(gpu, monkeypatch):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "auto")
    monkeypatch.delenv("IGG_STENCIL_VARIANT", raising=False)
    igg.init_global_grid(40, 36, 128, quiet=True, init_MPI=False)
    m = Diffusion3D(dtype=torch.float64)
    assert "single" in m.two_step_times and any(k.startswith("t0@r") for k in m.two_step_times)
    assert all(x > 0 for x in m.two_step_times.values())
    assert m.variant_times and all(re.fullmatch(r"\d+@.*", k) for k in m.variant_times)
    assert isinstance(m.two_step, bool)
