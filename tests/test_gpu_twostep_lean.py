"""The two-step pass after its march loop was unrolled over three phases and
its specialisations were added (csrc/include/igg/stencil2_impl.hpp,
csrc/kernels/stencil2q_kernels.hip): every instantiation - the general
kernel, the one for tiles that span the row, and both with the quotient array
as input - must leave, bitwise, what two single-step launches leave, and the
model that keeps the quotient array must compute what the single-step model
computes, also after its heat capacity changed."""
import pytest
import torch

import igg
from igg.ops import stencil

pytestmark = pytest.mark.gpu

KW = dict(lam=1.3, dt=0.004, dx=0.3, dy=0.25, dz=0.2)  # dx != dy != dz: a swapped axis shows
F64, F32 = torch.float64, torch.float32

# (shape, rounds, dtypes):
#   march lengths of every residue mod 3 (n0 - 1 positions per chunk);
#   x chunks of 4, 5 and 6 planes (rounds -1: a 4096-block target, so the
#   shortest chunks the launch forms: 21 inner planes = 4 x 5 + 1, 68 = 17 x 4,
#   11 = 6 + 5), each marched with a two-position lead-in;
#   both sides of "the tile spans the row" for every form's tile width;
#   a last tile row past n1; a box whose inner box is one point wide.
SHAPES = [((n0, 6, 8), 0, (F64, F32)) for n0 in (5, 6, 7, 8)]
SHAPES += [((23, 12, 64), -1, (F64, F32)), ((70, 40, 64), -1, (F64, F32)), ((13, 12, 64), -1, (F64,))]
SHAPES += [((6, 20, n2), 0, (F64,)) for n2 in (512, 516, 256, 260, 128, 132)]
SHAPES += [((5, 10, 1024), 0, (F32,)), ((5, 10, 1028), 0, (F32,))]
SHAPES += [((7, 33, 128), 0, (F64, F32)), ((3, 3, 4), 0, (F64, F32))]
CASES = [(s, r, dt) for s, r, dts in SHAPES for dt in dts]

_cache = {}


def _inputs(shape, dtype, gpu):
    """(T, Cp, Q, two single steps of T) of a case: computed once, never written."""
    key = (shape, dtype)
    if key not in _cache:
        g = torch.Generator().manual_seed(11)
        n = shape[0] * shape[1] * shape[2]
        # distinct at every point, the boundary planes included
        T = (torch.randperm(n, generator=g).to(torch.float64) / n + 0.5).reshape(shape).to(dtype).to(gpu)
        Cp = (1 + 5 * torch.rand(shape, generator=g, dtype=torch.float64)).to(dtype).to(gpu)
        Q = torch.empty_like(Cp)
        stencil.quotient_(Q, Cp, lam=KW["lam"], dt=KW["dt"])
        tmp, ref = T.clone(), T.clone()
        stencil.diffusion3d_(tmp, T, Cp, variant=1, **KW)
        stencil.diffusion3d_(ref, tmp, Cp, variant=1, **KW)
        torch.cuda.synchronize()
        _cache[key] = (T, Cp, Q, ref, T.clone(), Cp.clone(), Q.clone())
    return _cache[key]


def _canary(T):
    T2 = torch.full_like(T, float("nan"))
    for d in range(3):
        for i in (0, -1):
            T2.select(d, i).copy_(T.select(d, i))
    return T2


@pytest.mark.parametrize("halo_z", [False, True])
@pytest.mark.parametrize("form", stencil.TWOSTEP_FORMS)
@pytest.mark.parametrize("shape,rounds,dtype", CASES)
def test_pass_with_q_equals_pass_with_cp_equals_two_steps(gpu, shape, rounds, dtype, form, halo_z):
    T, Cp, Q, ref, T0, Cp0, Q0 = _inputs(shape, dtype, gpu)
    assert stencil.twostep_ok(T, form)
    a, b = _canary(T), _canary(T)
    stencil.diffusion3d_twostep_(a, T, Cp, form=form, rounds=rounds, halo_z=halo_z, **KW)
    stencil.diffusion3d_twostep_(b, T, Cp, form=form, rounds=rounds, halo_z=halo_z, Q=Q, **KW)
    torch.cuda.synchronize()
    print(shape, dtype, "form", form, "halo_z", halo_z, "points differing: Cp pass", int((a != ref).sum()),
          "Q pass", int((b != ref).sum()))
    assert not torch.isnan(a).any() and not torch.isnan(b).any()
    assert torch.equal(a, ref), (a != ref).nonzero()[:8].tolist()
    assert torch.equal(b, ref), (b != ref).nonzero()[:8].tolist()
    assert torch.equal(T, T0) and torch.equal(Cp, Cp0) and torch.equal(Q, Q0)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_quotient_is_the_kernels_division(gpu, dtype):
    # 315 elements: a scalar tail behind the 16-byte vectors in both dtypes
    g = torch.Generator().manual_seed(3)
    Cp = (1 + 5 * torch.rand((5, 7, 9), generator=g, dtype=torch.float64)).to(dtype).to(gpu)
    Cp0 = Cp.clone()
    Q = torch.full_like(Cp, float("nan"))
    stencil.quotient_(Q, Cp, lam=KW["lam"], dt=KW["dt"])
    # IEEE division of the scalar as the kernels hold it (dt*lam rounded to the dtype)
    want = torch.full_like(Cp, KW["dt"] * KW["lam"]) / Cp
    assert torch.equal(Q, want) and torch.equal(Cp, Cp0)
    # and what a single-step kernel multiplies by: T = 0 except plane 2 = 1 and
    # unit spacings make the update of plane 1 exactly fma(q, 1, 0) = q
    T = torch.zeros_like(Cp)
    T[2] = 1
    T2 = T.clone()
    stencil.diffusion3d_(T2, T, Cp, variant=1, lam=KW["lam"], dt=KW["dt"], dx=1.0, dy=1.0, dz=1.0)
    torch.cuda.synchronize()
    assert torch.equal(T2[1, 1:-1, 1:-1], Q[1, 1:-1, 1:-1])


NTS = (1, 2, 3, 7, 20)


def _pair(monkeypatch, quotient="1"):
    """(two-step model with the quotient setting, single-step model) on one grid."""
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_VARIANT", "11")
    igg.init_global_grid(40, 36, 128, quiet=True, init_MPI=False)
    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "1")
    monkeypatch.setenv("IGG_STENCIL_QUOTIENT", quotient)
    a = Diffusion3D(dtype=torch.float64)
    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "0")
    b = Diffusion3D(dtype=torch.float64)
    return a, b


def test_q_model_matches_single_step_model(gpu, monkeypatch):
    a, b = _pair(monkeypatch)
    assert a.two_step and a.Q is not None and b.Q is None
    assert a.Q.shape == a.Cp.shape and a.Q.dtype == a.Cp.dtype
    assert "Q" not in a._fields
    for nt in NTS:
        a.run(nt)
        b.run(nt)
        torch.cuda.synchronize()
        assert torch.equal(a.T, b.T), nt


def test_q_follows_cp_eager_and_captured(gpu, monkeypatch):
    a, b = _pair(monkeypatch, quotient="auto")  # no timing with TWOSTEP=1: auto means on
    assert a.Q is not None
    q = a.Q.data_ptr()
    a.run(4)
    b.run(4)
    for m in (a, b):
        m.Cp.mul_(1.5)
    a.run(6)
    b.run(6)
    torch.cuda.synchronize()
    assert torch.equal(a.T, b.T)
    a.capture()
    b.capture()
    graph, ptr = a.graph, a.T.data_ptr()
    a.run(20)
    b.run(20)
    for m in (a, b):
        m.Cp.mul_(1.5)
    a.run(40)
    b.run(40)
    torch.cuda.synchronize()
    assert torch.equal(a.T, b.T)
    assert a.graph is graph and a.T.data_ptr() == ptr and a.Q.data_ptr() == q
    # a write torch does not see (here: through a raw pointer of the same
    # storage) needs the explicit mark
    stencil.quotient_(a.Cp, a.Cp.clone(), lam=1.0, dt=12.0)  # Cp = 12 / Cp through the native kernel
    b.Cp.copy_(a.Cp)
    a.mark_cp_modified()
    a.run(20)
    b.run(20)
    torch.cuda.synchronize()
    assert torch.equal(a.T, b.T)


def test_quotient_off_allocates_nothing(gpu, monkeypatch):
    a, b = _pair(monkeypatch, quotient="0")
    assert a.two_step and a.Q is None
    a.run(6)
    b.run(6)
    torch.cuda.synchronize()
    assert torch.equal(a.T, b.T)


def test_auto_times_both_key_families(gpu, monkeypatch):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "auto")
    monkeypatch.setenv("IGG_STENCIL_QUOTIENT", "auto")
    monkeypatch.delenv("IGG_STENCIL_VARIANT", raising=False)
    igg.init_global_grid(40, 36, 128, quiet=True, init_MPI=False)
    m = Diffusion3D(dtype=torch.float64)
    keys = m.two_step_times
    assert "single" in keys
    assert any(k.startswith("t0@r") for k in keys) and any(k.startswith("t0q@r") for k in keys)
    assert all(x > 0 for x in keys.values())
    best = min((k for k in keys if k != "single"), key=keys.get)
    if m.two_step:
        assert (m.Q is not None) == ("q@" in best)
    else:
        assert m.Q is None
