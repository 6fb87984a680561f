"""CPU tier of the two-step pass: it is a GPU kernel, so a CPU model never
enables it and the op refuses CPU tensors; the kernel-resource baseline holds
the new unit without scratch."""
import json
from pathlib import Path

import pytest
import torch

import igg
from igg import IGGError
from igg.ops import stencil

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("mode", ["auto", "1"])
def test_cpu_model_never_enables_the_pass(monkeypatch, mode):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", mode)
    igg.init_global_grid(12, 10, 16, quiet=True, init_MPI=False)
    m = Diffusion3D(dtype=torch.float64, device="cpu")
    assert not m.two_step and not m._two_step_now() and m.two_step_times == {}


def test_cpu_run_matches_steps():
    from igg.models.diffusion3d import Diffusion3D

    igg.init_global_grid(12, 10, 16, quiet=True, init_MPI=False)
    a = Diffusion3D(dtype=torch.float64, device="cpu")
    b = Diffusion3D(dtype=torch.float64, device="cpu")
    a.run(5)
    for _ in range(5):
        b.step()
    assert torch.equal(a.T, b.T) and torch.equal(a.T2, b.T2)


def test_twostep_op_refuses_cpu_tensors():
    T = torch.rand(6, 6, 8, dtype=torch.float64)
    Cp = 1 + torch.rand(6, 6, 8, dtype=torch.float64)
    T2 = T.clone()
    assert not stencil.twostep_ok(T)
    with pytest.raises(IGGError):
        stencil.diffusion3d_twostep_(T2, T, Cp, lam=1.0, dt=0.01, dx=0.3, dy=0.25, dz=0.2)
    assert torch.equal(T2, T)


def test_variant_property_tracks_the_selection():
    from igg.models.diffusion3d import Diffusion3D

    igg.init_global_grid(12, 10, 16, quiet=True, init_MPI=False)
    m = Diffusion3D(dtype=torch.float64, device="cpu", variant=0)
    m.two_step = True  # as a selection with variant 0 would
    assert m.two_step
    m.variant = 5
    assert m.variant == 5 and not m.two_step
    m.variant = 0
    assert m.two_step and not m._two_step_now()  # still a CPU model


def test_resource_baseline_holds_the_unit_without_scratch():
    base = json.loads((ROOT / "profiles" / "kernel_resources.json").read_text())
    rows = base.get("stencil2_kernels")
    assert rows, "stencil2_kernels missing from profiles/kernel_resources.json"
    assert len(rows) == 2 * len(stencil.TWOSTEP_FORMS)  # every form in f32 and f64
    for k, r in rows.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)
