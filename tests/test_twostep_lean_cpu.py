"""CPU tier of the quotient input of the two-step pass: the setting's parsing,
a CPU model never builds the array, the op refuses arrays it cannot read, and
the kernel-resource baseline holds the specialisations' unit without scratch."""
import json
from pathlib import Path

import pytest
import torch

import igg
from igg import IGGError
from igg.ops import stencil

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("value,want", [(None, "auto"), ("auto", "auto"), (" AUTO ", "auto"), ("0", "0"), ("1", "1")])
def test_env_parsing(monkeypatch, value, want):
    from igg.models._pingpong import two_step_env

    if value is None:
        monkeypatch.delenv("IGG_STENCIL_QUOTIENT", raising=False)
    else:
        monkeypatch.setenv("IGG_STENCIL_QUOTIENT", value)
    assert two_step_env("IGG_STENCIL_QUOTIENT") == want


def test_env_rejects_other_values(monkeypatch):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_QUOTIENT", "yes")
    igg.init_global_grid(12, 10, 16, quiet=True, init_MPI=False)
    with pytest.raises(ValueError, match="IGG_STENCIL_QUOTIENT"):
        Diffusion3D(dtype=torch.float64, device="cpu")


@pytest.mark.parametrize("mode", ["auto", "1"])
def test_cpu_model_never_builds_q(monkeypatch, mode):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "1")
    monkeypatch.setenv("IGG_STENCIL_QUOTIENT", mode)
    igg.init_global_grid(12, 10, 16, quiet=True, init_MPI=False)
    m = Diffusion3D(dtype=torch.float64, device="cpu")
    assert m.Q is None and "Q" not in m._fields
    m.run(3)
    m.mark_cp_modified()
    m.run(2)
    assert m.Q is None


def test_quotient_op_refuses_cpu_tensors():
    Cp = 1 + torch.rand(6, 6, 8, dtype=torch.float64)
    Q = torch.zeros_like(Cp)
    with pytest.raises(IGGError):
        stencil.quotient_(Q, Cp, lam=1.0, dt=0.01)
    assert not Q.any()


def _q_check(Q, Cp, match):
    with pytest.raises(IGGError, match=match):
        stencil._check_q(Q, Cp)


def test_q_of_another_place_shape_or_dtype_is_refused():
    # the check the two-step op runs on its Q argument (no GPU needed: meta
    # tensors carry device, shape and dtype)
    Cp = torch.empty((6, 6, 8), dtype=torch.float64, device="meta")
    _q_check(torch.empty((6, 6, 8), dtype=torch.float64), Cp, "GPU")            # a CPU array
    Cpc = torch.empty((6, 6, 8), dtype=torch.float64)
    _q_check(torch.empty((6, 6, 8), dtype=torch.float64), Cpc, "GPU")           # CPU next to CPU
    _q_check(torch.empty((6, 8, 6), dtype=torch.float64, device="meta"), Cp, "must match")    # another shape
    _q_check(torch.empty((6, 6, 8), dtype=torch.float32, device="meta"), Cp, "must match")    # another dtype


def test_twostep_op_refuses_a_cpu_q_before_any_launch():
    T = torch.rand(6, 6, 8, dtype=torch.float64)
    Cp = 1 + torch.rand(6, 6, 8, dtype=torch.float64)
    T2 = T.clone()
    with pytest.raises(IGGError):
        stencil.diffusion3d_twostep_(T2, T, Cp, lam=1.0, dt=0.01, dx=0.3, dy=0.25, dz=0.2, Q=torch.zeros_like(Cp))
    assert torch.equal(T2, T)


def test_resource_baseline_holds_the_new_unit_without_scratch():
    base = json.loads((ROOT / "profiles" / "kernel_resources.json").read_text())
    rows = base.get("stencil2q_kernels")
    assert rows, "stencil2q_kernels missing from profiles/kernel_resources.json"
    passes = {k: r for k, r in rows.items() if "twostep" in k}
    # per (form, dtype): row-spanning tile, quotient input, and both
    assert len(passes) == 3 * 2 * len(stencil.TWOSTEP_FORMS)
    assert len(rows) == len(passes) + 2  # and the quotient kernel in f32 and f64
    for k, r in rows.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)
