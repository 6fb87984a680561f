"""CPU tier of the two-step acoustic pass: it is a GPU kernel, so a CPU model
never enables it and the op refuses CPU tensors; a bad IGG_ACOUSTIC_TWOSTEP is an
error; the build's code objects hold the new unit without scratch, spills or
LDS."""
import importlib.util as ilu
from pathlib import Path

import pytest
import torch

import igg
from igg import IGGError
from igg.models.acoustic2d import Acoustic2D, acoustic2d_reference
from igg.ops import stencil

ROOT = Path(__file__).resolve().parent.parent


def test_cpu_model_keeps_single_steps_and_matches_the_reference(monkeypatch):
    monkeypatch.setenv("IGG_ACOUSTIC_TWOSTEP", "1")
    igg.init_global_grid(20, 16, 1, quiet=True, init_MPI=False)
    m = Acoustic2D(dtype=torch.float64, device="cpu")
    assert m.two_step is False and not m._two_step_now() and m.two_step_times == {}
    assert m.two_step_chunk == 0 and not hasattr(m, "variant")
    P, Vx, Vy = m.P.clone(), m.Vx.clone(), m.Vy.clone()
    m.run(5)
    for _ in range(5):
        P, Vx, Vy = acoustic2d_reference(P, Vx, Vy, dt=m.dt, K=m.K, rho=m.rho, dx=m.dx, dy=m.dy)
    assert (m.P - P).abs().max().item() < 1e-12
    assert (m.Vx - Vx).abs().max().item() < 1e-12 and (m.Vy - Vy).abs().max().item() < 1e-12
    m.two_step = True  # settable, and still not eligible on a CPU model
    assert m.two_step and not m._two_step_now()


def test_cpu_model_under_auto_times_nothing(monkeypatch):
    monkeypatch.setenv("IGG_ACOUSTIC_TWOSTEP", "auto")
    igg.init_global_grid(20, 16, 1, quiet=True, init_MPI=False)
    m = Acoustic2D(dtype=torch.float64, device="cpu")
    assert m.two_step is False and m.two_step_times == {}


def test_twostep_op_refuses_cpu_tensors():
    P, Vx, Vy = torch.rand(6, 8), torch.rand(7, 8), torch.rand(6, 9)
    out = tuple(torch.full_like(t, float("nan")) for t in (P, Vx, Vy))
    assert not stencil.acoustic2d_twostep_ok(P)
    with pytest.raises(IGGError):
        stencil.acoustic2d_twostep_(*out, P, Vx, Vy, dt=0.01, K=1.0, rho=1.0, dx=0.3, dy=0.25)
    assert all(torch.isnan(t).all() for t in out)


def test_native_shape_rule():
    from igg._native import native

    ok = native.acoustic2d_twostep_ok
    assert ok(1, 8, 4) and ok(1, 4, 8) and ok(8192, 8192, 4)
    assert not ok(12, 10, 4) and not ok(12, 4, 4) and not ok(12, 2, 8) and not ok(12, 7, 8)
    assert not ok(0, 8, 4) and not ok(12, 8, 2)


@pytest.mark.parametrize("value", ["2", "on", ""])
def test_bad_environment_value_raises(monkeypatch, value):
    monkeypatch.setenv("IGG_ACOUSTIC_TWOSTEP", value)
    igg.init_global_grid(20, 16, 1, quiet=True, init_MPI=False)
    with pytest.raises(ValueError, match="IGG_ACOUSTIC_TWOSTEP"):
        Acoustic2D(dtype=torch.float64, device="cpu")


def test_code_objects_hold_the_unit_without_scratch_spills_or_lds():
    spec = ilu.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = ilu.module_from_spec(spec)
    spec.loader.exec_module(kr)
    objs = kr.objects()
    if not objs:
        pytest.skip("no HIP objects under build/native (run `python build.py`)")
    rows = kr.table(objs).get("acoustic2_kernels")
    assert rows and len(rows) == 2, rows  # f32 and f64
    for k, r in rows.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, (k, r)
