"""CPU tier of the three-step pass: the shared time loop's arithmetic with a
deeper pass (models/_pingpong.py) on a stub model - which launches ``run(nt)``
issues in which order and what ``capture(steps)`` records, and that a model
without the new hooks runs exactly as before -, the setting's parsing, a CPU
model never enables the pass, the op refuses CPU tensors, and the
kernel-resource baseline holds the new unit without scratch or spills."""
import json
import types
from pathlib import Path

import pytest
import torch

import igg
from igg import IGGError
from igg.models import _pingpong
from igg.models._pingpong import PingPongModel
from igg.ops import stencil

ROOT = Path(__file__).resolve().parent.parent
NEVER = 99


class _Graph:
    def __init__(self, log):
        self.log = log

    def replay(self):
        self.log.append("replay")


class Plain(PingPongModel):
    """A model as they were before the deep pass: none of the new hooks."""

    def __init__(self, key=None, ready_after=0):
        super().__init__()
        self.device = types.SimpleNamespace(type="cuda")
        self.fused = False
        self.log = []
        self.key = key  # pass key while the two-step pass is on, None: off
        self.ready_after = ready_after  # eager steps until the graph is ready
        self.replayed = []

    def _two_step_now(self):
        return self.key is not None

    def _pass_key(self):
        return self.key

    def _step(self):
        self.log.append("step")

    def _pass(self):
        self.log.append("pass")

    def _drain(self):
        self.log.append("drain")

    def _capture_start(self):
        self.log.append("start")

    def _graph_ready(self):
        return self.log.count("step") >= self.ready_after

    def _replayed(self, k):
        self.replayed.append(k)

    def with_graph(self, graph_steps, captured_key, captured_deep=None):
        self.graph = _Graph(self.log)
        self.graph_steps = graph_steps
        self._graph_two = captured_key
        self._graph_deep = captured_deep
        return self


class Deep(Plain):
    def __init__(self, key=8, deep=(0, 2), ready_after=0):
        super().__init__(key, ready_after)
        self.deep = deep  # deep key while the three-step pass is on, None: off

    def _deep_key(self):
        return self.deep

    def _deep_pass(self):
        self.log.append("deep")


def _rest(n, key, deep):
    """What run() issues for n steps no replay covers."""
    log = []
    if deep is not None:
        log, n = ["deep"] * (n // 3), n % 3
    if key is not None:
        log, n = log + ["pass"] * (n // 2), n % 2
    return log + ["step"] * n


def _steps(log):
    return 3 * log.count("deep") + 2 * log.count("pass") + log.count("step")


def _drained(nt):
    return ["drain"] if nt > 0 else []


def test_run_without_a_graph():
    for nt in range(46):
        m = Deep()
        m.run(nt)
        assert m.log == ["deep"] * (nt // 3) + ["pass"] * (nt % 3 // 2) + ["step"] * (nt % 3 % 2) + _drained(nt), nt
        assert _steps(m.log) == nt and m.replayed == []


@pytest.mark.parametrize("graph_steps", [6, 24, 40])
@pytest.mark.parametrize("r", [0, 1, 2, NEVER])
def test_run_with_a_matching_graph(graph_steps, r):
    for nt in range(46):
        m = Deep(ready_after=r).with_graph(graph_steps, 8, (0, 2))
        m.run(nt)
        eager = min(r, nt, 2)
        left = nt - eager
        replays = left // graph_steps if r <= 2 and r <= nt else 0
        assert m.log == (["step"] * eager + ["replay"] * replays + _rest(left - replays * graph_steps, 8, (0, 2))
                         + _drained(nt)), nt
        assert sum(m.replayed) == graph_steps * replays


@pytest.mark.parametrize("deep, captured", [((0, 2), None), (None, (0, 2)), ((0, 2), (0, 3))])
def test_run_ignores_a_graph_of_another_deep_key(deep, captured):
    for nt in range(46):
        m = Deep(deep=deep).with_graph(6, 8, captured)
        m.run(nt)
        assert m.log == _rest(nt, 8, deep) + _drained(nt), nt
        assert m.replayed == []


def _capture(monkeypatch, m, *steps):
    labels = []

    def fake_capture(record, what, uses_halo=True):
        labels.append((what, uses_halo))
        record()
        return "graph"

    monkeypatch.setattr(_pingpong, "capture_graph", fake_capture)
    m.capture(*steps)
    return labels


@pytest.mark.parametrize("steps", range(2, 26, 2))
def test_capture_records_deep_passes_then_passes_then_steps(monkeypatch, steps):
    m = Deep()
    labels = _capture(monkeypatch, m, steps)
    rest = steps % 6  # 0, 2 or 4: two single steps, or two two-step passes
    recorded = ["deep"] * (steps // 6 * 2) + ["pass"] * (rest // 4 * 2) + ["step"] * (rest % 4)
    assert m.log == ["start"] + recorded
    assert _steps(m.log) == steps
    # every part swaps the buffers an even number of times
    assert all(m.log.count(k) % 2 == 0 for k in ("deep", "pass", "step"))
    assert (m.graph, m.graph_steps, m._graph_two, m._graph_deep, m._graph_cfg) == ("graph", steps, 8, (0, 2), None)
    assert labels == [("Deep.capture", True)]


def test_capture_defaults(monkeypatch):
    for m, steps in ((Deep(), _pingpong.THREESTEP_GRAPH_STEPS), (Deep(deep=None), _pingpong.TWOSTEP_GRAPH_STEPS),
                     (Deep(key=None, deep=None), _pingpong.GRAPH_STEPS)):
        _capture(monkeypatch, m)
        assert m.graph_steps == steps
    # an even number of steps, and whole graphs make up the benchmark's 200
    assert _pingpong.THREESTEP_GRAPH_STEPS % 2 == 0 and 200 % _pingpong.THREESTEP_GRAPH_STEPS == 0


@pytest.mark.parametrize("steps", [0, 1, 3, 7, 9, 21, -2])
def test_capture_rejects_odd_and_zero(monkeypatch, steps):
    monkeypatch.setattr(_pingpong, "capture_graph", lambda *a, **k: pytest.fail("captured"))
    m = Deep().with_graph(6, 8, (0, 2))
    with pytest.raises(ValueError, match=r"Deep\.capture: steps must be even and >= 2"):
        m.capture(steps)
    assert m.log == [] and m.graph is not None  # nothing ran, the old graph stays


@pytest.mark.parametrize("key", [None, 8])
def test_a_model_without_the_hooks_runs_as_before(monkeypatch, key):
    for nt in range(46):
        want = (["pass"] * (nt // 2) + ["step"] * (nt % 2) if key is not None else ["step"] * nt) + _drained(nt)
        m = Plain(key)
        m.run(nt)
        assert m.log == want, nt
        for gs in (2, 10, 20):
            m = Plain(key).with_graph(gs, key)
            m.run(nt)
            left = nt % gs
            assert m.log == ["replay"] * (nt // gs) + (["pass"] * (left // 2) + ["step"] * (left % 2)
                                                       if key is not None else ["step"] * left) + _drained(nt), (nt, gs)
    for steps in (2, 4, 6, 10, 20, 24):
        m = Plain(key)
        _capture(monkeypatch, m, steps)
        recorded = ["pass"] * (steps // 4 * 2) + ["step"] * (steps % 4) if key is not None else ["step"] * steps
        assert m.log == ["start"] + recorded
        assert (m.graph_steps, m._graph_two, m._graph_deep) == (steps, key, None)
    m = Plain(key)
    with pytest.raises(NotImplementedError):
        m._deep_pass()


@pytest.mark.parametrize("value,want", [(None, "auto"), ("auto", "auto"), (" AUTO ", "auto"), ("0", "0"), ("1", "1")])
def test_env_parsing(monkeypatch, value, want):
    if value is None:
        monkeypatch.delenv("IGG_STENCIL_THREESTEP", raising=False)
    else:
        monkeypatch.setenv("IGG_STENCIL_THREESTEP", value)
    assert _pingpong.two_step_env("IGG_STENCIL_THREESTEP") == want


@pytest.mark.parametrize("value", ["yes", "2", "on", ""])
def test_env_rejects_other_values(monkeypatch, value):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_THREESTEP", value)
    igg.init_global_grid(12, 10, 16, quiet=True, init_MPI=False)
    with pytest.raises(ValueError, match="IGG_STENCIL_THREESTEP"):
        Diffusion3D(dtype=torch.float64, device="cpu")


@pytest.mark.parametrize("mode", ["auto", "1"])
def test_cpu_model_never_enables_the_pass(monkeypatch, mode):
    from igg.models.diffusion3d import Diffusion3D

    monkeypatch.setenv("IGG_STENCIL_THREESTEP", mode)
    igg.init_global_grid(12, 10, 16, quiet=True, init_MPI=False)
    a = Diffusion3D(dtype=torch.float64, device="cpu")
    b = Diffusion3D(dtype=torch.float64, device="cpu")
    assert not a.three_step and a._deep_key() is None and a.three_step_times == {} and a.Q is None
    a.three_step = True  # as a selection would: still a CPU model
    a.two_step = True
    assert a.three_step and a._deep_key() is None
    a.run(7)
    for _ in range(7):
        b.step()
    assert torch.equal(a.T, b.T) and torch.equal(a.T2, b.T2)


def test_threestep_op_refuses_cpu_tensors():
    T = torch.rand(6, 6, 8, dtype=torch.float64)
    Cp = 1 + torch.rand(6, 6, 8, dtype=torch.float64)
    T2 = T.clone()
    assert not stencil.threestep_ok(T)
    for Q in (torch.zeros_like(Cp), None):
        with pytest.raises(IGGError):
            stencil.diffusion3d_threestep_(T2, T, Cp, Q=Q, lam=1.0, dt=0.01, dx=0.3, dy=0.25, dz=0.2)
        assert torch.equal(T2, T)


def test_shapes_the_kernel_takes():
    ok = stencil.native.diffusion3d_threestep_ok
    assert len(stencil.THREESTEP_FORMS) >= 1
    assert ok([6, 20, 512], 8, 0) and ok([6, 20, 1024], 4, 0) and ok([3, 3, 4], 4, 0)
    assert not ok([6, 20, 516], 8, 0) and not ok([6, 20, 514], 8, 0)  # a row past the tile
    assert not ok([6, 20, 1028], 4, 0) and not ok([6, 20, 130], 4, 0)  # ..., no vector multiple
    assert not ok([2, 20, 64], 8, 0) and not ok([6, 20, 64], 8, len(stencil.THREESTEP_FORMS))


def test_resource_baseline_holds_the_unit_without_scratch():
    base = json.loads((ROOT / "profiles" / "kernel_resources.json").read_text())
    rows = base.get("stencil3_kernels")
    assert rows, "stencil3_kernels missing from profiles/kernel_resources.json"
    assert len(rows) == 2 * len(stencil.THREESTEP_FORMS)  # every form in f32 and f64
    for k, r in rows.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)
