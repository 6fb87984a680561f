"""The shared time loop's arithmetic (models/_pingpong.py PingPongModel.run /
capture) on a stub model: which launches ``run(nt)`` issues in which order -
eager realignment, graph replays, two-step passes, single steps, one exit
barrier - and what ``capture(steps)`` records. No grid, no tensors, no GPU."""
import types

import pytest

from igg.models import _pingpong
from igg.models._pingpong import PingPongModel

NEVER = 99


class _Graph:
    def __init__(self, log):
        self.log = log

    def replay(self):
        self.log.append("replay")


class Stub(PingPongModel):
    def __init__(self, key=None, ready_after=0):
        super().__init__()
        self.device = types.SimpleNamespace(type="cuda")
        self.fused = False
        self.log = []
        self.key = key  # pass key while the pass is on, None: off
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

    def with_graph(self, graph_steps, captured_key):
        self.graph = _Graph(self.log)
        self.graph_steps = graph_steps
        self._graph_two = captured_key
        return self


def _rest(n, key):
    return ["pass"] * (n // 2) + ["step"] * (n % 2) if key is not None else ["step"] * n


def _drained(nt):
    return ["drain"] if nt > 0 else []


@pytest.mark.parametrize("key", [None, 8])
def test_run_without_a_graph(key):
    for nt in range(46):
        m = Stub(key)
        m.run(nt)
        assert m.log == _rest(nt, key) + _drained(nt), nt
        assert m.replayed == []


@pytest.mark.parametrize("key", [None, (0, 3)])
@pytest.mark.parametrize("graph_steps", [2, 10, 20])
@pytest.mark.parametrize("r", [0, 1, 2, NEVER])
def test_run_with_a_matching_graph(key, graph_steps, r):
    for nt in range(46):
        m = Stub(key, ready_after=r).with_graph(graph_steps, key)
        m.run(nt)
        eager = min(r, nt, 2)
        left = nt - eager
        replays = left // graph_steps if r <= 2 and r <= nt else 0
        assert m.log == (["step"] * eager + ["replay"] * replays + _rest(left - replays * graph_steps, key)
                         + _drained(nt)), nt
        assert sum(m.replayed) == graph_steps * replays
        assert all(k % graph_steps == 0 for k in m.replayed)


@pytest.mark.parametrize("key, captured", [(None, 8), (8, None), (8, 4), ((0, 3), (0, 2))])
@pytest.mark.parametrize("graph_steps", [2, 10, 20])
def test_run_ignores_a_graph_of_another_setting(key, captured, graph_steps):
    for nt in range(46):
        m = Stub(key).with_graph(graph_steps, captured)
        m.run(nt)
        assert m.log == _rest(nt, key) + _drained(nt), nt
        assert m.replayed == []


def test_run_ignores_a_graph_of_another_capture_cfg():
    m = Stub(8).with_graph(2, 8)
    m._graph_cfg = ("fused", 1)  # the stub's _capture_cfg() is the base's None
    m.run(6)
    assert m.log == ["pass"] * 3 + ["drain"]


@pytest.mark.parametrize("key", [None, 8])
@pytest.mark.parametrize("steps", [2, 4, 6, 10, 20])
def test_capture_records_passes_then_steps(monkeypatch, key, steps):
    labels = []

    def fake_capture(record, what, uses_halo=True):
        labels.append((what, uses_halo))
        record()
        return "graph"

    monkeypatch.setattr(_pingpong, "capture_graph", fake_capture)
    m = Stub(key)
    m.capture(steps)
    recorded = ["pass"] * (steps // 4 * 2) + ["step"] * (steps % 4) if key is not None else ["step"] * steps
    assert m.log == ["start"] + recorded
    assert 2 * m.log.count("pass") + m.log.count("step") == steps
    assert (m.graph, m.graph_steps, m._graph_two, m._graph_cfg) == ("graph", steps, key, None)
    assert labels == [("Stub.capture", True)]


def test_capture_defaults(monkeypatch):
    monkeypatch.setattr(_pingpong, "capture_graph", lambda record, what, uses_halo=True: record())
    for key, steps in ((None, _pingpong.GRAPH_STEPS), (8, _pingpong.TWOSTEP_GRAPH_STEPS)):
        m = Stub(key)
        m.capture()
        assert m.graph_steps == steps


@pytest.mark.parametrize("steps", [0, 1, 3, 7, -2])
def test_capture_rejects_odd_and_zero(monkeypatch, steps):
    monkeypatch.setattr(_pingpong, "capture_graph", lambda *a, **k: pytest.fail("captured"))
    m = Stub(8).with_graph(4, 8)
    with pytest.raises(ValueError, match=r"Stub\.capture: steps must be even and >= 2"):
        m.capture(steps)
    assert m.log == [] and m.graph is not None  # nothing ran, the old graph stays


def test_capture_needs_a_gpu_model():
    m = Stub()
    m.device = types.SimpleNamespace(type="cpu")
    with pytest.raises(RuntimeError, match=r"Stub\.capture: hipGraphs need a GPU model"):
        m.capture(4)
    assert m.log == []
