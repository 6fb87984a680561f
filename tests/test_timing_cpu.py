"""utils.timing.interleaved_medians with a scripted clock: the order in which
it runs the candidates (warm all, then every round all of them in order) and
the per-candidate median per step it returns. No GPU: the events are fakes."""
import types

from igg.utils import timing


class _Events:
    """Stands in for torch.cuda: events whose ``elapsed_time`` hands out the
    scripted milliseconds in the order the samples are taken."""

    def __init__(self, ms, log):
        self.ms, self.log = list(ms), log

    def current_stream(self):
        return "stream"

    def Event(self, enable_timing=False):
        assert enable_timing
        return _Event(self)


class _Event:
    def __init__(self, clock):
        self.clock = clock

    def record(self, stream):
        assert stream == "stream"
        self.clock.log.append("record")

    def synchronize(self):
        self.clock.log.append("sync")

    def elapsed_time(self, other):
        assert other is not self
        return self.clock.ms.pop(0)


def test_interleaved_order_and_medians(monkeypatch):
    log = []
    # rounds x candidates, ms per sample of `steps` = 4 steps
    script = [[8.0, 40.0, 4.0],
              [4.0, 44.0, 12.0],
              [12.0, 36.0, 8.0],
              [400.0, 4.0, 8.0],
              [8.0, 40.0, 0.4]]
    clock = _Events([ms for row in script for ms in row], log)
    monkeypatch.setattr(timing, "torch", types.SimpleNamespace(cuda=clock))
    cands = ["a", ("b", 1), None]  # any objects, hashable or not: results come back by position
    med = timing.interleaved_medians(cands, lambda c, k: log.append((c, k)), steps=4, rounds=5, warm=2)
    assert med == [2.0, 10.0, 2.0]  # medians of the five samples, per step
    assert log == [(c, 2) for c in cands] + [x for _ in range(5) for c in cands
                                             for x in ("record", (c, 4), "record", "sync")]
    assert clock.ms == []


def test_even_round_count_takes_the_upper_median(monkeypatch):
    clock = _Events([3.0, 1.0, 2.0, 4.0], [])
    monkeypatch.setattr(timing, "torch", types.SimpleNamespace(cuda=clock))
    assert timing.interleaved_medians(["x"], lambda c, k: None, steps=1, rounds=4, warm=0) == [3.0]
