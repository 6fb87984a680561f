"""The package's one timing loop: interleaved rounds, medians.

Every A/B the package decides at run time (kernel variant, two-step pass,
field placement) times its candidates this way: each round visits every
candidate once, so a drifting clock or a neighbour's load hits all of them
alike, and the median of the rounds drops the odd sample out.
"""
from __future__ import annotations

import torch


def interleaved_medians(cands, run, steps: int, rounds: int, warm: int) -> list:
    """Median ms per step of each candidate, in the order of ``cands``.
    ``run(c, k)`` enqueues ``k`` steps of candidate ``c`` on the current
    stream. First ``run(c, warm)`` of every candidate (code objects, caches),
    then ``rounds`` times over all candidates in order: event, ``run(c,
    steps)``, event, synchronize, elapsed / ``steps``."""
    s = torch.cuda.current_stream()
    for c in cands:
        run(c, warm)
    times = [[] for _ in cands]
    for _ in range(rounds):
        for t, c in zip(times, cands):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            run(c, steps)
            e1.record(s)
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / steps)
    return [sorted(t)[len(t) // 2] for t in times]
