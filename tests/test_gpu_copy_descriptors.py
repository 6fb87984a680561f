"""Copy descriptors, GPU tier: every named case of tests/copy_oracle.py through
``copy2d_batch_kernel`` / ``copy3d_batch_kernel`` at every element size, with
plain and with system-scope stores, compared bitwise with the oracle over the
whole destination allocation; batches of more than MAX_BATCH regions, a
captured batch, and the row-chunk fallback of ``IGG_COPY_GATHER=0`` in a child
process. The CPU tier (tests/test_copy_descriptors.py) checks the plan and the
oracle themselves."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import igg  # noqa: E402,F401
from igg._native import native  # noqa: E402
from tests import copy_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _arena(fam, eb, base):
    """The arena of a family with its expected destination (computed once,
    read-only; the oracle asserts here, before anything runs on the GPU, that
    every index of every case lies inside the allocations)."""
    table = {"batch3": O.batch70, "batch2": O.batch70_2d}
    a = O.Arena(table[fam]() if fam in table else O.family(fam), eb, base)
    a.expected()
    return a


def _upload(a):
    dev = torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(a.src).to(dev), torch.from_numpy(a.dst).to(dev)


def _launch(a, src, dst, which, system):
    s = torch.cuda.current_stream().cuda_stream
    if any(a.cases[k].is3d for k in which):
        boxes, ptrs = a.args3d(src.data_ptr(), dst.data_ptr(), which)
        native.copy3d(boxes, ptrs, a.eb, True, s, system)
    else:
        native.copy2d(a.args2d(src.data_ptr(), dst.data_ptr(), which), a.eb, True, s, system)


def _plan(a, k, src, dst):
    c = a.cases[k]
    ptrs = a.pointers(k, src.data_ptr(), dst.data_ptr())
    if c.is3d:
        return native.copy3d_plan(list(c.box), ptrs, a.eb)
    return native.copy2d_plan(tuple(ptrs) + tuple(c.box), a.eb)


def _check_paths(a, src, dst):
    """Every case takes the path it is named for; at base 0 (torch's
    allocations are aligned to more than 16 bytes) also the vector width."""
    taken = {}
    for k, c in enumerate(a.cases):
        p = _plan(a, k, src, dst)
        if c.path is None:
            assert p["blocks"] == 0, c.name
            continue
        assert p["path"] == c.path, (c.name, a.eb, a.base, p)
        if a.base == 0:
            assert p["vec_bytes"] == c.vec.get(a.eb, 0), (c.name, a.eb, p)
        else:
            assert p["vec_bytes"] in (0, c.vec.get(a.eb, 0)), (c.name, a.eb, a.base, p)
        taken[c.name] = p
    return taken


def _compare(a, src, dst, what):
    torch.cuda.synchronize()
    bad = O.first_difference(dst.cpu().numpy(), a.expected(), a.eb)
    assert bad is None, f"{what}: {bad}"
    assert np.array_equal(src.cpu().numpy(), a.src), f"{what}: the source allocation changed"


@pytest.mark.parametrize("system", [False, True], ids=["plain", "system"])
@pytest.mark.parametrize("fam", O.FAMILIES3D + O.FAMILIES2D)
def test_named_cases_match_the_oracle(gpu, fam, system):
    """One launch per case; the cases of a family share one pair of
    allocations (a slot each), compared whole after the last launch."""
    for eb in O.ELEM_BYTES:
        for base in O.BASES:
            a = _arena(fam, eb, base)
            src, dst = _upload(a)
            _check_paths(a, src, dst)
            for k in range(len(a.cases)):
                _launch(a, src, dst, [k], system)
            _compare(a, src, dst, f"{fam} eb={eb} base={base} system={system}")


@pytest.mark.parametrize("system", [False, True], ids=["plain", "system"])
@pytest.mark.parametrize("fam", ["batch3", "batch2"])
def test_batch_of_70_regions(gpu, fam, system):
    """One call of 70 regions of every path: three launches (32 + 32 + 6),
    empty regions at 0, 31, 32 and 69; then a call of empty regions only."""
    for eb in O.ELEM_BYTES:
        a = _arena(fam, eb, 0)
        assert len(a.cases) == 70 and [k for k, c in enumerate(a.cases) if c.path is None] == [0, 31, 32, 69]
        src, dst = _upload(a)
        taken = _check_paths(a, src, dst)
        assert {p["path"] for p in taken.values()} == {"flat", "gather", "chunk"}
        _launch(a, src, dst, range(70), system)
        _compare(a, src, dst, f"{fam} eb={eb} system={system}")
        _launch(a, src, dst, [0, 31, 32, 69] * 9, system)  # 36 empty regions: nothing to launch
        _compare(a, src, dst, f"{fam} eb={eb} system={system}, empty call")


@pytest.mark.parametrize("fam", ["batch3", "batch2"])
def test_captured_batch_replays(gpu, fam):
    """The batch travels in the kernel arguments: a captured call must carry
    its three launches' descriptors into every replay."""
    eb = 8
    a = _arena(fam, eb, 0)
    src, dst = _upload(a)
    fresh = dst.clone()
    _launch(a, src, dst, range(70), False)  # eager first
    _compare(a, src, dst, f"{fam} eager")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        _launch(a, src, dst, range(70), False)
    for k in range(2):
        dst.copy_(fresh)
        torch.cuda.synchronize()
        g.replay()
        _compare(a, src, dst, f"{fam} replay {k}")
    del g


# ------------------------------------------------------- IGG_COPY_GATHER=0
GATHER_FAMILIES = ("gather_vec", "gather_scalar", "gather_outer", "layouts", "2d_gather")
CHILD_EBS = (4, 16)


def _child():
    """Runs in a fresh process with IGG_COPY_GATHER=0: the gather-family cases
    of both kernels on the row-chunk / flat paths; one line per case."""
    assert os.environ.get("IGG_COPY_GATHER") == "0"
    for fam in GATHER_FAMILIES:
        for eb in CHILD_EBS:
            a = _arena(fam, eb, 0)
            for k, c in enumerate(a.cases):
                if c.path != "gather":
                    continue
                one = O.Arena([c], eb, 0)
                want = one.expected()
                src, dst = _upload(one)
                p = _plan(one, 0, src, dst)
                _launch(one, src, dst, [0], False)
                torch.cuda.synchronize()
                bad = O.first_difference(dst.cpu().numpy(), want, eb)
                print(f"case {c.name} eb={eb} path={p['path']} vec={p['vec_bytes']} "
                      f"{'OK' if bad is None else 'MISMATCH ' + bad}", flush=True)
    print("child done", flush=True)


def test_gather_switched_off_in_a_child_process(gpu):
    env = dict(os.environ, IGG_COPY_GATHER="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--gather-off-child"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("case ")]
    want = sum(1 for fam in GATHER_FAMILIES for c in O.family(fam) if c.path == "gather") * len(CHILD_EBS)
    assert len(lines) == want and "child done" in r.stdout, (len(lines), want)
    for ln in lines:
        assert ln.endswith(" OK"), ln
        assert "path=gather" not in ln and " vec=0 " in ln, ln
    assert any("path=flat" in ln for ln in lines) and any("path=chunk" in ln for ln in lines)


if __name__ == "__main__":
    if sys.argv[1:] == ["--gather-off-child"]:
        _child()
    else:
        raise SystemExit("run with pytest")
