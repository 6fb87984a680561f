"""Wide halos on the host: ``halowidthx/y/z`` of ``init_global_grid``, the
ranges, the periodic single-process exchange against an oracle written from
the range table, multi-rank gloo exchanges and checkpoints."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import pytest
import torch

import igg
from igg.parallel import grid as G
from igg.parallel import halo as H
from tests._mp import MAX_TIMEOUT, ROOT, free_port

KW = dict(quiet=True, init_MPI=False, device_type="none")


def run_wide_ranks(nprocs: int, scenario: str, *args, timeout: float = 150.0, env_extra=None) -> list:
    """``tests/mp_worker_wide.py`` on ``nprocs`` local ranks; the first rank
    that fails stops the others, a timeout fails the test with every rank's
    output."""
    port = free_port()
    procs, logs = [], []
    for r in range(nprocs):
        env = dict(os.environ)
        env.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(r),
                    "WORLD_SIZE": str(nprocs), "LOCAL_RANK": str(r), "LOCAL_WORLD_SIZE": str(nprocs),
                    "OMP_NUM_THREADS": "1", "IGG_HOST_THREADS": "2",
                    "PYTHONPATH": ROOT + os.pathsep + env.get("PYTHONPATH", "")})
        env.update(env_extra or {})
        log = tempfile.TemporaryFile(mode="w+")
        logs.append(log)
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tests", "mp_worker_wide.py"), scenario, *map(str, args)],
            env=env, stdout=log, stderr=subprocess.STDOUT, text=True, cwd=ROOT))
    deadline = time.monotonic() + min(timeout, MAX_TIMEOUT)
    try:
        while True:
            codes = [p.poll() for p in procs]
            if any(c not in (None, 0) for c in codes) or all(c == 0 for c in codes) or time.monotonic() > deadline:
                break
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    outs = []
    for log in logs:
        log.seek(0)
        outs.append(log.read())
        log.close()
    codes = [p.returncode for p in procs]
    if any(c != 0 for c in codes):
        msg = "\n".join(f"--- rank {r} rc={c}\n{o[-2500:]}" for r, (c, o) in enumerate(zip(codes, outs)))
        raise AssertionError(f"scenario {scenario} failed or timed out:\n{msg}")
    return outs


# ------------------------------------------------------------------ validation
def test_default_widths_are_one():
    igg.init_global_grid(8, 8, 8, overlapx=4, **KW)
    gg = igg.get_global_grid()
    assert gg.halowidths.tolist() == [1, 1, 1]
    assert H.engine().grid.halowidths == [1, 1, 1]
    igg.finalize_global_grid(finalize_MPI=False)


def test_widths_are_stored_and_copied():
    igg.init_global_grid(12, 12, 12, overlapx=4, overlapy=6, overlapz=2, halowidthx=2, halowidthy=3, **KW)
    gg = igg.get_global_grid()
    assert gg.halowidths.tolist() == [2, 3, 1]
    assert H.engine().grid.halowidths == [2, 3, 1]
    gg.halowidths[0] = 7  # a deep copy: the grid itself is untouched
    assert igg.get_global_grid().halowidths.tolist() == [2, 3, 1]
    igg.finalize_global_grid(finalize_MPI=False)


@pytest.mark.parametrize("kw", [dict(halowidthx=0), dict(halowidthy=-1), dict(halowidthz=0)])
def test_width_below_one_is_refused(kw):
    with pytest.raises(igg.IGGError, match="must be greater than or equal to 1"):
        igg.init_global_grid(8, 8, 8, **kw, **KW)
    assert not igg.grid_is_initialized()


@pytest.mark.parametrize("kw", [dict(halowidthx=2), dict(halowidthy=2, overlapy=3), dict(halowidthz=3, overlapz=5)])
def test_width_needs_twice_the_overlap(kw):
    with pytest.raises(igg.IGGError, match=r"must be at least 2\*halowidthx"):
        igg.init_global_grid(16, 16, 16, **kw, **KW)
    assert not igg.grid_is_initialized()


def test_periodic_size_rule_stays():
    with pytest.raises(igg.IGGError, match=r"smaller than 2\*overlapx-1"):
        igg.init_global_grid(6, 8, 8, overlapx=4, halowidthx=2, periodx=1, **KW)
    igg.init_global_grid(7, 8, 8, overlapx=4, halowidthx=2, periodx=1, **KW)  # n = 2*o-1: slabs still disjoint
    igg.finalize_global_grid(finalize_MPI=False)


def test_field_with_too_little_overlap_is_refused():
    igg.init_global_grid(10, 10, 10, overlapx=4, overlapy=4, overlapz=4, halowidthx=2, halowidthy=2, halowidthz=2,
                         periodx=1, periody=1, periodz=1, **KW)
    A = torch.zeros(9, 10, 10, dtype=torch.float64)  # ol = 3 in x: a halo, but narrower than 2*2
    for fn in (lambda: igg.update_halo_(A), lambda: H.sendranges(1, 1, A), lambda: H.recvranges(2, 1, A)):
        with pytest.raises(igg.IGGError, match=r"ol\(A,dim\)<2\*halowidths\[dim\]"):
            fn()
    ft = H.field_tuple(A)
    with pytest.raises(igg.IGGError, match=r"ol\(A,dim\)<2\*halowidths\[dim\]"):
        igg.native.send_index(H.engine().grid, 0, 0, ft)
    # ol < 2: no halo there, as before (the other dimensions still exchange)
    B = torch.zeros(7, 10, 10, dtype=torch.float64)
    igg.update_halo_(B)
    with pytest.raises(igg.IGGError, match=r"ol\(A,dim\)<2\.$"):
        H.sendranges(1, 1, B)
    igg.finalize_global_grid(finalize_MPI=False)


def _geometry(fields):
    out = []
    for A in fields:
        for dim in (1, 2, 3):
            if G.ol(dim, A) < 2:
                continue
            out.append([H.sendranges(n, dim, A) for n in (1, 2)] + [H.recvranges(n, dim, A) for n in (1, 2)]
                       + [H.halosize(dim, A)])
    H.allocate_bufs(*fields)
    out.append([H.engine().pool_capacity(i, False) for i in range(len(fields))])
    out.append([tuple(H.sendbuf(1, 3, i + 1, A).shape) for i, A in enumerate(fields)])
    out.append(H.halo_plan_summary(*fields))
    return out


def test_defaults_match_a_grid_without_the_keywords():
    fields = [torch.zeros(9, 8, 7), torch.zeros(10, 8, 7), torch.zeros(9, 8, 8)]
    kw = dict(overlapx=3, overlapy=4, overlapz=2, periodx=1, periody=1, periodz=1)
    igg.init_global_grid(9, 8, 7, **kw, **KW)
    plain = _geometry(fields)
    igg.finalize_global_grid(finalize_MPI=False)
    igg.init_global_grid(9, 8, 7, halowidthx=1, halowidthy=1, halowidthz=1, **kw, **KW)
    assert _geometry(fields) == plain
    igg.finalize_global_grid(finalize_MPI=False)
    assert plain[0][0][0] == range(3, 4) and plain[0][4] == (8, 7)  # one plane, a 2-D halo


@pytest.mark.parametrize("w", [2, 3])
@pytest.mark.parametrize("o", [4, 5, 6, 7])
def test_ranges_follow_the_table(w, o):
    if o < 2 * w:
        with pytest.raises(igg.IGGError):
            igg.init_global_grid(20, 20, 20, overlapy=o, halowidthy=w, **KW)
        return
    n = 20
    igg.init_global_grid(n, n, n, overlapy=o, halowidthy=w, **KW)
    for dn in (-1, 0, 1):
        A = torch.zeros(n, n + dn, n)
        oa = o + dn
        if oa < 2 * w:
            with pytest.raises(igg.IGGError, match=r"ol\(A,dim\)<2\*halowidths"):
                H.sendranges(1, 2, A)
            continue
        m = n + dn
        zero_based = lambda r: (r[1].start - 1, r[1].stop - 1)  # noqa: E731
        assert zero_based(H.sendranges(1, 2, A)) == (oa - w, oa)
        assert zero_based(H.sendranges(2, 2, A)) == (m - oa, m - oa + w)
        assert zero_based(H.recvranges(1, 2, A)) == (0, w)
        assert zero_based(H.recvranges(2, 2, A)) == (m - w, m)
        assert H.sendranges(1, 2, A)[0] == range(1, n + 1) and H.sendranges(1, 2, A)[2] == range(1, n + 1)
        assert H.halosize(2, A) == (n, w, n)
    igg.finalize_global_grid(finalize_MPI=False)


def test_smaller_field_with_o4_w2_raises():
    igg.init_global_grid(12, 12, 12, overlapz=4, halowidthz=2, **KW)
    with pytest.raises(igg.IGGError, match=r"ol\(A,dim\)<2\*halowidths\[dim\]"):
        H.sendranges(2, 3, torch.zeros(12, 12, 11))
    igg.finalize_global_grid(finalize_MPI=False)


def test_buffers_gain_the_width():
    A = torch.zeros(11, 12, 13, dtype=torch.float64)
    igg.init_global_grid(11, 12, 13, overlapx=4, overlapy=4, overlapz=6, halowidthx=2, halowidthz=3, **KW)
    H.allocate_bufs(A)
    plane = igg.native.max_halo_elems(H.field_tuple(A))
    assert plane == 12 * 13
    assert H.engine().pool_capacity(0, False) >= 3 * plane * 8
    assert tuple(H.sendbuf(1, 3, 1, A).shape) == (11, 12, 3)
    assert tuple(H.recvbuf(2, 1, 1, A).shape) == (2, 12, 13)
    assert tuple(H.sendbuf(1, 2, 1, A).shape) == (11, 13)  # width 1 in y: a plane, as before
    s = H.halo_plan_summary(A)
    assert s[0]["dim"] == 1 and s[2]["dim"] == 3
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------- single-process periodic exchange
def _oracle(A: torch.Tensor, n, o, w) -> torch.Tensor:
    """update_halo of a periodic single-process grid from the range table:
    per dimension x, y, z the left send planes [ol-w, ol) land in the right
    receive planes [m-w, m), the right send planes [m-ol, m-ol+w) in [0, w)."""
    out = A.clone()
    for d in range(A.dim()):
        m = A.shape[d]
        oa = o[d] + m - n[d]
        if oa < 2:
            continue
        src = out.clone()
        left = [slice(None)] * A.dim()
        right = list(left)
        left[d], right[d] = slice(oa - w, oa), slice(m - w, m)
        out[tuple(right)] = src[tuple(left)]
        left[d], right[d] = slice(0, w), slice(m - oa, m - oa + w)
        out[tuple(left)] = src[tuple(right)]
    return out


def _fill(shape, dtype, order=None):
    v = torch.arange(1, 1 + int(torch.tensor(shape).prod()), dtype=torch.float64).view(shape)
    if dtype.is_complex:
        v = v.to(dtype) * (1 + 2j)
    else:
        v = (v % 30000).to(dtype) if dtype == torch.int16 else v.to(dtype)
    if order is not None:  # a dense tensor whose memory order is `order` (slowest first)
        inv = [order.index(d) for d in range(len(shape))]
        v = v.permute(order).contiguous().permute(inv)
        assert tuple(v.shape) == tuple(shape)
    return v


@pytest.mark.parametrize("mode", ["sequential", "onephase"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.int16, torch.complex128])
@pytest.mark.parametrize("w", [2, 3])
def test_periodic_exchange_matches_the_range_table(w, dtype, mode):
    n, o = (11, 12, 13), (2 * w,) * 3
    igg.init_global_grid(*n, periodx=1, periody=1, periodz=1, overlapx=o[0], overlapy=o[1], overlapz=o[2],
                         halowidthx=w, halowidthy=w, halowidthz=w, **KW)
    H.set_halo_mode(mode)
    for order in (None, (2, 0, 1), (1, 2, 0)):
        A = _fill(n, dtype, order)
        ref = _oracle(A, n, o, w)
        igg.update_halo_(A)
        assert torch.equal(A, ref), f"layout {order}"
    # two staggered fields in one call
    Vx, Vz = _fill((12, 12, 13), dtype), _fill((11, 12, 14), dtype)
    rx, rz = _oracle(Vx, n, o, w), _oracle(Vz, n, o, w)
    igg.update_halo_(Vx, Vz)
    assert torch.equal(Vx, rx) and torch.equal(Vz, rz)
    igg.finalize_global_grid(finalize_MPI=False)


def test_lower_dimensional_fields():
    igg.init_global_grid(12, 9, 1, periodx=1, periody=1, overlapx=4, overlapy=4, halowidthx=2, halowidthy=2, **KW)
    for shape in ((12,), (12, 9)):
        A = _fill(shape, torch.float64)
        ref = _oracle(A, (12, 9, 1), (4, 4, 2), 2)
        igg.update_halo_(A)
        assert torch.equal(A, ref)
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------------ multi-rank gloo
@pytest.mark.parametrize("periodic", [0, 1])
@pytest.mark.parametrize("nprocs,dims", [(2, (2, 1, 1)), (8, (2, 2, 2))])
def test_multirank_global_coordinates(nprocs, dims, periodic):
    """Both schedules, width 2 (tests/mp_worker_wide.py: scenario_halo); the
    one-phase exchange sends as many messages as with width 1."""
    outs = run_wide_ranks(nprocs, "halo", "cpu", periodic, *dims)
    for o in outs:
        m = re.search(r"wide halo OK MSGS2=(\d+) MSGS1=(\d+)", o)
        assert m, o[-2000:]
        assert int(m.group(1)) == int(m.group(2)) > 0


# ----------------------------------------------------------------- checkpoints
def test_checkpoint_records_and_checks_the_widths(tmp_path):
    prefix = str(tmp_path / "c")
    wide = dict(overlapx=4, overlapy=4, overlapz=4, halowidthx=2, halowidthy=2, halowidthz=2)
    igg.init_global_grid(10, 9, 8, **wide, **KW)
    A = torch.arange(720, dtype=torch.float64).view(10, 9, 8)
    igg.save_checkpoint(prefix, step=3, A=A)
    assert json.load(open(prefix + ".json"))["halowidths"] == [2, 2, 2]
    meta, f = igg.load_checkpoint(prefix)
    assert meta["step"] == 3 and torch.equal(f["A"], A)
    igg.finalize_global_grid(finalize_MPI=False)
    igg.init_global_grid(10, 9, 8, overlapx=4, overlapy=4, overlapz=4, **KW)  # same overlaps, width 1
    with pytest.raises(igg.IGGError, match="halowidths"):
        igg.load_checkpoint(prefix)
    # a manifest written before halo widths existed means one plane per side
    meta = json.load(open(prefix + ".json"))
    del meta["halowidths"]
    json.dump(meta, open(prefix + ".json", "w"))
    _, f = igg.load_checkpoint(prefix)
    assert torch.equal(f["A"], A)
    igg.finalize_global_grid(finalize_MPI=False)
    igg.init_global_grid(10, 9, 8, **wide, **KW)
    with pytest.raises(igg.IGGError, match="halowidths"):
        igg.load_checkpoint(prefix)
    igg.finalize_global_grid(finalize_MPI=False)
