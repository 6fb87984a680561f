"""The adjoint acoustic kernel (csrc/kernels/acoustic_adj_kernels.hip) against
its host twin (csrc/acoustic_adj_host.cpp), bit for bit, and the layers above
it on the GPU: ``igg.autograd.acoustic2d`` and ``Acoustic2D.adjoint_run``.

Every input is carved out of NaN padding and the three outputs out of ONE
sentinel-filled allocation that is compared whole: a read beyond an array that
reaches a result, or a store beyond an array, fails the comparison. The shapes
are the smallest at which the layout can go wrong. With ``W = 62*VJ`` columns
owned by a wave (VJ = 4 float32, 2 float64): the smallest vector row, one
vector less than a segment, exactly one segment (the column-``ny`` lane then
opens a segment of its own), one vector more, two segments; rows of x around
the chunk; and the one-point-per-lane form around its 62-column segment.

NaN results are compared as NaN (the host's and the device's default NaN
differ in the sign bit); every other value bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import igg
from igg._native import native
from igg.ops import stencil
from tests._mp import ROOT
from tests.mp_worker_acoustic_adjoint import dyadic_model, global_adjoint, identity_sides, run_ranks, single_rank_size
from tests.test_acoustic_adjoint_cpu import RKW, bits, check_boundary_rule, check_errors, random_fields, shapes

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
PAD = 1024
SENTINEL = -7.0


def canon(t):
    """Bits of ``t`` with every NaN replaced by one NaN."""
    t = t.clone()
    t[torch.isnan(t)] = float("nan")
    return bits(t)


def nan_padded(src, gpu):
    """``src`` on the device in the middle of a buffer of NaN (16-byte aligned)."""
    n = src.numel()
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=src.dtype, device=gpu)
    v = buf[PAD:PAD + n].view(src.shape)
    v.copy_(src)
    return v


def sentinel_outputs(shps, dtype, gpu):
    """(whole buffer, three views, their offsets): the outputs one after the
    other in one buffer of SENTINEL, PAD elements around and between them, each
    starting at a multiple of four elements."""
    offs, o = [], PAD
    for s in shps:
        offs.append(o)
        o += -(-(s[0] * s[1]) // 4) * 4 + PAD
    buf = torch.full((o,), SENTINEL, dtype=dtype, device=gpu)
    return buf, [buf[f:f + s[0] * s[1]].view(s) for f, s in zip(offs, shps)], offs


def whole(expected, offs, total):
    buf = torch.full((total,), SENTINEL, dtype=expected[0].dtype)
    for f, e in zip(offs, expected):
        buf[f:f + e.numel()] = e.flatten()
    return buf


def special_fields(nx, ny, dtype, seed):
    """Random fields with -0.0, infinities and NaN scattered in."""
    gin = random_fields(nx, ny, dtype, seed)
    gen = torch.Generator().manual_seed(seed + 7)
    for g in gin:
        flat = g.view(-1)
        for v in (-0.0, float("inf"), float("-inf"), float("nan"), 0.0):
            k = max(1, flat.numel() // 40)
            flat[torch.randint(0, flat.numel(), (k,), generator=gen)] = v
    return gin


def run_case(nx, ny, dtype, gpu, chunk=0, seed=0, special=False):
    gin = special_fields(nx, ny, dtype, seed) if special else random_fields(nx, ny, dtype, seed)
    want = [torch.empty_like(g) for g in gin]
    stencil.acoustic2d_adjoint_(*want, *gin, **RKW)
    gd = [nan_padded(g, gpu) for g in gin]
    buf, outs, offs = sentinel_outputs(shapes(nx, ny), dtype, gpu)
    stencil.acoustic2d_adjoint_(*outs, *gd, chunk=chunk, **RKW)
    torch.cuda.synchronize()
    got, exp = canon(buf.cpu()), canon(whole(want, offs, buf.numel()))
    assert torch.equal(got, exp), (nx, ny, dtype, chunk, int((got != exp).sum()),
                                   (got != exp).nonzero()[:6].flatten().tolist(), offs)
    for A, src in zip(gd, gin):
        assert torch.equal(canon(A.cpu()), canon(src)), "an input was written"


def vj_of(dtype):
    return 4 if dtype == F32 else 2


@pytest.mark.parametrize("dtype", [F32, F64])
def test_vector_form_equals_host_twin(gpu, dtype):
    vj = vj_of(dtype)
    W = 62 * vj
    c = native.acoustic2d_adjoint_chunk()
    nxs = sorted({1, 2, 3, max(c - 1, 1), c, c + 1, 2 * c + 1})
    n = 0
    for ny in (2 * vj, W - vj, W, W + vj, 2 * W):
        for nx in nxs:
            for chunk in (0, 1, 2, 5):
                run_case(nx, ny, dtype, gpu, chunk=chunk, seed=n % 5)
                n += 1
    assert n == 5 * len(nxs) * 4


@pytest.mark.parametrize("dtype", [F32, F64])
def test_one_point_per_lane_form_equals_host_twin(gpu, dtype):
    vj = vj_of(dtype)
    nys = [1, 3, 61, 62, 63, 125, vj] + ([2 * vj - 1] if dtype == F32 else [])
    # (float64: ny = 62 is a multiple of VJ and runs the vector form; 2*VJ - 1 would be 3)
    for ny in nys:
        for nx in (1, 2, 9):
            for chunk in (0, 1, 5):
                run_case(nx, ny, dtype, gpu, chunk=chunk, seed=ny % 5)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_special_values(gpu, dtype):
    vj = vj_of(dtype)
    for nx, ny in ((9, 62 * vj + vj), (5, 63), (3, 2 * vj)):
        run_case(nx, ny, dtype, gpu, seed=3, special=True)
        run_case(nx, ny, dtype, gpu, chunk=3, seed=4, special=True)


def test_set_chunk_changes_the_default(gpu):
    c = native.acoustic2d_adjoint_chunk()
    try:
        native.acoustic2d_adjoint_set_chunk(7)
        assert native.acoustic2d_adjoint_chunk() == 7
        run_case(16, 24, F32, gpu, seed=2)
    finally:
        native.acoustic2d_adjoint_set_chunk(0)
    assert native.acoustic2d_adjoint_chunk() == c


def test_boundary_and_nan_rules_on_the_device(gpu):
    def run(gin):
        gout = [torch.full_like(g, 7.0).to(gpu) for g in gin]
        stencil.acoustic2d_adjoint_(*gout, *(g.to(gpu) for g in gin), **RKW)
        return [g.cpu() for g in gout]

    check_boundary_rule(run)


def test_errors_on_the_device(gpu):
    check_errors(gpu)


def test_captured_graph_replayed_after_the_inputs_are_rewritten(gpu):
    nx, ny = 19, 256
    a, b = random_fields(nx, ny, F64, 30), random_fields(nx, ny, F64, 31)
    gd = [t.to(gpu) for t in a]
    out = [torch.zeros_like(t) for t in gd]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        stencil.acoustic2d_adjoint_(*out, *gd, **RKW)  # code objects loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stencil.acoustic2d_adjoint_(*out, *gd, **RKW)
    for src in (a, b):
        for d, s in zip(gd, src):
            d.copy_(s)
        for o in out:
            o.fill_(5.0)
        graph.replay()
        torch.cuda.synchronize()
        want = [torch.empty_like(t) for t in src]
        stencil.acoustic2d_adjoint_(*want, *src, **RKW)
        assert all(torch.equal(bits(o.cpu()), bits(w)) for o, w in zip(out, want))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_autograd_on_the_gpu_equals_the_cpu(gpu, dtype):
    nx, ny = 11, 72
    x, w = random_fields(nx, ny, dtype, 40), random_fields(nx, ny, dtype, 41)
    res = []
    for dev in (torch.device("cpu"), gpu):
        xs = [t.clone().to(dev).requires_grad_() for t in x]
        outs = igg.autograd.acoustic2d(*xs, **RKW)
        assert all(o.device == xs[0].device for o in outs)
        grads = torch.autograd.grad(outs, xs, [t.to(dev) for t in w])
        res.append([t.detach().cpu() for t in outs] + [t.cpu() for t in grads])
    for a, b in zip(*res):
        assert torch.equal(bits(a), bits(b))


def _model_pair(gpu, shape, periodic, dtype=F64):
    igg.init_global_grid(shape[0], shape[1], 1, periodx=periodic, periody=periodic, quiet=True, init_MPI=False)
    return dyadic_model(gpu, dtype), dyadic_model(torch.device("cpu"), dtype)


@pytest.mark.parametrize("twostep", ["0", "1"])
@pytest.mark.parametrize("periodic", [0, 1])
def test_adjoint_run_of_a_gpu_model_equals_the_cpu_model(gpu, monkeypatch, periodic, twostep):
    monkeypatch.setenv("IGG_ACOUSTIC_TWOSTEP", twostep)
    a, b = _model_pair(gpu, (20, 32), periodic)
    assert a.two_step == (twostep == "1" and not periodic)
    g = random_fields(20, 32, F64, 42)
    names = ("P", "Vx", "Vy", "P2", "Vx2", "Vy2")
    before = [getattr(a, k).clone() for k in names]
    want = b.adjoint_run(5, *g)
    got = a.adjoint_run(5, *(t.to(gpu) for t in g))
    assert all(t.device == a.P.device for t in got)
    assert all(torch.equal(bits(x.cpu()), bits(y)) for x, y in zip(got, want))
    assert all(torch.equal(getattr(a, k), v) for k, v in zip(names, before))
    # and it is the transpose of what run(5) does on this model, two-step pass included (exact: dyadic)
    lhs, rhs = identity_sides(a, 5)
    assert lhs == rhs and lhs != 0
    igg.finalize_global_grid(finalize_MPI=False)


def test_adjoint_run_of_a_fused_gpu_model(gpu):
    """Fused on a periodic grid: the fused step leaves bitwise single steps, so
    ``adjoint_run`` is its transpose too and equals the CPU model's. On a
    loopback grid ``accumulate_halo_`` has no transposed exchange:
    ``adjoint_run`` raises as it does and touches nothing."""
    a, b = _model_pair(gpu, (66, 64), 1)
    assert a.set_fused(True)
    g = random_fields(66, 64, F64, 43)
    want = b.adjoint_run(5, *g)
    got = a.adjoint_run(5, *(t.to(gpu) for t in g))
    assert a.fused and all(torch.equal(bits(x.cpu()), bits(y)) for x, y in zip(got, want))
    a.close()
    igg.finalize_global_grid(finalize_MPI=False)

    from igg.parallel import halo as H

    igg.init_global_grid(66, 64, 1, periodx=1, periody=1, quiet=True, init_MPI=False)
    H.enable_loopback((True, True, False))
    a = dyadic_model(gpu, F64)
    assert a.set_fused(True)
    a.run(2)
    before = [getattr(a, k).clone() for k in ("P", "Vx", "Vy")]
    gd = [t.to(gpu) for t in g]
    with pytest.raises(igg.IGGError, match="loopback"):
        a.adjoint_run(5, *gd)
    assert all(torch.equal(getattr(a, k), v) for k, v in zip(("P", "Vx", "Vy"), before))
    assert all(torch.equal(x.cpu(), y) for x, y in zip(gd, g))
    a.close()
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------- ranks sharing device 0
def _reference(dims, periodic, nt, path):
    igg.init_global_grid(*single_rank_size(dims), 1, periodx=periodic, periody=periodic, quiet=True, init_MPI=False,
                         device_type="none")
    m = dyadic_model(torch.device("cpu"), F64)
    G = global_adjoint(m, nt)
    igg.finalize_global_grid(finalize_MPI=False)
    np.savez(path, P=G[0].numpy(), Vx=G[1].numpy(), Vy=G[2].numpy())


@pytest.mark.parametrize("nprocs,dims,periodic", [(2, (2, 1), 1), (4, (2, 2), 0)])
def test_adjoint_run_ranks_on_one_device(gpu, nprocs, dims, periodic, tmp_path):
    path = str(tmp_path / "ref.npz")
    _reference(dims, periodic, 3, path)
    # ranks share one GPU: RCCL cannot, the messages are staged through the host
    run_ranks(nprocs, "gpu", *dims, periodic, 3, path, timeout=120,
              env_extra={"IGG_TRANSPORT": "staged", "IGG_ACOUSTIC_TWOSTEP": "0"})


@pytest.mark.multigpu
def test_adjoint_run_two_ranks_on_two_devices_over_rccl(gpu, tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: one rank per device over RCCL")
    path = str(tmp_path / "ref.npz")
    _reference((2, 1), 0, 3, path)
    run_ranks(2, "mgpu", 2, 1, 0, 3, path, timeout=150,
              env_extra={"IGG_TRANSPORT": "rccl", "IGG_ACOUSTIC_TWOSTEP": "0"})


# ------------------------------------------------------------- large offsets
def test_adjoint_where_byte_offsets_pass_2_to_32(gpu):
    """float32, ``ny = 1024`` and ``nx`` just above 2^20: every array passes
    2^32 bytes. The inputs are periodic along x with a period of 7 rows, so the
    outputs are too wherever no boundary face reaches - gP and gVy rows
    ``[1, nx-1)``, gVx rows ``[2, nx-1)`` - both ends equal the same kernel's
    output on a small array of the same data (itself equal to the host twin's),
    and nothing around the arrays is written. Helpers and method:
    tests/test_gpu_large_offsets.py."""
    from tests.test_gpu_large_offsets import (P, Guarded, aperiodic_cells, block, need_gib, no_wrap_aliases,
                                              small_extent, still_tiled, tile_)

    ny = 1024
    nx = (1 << 20) + 16
    assert nx * ny * 4 > (1 << 32) and no_wrap_aliases((nx, ny), 4, 0)
    need_gib(-(-(6 * (nx + 1) * (ny + 1) * 4 + 2 * nx * ny) // (1 << 30)) + 1)
    k = 2
    blocks = [(block((P, s[1]), 11 + i) - 0.5).to(F32).to(gpu) for i, s in enumerate(shapes(nx, ny))]
    nxs = small_extent(nx, k)
    src_s = [tile_(torch.empty(s, dtype=F32, device=gpu), b) for s, b in zip(shapes(nxs, ny), blocks)]
    out_s = [torch.full_like(t, float("nan")) for t in src_s]
    stencil.acoustic2d_adjoint_(*out_s, *src_s, **RKW)
    torch.cuda.synchronize()
    host = [torch.empty_like(t, device="cpu") for t in src_s]
    stencil.acoustic2d_adjoint_(*host, *(t.cpu() for t in src_s), **RKW)
    assert all(torch.equal(bits(a.cpu()), bits(b)) for a, b in zip(out_s, host))
    hold = {}
    try:
        src = [Guarded(s, F32, gpu) for s in shapes(nx, ny)]
        out = [Guarded(s, F32, gpu) for s in shapes(nx, ny)]
        hold.update({f"in{i}": g for i, g in enumerate(src)})
        hold.update({f"out{i}": g for i, g in enumerate(out)})
        for g, b in zip(src, blocks):
            tile_(g.a, b)
        for g in out:
            g.a.fill_(float("nan"))
        stencil.acoustic2d_adjoint_(*(g.a for g in out), *(g.a for g in src), **RKW)
        torch.cuda.synchronize()
        o = [g.a for g in out]
        names = ("gP", "gVx", "gVy")
        for name, t in zip(names, o):
            assert not torch.isnan(t).any(), (name, "an element was never stored")
        assert all(g.intact() for g in hold.values()), "a guard band was written"
        valid = {"gP": (1, nx - 1), "gVx": (2, nx - 1), "gVy": (1, nx - 1)}
        for name, t in zip(names, o):
            bad = aperiodic_cells(t, k, lo=valid[name][0], hi=valid[name][1])
            print(name, tuple(t.shape), "cells off the period:", bad)
            assert bad == 0, name
        m = P + k
        for name, t, ts in zip(names, o, out_s):
            assert torch.equal(t[:m], ts[:m]), (name, "head")
            assert torch.equal(t[-m:], ts[-m:]), (name, "tail")
        for g, b in zip(src, blocks):
            assert still_tiled(g.a, b)
    finally:
        hold.clear()
        src = out = o = None
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ the example
def test_example_on_the_gpu():
    args = [sys.executable, os.path.join(ROOT, "examples", "acoustic_adjoint.py"), "--nx", "64", "--nt", "12"]
    env = dict(os.environ, OMP_NUM_THREADS="1", IGG_HOST_THREADS="2")
    r = subprocess.run(args, capture_output=True, text=True, timeout=160, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "adjoint check OK" in r.stdout and "1 process(es)" in r.stdout
