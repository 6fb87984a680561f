"""The adjoint diffusion kernels (csrc/kernels/stencil_adj_kernels.hip) against
their host twins (csrc/stencil_adj_host.cpp), bit for bit, and the layers above
them on the GPU: ``igg.autograd.diffusion3d`` and ``Diffusion3D.adjoint_run``.

Every input is carved out of NaN padding and every output out of a sentinel
allocation that is compared whole: a read beyond an array that reaches a result
or a store beyond an array fails the comparison. The shapes are the smallest
at which the kernels' layout can go wrong - the scalar form and the smallest
vector row, rows of exactly one wave segment and of one vector more, one row
more and one fewer than a workgroup's row tile, one plane more than an x
chunk - in the Cp and the Q form, gCp plain and accumulated.
"""
import numpy as np
import pytest
import torch

import igg
from igg._native import native
from igg.ops import stencil
from tests.mp_worker_adjoint import adjoint_global, make_model, run_adjoint_ranks, single_rank_size
from tests.test_diffusion_adjoint_cpu import (RKW, bits, check_boundary_rule, check_errors, dyadic, random_fields)

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
PAD = 4096
SENTINEL = -7.0


def nan_padded(src, gpu):
    """``src`` on the device in the middle of a buffer of NaN."""
    n = src.numel()
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=src.dtype, device=gpu)
    v = buf[PAD:PAD + n].view(src.shape)
    v.copy_(src)
    return v


def sentinel_output(init, gpu):
    """(whole buffer, view): ``init`` in the middle of a buffer of SENTINEL."""
    n = init.numel()
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=init.dtype, device=gpu)
    v = buf[PAD:PAD + n].view(init.shape)
    v.copy_(init)
    return buf, v


def whole(expected):
    """What the whole buffer of ``sentinel_output`` must hold afterwards."""
    n = expected.numel()
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=expected.dtype)
    buf[PAD:PAD + n] = expected.flatten()
    return buf


def shapes_for(dtype):
    es = torch.empty(0, dtype=dtype).element_size()
    vz, rows = native.diffusion3d_adjoint_tile(64, es)
    assert vz == 16 // es and rows % 4 == 0
    assert native.diffusion3d_adjoint_tile(65, es) == (1, rows)
    base = [(3, 3, 3), (3, 3, 4), (4, 5, 6), (24, 20, 18), (9, 70, 5), (37, 33, 131), (20, 22, 72), (40, 33, 70)]
    seg = [(4, 5, 64 * vz), (4, 5, 64 * vz + vz), (5, 4, 65), (4, 4, 129)]   # one wave segment, one vector / point more
    tile = [(4, rows + 1, 2 * vz), (4, rows - 1, 2 * vz), (4, rows + 1, 7), (4, 2 * rows, 9)]
    return base + seg + tile


def run_case(shape, dtype, gpu, chunk=0, seed=0):
    """All four kernels of one shape against the host twins; returns the
    number of comparisons."""
    g, T, Cp = random_fields(shape, dtype, seed)
    old = random_fields(shape, dtype, seed + 50)[0]
    gd, Td, Cpd = nan_padded(g, gpu), nan_padded(T, gpu), nan_padded(Cp, gpu)
    Qd = nan_padded(torch.zeros_like(Cp), gpu)
    stencil.quotient_(Qd, Cpd, lam=RKW["lam"], dt=RKW["dt"])
    Q = torch.full_like(Cp, RKW["dt"] * RKW["lam"]) / Cp
    assert torch.equal(bits(Qd.cpu()), bits(Q)), "quotient_ is not the host's division"
    # the host twins
    hT, hCp, hAcc = torch.empty_like(g), torch.empty_like(g), old.clone()
    stencil.diffusion3d_adjoint_(hT, g, Cp, T=T, gCp=hCp, **RKW)
    stencil.diffusion3d_adjoint_(None, g, Cp, T=T, gCp=hAcc, accumulate=True, **RKW)
    fill = torch.full_like(g, 3.0)
    n = 0
    for name, want, init, kw in (
            ("gT from Cp", hT, fill, dict(gT=True)), ("gT from Q", hT, fill, dict(gT=True, Q=Qd)),
            ("gCp", hCp, fill, dict(T=Td, gCp=True)), ("gCp accumulated", hAcc, old, dict(T=Td, gCp=True, accumulate=True)),
            ("gT and gCp", None, fill, dict(gT=True, T=Td, gCp=True))):
        bufs = {k: sentinel_output(init, gpu) for k in ("gT", "gCp") if kw.get(k) is True}
        args = {k: v for k, v in kw.items() if k not in ("gT", "gCp")}
        stencil.diffusion3d_adjoint_(bufs["gT"][1] if "gT" in bufs else None, gd, Cpd,
                                     gCp=bufs["gCp"][1] if "gCp" in bufs else None, chunk=chunk, **args, **RKW)
        torch.cuda.synchronize()
        for k, (buf, _v) in bufs.items():
            w = want if want is not None else (hT if k == "gT" else hCp)
            got, exp = bits(buf.cpu()), bits(whole(w))
            assert torch.equal(got, exp), (shape, dtype, chunk, name, k, int((got != exp).sum()),
                                           (got != exp).nonzero()[:6].flatten().tolist())
            n += 1
    for A, src in ((gd, g), (Td, T), (Cpd, Cp)):
        assert torch.equal(bits(A.cpu()), bits(src)), "an input was written"
    return n


@pytest.mark.parametrize("dtype", [F32, F64])
def test_kernels_equal_host_twins(gpu, dtype):
    n = 0
    for i, shape in enumerate(shapes_for(dtype)):
        n += run_case(shape, dtype, gpu, seed=i)
    assert n == 6 * len(shapes_for(dtype))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_x_chunks(gpu, dtype):
    """One plane more than an x chunk, chunks of one plane, and a chunk longer
    than the array, on a vector and a scalar row."""
    for shape, chunk in (((5, 6, 8), 4), ((5, 6, 7), 4), ((9, 18, 16), 4), ((6, 5, 8), 1), ((6, 5, 5), 1),
                         ((7, 6, 8), 3), ((4, 6, 8), 100)):
        run_case(shape, dtype, gpu, chunk=chunk, seed=20)


def test_boundary_and_nan_rules_on_the_device(gpu):
    def run(g, T, Cp, Q):
        gT, gCp = torch.full_like(g, 7.0).to(gpu), torch.full_like(g, 7.0).to(gpu)
        stencil.diffusion3d_adjoint_(gT, g.to(gpu), Cp.to(gpu), T=T.to(gpu), gCp=gCp,
                                     Q=None if Q is None else Q.to(gpu), **RKW)
        return gT.cpu(), gCp.cpu()

    check_boundary_rule(run)


@pytest.mark.parametrize("shape", [(1, 4, 5), (4, 2, 8), (4, 5, 2), (2, 2, 2)])
def test_extents_below_three_on_the_device(gpu, shape):
    g, T, Cp = (A.to(gpu) for A in random_fields(shape, F64, 6))
    gT, gCp, acc = torch.full_like(g, 7.0), torch.full_like(g, 7.0), T.clone()
    stencil.diffusion3d_adjoint_(gT, g, Cp, T=T, gCp=gCp, **RKW)
    stencil.diffusion3d_adjoint_(None, g, Cp, T=T, gCp=acc, accumulate=True, **RKW)
    assert torch.equal(gT, g) and (gCp == 0).all() and torch.equal(acc, T)


def test_errors_on_the_device(gpu):
    check_errors(gpu)


def test_captured_graph_replayed_after_g_is_rewritten(gpu):
    shape = (9, 18, 24)
    g, T, Cp = random_fields(shape, F64, 30)
    g2 = random_fields(shape, F64, 31)[0]
    gd, Td, Cpd = g.to(gpu), T.to(gpu), Cp.to(gpu)
    gT, gCp = torch.zeros_like(gd), torch.zeros_like(gd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        stencil.diffusion3d_adjoint_(gT, gd, Cpd, T=Td, gCp=gCp, **RKW)  # code objects loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stencil.diffusion3d_adjoint_(gT, gd, Cpd, T=Td, gCp=gCp, **RKW)
    for src in (g, g2):
        gd.copy_(src)
        gT.fill_(5.0)
        gCp.fill_(5.0)
        graph.replay()
        torch.cuda.synchronize()
        hT, hCp = torch.empty_like(g), torch.empty_like(g)
        stencil.diffusion3d_adjoint_(hT, src, Cp, T=T, gCp=hCp, **RKW)
        assert torch.equal(bits(gT.cpu()), bits(hT)) and torch.equal(bits(gCp.cpu()), bits(hCp))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_autograd_on_the_gpu_equals_the_cpu(gpu, dtype):
    shape = (7, 18, 24)
    w, T, Cp = random_fields(shape, dtype, 40)
    grads = []
    for dev in (torch.device("cpu"), gpu):
        Tr, Cr = T.clone().to(dev).requires_grad_(), Cp.clone().to(dev).requires_grad_()
        out = igg.autograd.diffusion3d(Tr, Cr, **RKW)
        assert out.device == Tr.device
        (out * w.to(dev)).sum().backward()
        grads.append((out.detach().cpu(), Tr.grad.cpu(), Cr.grad.cpu()))
    (oc, tc, cc), (og, tg, cg) = grads
    assert torch.equal(bits(tc), bits(tg)) and torch.equal(bits(cc), bits(cg))
    # (the forward kernel and the host step round differently: compared within rounding)
    assert torch.allclose(oc, og, rtol=0, atol=(1e-5 if dtype == F32 else 1e-13))
    # dyadic data: the forward pass is exact on both
    w, T, Cp = dyadic(shape, dtype, 41)
    kw = dict(lam=1.0, dt=0.125, dx=1.0, dy=0.5, dz=0.25)
    assert torch.equal(igg.autograd.diffusion3d(T.to(gpu), Cp.to(gpu), **kw).cpu(), igg.autograd.diffusion3d(T, Cp, **kw))


def test_adjoint_run_of_a_gpu_model_equals_the_cpu_model(gpu, monkeypatch):
    monkeypatch.setenv("IGG_STENCIL_TWOSTEP", "0")
    from igg.models.diffusion3d import Diffusion3D

    igg.init_global_grid(12, 18, 24, periodx=1, periody=1, periodz=1, quiet=True, init_MPI=False)
    a = Diffusion3D(dtype=F64, device=gpu, variant=0)
    b = Diffusion3D(dtype=F64, device="cpu")
    b.Cp.copy_(a.Cp)  # (the device's exp and the host's differ in the last place)
    assert a.dt == b.dt
    g = random_fields(tuple(b.T.shape), F64, 42)[0]
    T0 = a.T.clone()
    want = b.adjoint_run(4, g)
    got = a.adjoint_run(4, g.to(gpu))
    assert got.device == a.T.device and torch.equal(bits(got.cpu()), bits(want)) and torch.equal(a.T, T0)
    # with the model's quotient array, once it is current
    assert a.Q is None and not a._q_current()
    a._alloc_q()
    assert not a._q_current()  # allocated, not built: Cp is read
    a._refresh_q()
    assert a._q_current()
    seen = []
    real = stencil.diffusion3d_adjoint_
    monkeypatch.setattr(stencil, "diffusion3d_adjoint_", lambda *p, **k: (seen.append(k.get("Q")), real(*p, **k))[1])
    got = a.adjoint_run(4, g.to(gpu))
    assert len(seen) == 4 and all(q is a.Q for q in seen)
    assert torch.equal(bits(got.cpu()), bits(want))
    a.Cp.mul_(2.0)  # Cp changed: the stale Q is not used
    seen.clear()
    a.adjoint_run(1, g.to(gpu))
    assert seen == [None]
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------- ranks sharing device 0
def _reference(dims, periodic, nt, path):
    per = int(periodic)
    igg.init_global_grid(*single_rank_size(dims), periodx=per, periody=per, periodz=per, quiet=True, init_MPI=False,
                         device_type="none")
    m, g, E = make_model(torch.device("cpu"))
    G = adjoint_global(m, g, nt, E)
    igg.finalize_global_grid(finalize_MPI=False)
    np.save(path, G.numpy())


@pytest.mark.parametrize("nprocs,dims,periodic", [(2, (2, 1, 1), 1), (4, (1, 2, 2), 0), (8, (2, 2, 2), 1)])
def test_adjoint_run_ranks_on_one_device(gpu, nprocs, dims, periodic, tmp_path):
    path = str(tmp_path / "ref.npy")
    _reference(dims, periodic, 3, path)
    # ranks share one GPU: RCCL cannot, the messages are staged through the host
    run_adjoint_ranks(nprocs, "adjoint_run", "gpu", *dims, periodic, 3, path, timeout=120,
                      env_extra={"IGG_TRANSPORT": "staged", "IGG_STENCIL_TWOSTEP": "0"})


@pytest.mark.multigpu
def test_adjoint_run_two_ranks_on_two_devices_over_rccl(gpu, tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: one rank per device over RCCL")
    path = str(tmp_path / "ref.npy")
    _reference((2, 1, 1), 0, 3, path)
    run_adjoint_ranks(2, "adjoint_run", "mgpu", 2, 1, 1, 0, 3, path, timeout=150,
                      env_extra={"IGG_TRANSPORT": "rccl", "IGG_STENCIL_TWOSTEP": "0"})


# ------------------------------------------------------------- large offsets
def test_adjoint_t_where_byte_offsets_pass_2_to_32(gpu):
    """``adjoint_t`` on a float32 array of more than 2^30 elements (byte
    offsets pass 2^32, plane and row bases 2^31 bytes), tiled along x from a
    block of 7 planes, in the Cp and the Q form: the output has the block's
    period from plane 2 to plane n-3 (a boundary plane's u = 0 reaches its
    neighbour plane), both ends equal the same kernel's output
    on a small array of the same data, and nothing around the arrays is
    written. Helpers and method: tests/test_gpu_large_offsets.py."""
    from tests.test_gpu_large_offsets import (P, Guarded, aperiodic_cells, block, gib_of, need_gib,
                                              no_wrap_aliases, small_extent, still_tiled, tile_)

    n1, n2 = 12, 1024
    n0 = -(-(1 << 30) // (n1 * n2)) + 16
    shape = (n0, n1, n2)
    assert n0 * n1 * n2 * 4 > (1 << 32) + 16 * n1 * n2 * 4 and no_wrap_aliases(shape, 4, 0)
    need_gib(gib_of(shape, F32, 4))
    k = 2
    bG = (block((P, n1, n2), 1) - 0.5).to(F32).to(gpu)         # g in [-0.5, 0.5)
    bC = block((P, n1, n2), 2, lo=1.0).to(F32).to(gpu)         # Cp in [1, 2)
    sshape = (small_extent(n0, k), n1, n2)
    Sg = tile_(torch.empty(sshape, dtype=F32, device=gpu), bG)
    Sc = tile_(torch.empty(sshape, dtype=F32, device=gpu), bC)
    Sq = torch.empty_like(Sc)
    stencil.quotient_(Sq, Sc, lam=RKW["lam"], dt=RKW["dt"])
    bQ = Sq[:P].clone()
    Sout = torch.full_like(Sg, float("nan"))
    stencil.diffusion3d_adjoint_(Sout, Sg, Sc, **RKW)
    torch.cuda.synchronize()
    assert not torch.isnan(Sout).any()
    hold = {}
    try:
        g = hold["g"] = Guarded(shape, F32, gpu)
        c = hold["c"] = Guarded(shape, F32, gpu)
        out = hold["out"] = Guarded(shape, F32, gpu)
        tile_(g.a, bG)
        for form, blk in (("Cp", bC), ("Q", bQ)):
            tile_(c.a, blk)
            out.a.fill_(float("nan"))
            if form == "Cp":
                stencil.diffusion3d_adjoint_(out.a, g.a, c.a, **RKW)
            else:
                stencil.diffusion3d_adjoint_(out.a, g.a, c.a, Q=c.a, **RKW)  # (Cp is not read where Q is given)
            torch.cuda.synchronize()
            assert not torch.isnan(out.a).any(), (form, "a cell was never stored")
            assert all(G.intact() for G in hold.values()), (form, "a guard band was written")
            bad = aperiodic_cells(out.a, k)
            print(form, shape, "cells off the period:", bad)
            assert bad == 0, form
            m = P + k
            assert torch.equal(out.a[:m], Sout[:m]) and torch.equal(out.a[n0 - m:], Sout[sshape[0] - m:]), form
            assert still_tiled(g.a, bG) and still_tiled(c.a, blk)
    finally:
        hold.clear()
        torch.cuda.empty_cache()
