"""The adjoint of the diffusion step on the host: ``ops.stencil.diffusion3d_adjoint_``
(csrc/stencil_adj_host.cpp, the kernels' bitwise twin), ``igg.autograd.diffusion3d``
and ``Diffusion3D.adjoint_run``.

The oracle is ``torch.autograd`` of a plain float64 formulation of the forward
step, and the transposed matrix of ``diffusion3d_`` itself. With dyadic data
(integer ``g`` and ``T`` in [-8, 8], ``Cp`` in {1, 2, 4}, ``dt*lam = 1/8``,
``1/d^2 = 1, 4, 16``) every operation is exact in float32 and float64 and the
comparisons are exact; with random data the bound is ``16 * eps * scale``:

    scale_T  = max|g| + 4 * sum(1/d^2) * max|q*g|
    scale_Cp = 4 * sum(1/d^2) * max|T| * max|q*g| / min Cp         (q = dt*lam/Cp)

``4 * sum(1/d^2) * max|w|`` bounds the absolute sum of the stencil's seven
terms, each rounded a few times: 16 roundings of that size bound one result.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import igg
from igg.ops import stencil
from tests._mp import ROOT, free_port
from tests.mp_worker_adjoint import (KW as DKW, adjoint_global, make_model, run_adjoint_ranks, single_rank_size)

F32, F64 = torch.float32, torch.float64
RD2 = (1.0, 4.0, 16.0)
DTLAM = 0.125
GRID = dict(quiet=True, init_MPI=False, device_type="none")
DYADIC_SHAPES = [(3, 3, 3), (4, 5, 6), (3, 4, 9)]


def plain_step(T, Cp, dtlam=DTLAM, rd2=RD2):
    """The forward step in plain torch: interior updated, boundary cells T's."""
    c = T[1:-1, 1:-1, 1:-1]
    lap = ((T[2:, 1:-1, 1:-1] - 2 * c + T[:-2, 1:-1, 1:-1]) * rd2[0]
           + (T[1:-1, 2:, 1:-1] - 2 * c + T[1:-1, :-2, 1:-1]) * rd2[1]
           + (T[1:-1, 1:-1, 2:] - 2 * c + T[1:-1, 1:-1, :-2]) * rd2[2])
    out = T.clone()
    out[1:-1, 1:-1, 1:-1] = c + dtlam / Cp[1:-1, 1:-1, 1:-1] * lap
    return out


def reference(g, T, Cp, kw):
    """(gT, gCp) by torch.autograd through the plain float64 formulation."""
    rd2 = (1 / kw["dx"] ** 2, 1 / kw["dy"] ** 2, 1 / kw["dz"] ** 2)
    T64, C64 = T.detach().double().clone().requires_grad_(), Cp.detach().double().clone().requires_grad_()
    return torch.autograd.grad(plain_step(T64, C64, kw["dt"] * kw["lam"], rd2), (T64, C64), g.double())


def dyadic(shape, dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randint(-8, 9, shape, generator=gen).to(dtype)
    T = torch.randint(-8, 9, shape, generator=gen).to(dtype)
    Cp = torch.pow(2.0, torch.randint(0, 3, shape, generator=gen).double()).to(dtype)
    return g, T, Cp


def random_fields(shape, dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    g = (torch.rand(shape, generator=gen, dtype=F64) * 2 - 1).to(dtype)
    T = (torch.rand(shape, generator=gen, dtype=F64) * 4 - 2).to(dtype)
    Cp = (1 + torch.rand(shape, generator=gen, dtype=F64)).to(dtype)
    return g, T, Cp


RKW = dict(lam=1.0, dt=0.01, dx=0.3, dy=0.25, dz=0.2)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int64)


def both(g, T, Cp, kw, **extra):
    gT, gCp = torch.full_like(g, 7.0), torch.full_like(g, 7.0)
    stencil.diffusion3d_adjoint_(gT, g, Cp, T=T, gCp=gCp, **kw, **extra)
    return gT, gCp


# ------------------------------------------------------------------ exactness
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("shape", DYADIC_SHAPES)
def test_dyadic_transposed_matrix(shape, dtype):
    """The matrix of ``diffusion3d_`` (output pre-filled with T) column by
    column from unit vectors; ``S^T y`` must be ``diffusion3d_adjoint_(y)``."""
    g, _T, Cp = dyadic(shape, dtype)
    n = g.numel()
    S = torch.empty(n, n, dtype=dtype)
    for j in range(n):
        e = torch.zeros(n, dtype=dtype)
        e[j] = 1
        e = e.view(shape)
        out = e.clone()
        stencil.diffusion3d_(out, e, Cp, **DKW)
        S[:, j] = out.flatten()
    gT = torch.full_like(g, 7.0)
    stencil.diffusion3d_adjoint_(gT, g, Cp, **DKW)
    assert torch.equal(gT.flatten().double(), S.double().t() @ g.flatten().double())


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("shape", DYADIC_SHAPES)
def test_dyadic_equals_autograd(shape, dtype):
    g, T, Cp = dyadic(shape, dtype, 1)
    gT, gCp = both(g, T, Cp, DKW)
    rT, rCp = reference(g, T, Cp, DKW)
    assert torch.equal(gT.double(), rT) and torch.equal(gCp.double(), rCp)
    assert gT.abs().max() > 0 and (gCp.abs().max() > 0 or min(shape) < 3)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("shape", [(9, 8, 11), (5, 70, 6)])
def test_random_within_rounding(shape, dtype):
    g, T, Cp = random_fields(shape, dtype)
    gT, gCp = both(g, T, Cp, RKW)
    rT, rCp = reference(g, T, Cp, RKW)
    eps = torch.finfo(dtype).eps
    srd2 = sum(1 / RKW[k] ** 2 for k in ("dx", "dy", "dz"))
    qg = ((RKW["dt"] * RKW["lam"] / Cp.double()) * g.double()).abs().max().item()
    scale_T = g.abs().max().item() + 4 * srd2 * qg
    scale_Cp = 4 * srd2 * T.abs().max().item() * qg / Cp.min().item()
    eT = (gT.double() - rT).abs().max().item()
    eCp = (gCp.double() - rCp).abs().max().item()
    print(shape, dtype, "gT error / (eps scale):", eT / (eps * scale_T), "gCp:", eCp / (eps * scale_Cp))
    assert eT <= 16 * eps * scale_T and eCp <= 16 * eps * scale_Cp


# -------------------------------------------------------------------- the forms
@pytest.mark.parametrize("dtype", [F32, F64])
def test_accumulate_is_old_plus_fresh(dtype):
    shape = (5, 6, 7)
    g, T, Cp = random_fields(shape, dtype, 2)
    _, fresh = both(g, T, Cp, RKW)
    old = random_fields(shape, dtype, 3)[1]
    acc = old.clone()
    stencil.diffusion3d_adjoint_(None, g, Cp, T=T, gCp=acc, accumulate=True, **RKW)
    want = old.clone()
    want[1:-1, 1:-1, 1:-1] = old[1:-1, 1:-1, 1:-1] + fresh[1:-1, 1:-1, 1:-1]
    assert torch.equal(bits(acc), bits(want))
    inner = torch.zeros(shape, dtype=torch.bool)
    inner[1:-1, 1:-1, 1:-1] = True
    assert torch.equal(bits(acc)[~inner], bits(old)[~inner]) and (fresh[~inner] == 0).all()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_q_form_equals_cp_form(dtype):
    shape = (6, 5, 9)
    g, _T, Cp = random_fields(shape, dtype, 4)
    Q = torch.full_like(Cp, RKW["dt"] * RKW["lam"]) / Cp  # one correctly rounded division, as quotient_ divides
    a, b = torch.full_like(g, 7.0), torch.full_like(g, 7.0)
    stencil.diffusion3d_adjoint_(a, g, Cp, **RKW)
    stencil.diffusion3d_adjoint_(b, g, Cp, Q=Q, **RKW)
    assert torch.equal(bits(a), bits(b))
    # Cp is not read where Q is given
    stencil.diffusion3d_adjoint_(b, g, torch.full_like(Cp, float("nan")), Q=Q, **RKW)
    assert torch.equal(bits(a), bits(b))


def boundary_mask(shape):
    m = torch.ones(shape, dtype=torch.bool)
    m[1:-1, 1:-1, 1:-1] = False
    return m


def check_boundary_rule(run):
    """``run(g, T, Cp, Q) -> (gT, gCp)`` on tensors of its device; everything
    here is compared on the host. Shared with the GPU tests."""
    shape = (5, 6, 8)
    g, T, Cp = random_fields(shape, F64, 5)
    Q = torch.full_like(Cp, RKW["dt"] * RKW["lam"]) / Cp
    bnd = boundary_mask(shape)
    gT, gCp = run(g, T, Cp, None)
    # boundary values of Cp and Q reach nothing: Cp == 0 (an infinite quotient), NaN
    for bad in (0.0, float("nan")):
        Cp0, Q0 = Cp.clone(), Q.clone()
        Cp0[bnd] = bad
        Q0[bnd] = float("inf") if bad == 0.0 else bad
        a, b = run(g, T, Cp0, None)
        assert torch.equal(bits(a), bits(gT)) and torch.equal(bits(b), bits(gCp)), bad
        a, _ = run(g, T, Cp0, Q0)
        assert torch.equal(bits(a), bits(gT)), bad
    assert (gCp[bnd] == 0).all()
    # a NaN in g at a boundary cell reaches gT of that cell only, and no gCp
    for at in ((0, 2, 3), (2, 5, 4), (3, 2, 0), (4, 5, 7)):
        gn = g.clone()
        gn[at] = float("nan")
        a, b = run(gn, T, Cp, None)
        nan = torch.isnan(a)
        assert nan[at] and int(nan.sum()) == 1, at
        a[at] = gT[at]
        assert torch.equal(bits(a), bits(gT)) and torch.equal(bits(b), bits(gCp)), at
    # at an interior cell: the cells of its 7-point star in gT, its own cell of gCp
    for at in ((1, 1, 1), (2, 3, 4), (3, 4, 6)):
        gn = g.clone()
        gn[at] = float("nan")
        a, b = run(gn, T, Cp, None)
        star = torch.zeros(shape, dtype=torch.bool)
        star[at] = True
        for d in range(3):
            for s in (-1, 1):
                j = list(at)
                j[d] += s
                star[tuple(j)] = True
        assert torch.equal(torch.isnan(a), star), at
        assert torch.equal(bits(a)[~star], bits(gT)[~star])
        own = torch.zeros(shape, dtype=torch.bool)
        own[at] = True
        assert torch.equal(torch.isnan(b), own) and torch.equal(bits(b)[~own], bits(gCp)[~own]), at


def test_boundary_rule():
    def run(g, T, Cp, Q):
        return both(g, T, Cp, RKW, Q=Q)

    check_boundary_rule(run)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("shape", [(1, 4, 5), (2, 4, 5), (4, 2, 5), (4, 5, 1), (4, 5, 2), (2, 2, 2), (1, 1, 1)])
def test_extents_below_three(shape, dtype):
    """No interior: gT = g, gCp = 0, and an accumulated gCp is untouched."""
    g, T, Cp = random_fields(shape, dtype, 6)
    gT, gCp = both(g, T, Cp, RKW)
    assert torch.equal(bits(gT), bits(g)) and (gCp == 0).all()
    acc = T.clone()
    stencil.diffusion3d_adjoint_(None, g, Cp, T=T, gCp=acc, accumulate=True, **RKW)
    assert torch.equal(bits(acc), bits(T))


def check_errors(device):
    """Every refused call names its argument and leaves every array as it was."""
    shape = (4, 5, 6)
    arrays = {k: v.to(device) for k, v in zip(("g", "T", "Cp"), random_fields(shape, F64, 7))}
    arrays["Q"] = torch.full_like(arrays["Cp"], 0.01) / arrays["Cp"]
    arrays["gT"] = torch.full(shape, 5.0, dtype=F64, device=device)
    arrays["gCp"] = torch.full(shape, 6.0, dtype=F64, device=device)
    before = {k: v.clone() for k, v in arrays.items()}
    A = arrays
    wide = torch.zeros((4, 5, 12), dtype=F64, device=device)
    cases = [
        ("gT", dict(gT=A["g"])),                                   # gT aliases g
        ("gT", dict(gT=A["g"].view(-1)[:120].view(shape))),        # (the same bytes through another tensor)
        ("gCp", dict(gCp=A["g"])), ("gCp", dict(gCp=A["Cp"])), ("gCp", dict(gCp=A["T"])),
        ("gCp", dict(gCp=A["Q"], Q=A["Q"])), ("gCp", dict(gCp=A["gT"])),
        ("gCp", dict(T=None)),                                     # gCp without T
        ("gT", dict(gT=torch.zeros((4, 5, 7), dtype=F64, device=device))),
        ("Cp", dict(Cp=torch.ones((4, 5, 7), dtype=F64, device=device))),
        ("Q", dict(Q=torch.ones((5, 5, 6), dtype=F64, device=device))),
        ("T", dict(T=torch.ones((4, 6, 6), dtype=F64, device=device))),
        ("gCp", dict(gCp=torch.zeros((3, 5, 6), dtype=F64, device=device))),
        ("Cp", dict(Cp=A["Cp"].float())), ("gT", dict(gT=A["gT"].float())), ("T", dict(T=A["T"].float())),
        ("Cp", dict(Cp=wide[:, :, ::2])), ("gT", dict(gT=wide[:, :, ::2])), ("gCp", dict(gCp=wide[:, :, 6:])),
        ("g", dict(g=A["g"].to(torch.int64), gT=A["gT"].to(torch.int64), Cp=A["Cp"].to(torch.int64), Q=None,
                   T=None, gCp=None)),
        ("g", dict(g=A["g"][0], gT=A["gT"][0], Cp=A["Cp"][0], Q=None, T=None, gCp=None)),
    ]
    if device.type != "cpu":
        cases += [("Cp", dict(Cp=A["Cp"].cpu())), ("gCp", dict(gCp=A["gCp"].cpu())), ("Q", dict(Q=A["Q"].cpu()))]
    for name, change in cases:
        kw = dict(gT=A["gT"], g=A["g"], Cp=A["Cp"], Q=A["Q"], T=A["T"], gCp=A["gCp"])
        kw.update(change)
        gT_, g_, Cp_ = kw.pop("gT"), kw.pop("g"), kw.pop("Cp")
        with pytest.raises(igg.IGGError, match=rf"\b{name}\b"):
            stencil.diffusion3d_adjoint_(gT_, g_, Cp_, **kw, **RKW)
        for k in arrays:
            assert torch.equal(bits(arrays[k]), bits(before[k])), (name, change.keys(), k)
        assert (wide == 0).all()


def test_errors_leave_arrays_unchanged():
    check_errors(torch.device("cpu"))


# ------------------------------------------------------------ igg.autograd.diffusion3d
def test_autograd_gradcheck():
    g, T, Cp = random_fields((4, 5, 6), F64, 8)
    f = lambda t, c: igg.autograd.diffusion3d(t, c, **RKW)
    assert torch.autograd.gradcheck(f, (T.clone().requires_grad_(), Cp.clone()))
    assert torch.autograd.gradcheck(f, (T.clone(), Cp.clone().requires_grad_()))
    assert torch.autograd.gradcheck(f, (T.clone().requires_grad_(), Cp.clone().requires_grad_()))
    # forward: the step itself, boundary cells T's
    out = f(T, Cp)
    want = T.clone()
    stencil.diffusion3d_(want, T, Cp, **RKW)
    assert torch.equal(out, want) and out.data_ptr() != T.data_ptr()


class _NativeSpy:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def diffusion3d_adjoint(self, gt, gcp, *a):
        self.calls.append((gt != 0, gcp != 0))
        return self.real.diffusion3d_adjoint(gt, gcp, *a)


def test_autograd_runs_only_what_is_needed(monkeypatch):
    spy = _NativeSpy(stencil.native)
    monkeypatch.setattr(stencil, "native", spy)
    g, T, Cp = random_fields((4, 5, 6), F64, 9)
    rT, rCp = reference(g, T, Cp, RKW)
    # only Cp: the Cp kernel alone, T is saved
    Cr = Cp.clone().requires_grad_()
    out = igg.autograd.diffusion3d(T, Cr, **RKW)
    assert len(out.grad_fn.saved_tensors) == 2
    out.backward(g)
    assert spy.calls == [(False, True)] and torch.allclose(Cr.grad, rCp, rtol=1e-12, atol=1e-14)
    # only T: the T kernel alone, and T is not kept for it
    spy.calls.clear()
    Tr = T.clone().requires_grad_()
    out = igg.autograd.diffusion3d(Tr, Cp, **RKW)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].data_ptr() != Tr.data_ptr() and torch.equal(saved[0], Cp)
    out.backward(g)
    assert spy.calls == [(True, False)] and torch.allclose(Tr.grad, rT, rtol=1e-12, atol=1e-14)
    # both, in one native call; neither: no call
    spy.calls.clear()
    Tr, Cr = T.clone().requires_grad_(), Cp.clone().requires_grad_()
    igg.autograd.diffusion3d(Tr, Cr, **RKW).backward(g)
    assert spy.calls == [(True, True)]
    spy.calls.clear()
    assert not igg.autograd.diffusion3d(T, Cp, **RKW).requires_grad and spy.calls == []


def test_autograd_three_steps_with_halo_exchange():
    """Three steps ``update_halo(diffusion3d(T))`` on one periodic rank against
    autograd through the plain formulation with halos taken from the opposite
    send planes; exact on dyadic float64 data."""
    n = (6, 5, 7)
    igg.init_global_grid(*n, periodx=1, periody=1, periodz=1, **GRID)
    w, T0, Cp = dyadic(n, F64, 10)

    def halo(A):
        for d in range(3):
            m = A.shape[d]
            idx = torch.cat([torch.tensor([m - 2]), torch.arange(1, m - 1), torch.tensor([1])])
            A = A.index_select(d, idx)
        return A

    Ta, Ca = T0.clone().requires_grad_(), Cp.clone().requires_grad_()
    Tb, Cb = T0.clone().requires_grad_(), Cp.clone().requires_grad_()
    A, B = Ta, Tb
    for _ in range(3):
        A = igg.autograd.update_halo(igg.autograd.diffusion3d(A, Ca, **DKW))
        B = halo(plain_step(B, Cb))
    assert torch.equal(A.detach(), B.detach())
    (A * w).sum().backward()
    (B * w).sum().backward()
    assert torch.equal(Ta.grad, Tb.grad) and torch.equal(Ca.grad, Cb.grad)
    assert Ta.grad.abs().max() > 0 and Ca.grad.abs().max() > 0
    igg.finalize_global_grid(finalize_MPI=False)


# ----------------------------------------------------------------- adjoint_run
def single_rank_reference(dims, periodic, nt, path):
    """The single-rank run on the ranks' global grid, saved for the workers."""
    per = int(periodic)
    igg.init_global_grid(*single_rank_size(dims), periodx=per, periody=per, periodz=per, **GRID)
    m, g, E = make_model(torch.device("cpu"))
    G = adjoint_global(m, g, nt, E)
    igg.finalize_global_grid(finalize_MPI=False)
    np.save(path, G.numpy())
    return G


@pytest.mark.parametrize("periodic", [0, 1])
def test_adjoint_run_is_the_transpose_of_run(periodic):
    """``<g, run(nt) T0> == <adjoint_run(nt, g), T0>`` on one rank, and against
    autograd through the plain formulation (exact: dyadic data)."""
    n = (6, 5, 7)
    igg.init_global_grid(*n, periodx=periodic, periody=periodic, periodz=periodic, **GRID)
    m, g, _E = make_model(torch.device("cpu"))
    T0 = dyadic(n, F64, 11)[1]
    if periodic:
        igg.update_halo_(T0)
    res = m.adjoint_run(3, g)
    m.T.copy_(T0)
    m.T2.copy_(T0)
    m.run(3)
    assert (g * m.T).sum().item() == (res * T0).sum().item()
    assert torch.equal(m.adjoint_run(0, g), g)
    with pytest.raises(igg.IGGError, match="g"):
        m.adjoint_run(1, g[:-1])
    igg.finalize_global_grid(finalize_MPI=False)


def test_adjoint_run_refuses_what_accumulate_halo_refuses():
    """ol = 4, w = 1, n = 4 < 5 in x: refused as soon as x has a neighbour
    (set by hand, as tests/test_accumulate_halo_cpu.py does)."""
    from igg.models.diffusion3d import Diffusion3D
    from igg.parallel import grid as G
    from igg.parallel import halo as HL

    igg.init_global_grid(4, 6, 5, overlapx=4, **GRID)
    m = Diffusion3D(dtype=F64, device="cpu")
    g = torch.ones_like(m.T)
    assert m.adjoint_run(1, g).shape == g.shape  # no neighbour in x: nothing to refuse
    gg = G.global_grid()
    gg.neighbors[1, 0] = 1
    HL.sync_grid()
    try:
        with pytest.raises(igg.IGGError, match="too small in dimension 1 to accumulate its halo"):
            m.adjoint_run(1, g)
        with pytest.raises(igg.IGGError, match="too small in dimension 1 to accumulate its halo"):
            m.adjoint_run(0, g)
    finally:
        gg.neighbors[1, 0] = igg.PROC_NULL
        HL.sync_grid()
    assert (g == 1).all()
    igg.finalize_global_grid(finalize_MPI=False)


RANKS = [(2, (2, 1, 1)), (4, (1, 2, 2)), (8, (2, 2, 2))]


@pytest.mark.parametrize("periodic", [0, 1])
@pytest.mark.parametrize("nprocs,dims", RANKS)
def test_adjoint_run_ranks_equal_single_rank(nprocs, dims, periodic, tmp_path):
    path = str(tmp_path / "ref.npy")
    G = single_rank_reference(dims, periodic, 3, path)
    assert G.abs().max() > 0
    run_adjoint_ranks(nprocs, "adjoint_run", "cpu", *dims, periodic, 3, path)


# ------------------------------------------------------------------ the example
@pytest.mark.parametrize("nprocs", [1, 2])
def test_example(nprocs):
    args = [os.path.join(ROOT, "examples", "diffusion3D_adjoint.py"), "--nx", "10", "--nt", "4"]
    if nprocs == 1:
        cmd = [sys.executable] + args
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nprocs}",
               "--master-addr", "127.0.0.1", "--master-port", str(free_port())] + args
    env = dict(os.environ, OMP_NUM_THREADS="1", IGG_HOST_THREADS="2")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=160, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "adjoint check OK" in r.stdout and f"{nprocs} process(es)" in r.stdout
