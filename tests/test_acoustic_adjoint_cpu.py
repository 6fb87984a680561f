"""The adjoint of the acoustic step on the host: ``ops.stencil.acoustic2d_adjoint_``
(csrc/acoustic_adj_host.cpp, the kernel's bitwise twin), ``igg.autograd.acoustic2d``
and ``Acoustic2D.adjoint_run``.

The oracles are the transposed matrix of ``native.acoustic2d`` itself and
``torch.autograd`` through ``acoustic2d_reference`` (float64). With dyadic
data (integers in [-8, 8], ``a = dt*K = 1/4``, ``b = dt/rho = 1/2``,
``1/dx = 2``, ``1/dy = 4``) every operation is exact in float32 and float64
and the comparisons are exact. With random data the bound is
``16 * eps * scale`` (the form of tests/test_diffusion_adjoint_cpu.py):

    scale_r  = max|gP2| + 2b (rdx max|gVx2| + rdy max|gVy2|)
    scale_P  = scale_r
    scale_Vx = max|gVx2| + 2a rdx scale_r           scale_Vy likewise

``scale_r`` bounds the absolute sum of r's five terms, ``scale_V`` that of a
face's three; a result takes fewer than 16 roundings of that size.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import igg
from igg._native import native
from igg.models.acoustic2d import acoustic2d_reference
from igg.ops import stencil
from tests._mp import ROOT, free_port
from tests.mp_worker_acoustic_adjoint import (DKW, MKW, dyadic_model, global_adjoint, int_fields, run_ranks,
                                              single_rank_size)

F32, F64 = torch.float32, torch.float64
GRID = dict(quiet=True, init_MPI=False, device_type="none")
DYADIC_SHAPES = [(1, 1), (1, 3), (2, 2), (3, 5), (5, 4)]
RKW = dict(dt=0.0123, K=1.7, rho=0.9, dx=0.3, dy=0.25)  # non-dyadic (the random-data cases)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int64)


def shapes(nx, ny):
    return (nx, ny), (nx + 1, ny), (nx, ny + 1)


def dyadic(nx, ny, dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randint(-8, 9, s, generator=gen).to(dtype) for s in shapes(nx, ny)]


def random_fields(nx, ny, dtype, seed=0, device="cpu"):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(s, generator=gen, dtype=F64) * 2 - 1).to(dtype).to(device) for s in shapes(nx, ny)]


def adjoint(gin, kw, **extra):
    gout = [torch.full_like(g, 7.0) for g in gin]
    stencil.acoustic2d_adjoint_(*gout, *gin, **kw, **extra)
    return gout


def forward_native(fields, kw):
    P, Vx, Vy = fields
    out = [torch.full_like(t, 7.0) for t in fields]
    native.acoustic2d(*(t.data_ptr() for t in out), P.data_ptr(), Vx.data_ptr(), Vy.data_ptr(), P.shape[0],
                      P.shape[1], kw["dt"] * kw["K"], kw["dt"] / kw["rho"], 1.0 / kw["dx"], 1.0 / kw["dy"],
                      P.element_size(), False, 0)
    return out


def reference(gin, kw):
    """Sᵀ g by torch.autograd through the float64 reference step, written with
    multiplications by 1/dx, 1/dy as the kernels are (for the dyadic values
    ``/dx`` and ``*rdx`` agree exactly)."""
    x = [torch.zeros_like(g, dtype=F64).requires_grad_() for g in gin]
    a, b, rdx, rdy = kw["dt"] * kw["K"], kw["dt"] / kw["rho"], 1.0 / kw["dx"], 1.0 / kw["dy"]
    P, Vx, Vy = x
    P2 = P - a * ((Vx[1:, :] - Vx[:-1, :]) * rdx + (Vy[:, 1:] - Vy[:, :-1]) * rdy)
    Vx2 = torch.cat([Vx[:1], Vx[1:-1] - b * (P2[1:] - P2[:-1]) * rdx, Vx[-1:]], 0)
    Vy2 = torch.cat([Vy[:, :1], Vy[:, 1:-1] - b * (P2[:, 1:] - P2[:, :-1]) * rdy, Vy[:, -1:]], 1)
    return torch.autograd.grad((P2, Vx2, Vy2), x, [g.double() for g in gin])


def flat(ts):
    return torch.cat([t.flatten() for t in ts])


def unflat(v, nx, ny):
    out, o = [], 0
    for s in shapes(nx, ny):
        n = s[0] * s[1]
        out.append(v[o:o + n].view(s).clone())
        o += n
    return out


# ------------------------------------------------------------------ exactness
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("shape", DYADIC_SHAPES)
def test_dyadic_transposed_matrix(shape, dtype):
    """The matrix of ``native.acoustic2d`` (host) column by column from unit
    vectors; the adjoint applied to unit vectors gives its transpose, exactly."""
    nx, ny = shape
    n = sum(s[0] * s[1] for s in shapes(nx, ny))
    S, St = torch.empty(n, n, dtype=dtype), torch.empty(n, n, dtype=dtype)
    for j in range(n):
        e = torch.zeros(n, dtype=dtype)
        e[j] = 1
        S[:, j] = flat(forward_native(unflat(e, nx, ny), DKW))
        St[:, j] = flat(adjoint(unflat(e, nx, ny), DKW))
    assert torch.equal(St, S.t())
    assert (S != 0).sum() > n or nx * ny == 1


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("shape", DYADIC_SHAPES)
def test_dyadic_equals_autograd(shape, dtype):
    gin = dyadic(*shape, dtype, 1)
    got, want = adjoint(gin, DKW), reference(gin, DKW)
    for a, b in zip(got, want):
        assert torch.equal(a.double(), b)
    assert got[0].abs().max() > 0
    # the reference step used here is acoustic2d_reference's
    x = dyadic(*shape, F64, 2)
    for a, b in zip(acoustic2d_reference(*x, **DKW), forward_native(x, DKW)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_random_within_rounding(dtype):
    nx, ny = 37, 53
    gin = random_fields(nx, ny, dtype)
    got, want = adjoint(gin, RKW), reference(gin, RKW)
    eps = torch.finfo(dtype).eps
    a, b, rdx, rdy = RKW["dt"] * RKW["K"], RKW["dt"] / RKW["rho"], 1 / RKW["dx"], 1 / RKW["dy"]
    mp, mx, my = (g.abs().max().item() for g in gin)
    scale_r = mp + 2 * b * (rdx * mx + rdy * my)
    scales = (scale_r, mx + 2 * a * rdx * scale_r, my + 2 * a * rdy * scale_r)
    ratios = [(g.double() - w).abs().max().item() / (eps * s) for g, w, s in zip(got, want, scales)]
    print(dtype, "error / (eps scale) of gP, gVx, gVy:", ratios)
    assert all(r <= 16 for r in ratios)


# --------------------------------------------------------------- boundary rule
def check_boundary_rule(run):
    """``run(gin) -> gout`` on tensors of its device; compared on the host.
    Shared with the GPU tests."""
    nx, ny = 6, 9
    gin = random_fields(nx, ny, F64, 3)
    base = run(gin)
    bad = [g.clone() for g in gin]
    nan = float("nan")
    bad[1][0, :] = nan
    bad[1][nx, :] = nan
    bad[2][:, 0] = nan
    bad[2][:, ny] = nan
    out = run(bad)
    assert torch.isfinite(out[0]).all()
    mx = torch.zeros_like(out[1], dtype=torch.bool)
    mx[0, :] = mx[nx, :] = True
    my = torch.zeros_like(out[2], dtype=torch.bool)
    my[:, 0] = my[:, ny] = True
    assert torch.equal(~torch.isfinite(out[1]), mx) and torch.equal(~torch.isfinite(out[2]), my)
    assert torch.equal(bits(out[0]), bits(base[0]))
    assert torch.equal(bits(out[1])[~mx], bits(base[1])[~mx]) and torch.equal(bits(out[2])[~my], bits(base[2])[~my])
    # the boundary faces: gV2 of the face plus the one cell next to it
    a, rdx, rdy = RKW["dt"] * RKW["K"], 1 / RKW["dx"], 1 / RKW["dy"]
    r = base[0]
    assert torch.equal(bits(base[1][0]), bits(gin[1][0] + (a * r[0]) * rdx))
    assert torch.equal(bits(base[1][nx]), bits(gin[1][nx] - (a * r[nx - 1]) * rdx))
    assert torch.equal(bits(base[2][:, 0]), bits(gin[2][:, 0] + (a * r[:, 0]) * rdy))
    assert torch.equal(bits(base[2][:, ny]), bits(gin[2][:, ny] - (a * r[:, ny - 1]) * rdy))
    # a NaN on an inner face reaches r of its two cells, hence their faces
    bad = [g.clone() for g in gin]
    bad[1][3, 4] = nan
    out = run(bad)
    want = torch.zeros_like(out[0], dtype=torch.bool)
    want[2:4, 4] = True
    assert torch.equal(torch.isnan(out[0]), want)
    wx = torch.zeros_like(out[1], dtype=torch.bool)
    wx[2:5, 4] = True
    assert torch.equal(torch.isnan(out[1]), wx)


def test_boundary_rule():
    check_boundary_rule(lambda gin: adjoint(gin, RKW))


# -------------------------------------------------------------------- refusals
def check_errors(device):
    """Every refused call leaves all six arrays as they were."""
    nx, ny = 4, 6
    names = ("gP", "gVx", "gVy", "gP2", "gVx2", "gVy2")
    gin = random_fields(nx, ny, F64, 4, device)
    arrays = dict(zip(names, [torch.full_like(g, 5.0) for g in gin] + gin))
    before = {k: v.clone() for k, v in arrays.items()}
    A = arrays
    z = lambda *s, dt=F64: torch.zeros(s, dtype=dt, device=device)
    wide = z(nx + 1, 2 * ny)
    pool = z(200)
    cases = [
        dict(gP=z(nx, ny + 1)), dict(gVx=z(nx, ny)), dict(gVy=z(nx + 1, ny)), dict(gVy=z(nx, ny)),
        dict(gP2=z(nx + 1, ny)), dict(gVx2=z(nx + 2, ny)), dict(gVy2=z(nx, ny + 2)),
        dict(gP=z(nx - 1, ny), gVx=z(nx, ny), gVy=z(nx - 1, ny + 1)),            # outputs of another grid
        dict(gP=z(nx * ny)), dict(gP2=z(1, nx, ny)),                             # not 2-D
        dict(gP=A["gP"].float()), dict(gVx2=A["gVx2"].float()), dict(gVy=A["gVy"].float()),
        {k: v.to(torch.int64) for k, v in A.items()},                            # no float type
        {k: v.to(torch.float16) for k, v in A.items()},
        dict(gVx=wide[:, ::2]), dict(gVx2=wide[:, :ny]), dict(gP=wide[:nx, ::2]),
        dict(gP=A["gP2"]), dict(gVx=A["gVx2"]), dict(gVy=A["gVy2"]),             # an output is an input
        dict(gP=A["gVx2"][:nx]), dict(gVx=A["gVx"], gP=A["gVx"][1:]),            # ... overlaps one, or an output
        dict(gP=pool[:nx * ny].view(nx, ny), gVy=pool[nx * ny - 1:nx * ny - 1 + nx * (ny + 1)].view(nx, ny + 1)),
        dict(gP=z(0, ny), gVx=z(1, ny), gVy=z(0, ny + 1), gP2=z(0, ny), gVx2=z(1, ny), gVy2=z(0, ny + 1)),
        dict(gP=z(nx, 0), gVx=z(nx + 1, 0), gVy=z(nx, 1), gP2=z(nx, 0), gVx2=z(nx + 1, 0), gVy2=z(nx, 1)),
    ]
    if device.type != "cpu":
        cases += [dict(gP=A["gP"].cpu()), dict(gVy2=A["gVy2"].cpu())]
    for change in cases:
        kw = dict(A)
        kw.update(change)
        with pytest.raises(igg.IGGError, match="acoustic2d_adjoint"):
            stencil.acoustic2d_adjoint_(*(kw[k] for k in names), **RKW)
        for k in arrays:
            assert torch.equal(bits(arrays[k]), bits(before[k])), (list(change), k)
        assert (wide == 0).all() and (pool == 0).all()
    with pytest.raises(igg.IGGError, match="chunk"):
        stencil.acoustic2d_adjoint_(*(A[k] for k in names), chunk=-1, **RKW)
    for k in arrays:
        assert torch.equal(bits(arrays[k]), bits(before[k]))


def test_errors_leave_arrays_unchanged():
    check_errors(torch.device("cpu"))


# ------------------------------------------------------ igg.autograd.acoustic2d
def test_autograd_gradcheck():
    x = random_fields(4, 5, F64, 5)
    f = lambda p, vx, vy: igg.autograd.acoustic2d(p, vx, vy, **RKW)
    assert torch.autograd.gradcheck(f, [t.clone().requires_grad_() for t in x])
    assert torch.autograd.gradcheck(f, (x[0].clone().requires_grad_(), x[1], x[2]))
    assert torch.autograd.gradcheck(f, (x[0], x[1], x[2].clone().requires_grad_()))
    out = f(*x)
    for a, b in zip(out, forward_native(x, RKW)):
        assert torch.equal(a, b)
    assert not out[0].requires_grad
    # inputs that need no gradient get none
    p = x[0].clone().requires_grad_()
    outs = igg.autograd.acoustic2d(p, x[1], x[2], **RKW)
    g = random_fields(4, 5, F64, 6)
    grads = torch.autograd.grad(outs, (p,), g)
    assert torch.equal(grads[0], adjoint(g, RKW)[0])


def test_autograd_three_steps_equal_adjoint_run():
    """Three steps ``acoustic2d`` + ``update_halo(Vx2, Vy2)`` on one periodic
    rank: the gradient equals ``adjoint_run(3)`` of a model on that grid,
    exactly on dyadic data."""
    igg.init_global_grid(6, 7, 1, periodx=1, periody=1, **GRID)
    m = dyadic_model(torch.device("cpu"), F64)
    x0 = [t.clone() for t in int_fields(m, 7)]
    g = int_fields(m, 8)
    x = [t.clone().requires_grad_() for t in x0]
    P, Vx, Vy = x
    for _ in range(3):
        P, Vx, Vy = igg.autograd.acoustic2d(P, Vx, Vy, **MKW)
        Vx, Vy = igg.autograd.update_halo(Vx, Vy)
    grads = torch.autograd.grad((P, Vx, Vy), x, g)
    want = m.adjoint_run(3, *g)
    for a, b in zip(grads, want):
        assert torch.equal(a, b)
    assert grads[0].abs().max() > 0
    igg.finalize_global_grid(finalize_MPI=False)


# ----------------------------------------------------------------- adjoint_run
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("periodic", [0, 1])
def test_adjoint_run_is_the_transpose_of_run(periodic, dtype):
    """``sum <g, run(3) x> == sum <adjoint_run(3, g), x>`` on one rank, exactly
    (dyadic model, integer fields); the model's fields are not touched."""
    igg.init_global_grid(6, 7, 1, periodx=periodic, periody=periodic, **GRID)
    m = dyadic_model(torch.device("cpu"), dtype)
    x = int_fields(m, 9)
    g = int_fields(m, 10)
    for dst, src in zip((m.P, m.Vx, m.Vy), x):
        dst.copy_(src)
    m.mark_modified()
    names = ("P", "Vx", "Vy", "P2", "Vx2", "Vy2")
    before = {k: getattr(m, k).clone() for k in names}
    ptrs = {k: getattr(m, k).data_ptr() for k in names}
    gcopy = [t.clone() for t in g]
    res = m.adjoint_run(3, *g)
    for k in names:
        assert getattr(m, k).data_ptr() == ptrs[k] and torch.equal(bits(getattr(m, k)), bits(before[k]))
    assert all(torch.equal(a, b) for a, b in zip(g, gcopy))
    m.run(3)
    lhs = sum((a.double() * b.double()).sum().item() for a, b in zip(g, (m.P, m.Vx, m.Vy)))
    rhs = sum((a.double() * b.double()).sum().item() for a, b in zip(res, x))
    assert lhs == rhs and lhs != 0
    # nt = 0: copies
    zero = m.adjoint_run(0, *g)
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(zero, g))
    # out=: fresh tensors, and in place (out is g)
    for nt in (2, 3):
        want = m.adjoint_run(nt, *g)
        out = [torch.full_like(t, 7.0) for t in g]
        got = m.adjoint_run(nt, *g, out=out)
        assert all(a is b for a, b in zip(got, out)) and all(torch.equal(a, b) for a, b in zip(out, want))
        mine = [t.clone() for t in g]
        got = m.adjoint_run(nt, *mine, out=mine)
        assert all(a is b for a, b in zip(got, mine)) and all(torch.equal(a, b) for a, b in zip(mine, want))
    igg.finalize_global_grid(finalize_MPI=False)


def test_adjoint_run_argument_errors():
    igg.init_global_grid(6, 7, 1, **GRID)
    m = dyadic_model(torch.device("cpu"), F64)
    g = int_fields(m, 11)
    with pytest.raises(igg.IGGError, match="nt"):
        m.adjoint_run(-1, *g)
    with pytest.raises(igg.IGGError, match="gP"):
        m.adjoint_run(1, g[0][:-1], g[1], g[2])
    with pytest.raises(igg.IGGError, match="gVx"):
        m.adjoint_run(1, g[0], g[1].float(), g[2])
    with pytest.raises(igg.IGGError, match="gVy"):
        m.adjoint_run(1, g[0], g[1], torch.zeros(6, 16, dtype=F64)[:, ::2])
    with pytest.raises(igg.IGGError, match="out"):
        m.adjoint_run(1, *g, out=g[0])
    with pytest.raises(igg.IGGError, match="out Vx"):
        m.adjoint_run(1, *g, out=[g[0].clone(), g[1][:-1].clone(), g[2].clone()])
    # out tensors that share bytes with one another, or with another field's g
    pool = torch.zeros(6 * 7 + 6 * 8 - 1, dtype=F64)
    with pytest.raises(igg.IGGError, match="overlaps"):
        m.adjoint_run(1, *g, out=[pool[:42].view(6, 7), g[1].clone(), pool[41:].view(6, 8)])
    with pytest.raises(igg.IGGError, match="overlaps"):
        m.adjoint_run(1, g[0], g[1], pool[41:].view(6, 8), out=[pool[:42].view(6, 7), g[1].clone(), g[2].clone()])
    assert (pool == 0).all()
    igg.finalize_global_grid(finalize_MPI=False)


def test_adjoint_run_refuses_what_accumulate_halo_refuses():
    """Vx has ol = 3 along x: n = 3 < 3 + 1 is refused as soon as x has a
    neighbour (set by hand, as tests/test_accumulate_halo_cpu.py does)."""
    from igg.parallel import grid as G
    from igg.parallel import halo as HL

    igg.init_global_grid(2, 6, 1, **GRID)
    m = dyadic_model(torch.device("cpu"), F64)
    g = [torch.ones_like(t) for t in (m.P, m.Vx, m.Vy)]
    assert m.adjoint_run(1, *g)[0].shape == g[0].shape  # no neighbour: nothing to refuse
    gg = G.global_grid()
    gg.neighbors[1, 0] = 1
    HL.sync_grid()
    try:
        with pytest.raises(igg.IGGError, match="too small in dimension 1 to accumulate its halo"):
            m.adjoint_run(1, *g)
    finally:
        gg.neighbors[1, 0] = igg.PROC_NULL
        HL.sync_grid()
    assert all((t == 1).all() for t in g)
    igg.finalize_global_grid(finalize_MPI=False)


# ----------------------------------------------------------------------- ranks
def single_rank_reference(dims, periodic, nt, path):
    """``adjoint_run(nt)`` of one rank on the ranks' global grid, saved for the workers."""
    igg.init_global_grid(*single_rank_size(dims), 1, periodx=periodic, periody=periodic, **GRID)
    m = dyadic_model(torch.device("cpu"), F64)
    G = global_adjoint(m, nt)
    igg.finalize_global_grid(finalize_MPI=False)
    np.savez(path, P=G[0].numpy(), Vx=G[1].numpy(), Vy=G[2].numpy())
    return G


@pytest.mark.parametrize("periodic", [0, 1])
@pytest.mark.parametrize("nprocs,dims", [(2, (2, 1)), (4, (2, 2))])
def test_adjoint_run_ranks(nprocs, dims, periodic, tmp_path):
    """(a) the inner-product identity summed over the ranks, (b) the ranks'
    results, copies added, equal the single rank's on the global grid."""
    path = str(tmp_path / "ref.npz")
    G = single_rank_reference(dims, periodic, 3, path)
    assert all(t.abs().max() > 0 for t in G)
    run_ranks(nprocs, "cpu", *dims, periodic, 3, path)


# ------------------------------------------------------------------ the example
@pytest.mark.parametrize("nprocs", [1, 2])
def test_example(nprocs):
    args = [os.path.join(ROOT, "examples", "acoustic_adjoint.py"), "--cpu", "--nx", "12", "--nt", "6"]
    if nprocs == 1:
        cmd = [sys.executable] + args
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nprocs}",
               "--master-addr", "127.0.0.1", "--master-port", str(free_port())] + args
    env = dict(os.environ, OMP_NUM_THREADS="1", IGG_HOST_THREADS="2")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=160, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "adjoint check OK" in r.stdout and f"{nprocs} process(es)" in r.stdout


# ------------------------------------------------------------ kernel resources
def test_kernel_resources_of_the_new_unit():
    """0 scratch, 0 spills and 0 LDS in every instantiation (the rows of
    tools/kernel_resources.py, read as tests/test_kernel_resources.py reads them)."""
    import importlib.util as ilu

    spec = ilu.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = ilu.module_from_spec(spec)
    spec.loader.exec_module(kr)
    objs = kr.objects()
    if not objs:
        pytest.skip("no HIP objects under build/native (run `python build.py`)")
    rows = kr.table(objs).get("acoustic_adj_kernels", {})
    assert len(rows) == 4, list(rows)  # f32 / f64, vector and one point per lane
    for k, r in rows.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, (k, r)
