"""Per-rank scenarios of the spread_g tests (parallel/spread_g.py), launched by
tests/test_spread_g_cpu.py and tests/test_gpu_spread_g.py, one process per
rank - and the helpers both test files share: the point rules and the oracle,
written here in plain Python and independent of the native code.

The oracle knows nothing of the decomposition: it loops over the points, puts
every contribution ``w * v`` into a dict cell -> list, folds each list in order
in float64 (Python floats) and updates the cell of the directly built global
array once, with one rounding to the array's dtype.
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import igg  # noqa: E402
from tests.mp_worker_sample_g import (_allgather, _device, extents, global_values, local_of_global,  # noqa: E402
                                      point_set, valid_mask)


# ------------------------------------------------------------------ the oracle
def axis_of(u: float, E: int, per: int):
    """``(g, upper corner, t)`` of a coordinate, or ``None`` where it is
    invalid: the documented rules of ``sample_g``, in Python floats."""
    if not math.isfinite(u):
        return None
    Ef = float(E)
    if per:
        w = u - Ef * math.floor(u / Ef)
        if w >= Ef:
            w -= Ef
        if w < 0.0:
            w += Ef
        f = min(max(math.floor(w), 0.0), Ef - 1.0)
        g = int(f)
        return g, (g + 1) % E, w - f
    if not (0.0 <= u <= Ef - 1.0):
        return None
    f = min(math.floor(u), Ef - 2.0)
    g = int(f)
    return g, g + 1, u - f


def contributions(P, E, periods) -> list:
    """Per point the list of ``(global corner tuple, weight)`` it reaches, in
    corner order (x outermost); empty for an invalid point."""
    nd = len(E)
    out = []
    for p in range(P.shape[0]):
        axes = [axis_of(float(P[p, d]), E[d], periods[d]) for d in range(nd)]
        if any(a is None for a in axes):
            out.append([])
            continue
        per_dim = [[(a[0], 1.0 - a[2]), (a[1], a[2])] for a in axes]
        mine = [((), 1.0)]
        for k, corners in enumerate(per_dim):
            mine = [(c + (g,), (w * f if k else f)) for c, w in mine for g, f in corners if f != 0.0]
        out.append(mine)
    return out


def fold(values: list) -> float:
    s = values[0]
    for v in values[1:]:
        s = s + v
    return s


def add_folded(A: torch.Tensor, per_cell: dict) -> None:
    """``A[cell] = T(double(A[cell]) + fold)`` for every cell of the dict."""
    for cell, vals in per_cell.items():
        s = fold(vals)
        if A.dtype == torch.float64:
            A[cell] = float(A[cell]) + s
        else:
            A[cell] = torch.tensor(float(A[cell]) + s, dtype=torch.float64).to(A.dtype)


def oracle_global(G: torch.Tensor, P: torch.Tensor, V: torch.Tensor, periods) -> torch.Tensor:
    """``spread_g(copies="all")`` on the directly built global array."""
    out = G.clone()
    per_cell = {}
    for p, mine in enumerate(contributions(P.reshape(-1, G.dim()), tuple(G.shape), periods)):
        for cell, w in mine:
            per_cell.setdefault(cell, []).append(w * float(V[p]))
    add_folded(out, per_cell)
    return out


def oracle_owner(A: torch.Tensor, P: torch.Tensor, V: torch.Tensor, gg) -> torch.Tensor:
    """``spread_g(copies="owner")`` on this rank's local field: the rank that
    ``sample_owner`` names adds into its local ``lo`` / ``lo + 1`` cells."""
    nd = A.dim()
    E = extents(gg, A.shape)
    periods = [int(v) for v in gg.periods][:nd]
    out = A.clone()
    per_cell = {}
    for p, mine in enumerate(contributions(P.reshape(-1, nd), E, periods)):
        if not mine:
            continue
        axes = [axis_of(float(P.reshape(-1, nd)[p, d]), E[d], periods[d]) for d in range(nd)]
        lo = igg.sample_owner(gg.nxyz, gg.overlaps, gg.dims, gg.periods, gg.coords, tuple(A.shape),
                              tuple(a[0] for a in axes))
        if lo is None:
            continue
        for cell, w in mine:
            local = tuple(lo[d] + (0 if cell[d] == axes[d][0] else 1) for d in range(nd))
            per_cell.setdefault(local, []).append(w * float(V[p]))
    add_folded(out, per_cell)
    return out


def dyadic_points(E, periods, npts, seed) -> torch.Tensor:
    """Points at multiples of 1/4: inside ``[0, E-1]``, and beyond it in a
    periodic dimension (the wrap of a dyadic coordinate is exact)."""
    rng = np.random.default_rng(seed)
    cols = []
    for d in range(len(E)):
        lo, hi = (-2 * E[d], 3 * E[d]) if periods[d] else (0, E[d] - 1)
        cols.append(rng.integers(4 * lo, 4 * hi + 1, size=npts) / 4.0)
    return torch.from_numpy(np.stack(cols, axis=1).astype(np.float64)).contiguous()


def _setup(dev, dtype, dimx, dimy, dimz, periodic, overlap, nd, stagger):
    device = _device(dev)
    dt = getattr(torch, dtype)
    per, o, nd, stagger = int(periodic), int(overlap), int(nd), int(stagger)
    n = (9, 8, 7)
    grid_n = n[:nd] + (1,) * (3 - nd)
    me = igg.init_global_grid(
        *grid_n, dimx=int(dimx), dimy=int(dimy), dimz=int(dimz), periodx=per & 1, periody=(per >> 1) & 1,
        periodz=(per >> 2) & 1, overlapx=o, overlapy=o, overlapz=o, quiet=True, select_device=False,
        device_type="none" if dev == "cpu" else "AMDGPU")[0]
    gg = igg.get_global_grid()
    periods = [int(p) for p in gg.periods][:nd]
    shape = tuple(n[d] + (stagger if d == 0 else -stagger if d == 1 else 0) for d in range(nd))
    return device, dt, me, gg, periods, shape, extents(gg, shape)


def _permuted(A):
    perm = list(range(A.dim()))[::-1]
    return A.permute(perm).contiguous().permute(perm)


# ------------------------------------------------------------------ scenarios
def scenario_all(dev, dtype, dimx, dimy, dimz, periodic, overlap, nd, stagger="0"):
    """copies="all": gather_g of the result equals the oracle on the directly
    built global array, bit for bit; update_halo_ afterwards changes no bit."""
    device, dt, me, gg, periods, shape, E = _setup(dev, dtype, dimx, dimy, dimz, periodic, overlap, nd, stagger)
    Gs = [global_values(E, s, dt) for s in (1, 2)]
    fields = [local_of_global(G, shape).to(device) for G in Gs]
    if len(shape) > 1:
        fields[1] = _permuted(fields[1])
    Pc = torch.cat([point_set(E, periods, [int(v) for v in gg.nxyz], [int(v) for v in gg.overlaps],
                              [int(v) for v in gg.dims], nrandom=120),
                    dyadic_points(E, periods, 60, 3)])
    Pc = torch.cat([Pc, Pc[:40]])  # cells shared by several points
    rng = np.random.default_rng(77)
    Vc = torch.from_numpy(rng.standard_normal((2, Pc.shape[0])) * 10.0 ** rng.integers(-3, 4, size=(2, Pc.shape[0])))
    ok = valid_mask(Pc, E, periods)
    assert int(ok.sum()) >= 150 and int((~ok).sum()) >= 6
    before = [A.clone() for A in fields]
    igg.spread_g(tuple(fields), Pc.to(device), Vc.to(device))
    for k, (A, G) in enumerate(zip(fields, Gs)):
        assert A.stride() == before[k].stride()
        want = oracle_global(G, Pc, Vc[k], periods)
        got = torch.empty(E, dtype=dt) if me == 0 else None
        igg.gather_g(A, got)
        if me == 0:
            assert not torch.equal(bits_of(want), bits_of(G))
            assert torch.equal(bits_of(got), bits_of(want)), \
                f"field {k}: {int((bits_of(got) != bits_of(want)).sum())} global cells differ from the oracle"
        # every copy of a global cell holds that cell: nothing for update_halo_ to change
        assert torch.equal(bits_of(A), bits_of(local_of_global(want, shape))), f"rank {me} field {k}: a copy differs"
        B = A.clone()
        igg.update_halo_(B)
        assert torch.equal(bits_of(B), bits_of(A)), f"rank {me} field {k}: update_halo_ changed a bit"
    # a single tensor equals the tuple's first field
    one = before[0].clone()
    igg.spread_g(one, Pc.to(device), Vc[0].to(device))
    assert torch.equal(bits_of(one), bits_of(fields[0]))
    igg.finalize_global_grid()
    print(f"rank {me} spread_g OK")


def bits_of(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _sum_ranks(x: float) -> float:
    parts = _allgather(torch.tensor([x], dtype=torch.float64))
    s = 0.0
    for p in parts:
        s += float(p[0])
    return s


def scenario_owner(dev, dtype, dimx, dimy, dimz, periodic, overlap, nd, stagger="0"):
    """copies="owner": sum over the ranks of <A_r, spread_r> equals <sample_g(A),
    V> - exactly on dyadic data, within the count of rounded operations on
    random float64 data - and this rank's part equals the oracle's."""
    device, dt, me, gg, periods, shape, E = _setup(dev, dtype, dimx, dimy, dimz, periodic, overlap, nd, stagger)
    nd = len(shape)
    A = local_of_global(global_values(E, 5, dt), shape).to(device)
    # exact: weights are multiples of 4^-nd, the field of 1/64, the values small integers
    Pc = dyadic_points(E, periods, 200, 9)
    rng = np.random.default_rng(31)
    Vc = torch.from_numpy(rng.integers(-8, 9, size=200).astype(np.float64))
    Z = torch.zeros(shape, dtype=dt, device=device)
    igg.spread_g(Z, Pc.to(device), Vc.to(device), copies="owner")
    assert torch.equal(bits_of(Z), bits_of(oracle_owner(torch.zeros(shape, dtype=dt), Pc, Vc, gg))), f"rank {me}"
    lhs = _sum_ranks(float((A.double() * Z.double()).sum()))
    s = igg.sample_g(A, Pc.to(device)).cpu()
    assert not torch.isnan(s).any()
    rhs = float((s * Vc).sum())
    assert lhs == rhs and rhs != 0.0, (lhs, rhs)
    if dt == torch.float64:
        Pr = point_set(E, periods, [int(v) for v in gg.nxyz], [int(v) for v in gg.overlaps],
                       [int(v) for v in gg.dims], nrandom=150)
        ok = valid_mask(Pr, E, periods)
        Vr = torch.from_numpy(rng.standard_normal(Pr.shape[0]))
        Ar = local_of_global(torch.from_numpy(rng.standard_normal(E)), shape).to(device)  # (the same on every rank)
        Zr = torch.zeros(shape, dtype=dt, device=device)
        igg.spread_g(Zr, Pr.to(device), Vr.to(device), copies="owner")
        lhs = _sum_ranks(float((Ar * Zr).sum()))
        sr = igg.sample_g(Ar, Pr.to(device)).cpu()
        assert torch.equal(torch.isnan(sr), ~ok)
        rhs = float((sr[ok] * Vr[ok]).sum())
        scale = float((igg.sample_g(Ar.abs(), Pr.to(device)).cpu()[ok] * Vr[ok].abs()).sum())  # sum |w*A*v|
        npts = int(ok.sum())
        bound = (npts * 2 ** nd + 4 * nd) * 2.0 ** -52 * scale
        print(f"rank {me}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
        assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    igg.finalize_global_grid()
    print(f"rank {me} spread_g OK")


def scenario_autograd(dev, dtype, dimx, dimy, dimz, periodic, overlap, nd):
    """loss = <c, sample_g(update_halo(A), P)>, replicated: the gradient of
    igg.autograd against differences of the loss, cell by cell and rank by
    rank (the loss is linear in A, so a difference with step 1 is its slope)."""
    device, dt, me, gg, periods, shape, E = _setup(dev, dtype, dimx, dimy, dimz, periodic, overlap, nd, 0)
    rng = np.random.default_rng(5)  # the same on every rank
    Pc = point_set(E, periods, [int(v) for v in gg.nxyz], [int(v) for v in gg.overlaps], [int(v) for v in gg.dims],
                   nrandom=60)
    Pc = Pc[valid_mask(Pc, E, periods)]
    c = torch.from_numpy(rng.standard_normal(Pc.shape[0])).to(device)
    P = Pc.to(device)
    rngl = np.random.default_rng(100 + me)
    A0 = torch.from_numpy(rngl.standard_normal(shape)).to(dt).to(device)

    def loss(A):
        return (igg.autograd.sample_g(igg.autograd.update_halo(A), P) * c).sum()

    A = A0.clone().requires_grad_(True)
    L0 = loss(A)
    L0.backward()
    g = A.grad.cpu()
    assert g.shape == shape and g.dtype == dt
    # a loss is a sum of c_p * (a convex combination of cells): its rounding error is a few eps * sum|c| * max|A|
    scale = float(c.abs().sum()) * (max(float(a.max()) for a in _allgather(A0.abs().max().reshape(1).double())) + 1.0)
    nprocs = int(gg.nprocs)
    cells = [tuple(int(v) for v in rng.integers(0, shape[d], size=24)) for d in range(len(shape))]
    checked = 0
    for r in range(nprocs):
        for k in range(24):
            idx = tuple(cells[d][k] for d in range(len(shape)))
            B = A0.clone()
            if r == me:
                B[idx] += 1.0
            with torch.no_grad():
                L1 = loss(B)
            if r == me:
                slope = float(L1 - L0.detach())
                tol = 64 * float(torch.finfo(dt).eps) * scale
                assert abs(slope - float(g[idx])) <= tol, (me, idx, slope, float(g[idx]), tol)
                checked += 1
    assert checked == 24 and float(g.abs().sum()) > 0
    igg.finalize_global_grid()
    print(f"rank {me} spread_g OK")


if __name__ == "__main__":
    name, *args = sys.argv[1:]
    globals()[f"scenario_{name}"](*args)
