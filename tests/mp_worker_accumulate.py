"""Per-rank scenarios of the accumulate_halo_ tests (parallel/accumulate.py),
launched by tests/test_accumulate_halo_cpu.py and
tests/test_gpu_accumulate_halo.py, one process per rank - and the plain numpy
emulation of the exchange and of its transpose that both test files check
against.

The emulation follows the definition, not the engine: it holds every rank's
local array, walks the ranks' Cartesian coordinates and moves whole slabs with
numpy slices. Every rank regenerates all ranks' inputs from seeds, emulates
the call on all of them and compares its own block. Values are integers of
magnitude at most 1024 (exact in f32 and f64), so every comparison is exact.
"""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import igg  # noqa: E402


def _device(kind):
    if kind == "mgpu":  # one rank per device
        r = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(r)
        return torch.device("cuda", r)
    if kind == "gpu":  # every rank on device 0
        torch.cuda.set_device(0)
        return torch.device("cuda", 0)
    return torch.device("cpu")


# ------------------------------------------------------------------ emulation
class Topology:
    """What the emulation knows of the grid: sizes, not the engine."""

    def __init__(self, dims, periods, nxyz, overlaps, widths):
        self.dims, self.periods = [int(x) for x in dims], [int(x) for x in periods]
        self.nxyz, self.overlaps, self.widths = [int(x) for x in nxyz], [int(x) for x in overlaps], [int(x) for x in widths]
        self.ranks = list(itertools.product(*[range(n) for n in self.dims]))  # row-major: the last coordinate fastest

    @classmethod
    def of_grid(cls):
        gg = igg.get_global_grid()
        return cls(gg.dims, gg.periods, gg.nxyz, gg.overlaps, gg.halowidths)

    def neighbor(self, coords, d, side):
        """Coordinates of the neighbour on ``side`` (0 left, 1 right) in ``d``, or None."""
        c = list(coords)
        c[d] += -1 if side == 0 else 1
        if not 0 <= c[d] < self.dims[d]:
            if not self.periods[d]:
                return None
            c[d] %= self.dims[d]
        return tuple(c)

    def slabs(self, shape, d):
        """(receive slabs, send slabs) of a field in ``d`` as slices [left, right], or None without a halo."""
        if d >= len(shape):
            return None
        m, w = shape[d], self.widths[d]
        ol = self.overlaps[d] + m - self.nxyz[d]
        if ol < 2:
            return None
        return [slice(0, w), slice(m - w, m)], [slice(ol - w, ol), slice(m - ol, m - ol + w)]


def _at(d, sl):
    return (slice(None),) * d + (sl,)


def emulate_exchange(topo, arrs):
    """update_halo_ on {coords: array}: x, y, z; a halo slab with a neighbour
    becomes that neighbour's send slab."""
    arrs = {c: a.copy() for c, a in arrs.items()}
    for d in range(3):
        old = {c: a.copy() for c, a in arrs.items()}
        for c, a in arrs.items():
            sl = topo.slabs(a.shape, d)
            if sl is None:
                continue
            recv, send = sl
            for side in (0, 1):
                nb = topo.neighbor(c, d, side)
                if nb is not None:
                    a[_at(d, recv[side])] = old[nb][_at(d, send[1 - side])]
    return arrs


def emulate_accumulate(topo, arrs):
    """accumulate_halo_ on {coords: array}: z, y, x; a halo slab with a
    neighbour goes to that neighbour and becomes zero; the left neighbour's
    message is added into the left send slab, then the right neighbour's into
    the right one."""
    arrs = {c: a.copy() for c, a in arrs.items()}
    for d in (2, 1, 0):
        old = {c: a.copy() for c, a in arrs.items()}
        for c, a in arrs.items():
            sl = topo.slabs(a.shape, d)
            if sl is None:
                continue
            for side in (0, 1):
                if topo.neighbor(c, d, side) is not None:
                    a[_at(d, sl[0][side])] = 0
        for c, a in arrs.items():
            sl = topo.slabs(a.shape, d)
            if sl is None:
                continue
            recv, send = sl
            for side in (0, 1):  # left first
                nb = topo.neighbor(c, d, side)
                if nb is not None:
                    a[_at(d, send[side])] += old[nb][_at(d, recv[1 - side])]
    return arrs


def rank_input(seed, rank_index, shape, np_dtype, integers=True):
    g = np.random.default_rng(1000 * seed + rank_index)
    if integers:
        return g.integers(-1024, 1025, size=shape).astype(np_dtype)
    return g.standard_normal(size=shape).astype(np_dtype)


# -------------------------------------------------------------------- scenarios
def _shapes(n, kind, w=1):
    if kind == "plain":
        return [n]
    # the grid's size and staggered fields, grouped in one call (a smaller field
    # has a smaller overlap, which a halo width of 2 does not admit)
    return [n, (n[0] + 1, n[1], n[2]), (n[0], n[1] - 1 if w == 1 else n[1] + 1, n[2] + 1)]


def _run_case(me, topo, device, dt, shapes, seed, integers=True):
    """accumulate_halo_ of `shapes` in one call against the emulation; the
    adjoint identity with one allreduce. Returns this rank's results."""
    import torch.distributed as dist

    npdt = np.float64 if dt == torch.float64 else np.float32
    mine = topo.ranks.index(tuple(int(c) for c in igg.get_global_grid().coords))
    assert mine == me, (mine, me)
    ys = [{c: rank_input(seed + 10 * k, r, s, npdt, integers) for r, c in enumerate(topo.ranks)}
          for k, s in enumerate(shapes)]
    xs = [{c: rank_input(seed + 10 * k + 5, r, s, npdt, integers) for r, c in enumerate(topo.ranks)}
          for k, s in enumerate(shapes)]
    c_me = topo.ranks[me]
    Y = [torch.from_numpy(y[c_me].copy()).to(device) for y in ys]
    igg.accumulate_halo_(*Y)
    for k, (y, got) in enumerate(zip(ys, Y)):
        want = emulate_accumulate(topo, y)[c_me]
        g = got.cpu().numpy()
        if not np.array_equal(g, want) or np.signbit(g[want == 0]).any():
            bad = np.argwhere(g != want)[:5].tolist()
            raise AssertionError(f"rank {me} field {k} {shapes[k]}: differs from the emulation at {bad}: got "
                                 f"{[g[tuple(b)] for b in bad]}, want {[want[tuple(b)] for b in bad]}")
    # <H x, y> == <x, H^T y>, summed over all local cells of all ranks
    X = [torch.from_numpy(x[c_me].copy()).to(device) for x in xs]
    HX = [x.clone() for x in X]
    igg.update_halo_(*HX)
    lhs = sum(float((hx.double().cpu() * torch.from_numpy(y[c_me]).double()).sum()) for hx, y in zip(HX, ys))
    rhs = sum(float((x.double().cpu() * hty.double().cpu()).sum()) for x, hty in zip(X, Y))
    both = torch.tensor([lhs, rhs], dtype=torch.float64)
    dist.all_reduce(both, group=igg.get_global_grid().comm.gloo)
    if integers:
        assert both[0].item() == both[1].item(), f"rank {me} {shapes}: <Hx,y>={both[0].item()} != <x,H'y>={both[1].item()}"
    return Y, ys


def scenario_accumulate(dev, dtype, dimx, dimy, dimz, periodic, overlap, halowidth, n="9,8,10"):
    device = _device(dev)
    dt = getattr(torch, dtype)
    per, o, w = int(periodic), int(overlap), int(halowidth)
    n = tuple(int(v) for v in n.split(","))
    me, dims, nprocs, coords, comm = igg.init_global_grid(
        *n, dimx=int(dimx), dimy=int(dimy), dimz=int(dimz), periodx=per & 1, periody=(per >> 1) & 1,
        periodz=(per >> 2) & 1, overlapx=o, overlapy=o, overlapz=o, halowidthx=w, halowidthy=w, halowidthz=w,
        quiet=True, select_device=False, device_type="none" if dev == "cpu" else "AMDGPU")
    topo = Topology.of_grid()
    assert len(topo.ranks) == nprocs
    _run_case(me, topo, device, dt, _shapes(n, "plain"), seed=1)
    _run_case(me, topo, device, dt, _shapes(n, "staggered", w), seed=2)
    # conservation: with overlap == 2 * width the owned box is [w, m - w) (to the
    # field's edge on a side without a neighbour): every halo cell with a
    # neighbour lands in an owned cell, so the call moves values and loses none
    if o == 2 * w:
        import torch.distributed as dist

        y = torch.from_numpy(rank_input(3, me, n, np.float64)).to(dt).to(device)
        before = torch.tensor([float(y.double().sum())], dtype=torch.float64)
        dist.all_reduce(before, group=igg.get_global_grid().comm.gloo)
        igg.accumulate_halo_(y)
        after = float(igg.sum_g(y))
        assert after == before.item(), f"rank {me}: sum_g after {after} != the local sums before {before.item()}"
    if dev != "cpu":
        # the GPU result against this worker's CPU result, bit for bit, on non-integer values
        gg = igg.get_global_grid()
        for shapes in ([n], _shapes(n, "staggered", w)):
            ys = [rank_input(7 + k, me, s, np.float64 if dt == torch.float64 else np.float32, integers=False)
                  for k, s in enumerate(shapes)]
            G = [torch.from_numpy(y.copy()).to(device) for y in ys]
            C = [torch.from_numpy(y.copy()) for y in ys]
            for _ in range(2):
                igg.accumulate_halo_(*G)
                igg.accumulate_halo_(*C)
            for k, (g, c) in enumerate(zip(G, C)):
                assert torch.equal(g.cpu().view(torch.uint8), c.view(torch.uint8)), \
                    f"rank {me} field {k} {shapes[k]}: GPU and CPU results differ in " \
                    f"{int((g.cpu() != c).sum())} cells"
        assert gg.nprocs == nprocs
    igg.finalize_global_grid()
    print(f"rank {me} accumulate OK")


def scenario_autograd(dev, dtype, dimx, dimy, dimz, periodic):
    """The gradient of sum(c * update_halo(A)) is accumulate_halo_(c); one
    finite-difference check of the same loss."""
    import torch.distributed as dist

    device = _device(dev)
    dt = getattr(torch, dtype)
    per = int(periodic)
    n = (6, 5, 4)
    me, dims, nprocs, coords, comm = igg.init_global_grid(
        *n, dimx=int(dimx), dimy=int(dimy), dimz=int(dimz), periodx=per & 1, periody=(per >> 1) & 1,
        periodz=(per >> 2) & 1, quiet=True, select_device=False, device_type="none" if dev == "cpu" else "AMDGPU")
    gloo = igg.get_global_grid().comm.gloo
    c = torch.from_numpy(rank_input(4, me, n, np.float64)).to(dt).to(device)
    A = torch.from_numpy(rank_input(5, me, n, np.float64)).to(dt).to(device).requires_grad_(True)
    B = torch.from_numpy(rank_input(6, me, (n[0] + 1, n[1], n[2]), np.float64)).to(dt).to(device).requires_grad_(True)
    cB = torch.from_numpy(rank_input(8, me, tuple(B.shape), np.float64)).to(dt).to(device)
    A0 = A.detach().clone()
    loss = (c * igg.autograd.update_halo(A)).sum()
    loss.backward()
    want = c.clone()
    igg.accumulate_halo_(want)
    assert torch.equal(A.grad, want), f"rank {me}: gradient differs from accumulate_halo_(c)"
    assert torch.equal(A.detach(), A0), "the input was modified"
    # two fields in one call
    A.grad = None
    outA, outB = igg.autograd.update_halo(A, B)
    ((c * outA).sum() + (cB * outB).sum()).backward()
    wa, wb = c.clone(), cB.clone()
    igg.accumulate_halo_(wa, wb)
    assert torch.equal(A.grad, wa) and torch.equal(B.grad, wb), f"rank {me}: grouped gradients differ"

    # finite differences of the global loss L(A) = sum over ranks of sum(c * H(A)):
    # L is linear, so (L(A + h*e) - L(A)) / h is the gradient component exactly in f64 on integers
    def global_loss(field):
        with torch.no_grad():
            t = torch.tensor([float((c.double() * igg.autograd.update_halo(field).double()).sum())],
                             dtype=torch.float64)
        dist.all_reduce(t, group=gloo)
        return t.item()

    base = global_loss(A0)
    for owner, cell in ((0, (1, 2, 1)), (nprocs - 1, (n[0] - 2, 0, 3)), (0, (n[0] - 2, n[1] - 2, n[2] - 2))):
        P = A0.clone()
        if me == owner:
            P[cell] += 2.0
        fd = (global_loss(P) - base) / 2.0
        if me == owner:
            assert fd == wa[cell].item(), f"rank {me} cell {cell}: finite difference {fd}, gradient {wa[cell].item()}"
    igg.finalize_global_grid()
    print(f"rank {me} accumulate OK")


if __name__ == "__main__":
    name, *args = sys.argv[1:]
    globals()[f"scenario_{name}"](*args)
