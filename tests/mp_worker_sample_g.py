"""Per-rank scenarios of the sample_g tests (parallel/sample_g.py), launched
by tests/test_sample_g_cpu.py and tests/test_gpu_sample_g.py, one process per
rank - and the helpers both test files share: the global field built from
global indices, the point sets, and the oracle, ``native.host_sample`` applied
to the directly built global array by the test itself.

The oracle knows nothing of the decomposition: it sees one array holding the
whole global index range (a periodic dimension gets its first plane appended,
so that the upper corner of the last cell is the next element) and a table
with the single segment ``[0, E)``.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import igg  # noqa: E402
from igg._native import native  # noqa: E402
from igg.parallel.gather_g import _extent  # noqa: E402

NAN_BITS = 0x7FF8000000000000


def _device(kind):
    if kind == "mgpu":  # one rank per device
        r = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(r)
        return torch.device("cuda", r)
    if kind == "gpu":  # every rank on device 0
        torch.cuda.set_device(0)
        return torch.device("cuda", 0)
    return torch.device("cpu")


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int64)


# ------------------------------------------------------------ field and oracle
def global_values(E, seed, dtype=torch.float64) -> torch.Tensor:
    """A pseudo-random field over the global index range ``E`` (a tuple), a
    function of the global indices alone: multiples of 1/64 in (-16, 16),
    exact in f32 and f64."""
    idx = np.indices(E).astype(np.int64)
    h = np.full(E, 12345 + 7919 * seed, dtype=np.int64)
    for d in range(len(E)):
        h = (h * 1103515245 + (idx[d] + 1) * (2654435761 + 97 * d)) % 2147483647
    return torch.from_numpy(((h % 2047) - 1023).astype(np.float64) / 64.0).to(dtype)


def local_of_global(G: torch.Tensor, shape) -> torch.Tensor:
    """This rank's local field of ``shape``: every local cell, halo and
    overlap included, holds its global cell (``indices_g``)."""
    A = torch.empty(shape, dtype=G.dtype)
    ix = [igg.indices_g(d, A) for d in range(len(shape))]
    return G[np.ix_(*[i.numpy() for i in ix])].clone()


def oracle(Gs, P: torch.Tensor, periods, me0=True) -> torch.Tensor:
    """``host_sample`` of the global arrays ``Gs`` (a list, one shape) at the
    CPU points ``P``: float64 ``(len(Gs), npts)``."""
    nd = Gs[0].dim()
    padded, table = [], []
    for G in Gs:
        for d in range(nd):
            if periods[d]:
                G = torch.cat([G, G.narrow(d, 0, 1)], dim=d)
        padded.append(G.contiguous())
    for d in range(nd):
        E = int(Gs[0].shape[d])
        table.append((E, int(periods[d]), int(padded[0].shape[d]), [[0, E, 0]]))
    P = P.reshape(-1, nd).contiguous()
    npts = int(P.shape[0])
    out = torch.full((len(Gs), npts), 7.0, dtype=torch.float64)
    native.host_sample(table, [(G.data_ptr(), list(G.stride())) for G in padded], padded[0].element_size(),
                       P.data_ptr(), nd, 1, npts, out.data_ptr(), npts, me0)
    return out


def extents(gg, shape) -> tuple:
    return tuple(_extent(int(gg.nxyz[d]), int(gg.overlaps[d]), int(gg.dims[d]), int(gg.periods[d]), int(shape[d]))
                 for d in range(len(shape)))


def point_set(E, periods, nxyz, overlaps, dims, seed=0, nrandom=200) -> torch.Tensor:
    """About 300 points of the index space ``E``: random ones (a periodic
    dimension also outside of [0, E)), points exactly on rank boundaries and
    in the overlaps, the domain's corners, the wrap, and invalid ones."""
    nd = len(E)
    rng = np.random.default_rng(1000 + seed)
    lo = [-1.5 * E[d] if periods[d] else 0.0 for d in range(nd)]
    hi = [2.5 * E[d] if periods[d] else E[d] - 1.0 for d in range(nd)]
    pts = [rng.uniform(lo, hi, size=(nrandom, nd))]
    # lattice values of interest per dimension: rank boundaries, overlaps, edges, the wrap
    special = []
    for d in range(nd):
        s = {0.0, 0.5, E[d] - 1.0, E[d] - 1.5, E[d] - 2.0, 1.0}
        for c in range(1, dims[d] + 1):
            b = c * (nxyz[d] - overlaps[d])
            for k in range(-1, overlaps[d] + 1):
                for frac in (0.0, 0.25):
                    v = b + k + frac
                    if periods[d] or 0.0 <= v <= E[d] - 1.0:
                        s.add(float(v))
        if periods[d]:
            s |= {float(E[d]), E[d] - 0.5, -0.25, -1.0, E[d] + 0.75, -float(E[d]), 2.0 * E[d] + 0.5}
        special.append(sorted(s))
    n = max(len(s) for s in special)
    for shift in range(3):  # each value of a dimension with three partners of the others
        pts.append(np.array([[special[d][(i * (d + 1) + shift * d) % len(special[d])] for d in range(nd)]
                             for i in range(n)]))
    # the corners of the domain
    pts.append(np.array(np.meshgrid(*[[0.0, E[d] - 1.0] for d in range(nd)], indexing="ij")).reshape(nd, -1).T)
    # invalid points: non-finite coordinates everywhere, out of the domain where it has an edge
    bad = [np.nan, np.inf, -np.inf]
    for d in range(nd):
        if not periods[d]:
            bad += [-0.25, E[d] - 0.75, -1e300]
        for v in bad[-3:] if not periods[d] else bad[:3]:
            p = np.array([1.25] * nd)
            p[d] = v
            pts.append(p[None, :])
        for v in bad[:3]:
            p = np.array([0.5] * nd)
            p[d] = v
            pts.append(p[None, :])
    return torch.from_numpy(np.concatenate(pts, axis=0).astype(np.float64)).contiguous()


def valid_mask(P: torch.Tensor, E, periods) -> torch.Tensor:
    ok = torch.isfinite(P).all(dim=1)
    for d in range(len(E)):
        if not periods[d]:
            ok &= (P[:, d] >= 0) & (P[:, d] <= E[d] - 1)
    return ok


def _allgather(t: torch.Tensor) -> list:
    import torch.distributed as dist

    gg = igg.get_global_grid()
    t = t.cpu().contiguous()
    outs = [torch.empty_like(t) for _ in range(int(gg.nprocs))]
    dist.all_gather(outs, t, group=gg.comm.gloo)
    return outs


# ------------------------------------------------------------------ scenarios
def scenario_sample(dev, dtype, dimx, dimy, dimz, periodic, overlap, nd, stagger="0", exchange="0"):
    """sample_g of fields built from global indices against the oracle, bit
    for bit; local partials; a tuple of fields; a Recorder. ``exchange``: the
    halo planes hold garbage and ``update_halo_`` runs first."""
    device = _device(dev)
    dt = getattr(torch, dtype)
    per, o, nd, stagger = int(periodic), int(overlap), int(nd), int(stagger)
    n = (9, 8, 7)
    grid_n = n[:nd] + (1,) * (3 - nd)
    me, dims, nprocs, coords, comm = igg.init_global_grid(
        *grid_n, dimx=int(dimx), dimy=int(dimy), dimz=int(dimz), periodx=per & 1, periody=(per >> 1) & 1,
        periodz=(per >> 2) & 1, overlapx=o, overlapy=o, overlapz=o, quiet=True, select_device=False,
        device_type="none" if dev == "cpu" else "AMDGPU")
    gg = igg.get_global_grid()
    periods = [int(p) for p in gg.periods][:nd]
    shape = tuple(n[d] + (stagger if d == 0 else -stagger if d == 1 else 0) for d in range(nd))
    E = extents(gg, shape)
    Gs = [global_values(E, s, dt) for s in (1, 2, 3)]
    locs = [local_of_global(G, shape) for G in Gs]
    if int(exchange):
        for A in locs:
            for d in range(nd):
                for side, at in ((0, 0), (1, shape[d] - 1)):
                    if igg.parallel.grid.has_neighbor(side + 1, d + 1):
                        A.narrow(d, at, 1).fill_(-777.0)
    fields = [A.to(device) for A in locs]
    # the second field in a permuted layout: strides may differ
    if nd > 1:
        perm = list(range(nd))[::-1]
        fields[1] = fields[1].permute(perm).contiguous().permute(perm)
        assert fields[1].stride() != fields[0].stride()
    if int(exchange):
        igg.update_halo_(*fields)
    Pc = point_set(E, periods, [int(v) for v in gg.nxyz], [int(v) for v in gg.overlaps], [int(v) for v in gg.dims])
    P = Pc.to(device)
    want = oracle(Gs, Pc, periods)
    ok = valid_mask(Pc, E, periods)
    assert int(ok.sum()) >= 200 and int((~ok).sum()) >= 6, (int(ok.sum()), int((~ok).sum()))
    assert (bits(want[:, ~ok]) == NAN_BITS).all() and not torch.isnan(want[:, ok]).any()

    got3 = igg.sample_g(tuple(fields), P)
    assert got3.shape == want.shape and got3.dtype == torch.float64 and got3.device == P.device
    assert torch.equal(bits(got3), bits(want)), \
        f"rank {me}: {int((bits(got3) != bits(want)).sum())} values differ from the oracle"
    for k in range(3):  # a tuple of 3 fields equals three single calls; a transposed P
        one = igg.sample_g(fields[k], P.t().contiguous().t() if k == 1 else P)
        assert one.shape == (P.shape[0],) and torch.equal(bits(one), bits(want[k])), f"rank {me} field {k}"
    # local partials: one rank is non-zero in bits per valid point (a value of +0.0 excepted: the field has none
    # at these points or the oracle says so); the NaN of an invalid point comes from rank 0 alone
    part = igg.sample_g(fields[0], P, local=True)
    parts = torch.stack([bits(p) for p in _allgather(part)])
    nonzero = (parts != 0).sum(dim=0)
    zero_value = bits(want[0]) == 0
    assert (nonzero[ok & ~zero_value] == 1).all(), f"rank {me}: a valid point has {nonzero[ok].tolist()} owners"
    assert (nonzero[ok & zero_value] == 0).all()
    assert (parts[0][~ok] == NAN_BITS).all() and (parts[1:, ~ok] == 0).all()
    assert torch.equal(parts.sum(dim=0), bits(want[0]))
    # out=
    out = torch.full((3, P.shape[0]), 5.0, dtype=torch.float64, device=device)
    assert igg.sample_g(tuple(fields), P, out=out) is out and torch.equal(bits(out), bits(want))

    # Recorder: 5 records equal 5 stacked sample_g calls; overflow raises; reset works
    rec = igg.Recorder(tuple(fields[:2]), P, 5)
    rows = []
    for step in range(5):
        cur = [A + float(step) for A in fields[:2]] if not int(exchange) else fields[:2]
        rec.record(*cur)
        rows.append(igg.sample_g(tuple(cur), P))
    res = rec.result()
    assert res.shape == (5, 2, P.shape[0]) and torch.equal(bits(res), bits(torch.stack(rows)))
    assert torch.equal(bits(rec.result()), bits(res))  # again
    rec.record(*fields[:2])
    try:
        rec.result()
    except igg.IGGError:
        pass
    else:
        raise AssertionError("Recorder.result() after an overflow must raise")
    rec.reset()
    assert rec.result().shape == (0, 2, P.shape[0])
    rec.record(*fields[:2])
    one = igg.Recorder(fields[0], P, 2)
    one.record(fields[0])
    assert torch.equal(bits(rec.result()[0]), bits(want[:2])) and torch.equal(bits(one.result()), bits(want[:1]))
    igg.finalize_global_grid()
    print(f"rank {me} sample_g OK")


if __name__ == "__main__":
    name, *args = sys.argv[1:]
    globals()[f"scenario_{name}"](*args)
