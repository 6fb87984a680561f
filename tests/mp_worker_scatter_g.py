"""Per-rank scenario of the scatter_g tests (parallel/scatter_g.py), launched by
tests/test_scatter_g_cpu.py and tests/test_gpu_scatter_g.py, one process per rank.

The global array holds an integer function of the GLOBAL index (|x| <= 1024:
exact in f32 and f64) and a rank's expected field is built from ``coords_g`` -
not from the code under test: every local cell whose global index lies in the
box holds the global cell of that index, every other cell keeps the sentinel
the field was filled with. After a scatter of the whole field ``update_halo_``
must change no bit and ``gather_g`` must return the global array."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import igg  # noqa: E402
from tests.mp_worker_gather_g import N, _device, _extents, _global_array, _indices_from_coords  # noqa: E402

SENTINEL = -7777


def _bounds(ext, box):
    box = box if box is not None else (None,) * len(ext)
    return [(0, ext[d]) if b is None else (b, b + 1) if isinstance(b, int) else tuple(b) for d, b in enumerate(box)]


def _expected(gg, shape, Fg, ext, box, dtype):
    """The field after the scatter, from coords_g alone."""
    probe = torch.empty(shape, device="meta")
    nd = len(shape)
    idx = [_indices_from_coords(gg, d, probe) for d in range(nd)]
    view = [[-1 if e == d else 1 for e in range(nd)] for d in range(nd)]
    inside = torch.ones(shape, dtype=torch.bool)
    for d, (lo, hi) in enumerate(_bounds(ext, box)):
        inside &= ((idx[d] >= lo) & (idx[d] < hi)).view(view[d])
    vals = Fg[tuple(i.view(v) for i, v in zip(idx, view))]
    return torch.where(inside, vals, torch.full_like(vals, SENTINEL)).to(dtype)


def _halo_exchangeable(gg, shape) -> bool:
    """update_halo_ takes this field (a wide halo needs an overlap of twice its width)."""
    for d in range(len(shape)):
        ol = int(gg.overlaps[d]) + shape[d] - int(gg.nxyz[d])
        if int(gg.halowidths[d]) > 1 and 2 <= ol < 2 * int(gg.halowidths[d]):
            return False
    return any(int(gg.overlaps[d]) + shape[d] - int(gg.nxyz[d]) >= 2 for d in range(len(shape)))


def _check(me, gg, shape, Fg, ext, dtype, device, *, root=0, box=None, gdtype=None, cpu_src=False, tag=""):
    gdtype = gdtype or dtype
    G = None
    if me == root:
        sl = tuple(slice(lo, hi) for lo, hi in _bounds(ext, box))
        G = Fg[sl].to(gdtype).contiguous().to("cpu" if cpu_src else device)
        assert tuple(G.shape) == igg.selection_shape_g(torch.empty(shape, device="meta"), box)
        G0 = G.clone()
    A = torch.full(shape, SENTINEL, dtype=dtype, device=device)
    igg.scatter_g(G, A, root=root, box=box)
    want = _expected(gg, shape, Fg, ext, box, dtype)
    got = A.cpu()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()[:5].tolist()
        raise AssertionError(f"rank {me} {tag} {shape} box={box} {gdtype}->{dtype}: differs at {bad}: got "
                             f"{[got[tuple(b)].item() for b in bad]}, want {[want[tuple(b)].item() for b in bad]}")
    if me == root:
        assert torch.equal(G, G0), f"{tag}: A_global was modified"
    if box is None:
        if _halo_exchangeable(gg, shape):
            igg.update_halo_(A)
            assert torch.equal(A.cpu(), want), f"rank {me} {tag} {shape}: update_halo_ changed the scattered field"
        # (gather_g reads owned cells only: the round trip also shows that every owned cell arrived)
        R = torch.full(tuple(ext), SENTINEL + 1, dtype=dtype, device=device) if me == root else None
        igg.gather_g(A, R, root=root)
        if me == root:
            assert torch.equal(R.cpu(), Fg.to(gdtype).to(dtype)), f"rank {me} {tag} {shape}: round trip differs"


def scenario_scatter(dev, dtype, dimx, dimy, dimz, periodic, overlap, halowidth):
    device = _device(dev)
    dt = getattr(torch, dtype)
    per, o, w = int(periodic), int(overlap), int(halowidth)
    me, dims, nprocs, coords, comm = igg.init_global_grid(
        *N, dimx=int(dimx), dimy=int(dimy), dimz=int(dimz), periodx=per & 1, periody=(per >> 1) & 1,
        periodz=(per >> 2) & 1, overlapx=o, overlapy=o, overlapz=o, halowidthx=w, halowidthy=w, halowidthz=w,
        quiet=True, select_device=False, device_type="none" if dev == "cpu" else "AMDGPU")
    gg = igg.get_global_grid()
    last = nprocs - 1
    other = torch.float32 if dt == torch.float64 else torch.float64
    for shape in (N, (N[0] + 1, N[1], N[2]), (N[0], N[1] - 1, N[2])):  # the grid's size, two staggered ones
        ext = _extents(gg, shape)
        Fg = _global_array(ext)
        kw = dict(me=me, gg=gg, shape=shape, Fg=Fg, ext=ext, dtype=dt, device=device)
        # first, a box that misses ranks: they receive nothing, yet must not leave the others waiting
        _check(**kw, box=((2, 4), None, (ext[2] - 2, ext[2])), tag="box that misses ranks")
        _check(**kw, tag="whole")
        _check(**kw, box=(N[0] - o, None, None), tag="x-plane two ranks hold")
        _check(**kw, gdtype=other, root=last, tag="converted whole, last root")
        _check(**kw, box=(N[0] - o, None, None), gdtype=other, tag="converted plane")
        if dev != "cpu":
            _check(**kw, cpu_src=True, tag="A_global on the CPU")
    # the other conversion, another same-dtype path, and fields of fewer dimensions
    ext = _extents(gg, N)
    Fg = _global_array(ext)
    _check(me, gg, N, Fg, ext, other, device, gdtype=dt, tag="the other conversion")
    _check(me, gg, N, Fg, ext, torch.int32, device, root=last, tag="int32, last root")
    for shape in (N[:2], N[:1]):
        ext = _extents(gg, shape)
        Fg2 = _global_array(ext)
        _check(me, gg, shape, Fg2, ext, dt, device, tag="low-dimensional")
        _check(me, gg, shape, Fg2, ext, dt, device, box=((1, ext[0] - 1),) + (None,) * (len(shape) - 1), root=last,
               gdtype=other, tag="low-dimensional box")
    igg.finalize_global_grid()
    print(f"rank {me} scatter_g OK")


if __name__ == "__main__":
    name, *args = sys.argv[1:]
    globals()[f"scenario_{name}"](*args)
