"""``gather_g`` - assemble the true GLOBAL field on a root rank: whole, a box
of it, or every ``step``-th cell.

``gather_`` (the reference's ``gather!``) concatenates equal local blocks into
a ``dims*size`` array; overlap cells appear twice and it is left to the user to
make a global field of that. ``gather_g`` moves OWNED cells only
(``owned_ranges``: the owned boxes tile the global index range and hold no
plane ``update_halo_`` writes), so every global cell arrives exactly once,
whatever the overlap, periodicity or staggering, no ``update_halo_`` or
``sync_halo()`` is needed first, and only the selected cells travel.

The plan (``selection_pieces``) is a pure function of the grid parameters and
a rank's Cartesian coordinates: the root plans every sender itself, nothing is
negotiated. GPU path: a sender packs its pieces into a compact staging buffer
(one batched ``copy3d`` launch, or the converting kernel of
csrc/kernels/select_kernels.hip for float64 -> float32, so half the bytes
travel), one ``Transport.exchange`` phase brings them to the root, which
places them into ``A_global`` with one batched ``copy3d`` launch; the root's
own pieces go straight from the field into ``A_global``.
"""
from __future__ import annotations

import itertools

import torch

from .._native import IGGError, native
from ..utils import config
from . import grid as _grid

__all__ = ["indices_g", "selection_shape_g", "selection_pieces", "gather_g"]

_bufs: dict = {}  # grow-only staging buffers: "send" / "recv" (device), "host"


def free_buffers() -> None:
    """Drop the staging buffers (``free_gather_buffer`` / ``finalize_global_grid``)."""
    _bufs.clear()


def _buffer(key: str, nbytes: int, device) -> torch.Tensor:
    b = _bufs.get(key)
    if b is None or b.numel() < nbytes or b.device != device:
        _bufs.pop(key, None)
        b = _bufs[key] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
    return b


# ------------------------------------------------------------------ the plan
def _field_overlap(n: int, o: int, m: int) -> int:
    return max(o + m - n, 0)


def _extent(n: int, o: int, D: int, per: int, m: int) -> int:
    """Global extent of a field of local size ``m`` in one dimension."""
    return D * (n - o) if per else D * (n - o) + o + (m - n)


def _global_index(n: int, o: int, D: int, per: int, c: int, m: int, i: int) -> int:
    if per:
        return (c * (n - o) + i - 1 + (n - m) // 2) % (D * (n - o))
    return c * (n - o) + i


def _owned(n: int, o: int, D: int, per: int, c: int, m: int) -> tuple:
    """``owned_ranges`` of one dimension, from the parameters alone."""
    of = _field_overlap(n, o, m)
    lo = of // 2
    a, b = lo, m - (of - lo)
    if not per:
        if c == 0:
            a = 0
        if c == D - 1:
            b = m
    return a, b


def _segments(n: int, o: int, D: int, per: int, c: int, m: int) -> list:
    """The owned range of one dimension as ``(g0, g1, i0)``: global indices
    ``[g0, g1)`` sit at local indices ``i0, i0 + 1, ...``. One segment, or two
    where a periodic rank's owned range wraps past the global extent."""
    a, b = _owned(n, o, D, per, c, m)
    if b <= a:
        return []
    g0 = _global_index(n, o, D, per, c, m, a)
    if not per:
        return [(g0, g0 + (b - a), a)]
    ng = D * (n - o)
    if g0 + (b - a) <= ng:
        return [(g0, g0 + (b - a), a)]
    return [(g0, ng, a), (0, g0 + (b - a) - ng, a + (ng - g0))]


def normalize_selection(nxyz, overlaps, dims, periods, shape, box=None, step=1, who="gather_g") -> list:
    """``[(lo, hi, step)]`` per dimension of ``shape`` from ``box`` (per
    dimension ``None``, an int ``g`` meaning ``[g, g + 1)``, or ``(lo, hi)``)
    and ``step`` (an int or one per dimension); raises ``IGGError`` on a wrong
    length, ``step < 1`` or an empty or out-of-range box, in the name of
    ``who``."""
    nd = len(shape)
    if box is None:
        box = (None,) * nd
    if not isinstance(box, (tuple, list)) or len(box) != nd:
        raise IGGError(f"{who}: `box` needs one entry per dimension of the field ({nd}).")
    if not isinstance(step, (tuple, list)):
        step = (step,) * nd
    if len(step) != nd:
        raise IGGError(f"{who}: `step` needs one entry per dimension of the field ({nd}).")
    sel = []
    for d in range(nd):
        ext = _extent(int(nxyz[d]), int(overlaps[d]), int(dims[d]), int(periods[d]), int(shape[d]))
        s = step[d]
        if not isinstance(s, int) or isinstance(s, bool) or s < 1:
            raise IGGError(f"{who}: `step` must be an integer >= 1 (got {s!r} in dimension {d}).")
        b = box[d]
        if b is None:
            lo, hi = 0, ext
        elif isinstance(b, int) and not isinstance(b, bool):
            lo, hi = b, b + 1
        else:
            try:
                lo, hi = (int(v) for v in b)
            except (TypeError, ValueError):
                raise IGGError(f"{who}: `box` entry {b!r} is not None, an int or a (lo, hi) pair.") from None
        if lo < 0 or hi > ext or lo >= hi:
            raise IGGError(f"{who}: box [{lo}, {hi}) of dimension {d} is empty or outside of [0, {ext}).")
        sel.append((lo, hi, s))
    return sel


def _sel_shape(sel) -> tuple:
    return tuple(-(-(hi - lo) // s) for lo, hi, s in sel)


def selection_pieces(nxyz, overlaps, dims, periods, coords, shape, box=None, step=1) -> list:
    """The pieces of a global selection that the rank at ``coords`` owns, as
    ``(src_start, count, dst_start)`` triples of 3-tuples: output cell
    ``dst_start + k`` holds the rank's local cell ``src_start + k*step``,
    ``k < count`` per dimension (dimensions the field does not have: start 0,
    count 1). A pure function of its arguments - callable for any rank without
    communication. Up to two segments per periodic dimension (the last rank's
    owned range can wrap past the global extent), hence up to 8 pieces; a rank
    whose owned box misses the selection has none, and of the ranks that hold
    copies of a 1-D or 2-D field only those at coordinate 0 of the dimensions
    the field does not have contribute."""
    nd = len(shape)
    sel = normalize_selection(nxyz, overlaps, dims, periods, shape, box, step)
    if any(int(coords[d]) != 0 for d in range(nd, 3)):
        return []
    per_dim = []
    for d in range(nd):
        lo, hi, s = sel[d]
        parts = []
        for g0, g1, i0 in _segments(int(nxyz[d]), int(overlaps[d]), int(dims[d]), int(periods[d]), int(coords[d]),
                                    int(shape[d])):
            k0 = -(-(max(g0, lo) - lo) // s)
            k1 = -(-(min(g1, hi) - lo) // s)
            if k1 > k0:
                parts.append((i0 + (lo + k0 * s - g0), k1 - k0, k0))
        per_dim.append(parts)
    pad = [[(0, 1, 0)]] * (3 - nd)
    out = []
    for combo in itertools.product(*per_dim, *pad):
        out.append((tuple(p[0] for p in combo), tuple(p[1] for p in combo), tuple(p[2] for p in combo)))
    return out


# ---------------------------------------------------------------- public, small
def _check_field(A) -> None:
    if not isinstance(A, torch.Tensor) or A.dim() < 1 or A.dim() > 3:
        raise IGGError(f"Fields must have 1 to 3 dimensions (got {A.dim() if isinstance(A, torch.Tensor) else A!r}).")


def indices_g(dim0: int, A: torch.Tensor) -> torch.Tensor:
    """Global index of every local index of axis ``dim0`` (0-based) of ``A``:
    an int64 1-D CPU tensor, the integer counterpart of ``coords_g``.

    With ``n = nxyz[d]``, the grid's overlap ``o``, ``m = A.shape[d]``, this
    rank's coordinate ``c`` and ``D = dims[d]``: ``g = c*(n-o) + i`` in a
    non-periodic dimension (global extent ``D*(n-o) + o + (m-n)``, which is
    ``nx_g(A)``), and ``g = (c*(n-o) + i - 1 + (n-m)//2) mod D*(n-o)`` in a
    periodic one: ``floor(x_g/dx)``, the global array is ordered by the
    coordinate ``x_g`` returns after its wrap. The periodic global extent is
    ``D*(n-o)`` for every ``m`` - for a staggered field that is NOT
    ``nx_g(A)``. Over the owned cells of all ranks every global index occurs
    exactly once."""
    gg = _grid.global_grid()
    _check_field(A)
    if not 0 <= dim0 < A.dim():
        raise IGGError(f"indices_g: the field has no axis {dim0}.")
    n, o, D, per = int(gg.nxyz[dim0]), int(gg.overlaps[dim0]), int(gg.dims[dim0]), int(gg.periods[dim0])
    c, m = int(gg.coords[dim0]), int(A.shape[dim0])
    g = c * (n - o) + torch.arange(m, dtype=torch.int64)
    if per:
        g = (g - 1 + (n - m) // 2) % (D * (n - o))
    return g


def selection_shape_g(A: torch.Tensor, box=None, step=1) -> tuple:
    """Shape of the ``A_global`` that ``gather_g(A, A_global, box=box,
    step=step)`` fills (no collective): per dimension of ``A`` the number of
    selected global indices ``lo, lo + step, ... < hi``."""
    gg = _grid.global_grid()
    _check_field(A)
    return _sel_shape(normalize_selection(gg.nxyz, gg.overlaps, gg.dims, gg.periods, A.shape, box, step))


# ----------------------------------------------------------------- gather_g
def _pad3(v, fill) -> list:
    return list(v) + [fill] * (3 - len(v))


def _dense_strides(count) -> list:
    return [count[1] * count[2], count[2], 1]


def _numel(count) -> int:
    return count[0] * count[1] * count[2]


def _device_transport(comm):
    """The grid's device transport for one exchange phase: RCCL, or the
    host-staged transport where ranks share a GPU (RCCL refuses duplicate
    devices) or ``IGG_TRANSPORT=staged`` - the rule of ``update_halo_`` and
    ``reduce_g``. Collective on first use, remembered per communicator."""
    staged = getattr(comm, "_gather_g_staged", None)
    if staged is None:
        from .transport_select import _shared_device

        staged = comm._gather_g_staged = bool(_shared_device(comm)) or config.transport_choice() == "staged"
    return comm.device_transport("staged" if staged else "rccl")


def _move(A, jobs, convert, stream) -> None:
    """One batched launch over the GPU field ``A``: ``jobs`` are (element
    offset of the first source cell, count, src strides, dst address, dst
    strides). The byte mover for the same dtype, the converting kernel else."""
    eb = A.element_size()
    if convert:
        native.select_convert([(A.data_ptr() + eb * off, dp, list(cnt), list(ss), list(ds))
                               for off, cnt, ss, dp, ds in jobs], stream)
    else:
        native.copy3d([list(cnt) + list(ss) + list(ds) for _o, cnt, ss, _p, ds in jobs],
                      [(A.data_ptr() + eb * off, dp) for off, _c, _s, dp, _d in jobs], eb, True, stream)


def gather_g(A: torch.Tensor, A_global: torch.Tensor | None, *, root: int = 0, box=None, step=1,
             dtype=None) -> None:
    """Assemble the global field of ``A`` - or the selected part of it - in
    ``A_global`` on rank ``root``. Collective.

    A selection is, per dimension of ``A``, a half-open range ``[lo, hi)`` of
    global indices (``indices_g``) and a step ``s >= 1``: output index ``k``
    holds global index ``lo + k*s``. ``box`` takes per dimension ``None``
    (everything), an int ``g`` (the plane ``[g, g + 1)``: the axis stays, with
    length 1) or a pair ``(lo, hi)``; ``step`` is an int or one per dimension.
    Ranges lie inside ``[0, extent)``: no wrap-around, no negative indices.

    ``A``: 1 to 3 dimensions, any dense layout, CPU or GPU. ``A_global`` is
    ``None`` off the root; on the root a contiguous tensor of shape
    ``selection_shape_g(A, box, step)`` and the output dtype, on ``A``'s
    device or on the CPU. ``dtype``: ``None`` (that of ``A``) or
    ``torch.float32`` for a float64 field - converted at the sender (round to
    nearest even), so half the bytes travel.

    Only owned cells are read (``owned_ranges``): no ``update_halo_`` or
    ``sync_halo()`` is needed first, and the result is the same before and
    after an exchange. A rank that owns nothing of the selection sends
    nothing. GPU fields: pack, one exchange phase (RCCL; host-staged where
    ranks share a GPU) and placement run on the current stream without a host
    synchronisation of their own; the call cannot be captured in a hipGraph.
    The staging buffers grow only and are freed by ``free_gather_buffer()``
    and ``finalize_global_grid``."""
    gg = _grid.global_grid()
    _check_field(A)
    nd = A.dim()
    sel = normalize_selection(gg.nxyz, gg.overlaps, gg.dims, gg.periods, A.shape, box, step)
    if dtype is None or dtype == A.dtype:
        out_dtype = A.dtype
    elif dtype == torch.float32 and A.dtype == torch.float64:
        out_dtype = torch.float32
    else:
        raise IGGError(f"gather_g: dtype must be None or torch.float32 for a float64 field (got {dtype} for {A.dtype}).")
    convert = out_dtype != A.dtype
    nprocs, me = int(gg.nprocs), int(gg.me)
    root = int(root)
    if not 0 <= root < nprocs:
        raise IGGError(f"gather_g: root {root} out of range 0..{nprocs - 1}.")
    out_shape = _sel_shape(sel)
    if me == root:
        if A_global is None:
            raise IGGError("gather_g: A_global can't be None on the root.")
        if not isinstance(A_global, torch.Tensor) or tuple(A_global.shape) != out_shape:
            raise IGGError(f"gather_g: A_global must have shape {out_shape} "
                           f"(got {tuple(A_global.shape) if isinstance(A_global, torch.Tensor) else A_global!r}).")
        if A_global.dtype != out_dtype:
            raise IGGError(f"gather_g: A_global must have dtype {out_dtype} (got {A_global.dtype}).")
        if not A_global.is_contiguous():
            raise IGGError("gather_g: A_global must be a contiguous tensor.")
    device = bool(A.is_cuda)
    if device and torch.cuda.is_current_stream_capturing():
        raise IGGError("gather_g cannot be captured in a hipGraph (it sizes buffers and may stage through the host).")
    steps = _pad3([s for _lo, _hi, s in sel], 1)
    astr = _pad3(A.stride(), 0)
    src_strides = [astr[d] * steps[d] for d in range(3)]
    dims = [int(d) for d in gg.dims]

    def pieces_of(rank: int) -> list:
        coords = native.cart_coords(rank, dims)
        return selection_pieces(gg.nxyz, gg.overlaps, gg.dims, gg.periods, coords, A.shape, box, step)

    def src_offset(start) -> int:
        return sum(start[d] * astr[d] for d in range(3))

    stream = torch.cuda.current_stream().cuda_stream if device else 0
    ob = torch.empty(0, dtype=out_dtype).element_size()
    mine = selection_pieces(gg.nxyz, gg.overlaps, gg.dims, gg.periods, gg.coords, A.shape, box, step)
    tr = None
    if nprocs > 1:
        # (creating the device transport is collective: every rank asks for it, also one that sends nothing)
        tr = _device_transport(gg.comm) if device else gg.comm.host_transport()

    if me != root:
        nbytes = sum(_numel(cnt) for _s, cnt, _d in mine) * ob
        if nbytes == 0:
            return  # owns nothing of the selection: takes no part
        buf = _buffer("send" if device else "host", nbytes, A.device)
        if device:
            jobs, off = [], 0
            for start, cnt, _dst in mine:  # piece after piece, each C-contiguous
                jobs.append((src_offset(start), cnt, src_strides, buf.data_ptr() + off, _dense_strides(cnt)))
                off += _numel(cnt) * ob
            _move(A, jobs, convert, stream)
        else:
            _host_pack(A, mine, steps, buf, out_dtype)
        tr.exchange([], [(buf.data_ptr(), nbytes, root, 0)], device, stream)
        return

    # ---- the root
    direct = A_global.device == A.device
    dst = A_global if direct else torch.empty(out_shape, dtype=out_dtype, device=A.device)
    gstr = _pad3(dst.stride(), 0)

    def dst_addr(dstart) -> int:
        return dst.data_ptr() + ob * sum(dstart[d] * gstr[d] for d in range(3))

    recvs, place, total = [], [], 0
    for p in range(nprocs):
        if p == me:
            continue
        pcs = pieces_of(p)
        nb = sum(_numel(cnt) for _s, cnt, _d in pcs) * ob
        if nb == 0:
            continue
        recvs.append((total, nb, p, 0))
        off = total
        for _start, cnt, dstart in pcs:
            place.append((off, cnt, dstart))
            off += _numel(cnt) * ob
        total += nb
    rbuf = _buffer("recv" if device else "host", total, A.device) if total else None
    # the root's own pieces: straight from the field into their boxes of the global array
    if mine:
        if device:
            _move(A, [(src_offset(s), cnt, src_strides, dst_addr(d), gstr) for s, cnt, d in mine], convert, stream)
        else:
            for s, cnt, d in mine:
                _global_box(dst, d, cnt, nd).copy_(_local_lattice(A, s, cnt, steps, nd))
    if recvs:
        tr.exchange([(rbuf.data_ptr() + o, nb, p, t) for o, nb, p, t in recvs], [], device, stream)
        if device:
            native.copy3d([list(cnt) + _dense_strides(cnt) + gstr for _o, cnt, _d in place],
                          [(rbuf.data_ptr() + o, dst_addr(d)) for o, _c, d in place], ob, True, stream)
        else:
            for o, cnt, d in place:
                flat = rbuf[o:o + _numel(cnt) * ob].view(out_dtype)
                _global_box(dst, d, cnt, nd).copy_(flat.view(cnt[:nd]))
    if not direct:
        A_global.copy_(dst)


def _local_lattice(A, start, cnt, steps, nd) -> torch.Tensor:
    return A[tuple(slice(start[d], start[d] + (cnt[d] - 1) * steps[d] + 1, steps[d]) for d in range(nd))]


def _global_box(G, dstart, cnt, nd) -> torch.Tensor:
    return G[tuple(slice(dstart[d], dstart[d] + cnt[d]) for d in range(nd))]


def _host_pack(A, pieces, steps, buf, out_dtype) -> None:
    """CPU sender: the pieces, each C-contiguous, one after the other."""
    nd, off = A.dim(), 0
    ob = torch.empty(0, dtype=out_dtype).element_size()
    for start, cnt, _dst in pieces:
        n = _numel(cnt)
        buf[off:off + n * ob].view(out_dtype).view(cnt[:nd]).copy_(_local_lattice(A, start, cnt, steps, nd))
        off += n * ob
