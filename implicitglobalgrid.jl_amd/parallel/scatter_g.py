"""``scatter_g`` - distribute a GLOBAL field, or a box of it, from a root rank
into the local fields of every rank: the inverse of ``gather_g``.

Every local cell of a field has a global index (``indices_g``); ``scatter_g``
gives each local cell whose index lies in the box the global cell of that
index - halo and overlap cells included, on one rank or on several. The
receive plane of a rank and the send plane of its neighbour have the same
global index, for every overlap and staggering, so a field scattered whole is
halo-consistent: ``update_halo_`` changes no bit of it.

The plan (``scatter_pieces``) is a pure function of the grid parameters and a
rank's Cartesian coordinates, like ``selection_pieces``: the root plans every
receiver, each receiver plans itself. GPU path: the root packs the pieces of
all other ranks into one staging buffer (one batched ``copy3d`` launch, or the
converting kernel where a float64 global array feeds float32 fields), one
``Transport.exchange`` phase carries one message per receiving rank, and each
receiver places its message with one batched launch (``copy3d``, or the
widening kernel of csrc/kernels/select_kernels.hip where a float32 global
array feeds float64 fields - half the bytes travel); the root's own pieces go
straight from ``A_global`` into ``A``.
"""
from __future__ import annotations

import itertools

import torch

from .._native import IGGError, native
from . import grid as _grid
from .gather_g import (_buffer, _check_field, _dense_strides, _device_transport, _global_box, _numel, _pad3,
                       _sel_shape, normalize_selection)

__all__ = ["scatter_pieces", "scatter_g"]

_WIRE = {torch.float32: 0, torch.float64: 1}  # what travels for a float64 field (told by the root)


# ------------------------------------------------------------------ the plan
def _runs(n: int, o: int, D: int, per: int, c: int, m: int) -> list:
    """The local range ``[0, m)`` of one dimension as maximal runs ``(i0, len,
    g0)``: local indices ``i0 .. i0 + len - 1`` have the global indices ``g0,
    g0 + 1, ...``. One run without periodicity; a periodic wrap ends a run, so
    a local range longer than the period has three or more."""
    if not per:
        return [(0, m, c * (n - o))]
    ng = D * (n - o)
    out, i = [], 0
    g = (c * (n - o) - 1 + (n - m) // 2) % ng  # indices_g at i = 0
    while i < m:
        ln = min(ng - g, m - i)
        out.append((i, ln, g))
        i, g = i + ln, 0
    return out


def scatter_pieces(nxyz, overlaps, dims, periods, coords, shape, box=None) -> list:
    """What the rank at ``coords`` receives of the global box ``box``, as
    ``(dst_start, count, src_start)`` triples of 3-tuples: local cell
    ``dst_start + k`` receives cell ``src_start + k`` of ``A_global``, ``k <
    count`` per dimension; ``A_global`` is indexed relative to the box's lower
    corner (dimensions the field does not have: start 0, count 1). A pure
    function of its arguments - callable for any rank without communication.

    Every local cell whose global index (``indices_g``) lies in the box is
    covered exactly once, halo and overlap cells included; cells outside the
    box are in no piece. Per dimension the local range is cut where the
    global index wraps, so a periodic dimension gives two runs, or more where
    the local size exceeds the period (``n=9, o=4, D=1``: three) - the number
    of pieces has no fixed bound. The copies of a 1-D or 2-D field on ranks
    that differ only in a dimension the field does not have all receive."""
    nd = len(shape)
    sel = normalize_selection(nxyz, overlaps, dims, periods, shape, box, 1, who="scatter_g")
    per_dim = []
    for d in range(nd):
        lo, hi, _s = sel[d]
        parts = []
        for i0, ln, g0 in _runs(int(nxyz[d]), int(overlaps[d]), int(dims[d]), int(periods[d]), int(coords[d]),
                                int(shape[d])):
            a, b = max(g0, lo), min(g0 + ln, hi)
            if b > a:
                parts.append((i0 + (a - g0), b - a, a - lo))
        per_dim.append(parts)
    pad = [[(0, 1, 0)]] * (3 - nd)
    out = []
    for combo in itertools.product(*per_dim, *pad):
        out.append((tuple(p[0] for p in combo), tuple(p[1] for p in combo), tuple(p[2] for p in combo)))
    return out


# ----------------------------------------------------------------- scatter_g
def _launch(kind: str, jobs, eb: int, stream) -> None:
    """One batched launch: ``jobs`` are (src address, dst address, count, src
    strides, dst strides), strides in elements. ``copy``: the byte mover for
    elements of ``eb`` bytes; ``narrow``: f64 -> f32; ``widen``: f32 -> f64."""
    if not jobs:
        return
    if kind == "copy":
        native.copy3d([list(c) + list(ss) + list(ds) for _s, _d, c, ss, ds in jobs],
                      [(s, d) for s, d, _c, _ss, _ds in jobs], eb, True, stream)
    else:
        fn = native.select_convert if kind == "narrow" else native.select_widen
        fn([(s, d, list(c), list(ss), list(ds)) for s, d, c, ss, ds in jobs], stream)


def _local_box(A, start, cnt, nd) -> torch.Tensor:
    return A[tuple(slice(start[d], start[d] + cnt[d]) for d in range(nd))]


def scatter_g(A_global: torch.Tensor | None, A: torch.Tensor, *, root: int = 0, box=None) -> None:
    """Fill the local fields ``A`` of all ranks from the global field
    ``A_global`` - or a box of it - held by rank ``root``. Collective; the
    inverse of ``gather_g``.

    Every local cell of ``A`` whose global index (``indices_g``) lies in the
    box receives the global cell of that index, halo and overlap cells
    included, on every rank that holds such a cell; the other cells are not
    touched. After a scatter of the whole field ``A`` is halo-consistent:
    ``update_halo_(A)`` changes no bit, so no exchange is needed afterwards.
    ``box`` is as in ``gather_g`` - per dimension ``None``, an int ``g`` (the
    plane ``[g, g + 1)``) or ``(lo, hi)`` - and names the range of global
    indices that ``A_global`` covers; there is no ``step``.

    ``A``: 1 to 3 dimensions, any dense layout, CPU or GPU. ``A_global`` is
    ``None`` off the root; on the root a contiguous tensor of shape
    ``selection_shape_g(A, box)``, on ``A``'s device or on the CPU (for a GPU
    field a CPU ``A_global`` is first copied to the device, whole). Its dtype
    is that of ``A``, or ``float32`` for a ``float64`` field (float32 travels
    and is widened at the receivers, exact), or ``float64`` for a ``float32``
    field (narrowed by the root's pack, round to nearest even, so float32
    travels); anything else is refused. For a float64 field the root tells
    the other ranks which of the two travels (one small host broadcast).

    GPU fields: the root packs the pieces of all other ranks into one staging
    buffer - about one copy of the selected global field -, one exchange phase
    (RCCL; host-staged where ranks share a GPU) carries one message per
    receiving rank, and each receiver places its message with one launch, all
    on the current stream without a host synchronisation of their own; the
    call cannot be captured in a hipGraph. A rank none of whose cells lies in
    the box receives nothing. The staging buffers are ``gather_g``'s: they
    grow only and are freed by ``free_gather_buffer()`` and
    ``finalize_global_grid``. Every argument error is raised before anything
    is written or sent."""
    gg = _grid.global_grid()
    _check_field(A)
    nd = A.dim()
    sel = normalize_selection(gg.nxyz, gg.overlaps, gg.dims, gg.periods, A.shape, box, 1, who="scatter_g")
    nprocs, me = int(gg.nprocs), int(gg.me)
    root = int(root)
    if not 0 <= root < nprocs:
        raise IGGError(f"scatter_g: root {root} out of range 0..{nprocs - 1}.")
    src_shape = _sel_shape(sel)
    wire = A.dtype  # what travels
    if me == root:
        if A_global is None:
            raise IGGError("scatter_g: A_global can't be None on the root.")
        if not isinstance(A_global, torch.Tensor) or tuple(A_global.shape) != src_shape:
            raise IGGError(f"scatter_g: A_global must have shape {src_shape} "
                           f"(got {tuple(A_global.shape) if isinstance(A_global, torch.Tensor) else A_global!r}).")
        pair = (A_global.dtype, A.dtype)
        if pair[0] != pair[1] and pair not in ((torch.float32, torch.float64), (torch.float64, torch.float32)):
            raise IGGError(f"scatter_g: A_global must have the field's dtype {A.dtype}, or be float32 for a float64 "
                           f"field or float64 for a float32 field (got {A_global.dtype}).")
        if not A_global.is_contiguous():
            raise IGGError("scatter_g: A_global must be a contiguous tensor.")
        if A_global.device != A.device and A_global.device.type != "cpu":
            raise IGGError(f"scatter_g: A_global must be on the field's device or on the CPU (got {A_global.device}).")
        if pair[1] == torch.float64:
            wire = pair[0]
    device = bool(A.is_cuda)
    if device and torch.cuda.is_current_stream_capturing():
        raise IGGError("scatter_g cannot be captured in a hipGraph (it sizes buffers and may stage through the host).")
    if A.dtype == torch.float64 and nprocs > 1:
        # float64 or float32 may travel for a float64 field: only the root knows which
        code = torch.tensor([_WIRE[wire] if me == root else -1], dtype=torch.int32)
        gg.comm.bcast_(code, root)
        wire = torch.float64 if int(code.item()) == _WIRE[torch.float64] else torch.float32
    wb = torch.empty(0, dtype=wire).element_size()
    eb = A.element_size()
    place_kind = "widen" if wire != A.dtype else "copy"
    astr = _pad3(A.stride(), 0)
    dims = [int(d) for d in gg.dims]

    def pieces_of(rank: int) -> list:
        coords = native.cart_coords(rank, dims)
        return scatter_pieces(gg.nxyz, gg.overlaps, gg.dims, gg.periods, coords, A.shape, box)

    def dst_addr(start) -> int:
        return A.data_ptr() + eb * sum(start[d] * astr[d] for d in range(3))

    stream = torch.cuda.current_stream().cuda_stream if device else 0
    mine = scatter_pieces(gg.nxyz, gg.overlaps, gg.dims, gg.periods, gg.coords, A.shape, box)
    tr = None
    if nprocs > 1:
        # (creating the device transport is collective: every rank asks for it, also one that receives nothing)
        tr = _device_transport(gg.comm) if device else gg.comm.host_transport()

    if me != root:
        nbytes = sum(_numel(cnt) for _d, cnt, _s in mine) * wb
        if nbytes == 0:
            return  # none of its cells lies in the box: takes no part
        buf = _buffer("recv" if device else "host", nbytes, A.device)
        tr.exchange([(buf.data_ptr(), nbytes, root, 0)], [], device, stream)
        off, jobs = 0, []
        for dstart, cnt, _s in mine:  # piece after piece, each C-contiguous
            if device:
                jobs.append((buf.data_ptr() + off, dst_addr(dstart), cnt, _dense_strides(cnt), astr))
            else:
                flat = buf[off:off + _numel(cnt) * wb].view(wire)
                _local_box(A, dstart, cnt, nd).copy_(flat.view(cnt[:nd]))
            off += _numel(cnt) * wb
        _launch(place_kind, jobs, eb, stream)
        return

    # ---- the root
    src = A_global if A_global.device == A.device else A_global.to(A.device)
    gb = src.element_size()
    gstr = _pad3(src.stride(), 0)
    pack_kind = "narrow" if src.dtype != wire else "copy"

    def src_addr(sstart) -> int:
        return src.data_ptr() + gb * sum(sstart[d] * gstr[d] for d in range(3))

    sends, pack, total = [], [], 0
    for p in range(nprocs):
        if p == me:
            continue
        pcs = pieces_of(p)
        nb = sum(_numel(cnt) for _d, cnt, _s in pcs) * wb
        if nb == 0:
            continue
        sends.append((total, nb, p, 0))
        off = total
        for _dstart, cnt, sstart in pcs:
            pack.append((off, cnt, sstart))
            off += _numel(cnt) * wb
        total += nb
    if sends:
        sbuf = _buffer("send" if device else "host", total, A.device)
        if device:
            _launch(pack_kind, [(src_addr(s), sbuf.data_ptr() + o, cnt, gstr, _dense_strides(cnt))
                                for o, cnt, s in pack], gb, stream)
        else:
            for o, cnt, s in pack:
                sbuf[o:o + _numel(cnt) * wb].view(wire).view(cnt[:nd]).copy_(_global_box(src, s, cnt, nd))
        tr.exchange([], [(sbuf.data_ptr() + o, nb, p, t) for o, nb, p, t in sends], device, stream)
    # the root's own pieces: straight from the global array into the field
    if mine:
        if device:
            kind = "copy" if src.dtype == A.dtype else "widen" if A.dtype == torch.float64 else "narrow"
            _launch(kind, [(src_addr(s), dst_addr(d), cnt, gstr, astr) for d, cnt, s in mine], eb, stream)
        else:
            for d, cnt, s in mine:
                _local_box(A, d, cnt, nd).copy_(_global_box(src, s, cnt, nd))
