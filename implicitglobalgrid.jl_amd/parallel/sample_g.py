"""``sample_g`` - a field's values at arbitrary points of the GLOBAL grid, and
``Recorder``, time series of them without a collective per step.

A point is a position ``u`` in the global index space of the field: the
0-based, fractional form of ``indices_g`` (``index_g`` converts a physical
coordinate). The value there is the multilinear interpolation of the ``2^nd``
cells around it. **A point belongs to the rank that owns the lower corner of
its cell** (``sample_owner``); with a field overlap of at least 1 that rank
holds the upper corner in every dimension too, at local index ``i + 1``. So
exactly one rank interpolates a point, every other rank writes the bit
pattern 0, and one integer sum over the ranks hands every rank the owner's 64
bits. The weights come from the global coordinate and the corner values are
the same bits on every rank that holds them after an exchange: the result
does not depend on the decomposition, bit for bit.

GPU float32/float64 fields take the HIP kernel (csrc/kernels/
sample_kernels.hip: one launch for all fields, no workspace, no host
synchronisation, capturable); CPU tensors take ``native.host_sample``, the
same expressions on the host.
"""
from __future__ import annotations

import torch

from .._native import IGGError, native
from . import grid as _grid
from .gather_g import _extent, _segments

__all__ = ["sample_g", "sample_owner", "index_g", "Recorder"]


def sample_owner(nxyz, overlaps, dims, periods, coords, shape, g):
    """The local lower-corner index tuple of the cell whose lower corner is
    the global index tuple ``g`` if the rank at ``coords`` owns it, else
    ``None``. A pure function of the grid parameters (as ``selection_pieces``).

    Per dimension of the field: ``g_d`` lies in one of the rank's owned
    segments ``(g0, g1, i0)`` and the local index is ``i0 + (g_d - g0)``; the
    upper corner is local ``i + 1``. Of the ranks that hold copies of a 1-D or
    2-D field only those at coordinate 0 of the missing dimensions own
    anything. Raises ``IGGError`` where the field's overlap is below 1 in a
    dimension that is periodic or has more than one rank: there the owner of a
    cell does not hold its upper corner."""
    nd = len(shape)
    if len(g) != nd:
        raise IGGError(f"sample_owner: `g` needs one index per dimension of the field ({nd}).")
    _check_overlap(nxyz, overlaps, dims, periods, shape, "sample_owner")
    if any(int(coords[d]) != 0 for d in range(nd, 3)):
        return None
    out = []
    for d in range(nd):
        for g0, g1, i0 in _segments(int(nxyz[d]), int(overlaps[d]), int(dims[d]), int(periods[d]), int(coords[d]),
                                    int(shape[d])):
            if g0 <= int(g[d]) < g1:
                out.append(i0 + (int(g[d]) - g0))
                break
        else:
            return None
    return tuple(out)


def _check_overlap(nxyz, overlaps, dims, periods, shape, who) -> None:
    for d in range(len(shape)):
        of = int(overlaps[d]) + int(shape[d]) - int(nxyz[d])
        if of < 1 and (int(periods[d]) or int(dims[d]) > 1):
            raise IGGError(f"{who}: the field's overlap in dimension {d} is {of}; at least 1 is needed where the "
                           "dimension is periodic or has more than one rank (the owner of a cell must hold its "
                           "upper corner).")


def index_g(dim0: int, x, d: float, A: torch.Tensor):
    """The position in the global index space of axis ``dim0`` (0-based) of
    ``A`` of the physical coordinate ``x`` (a float or a tensor), consistent
    with ``x_g`` / ``coords_g`` and ``indices_g``: ``x/d - 0.5*(n - m)`` in a
    non-periodic dimension, ``x/d - 0.5*((n - m) mod 2)`` in a periodic one
    (``n = nxyz[dim0]``, ``m = A.shape[dim0]``). For the coordinate of a cell
    it is that cell's global index."""
    gg = _grid.global_grid()
    if not isinstance(A, torch.Tensor) or not 0 <= dim0 < A.dim() or A.dim() > 3:
        raise IGGError(f"index_g: the field has no axis {dim0}.")
    n, m = int(gg.nxyz[dim0]), int(A.shape[dim0])
    shift = 0.5 * ((n - m) % 2) if int(gg.periods[dim0]) else 0.5 * (n - m)
    return x / d - shift


# ------------------------------------------------------------------ the plan
def _fields_of(fields, who) -> tuple:
    single = isinstance(fields, torch.Tensor)
    fs = (fields,) if single else tuple(fields) if isinstance(fields, (tuple, list)) else ()
    if not fs or not all(isinstance(A, torch.Tensor) for A in fs):
        raise IGGError(f"{who}: `fields` must be a tensor or a tuple of tensors.")
    A0 = fs[0]
    if A0.dim() < 1 or A0.dim() > 3:
        raise IGGError(f"Fields must have 1 to 3 dimensions (got {A0.dim()}).")
    if any(A.shape != A0.shape or A.dtype != A0.dtype or A.device != A0.device for A in fs):
        raise IGGError(f"{who}: the fields must share one shape, one dtype and one device.")
    if not A0.dtype.is_floating_point:
        raise IGGError(f"{who}: the fields must have a real floating dtype (got {A0.dtype}).")
    if A0.is_cuda and A0.dtype not in (torch.float32, torch.float64):
        raise IGGError(f"{who}: GPU fields must be float32 or float64 (got {A0.dtype}).")
    return single, fs


def _table(gg, shape, who) -> list:
    """Per dimension ``(E, periodic, m, segments)``: the kernel's table."""
    nd = len(shape)
    _check_overlap(gg.nxyz, gg.overlaps, gg.dims, gg.periods, shape, who)
    mine = all(int(gg.coords[d]) == 0 for d in range(nd, 3))
    table = []
    for d in range(nd):
        par = (int(gg.nxyz[d]), int(gg.overlaps[d]), int(gg.dims[d]), int(gg.periods[d]))
        E = _extent(*par, int(shape[d]))
        if E < 2:
            raise IGGError(f"{who}: the global extent of dimension {d} is {E}; at least 2 cells are needed.")
        segs = _segments(*par, int(gg.coords[d]), int(shape[d])) if mine else []
        table.append((E, par[3], int(shape[d]), [list(s) for s in segs]))
    return table


def _points(P, A0, who) -> tuple:
    """``(P, npts, stride of a point, stride of an axis)``."""
    nd = A0.dim()
    if not isinstance(P, torch.Tensor) or P.dtype != torch.float64 or P.device != A0.device:
        raise IGGError(f"{who}: `P` must be a float64 tensor on {A0.device}.")
    if P.dim() == 1 and nd == 1:
        return P, int(P.shape[0]), int(P.stride(0)), 0
    if P.dim() != 2 or int(P.shape[1]) != nd:
        raise IGGError(f"{who}: `P` must have shape (npts, {nd}) (got {tuple(P.shape)}).")
    return P, int(P.shape[0]), int(P.stride(0)), int(P.stride(1))


def _launch(fs, table, pts, dst, out_fs, me0, row=None, nrows=0, row_stride=0) -> None:
    """One sampling pass into ``dst`` (float64): the kernel, or the host form
    of it (other CPU dtypes as float64 copies)."""
    P, npts, ps0, ps1 = pts
    A0 = fs[0]
    if A0.is_cuda:
        native.sample(table, [(A.data_ptr(), list(A.stride())) for A in fs], A0.element_size(), P.data_ptr(), ps0,
                      ps1, npts, dst.data_ptr(), out_fs, me0, row.data_ptr() if row is not None else 0, nrows,
                      row_stride, torch.cuda.current_stream().cuda_stream)
    else:
        if A0.dtype not in (torch.float32, torch.float64):
            fs = [A.double() for A in fs]
        native.host_sample(table, [(A.data_ptr(), list(A.stride())) for A in fs], fs[0].element_size(), P.data_ptr(),
                           ps0, ps1, npts, dst.data_ptr(), out_fs, me0, row.data_ptr() if row is not None else 0,
                           nrows, row_stride)


def _combine(gg, res: torch.Tensor, who: str) -> None:
    """The integer sum over the ranks: one owner per point and 0 bits
    elsewhere, so the sum is the owner's bit pattern (a float sum would turn
    -0.0 into +0.0)."""
    from ..ops.reduce import _allreduce

    if int(gg.nprocs) == 1 or res.numel() == 0:
        return
    if res.is_cuda and torch.cuda.is_current_stream_capturing():
        staged = getattr(gg.comm, "_reduce_staged", None)
        if staged is None or staged:
            raise IGGError(f"{who} cannot be captured in a hipGraph where its collective stages through the host "
                           "(ranks sharing a GPU), nor before one eager call has chosen the transport.")
    _allreduce(gg.comm, res.view(torch.int64), "sum")


def sample_g(fields, P: torch.Tensor, *, out=None, local: bool = False) -> torch.Tensor:
    """The fields' values at the points ``P`` of the global grid, multilinearly
    interpolated, identical bits on every rank. Collective unless ``local``.

    ``fields``: one tensor or a tuple of tensors of one shape, dtype and
    device (strides may differ), 1-D to 3-D, any dense layout. ``P``: float64
    on the fields' device, shape ``(npts, nd)`` with any strides (a transposed
    ``(nd, npts)`` array is fine), or ``(npts,)`` for a 1-D field. A row is a
    point ``u`` in the global index space of the field - the fractional form
    of ``indices_g``, extents as ``selection_shape_g`` - see ``index_g``.
    Returns float64 ``(npts,)`` for one tensor, ``(nfields, npts)`` for a
    tuple; ``out=`` must be a contiguous float64 tensor of that shape on the
    fields' device. ``npts == 0`` is legal.

    Per dimension, all in float64 with separately rounded operations. Not
    periodic: valid iff ``0 <= u <= E-1``; ``g = min(floor(u), E-2)``,
    ``t = u - g``. Periodic: every finite ``u`` is valid; ``w = u -
    E*floor(u/E)``, folded into ``[0, E)``; ``g = min(floor(w), E-1)``,
    ``t = w - g``, the upper corner is ``(g+1) mod E``. ``lerp(a, b, t)`` is
    ``a`` if ``t == 0``, ``b`` if ``t == 1``, else ``(1-t)*a + t*b``: a corner
    of weight zero never reaches the result. Dimensions collapse in index
    order, the last axis first, whatever the memory layout. A point that is
    invalid in any dimension or has a non-finite coordinate yields the quiet
    NaN ``0x7FF8000000000000``, and so does every NaN result; nothing is
    raised for point values, which never come to the host.

    The rank that owns a point's lower corner (``sample_owner``) interpolates;
    every other rank writes 0 bits (the NaN of an invalid point comes from
    rank 0 alone, also under ``local=True``), and unless ``local=True`` one
    ``comm.allreduce_`` of the result as int64 on the current stream combines
    the ranks (none on a single rank; ranks that share a GPU stage through
    the host), reproducing the owner's bits: -0.0 and infinities included.

    Precondition, not checked: the cells next to the owned box hold what
    ``update_halo_`` gives them (call ``sync_halo()`` first on a fused model).
    Raises ``IGGError`` if the field's overlap is below 1 in a dimension that
    is periodic or has more than one rank, if a global extent is below 2, or
    on a wrong ``P``, mixed fields or a wrong ``out``. The call allocates no
    workspace and its plan depends on no point value: it can be captured in a
    hipGraph on one process and over RCCL (after one eager call), and ``P``
    may be rewritten between replays."""
    gg = _grid.global_grid()
    single, fs = _fields_of(fields, "sample_g")
    A0 = fs[0]
    pts = _points(P, A0, "sample_g")
    npts = pts[1]
    table = _table(gg, A0.shape, "sample_g")
    shape = (npts,) if single else (len(fs), npts)
    if out is not None:
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float64
                or out.device != A0.device or not out.is_contiguous()):
            raise IGGError(f"sample_g: `out` must be a contiguous float64 tensor of shape {shape} on {A0.device}.")
        res = out
    else:
        res = torch.empty(shape, dtype=torch.float64, device=A0.device)
    if npts:
        _launch(fs, table, pts, res, npts, int(gg.me) == 0)
    if not local:
        _combine(gg, res, "sample_g")
    return res


class Recorder:
    """Time series at fixed points without a collective per step (a
    seismogram): ``Recorder(fields_like, P, nrows)``.

    ``fields_like`` (a tensor or a tuple, as in ``sample_g``) fixes the shape,
    dtype, device and number of the fields, ``P`` the points. The recorder
    holds a zeroed device buffer ``(nrows, nfields, npts)`` and a device int64
    row counter. ``record(*fields)`` is one sampling launch that reads the
    counter on the device and writes this rank's partials (as ``local=True``)
    into that row - nothing if the counter has reached ``nrows`` - followed by
    one stream-ordered increment: no collective, no host synchronisation,
    capturable, and a replayed graph fills the next row. ``result()`` reads
    the count (the only host synchronisation), raises ``IGGError`` if more
    rows were recorded than fit, combines a copy of the written rows over the
    ranks once, as int64, and returns float64 ``(count, [nfields,] npts)``,
    identical on every rank; it can be called again. ``reset()`` zeroes the
    buffer and the counter. ``P`` is used as passed: rewriting it moves the
    receivers."""

    def __init__(self, fields_like, P: torch.Tensor, nrows: int):
        gg = _grid.global_grid()
        self._single, fs = _fields_of(fields_like, "Recorder")
        A0 = fs[0]
        if not isinstance(nrows, int) or isinstance(nrows, bool) or nrows < 1:
            raise IGGError(f"Recorder: `nrows` must be an integer >= 1 (got {nrows!r}).")
        self._like = (len(fs), tuple(A0.shape), A0.dtype, A0.device)
        self._pts = _points(P, A0, "Recorder")
        self._table = _table(gg, A0.shape, "Recorder")
        self._me0 = int(gg.me) == 0
        self.nrows = nrows
        nf, npts = len(fs), self._pts[1]
        self._buf = torch.zeros((nrows, nf, npts), dtype=torch.float64, device=A0.device)
        self._count = torch.zeros(1, dtype=torch.int64, device=A0.device)

    def record(self, *fields) -> None:
        """Sample ``fields`` into the next row."""
        _single, fs = _fields_of(fields, "Recorder.record")
        if (len(fs), tuple(fs[0].shape), fs[0].dtype, fs[0].device) != self._like:
            raise IGGError("Recorder.record: the fields differ from those the recorder was made for "
                           f"(number, shape, dtype, device: {self._like}).")
        nf, npts = self._like[0], self._pts[1]
        if npts:
            _launch(fs, self._table, self._pts, self._buf, npts, self._me0, self._count, self.nrows, nf * npts)
        self._count.add_(1)

    def result(self) -> torch.Tensor:
        """The rows recorded so far, combined over the ranks. Collective."""
        count = int(self._count.item())
        if count > self.nrows:
            raise IGGError(f"Recorder: {count} rows were recorded into a buffer of {self.nrows}; the rows past the "
                           "last were not kept.")
        rows = self._buf[:count].clone()
        _combine(_grid.global_grid(), rows, "Recorder.result")
        return rows[:, 0] if self._single else rows

    def reset(self) -> None:
        """Zero the buffer and the counter."""
        self._buf.zero_()
        self._count.zero_()
