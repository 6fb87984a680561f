"""``spread_g`` - point values added into the fields at arbitrary points of the
GLOBAL grid: the transpose ``Sᵀ`` of ``sample_g``'s operator ``S``; and
``Source``, a table of them injected row by row without a collective per step.

A point ``u`` and its per-dimension ``(g, t, valid)`` are exactly
``sample_g``'s (one shared function). The lower corner ``g`` takes the factor
``1 - t``, the upper one (``g + 1``, wrapped where periodic) the factor ``t``;
a corner's weight is ``((fx*fy)*fz)`` in float64 and a corner with a zero
factor in any dimension receives nothing. A cell folds the contributions
``w * v_p`` of all points that reach it in ascending point index, in float64,
and is then updated once: ``A[cell] = T(double(A[cell]) + s)``. No atomics:
the order is fixed, so the result is bitwise reproducible and the GPU equals
the host bit for bit.

``copies="all"`` (sources) adds into every local cell whose global index
(``indices_g``) is a corner's - halo and overlap copies included - so fields
that were halo-consistent stay so and the result does not depend on the
decomposition. ``copies="owner"`` (the strict transpose) adds only on the rank
that owns the point's lower corner (``sample_owner``), into the cells
``sample_g`` read there.

The work is split as in ``Recorder``: an eager **plan** (a CSR structure by
touched cell; on the GPU two HIP kernels around a torch ``cumsum``, ``sort``
and ``unique_consecutive``) and a per-step **apply** launch (csrc/kernels/
spread_kernels.hip: one lane per touched cell, no workspace, no host
synchronisation, capturable). CPU tensors take ``native.host_spread_plan`` and
``native.host_spread_apply``, the same expressions on the host.
"""
from __future__ import annotations

import itertools

import torch

from .._native import IGGError, native
from . import grid as _grid
from .gather_g import _extent, _segments
from .sample_g import _check_overlap, _points, sample_owner
from .scatter_g import _runs

__all__ = ["spread_g", "spread_plan", "spread_targets", "SpreadPlan", "Source"]

_COPIES = {"all": 0, "owner": 1}


def _copies(copies, who) -> int:
    if not isinstance(copies, str) or copies not in _COPIES:
        raise IGGError(f"{who}: `copies` must be 'all' or 'owner' (got {copies!r}).")
    return _COPIES[copies]


def spread_targets(nxyz, overlaps, dims, periods, coords, shape, g, copies="all") -> list:
    """The local index tuples of the rank at ``coords`` that receive what a
    point adds to the global index tuple ``g``. A pure function of the grid
    parameters (as ``sample_owner``).

    ``copies="all"``: every local cell whose global index (``indices_g``) is
    ``g``, each once, from the runs of ``scatter_g`` per dimension - halo and
    overlap cells included, and the copies of a 1-D or 2-D field on ranks that
    differ only in a missing dimension all have them. ``copies="owner"``:
    ``[sample_owner(...)]`` if this rank owns ``g``, else ``[]`` (its overlap
    requirement and error included)."""
    nd = len(shape)
    mode = _copies(copies, "spread_targets")
    if len(g) != nd:
        raise IGGError(f"spread_targets: `g` needs one index per dimension of the field ({nd}).")
    if mode == 1:
        i = sample_owner(nxyz, overlaps, dims, periods, coords, shape, g)
        return [] if i is None else [i]
    per_dim = []
    for d in range(nd):
        hits = [i0 + (int(g[d]) - g0)
                for i0, ln, g0 in _runs(int(nxyz[d]), int(overlaps[d]), int(dims[d]), int(periods[d]),
                                        int(coords[d]), int(shape[d]))
                if g0 <= int(g[d]) < g0 + ln]
        per_dim.append(hits)
    return [tuple(c) for c in itertools.product(*per_dim)]


# ------------------------------------------------------------------ arguments
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
    if A0.dtype not in (torch.float32, torch.float64):
        raise IGGError(f"{who}: the fields must be float32 or float64 (got {A0.dtype}).")
    return single, fs


def _table(gg, shape, mode, who) -> list:
    """Per dimension ``(E, periodic, m, segments, runs)``: the kernels' table."""
    nd = len(shape)
    if mode == 1:
        _check_overlap(gg.nxyz, gg.overlaps, gg.dims, gg.periods, shape, who)
    mine = all(int(gg.coords[d]) == 0 for d in range(nd, 3))
    table = []
    for d in range(nd):
        par = (int(gg.nxyz[d]), int(gg.overlaps[d]), int(gg.dims[d]), int(gg.periods[d]))
        E = _extent(*par, int(shape[d]))
        if E < 2:
            raise IGGError(f"{who}: the global extent of dimension {d} is {E}; at least 2 cells are needed.")
        segs, runs = [], []
        if mode == 1:
            segs = [list(s) for s in _segments(*par, int(gg.coords[d]), int(shape[d]))] if mine else []
        else:
            runs = [list(r) for r in _runs(*par, int(gg.coords[d]), int(shape[d]))]
            if len(runs) > int(native.SPREAD_MAX_RUNS):
                raise IGGError(f"{who}: the local range of dimension {d} wraps the period {len(runs) - 1} times "
                               f"({len(runs)} runs); at most {int(native.SPREAD_MAX_RUNS)} runs are supported.")
        table.append((E, par[3], int(shape[d]), segs, runs))
    return table


def _values(V, nf, single, npts, device, who) -> tuple:
    """``(V, stride of a field, stride of a point)``."""
    if not isinstance(V, torch.Tensor) or V.dtype != torch.float64 or V.device != device:
        raise IGGError(f"{who}: `V` must be a float64 tensor on {device}.")
    if single and tuple(V.shape) == (npts,):
        return V, 0, int(V.stride(0))
    if not single and tuple(V.shape) == (nf, npts):
        return V, int(V.stride(0)), int(V.stride(1))
    want = (npts,) if single else (nf, npts)
    raise IGGError(f"{who}: `V` must have shape {want} (got {tuple(V.shape)}).")


def _refuse_capture(A0, who) -> None:
    if A0.is_cuda and torch.cuda.is_current_stream_capturing():
        raise IGGError(f"{who} builds a plan, which synchronises with the host: it cannot run inside a stream "
                       "capture. Build the plan first (spread_plan) and capture plan.apply.")


# ------------------------------------------------------------------ the plan
class SpreadPlan:
    """Where fixed points add into the fields of one shape on this rank: a CSR
    structure by touched local cell, built by ``spread_plan``.

    ``cells`` (int64, ``ncells``): the touched cells as linear C-order indices
    into the field's shape, ascending - so one plan serves fields of any
    strides; ``start`` (int64, ``ncells + 1``): cell ``i`` has the entries
    ``start[i] .. start[i+1] - 1``; ``point`` (int64) and ``weight``
    (float64), ``nentries`` each, sorted by (cell, point). All on the fields'
    device; the GPU plan and the host plan are equal as tensors."""

    def __init__(self, shape, device, npts, cells, start, point, weight):
        self.shape, self.device, self.npts = tuple(shape), device, int(npts)
        self.cells, self.start, self.point, self.weight = cells, start, point, weight
        self.ncells, self.nentries = int(cells.numel()), int(point.numel())

    def _launch(self, fs, V, v_fs, v_ps, row=None, nrows=0, row_stride=0, max_blocks=0) -> None:
        if not self.ncells:
            return
        A0 = fs[0]
        args = (list(self.shape), [(A.data_ptr(), list(A.stride())) for A in fs], A0.element_size(), self.ncells,
                self.cells.data_ptr(), self.start.data_ptr(), self.point.data_ptr(), self.weight.data_ptr(),
                V.data_ptr(), v_fs, v_ps, row.data_ptr() if row is not None else 0, nrows, row_stride)
        if A0.is_cuda:
            native.spread_apply(*args, torch.cuda.current_stream().cuda_stream, max_blocks)
        else:
            native.host_spread_apply(*args)

    def _check_fields(self, fields, who) -> tuple:
        _single, fs = _fields_of(fields, who)
        if tuple(fs[0].shape) != self.shape or fs[0].device != self.device:
            raise IGGError(f"{who}: the fields differ from those the plan was made for (shape {self.shape} on "
                           f"{self.device}).")
        return fs

    def apply(self, V: torch.Tensor, *fields) -> None:
        """Add the point values ``V`` into ``fields``: one launch (per 8
        fields), nothing allocated, no host synchronisation, capturable.
        ``V``: float64 on the fields' device, ``(nfields, npts)`` with any
        strides, or ``(npts,)`` for one field. The fields may have any dense
        layout, float32 or float64."""
        fs = self._check_fields(fields, "SpreadPlan.apply")
        single = len(fs) == 1 and isinstance(V, torch.Tensor) and V.dim() == 1
        V, v_fs, v_ps = _values(V, len(fs), single, self.npts, self.device, "SpreadPlan.apply")
        self._launch(fs, V, v_fs, v_ps)


def _build_plan(A0, table, pts, mode, max_blocks=0) -> SpreadPlan:
    P, npts, ps0, ps1 = pts
    dev = A0.device
    i64 = dict(dtype=torch.int64, device=dev)
    if A0.is_cuda:
        stream = torch.cuda.current_stream().cuda_stream
        count = torch.empty(npts, **i64)
        native.spread_count(table, mode, P.data_ptr(), ps0, ps1, npts, count.data_ptr(), stream, max_blocks)
        cum = torch.cumsum(count, 0)
        total = int(cum[-1].item()) if npts else 0  # (the plan's one host synchronisation)
        key, point = torch.empty(total, **i64), torch.empty(total, **i64)
        weight = torch.empty(total, dtype=torch.float64, device=dev)
        native.spread_fill(table, mode, P.data_ptr(), ps0, ps1, npts, cum.data_ptr(), total, key.data_ptr(),
                           point.data_ptr(), weight.data_ptr(), stream, max_blocks)
        # entries are in point order: a stable sort by cell leaves every segment sorted by point
        key, order = torch.sort(key, stable=True)
        cells, per_cell = torch.unique_consecutive(key, return_counts=True)
        start = torch.zeros(cells.numel() + 1, **i64)
        torch.cumsum(per_cell, 0, out=start[1:])
        return SpreadPlan(A0.shape, dev, npts, cells, start, point[order], weight[order])
    raw = native.host_spread_plan(table, mode, P.data_ptr(), ps0, ps1, npts)
    dts = (torch.int64, torch.int64, torch.int64, torch.float64)
    cells, start, point, weight = (torch.frombuffer(bytearray(b), dtype=dt) if len(b) else torch.empty(0, dtype=dt)
                                   for b, dt in zip(raw, dts))
    return SpreadPlan(A0.shape, dev, npts, cells, start, point, weight)


def spread_plan(fields_like, P: torch.Tensor, *, copies: str = "all") -> SpreadPlan:
    """The plan of ``spread_g`` for the points ``P`` and fields shaped like
    ``fields_like`` (a tensor or a tuple, as in ``spread_g``): a ``SpreadPlan``
    with ``ncells``, ``nentries``, the tensors ``cells``, ``start``, ``point``
    and ``weight``, and ``apply(V, *fields)``. Built eagerly: it allocates
    workspace proportional to the real number of targets and synchronises
    once, so it is refused inside a stream capture. Not collective. The plan
    is a snapshot of ``P``: points of sources and receivers do not move."""
    gg = _grid.global_grid()
    mode = _copies(copies, "spread_plan")
    _single, fs = _fields_of(fields_like, "spread_plan")
    A0 = fs[0]
    pts = _points(P, A0, "spread_plan")
    table = _table(gg, A0.shape, mode, "spread_plan")
    _refuse_capture(A0, "spread_plan")
    return _build_plan(A0, table, pts, mode)


def spread_g(fields, P: torch.Tensor, V: torch.Tensor, *, copies: str = "all") -> None:
    """Add the values ``V`` at the points ``P`` of the global grid into
    ``fields``, in place: the transpose of ``sample_g``. Not collective; eager
    only (it builds a plan, which synchronises; ``IGGError`` inside a stream
    capture - use ``spread_plan(...).apply`` or ``Source`` there).

    ``fields``: one tensor or a tuple of tensors of one shape, dtype and
    device (strides may differ), 1-D to 3-D, any dense layout, float32 or
    float64, CPU or GPU. ``P``: as in ``sample_g`` (float64 ``(npts, nd)``, any
    strides, or ``(npts,)`` for a 1-D field). ``V``: float64 on the fields'
    device, ``(npts,)`` for a tensor, ``(nfields, npts)`` for a tuple.
    ``npts == 0`` is legal.

    Per dimension a point's ``(g, t, valid)`` are ``sample_g``'s. The lower
    corner ``g`` has the factor ``1 - t``, the upper corner (``g + 1``, or
    ``(g+1) mod E`` where periodic) the factor ``t``; a corner's weight is
    ``((fx*fy)*fz)`` in float64, each operation rounded separately, and a
    corner with a zero factor in any dimension receives nothing (as a corner
    of weight zero never reaches ``sample_g``'s result). A point that is
    invalid in any dimension or has a non-finite coordinate contributes
    nothing on any rank; nothing is raised for point values. A cell folds the
    contributions ``w * v_p`` of the points that reach it in ascending point
    index, ``s = c_first; s = s + c_next; ...`` in float64, and then ``A[cell]
    = T(double(A[cell]) + s)`` with one rounding to the field's dtype; a cell
    no point reaches is not written at all. No atomics: two runs give the same
    bits, and the GPU gives the host's bits.

    ``copies="all"`` (the default, for sources): on every rank every local
    cell whose global index (``indices_g``) equals the corner's receives -
    halo and overlap cells included, both copies on a self-periodic rank, and
    the copies of a 1-D or 2-D field on ranks that differ only in a missing
    dimension (``spread_targets``; the runs of ``scatter_g``, at most 4 per
    dimension or ``IGGError``). Every copy of a global cell gets the same
    addends in the same order: halo-consistent fields stay so
    (``update_halo_`` afterwards changes no bit) and ``gather_g`` of the
    result is the same bits for every decomposition. ``copies="owner"`` (the
    strict transpose of ``sample_g``): only the rank that owns the point's
    lower corner (``sample_owner``) adds, into its local ``lo`` / ``lo + 1``
    cells, exactly those ``sample_g`` read there: ``sum over ranks of <A_r,
    spread_g(V)_r> == <sample_g(A), V>``. It needs ``sample_g``'s field
    overlap and raises its error.

    Preconditions, not checked: ``P`` and ``V`` hold the same bits on every
    rank. Every refused call leaves the fields untouched."""
    gg = _grid.global_grid()
    mode = _copies(copies, "spread_g")
    single, fs = _fields_of(fields, "spread_g")
    A0 = fs[0]
    pts = _points(P, A0, "spread_g")
    V, v_fs, v_ps = _values(V, len(fs), single, pts[1], A0.device, "spread_g")
    table = _table(gg, A0.shape, mode, "spread_g")
    _refuse_capture(A0, "spread_g")
    if not pts[1]:
        return
    _build_plan(A0, table, pts, mode)._launch(fs, V, v_fs, v_ps)


class Source:
    """A table of point values injected row by row without a collective per
    step (a shot's wavelet): ``Source(fields_like, P, W, copies="all")``, the
    mirror of ``Recorder``.

    ``fields_like`` (a tensor or a tuple, as in ``spread_g``) fixes the shape,
    dtype, device and number of the fields, ``P`` the points (the plan is
    built here, eagerly). ``W`` is a float64 table ``(nrows, npts)`` for a
    tensor or ``(nrows, nfields, npts)`` on the fields' device. The source
    holds a device int64 row counter. ``inject(*fields)`` is one apply launch
    that reads the counter on the device and adds that row into the fields -
    nothing once the rows are used up - followed by one stream-ordered
    increment: no collective, no host synchronisation, capturable, and a
    replayed graph injects the next row. ``reset()`` zeroes the counter. ``W``
    is used as passed: rewriting it changes the wavelet."""

    def __init__(self, fields_like, P: torch.Tensor, W: torch.Tensor, *, copies: str = "all"):
        gg = _grid.global_grid()
        mode = _copies(copies, "Source")
        self._single, fs = _fields_of(fields_like, "Source")
        A0 = fs[0]
        pts = _points(P, A0, "Source")
        nf, npts = len(fs), pts[1]
        if not isinstance(W, torch.Tensor) or W.dtype != torch.float64 or W.device != A0.device:
            raise IGGError(f"Source: `W` must be a float64 tensor on {A0.device}.")
        if self._single and W.dim() == 2 and int(W.shape[1]) == npts:
            self._strides = (int(W.stride(0)), 0, int(W.stride(1)))
        elif W.dim() == 3 and tuple(W.shape[1:]) == (nf, npts):
            self._strides = (int(W.stride(0)), int(W.stride(1)), int(W.stride(2)))
        else:
            want = f"(nrows, {npts})" if self._single else f"(nrows, {nf}, {npts})"
            raise IGGError(f"Source: `W` must have shape {want} (got {tuple(W.shape)}).")
        table = _table(gg, A0.shape, mode, "Source")
        _refuse_capture(A0, "Source")
        self._like = (nf, tuple(A0.shape), A0.dtype, A0.device)
        self.W, self.nrows = W, int(W.shape[0])
        self.plan = _build_plan(A0, table, pts, mode)
        self._count = torch.zeros(1, dtype=torch.int64, device=A0.device)

    def inject(self, *fields) -> None:
        """Add the next row of ``W`` into ``fields``."""
        _single, fs = _fields_of(fields, "Source.inject")
        if (len(fs), tuple(fs[0].shape), fs[0].dtype, fs[0].device) != self._like:
            raise IGGError("Source.inject: the fields differ from those the source was made for "
                           f"(number, shape, dtype, device: {self._like}).")
        rs, v_fs, v_ps = self._strides
        self.plan._launch(fs, self.W, v_fs, v_ps, self._count, self.nrows, rs)
        self._count.add_(1)

    def reset(self) -> None:
        """Zero the row counter: the next ``inject`` adds row 0."""
        self._count.zero_()
