"""Reductions over the implicit GLOBAL grid: every global cell counted once.

A field of the local grid overlaps its neighbours' fields, so a sum, a mean, a
norm or a dot product of the local arrays counts an overlap cell twice (four
times on an edge, eight at a corner), and a periodic single rank counts its
own halo. These reductions walk the OWNED box of each field only
(``owned_ranges``) and combine the ranks with one ``comm.allreduce_``.

``project_g`` is the form between ``reduce_g`` and ``gather_g``: it reduces over
some axes of the global grid and keeps the others (a plane-mean profile, a
column maximum), with the same ownership, NaN rule and single collective.

On the GPU, float32 and float64 fields of any dense layout are read once by
the HIP reduction kernels (csrc/kernels/reduce_kernels.hip; for ``project_g``
csrc/kernels/project_kernels.hip): f64 accumulation,
a fixed block count per box and a fixed combination order, so the result is
bitwise the same from run to run; no atomics, no host synchronisation, and the
launches can be captured in a hipGraph (after one eager call, which allocates
the workspace). Other dtypes and CPU tensors take the same reduction in torch
on ``owned_view``.
"""
from __future__ import annotations

import itertools
import math

import torch

from .._native import IGGError, native
from ..parallel import grid as _grid
from ..parallel.gather_g import _extent, _segments

__all__ = ["owned_ranges", "owned_view", "reduce_g", "sum_g", "max_g", "min_g", "maxabs_g", "dot_g",
           "maxabs_diff_g", "norm_g", "norm_diff_g", "mean_g", "project_g"]

# op name -> native op code (csrc/include/igg/reduce.hpp)
_OPS = {"sum": 0, "sumsq": 1, "max": 2, "min": 3, "maxabs": 4, "dot": 5, "sumsq_diff": 6, "maxabs_diff": 7}
_TWO = ("dot", "sumsq_diff", "maxabs_diff")
_MAX = ("max", "min", "maxabs", "maxabs_diff")


def owned_ranges(A: torch.Tensor) -> tuple:
    """The box of ``A`` this rank owns: one ``(lo, hi)`` pair of local indices
    (0-based, half-open) per dimension of ``A``.

    In dimension ``d`` with ``m = A.shape[d]``, the field's own overlap
    ``o = max(ol(d, A), 0)`` (the grid's plus ``m - nxyz[d]``: staggered sizes
    work) and ``lo = o // 2``: an interior rank, and every rank of a periodic
    dimension (a single periodic rank too), owns ``[lo, m - (o - lo))``; in a
    non-periodic dimension the first rank extends the lower bound to 0 and the
    last rank the upper bound to ``m`` (a single non-periodic rank owns
    ``[0, m)``). Only ``dims``, ``coords``, ``periods``, ``overlaps``, ``nxyz``
    and the shape of ``A`` enter - not the neighbour table, so
    ``enable_loopback`` changes nothing.

    * Partition: over all ranks the owned ranges tile the global index range of
      ``A`` without gap or overlap - ``D*(n - o_grid) + ol(d, A)`` cells in a
      non-periodic dimension of ``D`` ranks, ``D*(n - o_grid)`` in a periodic
      one; rank ``c`` ends where rank ``c + 1`` begins, at global index
      ``(c + 1)*(n - o_grid) + lo``.
    * No received plane: where ``ol(d, A) >= 2*halowidth`` no owned plane is
      one that ``update_halo_`` writes, so a reduction gives the same answer
      before and after an exchange, and on a fused model whose halos are stale.
    """
    gg = _grid.global_grid()
    if A.dim() < 1 or A.dim() > 3:
        raise IGGError(f"Fields must have 1 to 3 dimensions (got {A.dim()}).")
    out = []
    for d in range(A.dim()):
        m = int(A.shape[d])
        o = max(_grid.ol(d + 1, A), 0)
        lo = o // 2
        a, b = lo, m - (o - lo)
        if not int(gg.periods[d]):
            if int(gg.coords[d]) == 0:
                a = 0
            if int(gg.coords[d]) == int(gg.dims[d]) - 1:
                b = m
        out.append((a, b))
    return tuple(out)


def owned_view(A: torch.Tensor) -> torch.Tensor:
    """The strided view of ``A``'s owned box (``owned_ranges``)."""
    return A[tuple(slice(a, b) for a, b in owned_ranges(A))]


def global_cells(A: torch.Tensor) -> int:
    """Cells of ``A``'s global index range: the sum over all ranks of the
    owned boxes' sizes, from the partition (no collective)."""
    gg = _grid.global_grid()
    if A.dim() < 1 or A.dim() > 3:
        raise IGGError(f"Fields must have 1 to 3 dimensions (got {A.dim()}).")
    n = 1
    for d in range(A.dim()):
        m = int(A.shape[d])
        o = max(_grid.ol(d + 1, A), 0)
        n *= int(gg.dims[d]) * (m - o) + (0 if int(gg.periods[d]) else o)
    return n


def _others(fields, other) -> tuple:
    if other is None:
        raise IGGError("reduce_g: a two-input op needs `other`.")
    others = (other,) if isinstance(other, torch.Tensor) else tuple(other)
    if len(others) != len(fields):
        raise IGGError(f"reduce_g: `other` has {len(others)} tensors for {len(fields)} fields.")
    for A, B in zip(fields, others):
        if not isinstance(B, torch.Tensor) or B.shape != A.shape or B.dtype != A.dtype or B.device != A.device:
            raise IGGError("reduce_g: every tensor of `other` must match its field's shape, dtype and device.")
    return others


def _allreduce(comm, t: torch.Tensor, op: str) -> None:
    """``comm.allreduce_`` on the current stream. Ranks that SHARE a GPU (a
    rehearsal of a multi-GPU run on one device) have no RCCL communicator -
    RCCL refuses duplicate devices - so there, and only there, the few result
    values are staged through the host over gloo, as ``update_halo_`` does
    with its halos. The check is collective and made once per communicator."""
    if t.is_cuda:
        staged = getattr(comm, "_reduce_staged", None)
        if staged is None:
            from ..parallel.transport_select import _shared_device

            staged = comm._reduce_staged = bool(_shared_device(comm))
        if staged:
            h = t.cpu()
            comm.allreduce_(h, op)
            t.copy_(h)
            return
    comm.allreduce_(t, op)


def _torch_local(op: str, fields, others, res: torch.Tensor, travel) -> None:
    """The reduction in torch on the owned views (CPU tensors, other dtypes):
    f64 terms and accumulation; torch's max propagates NaN."""
    for k, A in enumerate(fields):
        x = owned_view(A).double()
        y = owned_view(others[k]).double() if others else None
        if op == "sum":
            v = x.sum()
        elif op == "sumsq":
            v = (x * x).sum()
        elif op == "dot":
            v = (x * y).sum()
        elif op == "sumsq_diff":
            v = ((x - y) * (x - y)).sum()
        elif op == "max":
            v = x.max()
        elif op == "min":
            v = (-x).max() if travel is not None else x.min()
        elif op == "maxabs":
            v = x.abs().max()
        else:
            v = (x - y).abs().max()
        if travel is not None:
            nan = torch.isnan(v)
            travel[k] = torch.where(nan, torch.full_like(v, -math.inf), v)
            travel[len(fields) + k] = nan.double()
        else:
            res[k] = v


def reduce_g(op: str, *fields, other=None, out=None, local: bool = False) -> torch.Tensor:
    """Reduce ``fields`` over the global grid, every global cell once.

    ``op``: ``sum``, ``sumsq``, ``max``, ``min``, ``maxabs``, or a two-input
    form ``dot``, ``sumsq_diff``, ``maxabs_diff`` with ``other`` one tensor or
    a tuple of the same length, shapes and dtype as ``fields``. One field
    gives a 0-dim tensor, several fields (one dtype and device, any shapes and
    staggered sizes) a 1-D tensor with an entry per field: float64, on the
    fields' device. With ``out=`` the result is written into that tensor (a
    captured graph refreshes it on replay). Nothing synchronises with the
    host: the caller's ``.item()`` does.

    Unless ``local=True`` (this rank's owned box only), one ``comm.allreduce_``
    per call combines the ranks on the current stream (RCCL for GPU tensors,
    gloo for CPU tensors; none on a single rank; ranks that share one GPU
    stage the result through the host); every rank receives identical bits. ``min`` travels as ``-max(-x)``. A NaN in any rank's owned
    box makes the result NaN on every rank, for every op; a NaN outside every
    owned box never reaches a result. The max-type ops send ``(value with NaN
    as -inf, NaN flag)`` under ``max`` and restore the NaN afterwards, so the
    result does not depend on how the collective's max treats NaN.

    Sums, squares, products and differences are formed and accumulated in
    float64 whatever the input type; max, min and abs are exact. float32 and
    float64 GPU tensors of any dense layout are reduced by the HIP kernels,
    everything else by torch on ``owned_view`` with the same semantics.
    """
    gg = _grid.global_grid()
    if op not in _OPS:
        raise IGGError(f"reduce_g: op must be one of {sorted(_OPS)} (got {op!r}).")
    if not fields or not all(isinstance(A, torch.Tensor) for A in fields):
        raise IGGError("reduce_g: at least one tensor field is needed.")
    A0 = fields[0]
    if any(A.dtype != A0.dtype or A.device != A0.device for A in fields):
        raise IGGError("reduce_g: the fields must share one dtype and one device.")
    others = _others(fields, other) if op in _TWO else ()
    if op not in _TWO and other is not None:
        raise IGGError(f"reduce_g: op {op!r} takes no `other`.")
    n = len(fields)
    shape = () if n == 1 else (n,)
    if out is not None:
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float64
                or out.device != A0.device or not out.is_contiguous()):
            raise IGGError(f"reduce_g: `out` must be a contiguous float64 tensor of shape {shape} on {A0.device}.")
        res = out
    else:
        res = torch.empty(shape, dtype=torch.float64, device=A0.device)
    ranges = [owned_ranges(A) for A in fields]
    multi = not local and int(gg.nprocs) > 1
    maxt = op in _MAX
    # across ranks the max-type ops travel as (value with NaN as -inf, NaN flag) under max
    travel = torch.empty(2 * n, dtype=torch.float64, device=A0.device) if (multi and maxt) else None
    res1 = res.reshape(n)  # a view: `res` is contiguous
    if A0.is_cuda and A0.dtype in (torch.float32, torch.float64):
        jobs = []
        for k, A in enumerate(fields):
            B = others[k] if others else None
            jobs.append((A.data_ptr(), B.data_ptr() if B is not None else 0, list(A.shape), list(A.stride()),
                         list(B.stride()) if B is not None else [], [r[0] for r in ranges[k]],
                         [r[1] for r in ranges[k]]))
        dst = travel if travel is not None else res1
        native.reduce(_OPS[op], jobs, A0.element_size(), dst.data_ptr(),
                      dst.data_ptr() + 8 * n if travel is not None else 0, torch.cuda.current_stream().cuda_stream)
    else:
        _torch_local(op, fields, others, res1, travel)
    if multi:
        if travel is not None:
            _allreduce(gg.comm, travel, "max")
            v = torch.where(travel[n:] > 0, torch.full_like(travel[:n], math.nan), travel[:n])
            res1.copy_(-v if op == "min" else v)
        else:
            _allreduce(gg.comm, res1, "sum")
    return res


def sum_g(A: torch.Tensor, **kw) -> torch.Tensor:
    """Sum of ``A`` over the global grid (``reduce_g("sum", A)``)."""
    return reduce_g("sum", A, **kw)


def max_g(A: torch.Tensor, **kw) -> torch.Tensor:
    """Maximum of ``A`` over the global grid."""
    return reduce_g("max", A, **kw)


def min_g(A: torch.Tensor, **kw) -> torch.Tensor:
    """Minimum of ``A`` over the global grid."""
    return reduce_g("min", A, **kw)


def maxabs_g(A: torch.Tensor, **kw) -> torch.Tensor:
    """Maximum of ``|A|`` over the global grid."""
    return reduce_g("maxabs", A, **kw)


def dot_g(A: torch.Tensor, B: torch.Tensor, **kw) -> torch.Tensor:
    """Dot product of ``A`` and ``B`` over the global grid."""
    return reduce_g("dot", A, other=B, **kw)


def maxabs_diff_g(A: torch.Tensor, B: torch.Tensor, **kw) -> torch.Tensor:
    """Maximum of ``|A - B|`` over the global grid (a residual)."""
    return reduce_g("maxabs_diff", A, other=B, **kw)


def norm_g(A: torch.Tensor, **kw) -> torch.Tensor:
    """L2 norm of ``A`` over the global grid: the square root of ``sumsq``."""
    r = reduce_g("sumsq", A, **kw)
    return r.sqrt_() if "out" in kw and kw["out"] is not None else torch.sqrt(r)


def norm_diff_g(A: torch.Tensor, B: torch.Tensor, **kw) -> torch.Tensor:
    """L2 norm of ``A - B`` over the global grid."""
    r = reduce_g("sumsq_diff", A, other=B, **kw)
    return r.sqrt_() if "out" in kw and kw["out"] is not None else torch.sqrt(r)


def mean_g(A: torch.Tensor, **kw) -> torch.Tensor:
    """Mean of ``A`` over the global grid: the global sum divided by the
    global cell count, which follows from the partition (no second collective)."""
    if kw.get("local"):
        raise IGGError("mean_g: the mean is over the global grid (no `local`).")
    r = reduce_g("sum", A, **kw)
    # (a tensor divisor: torch's GPU division by a Python scalar multiplies by its reciprocal)
    return r.div_(torch.full_like(r, float(global_cells(A))))


# ------------------------------------------------------------------ project_g
def _keep_axes(A: torch.Tensor, keep) -> tuple:
    """``keep`` as a strictly increasing tuple of axes of ``A``: non-empty and
    not every axis (those are ``reduce_g`` and ``gather_g``)."""
    if isinstance(keep, int) and not isinstance(keep, bool):
        keep = (keep,)
    if not isinstance(keep, (tuple, list)) or any(not isinstance(k, int) or isinstance(k, bool) for k in keep):
        raise IGGError(f"project_g: `keep` must be an axis or a tuple of axes (got {keep!r}).")
    keep = tuple(keep)
    if not keep:
        raise IGGError("project_g: `keep` names no axis - a reduction over every axis is reduce_g.")
    if any(k < 0 or k >= A.dim() for k in keep) or any(b <= a for a, b in zip(keep, keep[1:])):
        raise IGGError(f"project_g: `keep` must be strictly increasing axes of the {A.dim()}-D field (got {keep}).")
    if A.dim() == 1 or len(keep) == A.dim():
        raise IGGError("project_g: `keep` names every axis of the field - nothing is reduced: that is gather_g.")
    return keep


def _project_torch(op: str, A, B, red, negated: bool) -> torch.Tensor:
    """The projection of the owned view in torch (CPU tensors, other dtypes):
    f64 terms and accumulation; torch's amax / amin propagate NaN."""
    x = owned_view(A).double()
    y = owned_view(B).double() if B is not None else None
    if op == "sum":
        return x.sum(dim=red)
    if op == "sumsq":
        return (x * x).sum(dim=red)
    if op == "dot":
        return (x * y).sum(dim=red)
    if op == "sumsq_diff":
        return ((x - y) * (x - y)).sum(dim=red)
    if op == "max":
        return x.amax(dim=red)
    if op == "min":
        return (-x).amax(dim=red) if negated else x.amin(dim=red)
    if op == "maxabs":
        return x.abs().amax(dim=red)
    return (x - y).abs().amax(dim=red)


def project_g(op: str, A: torch.Tensor, keep, *, other=None, out=None, local: bool = False) -> torch.Tensor:
    """Reduce ``A`` over some axes of the global grid and keep the others:
    the form between ``reduce_g`` (one number) and ``gather_g`` (every cell).

    ``keep``: an axis of the 2-D or 3-D field ``A`` or a strictly increasing
    tuple of axes, 0-based, non-empty and not every axis. ``op``: one of the
    ops of ``reduce_g`` (``other`` as there) or ``"mean"``, the sum divided by
    the product of the global extents of the reduced axes. The result is a
    contiguous float64 tensor on ``A``'s device whose shape is the global
    extent of ``A`` along each kept axis (the matching entries of
    ``selection_shape_g(A)``: ``D*(n-o)`` in a periodic dimension); cell
    ``[g...]`` is ``op`` over all global cells whose kept-axis global indices
    (``indices_g``) are ``g...``. ``project_g(op, A, keep)`` equals the same
    torch reduction, over the reduced axes, of the array ``gather_g(A, G)``
    assembles - on every rank, with identical bits. With ``out=`` the result
    is written into that tensor (a captured graph refreshes it on replay).
    ``local=True`` returns this rank's own contribution in the same global
    shape, with the op's identity elsewhere (0 for the sums, ``-inf`` for
    ``max``, ``maxabs`` and ``maxabs_diff``, ``+inf`` for ``min``) and no
    collective.

    Only owned cells are read (``owned_ranges``): no ``update_halo_`` or
    ``sync_halo()`` is needed first. Terms and accumulation are float64; max,
    min and abs are exact. A NaN in an owned cell makes NaN exactly the output
    cells whose line or plane contains it, on every rank, for every op; a NaN
    outside every owned box reaches nothing. One ``comm.allreduce_`` per call
    over the global-shaped buffer combines the ranks (none on a single rank;
    ranks that share a GPU stage through the host): sums travel with zeros in
    the cells a rank does not contribute to, the max-type ops as ``(value with
    NaN as -inf, NaN flag)`` under ``max`` - twice the cells - and ``min`` as
    ``-max(-x)``. Of the ranks that hold copies of a field with fewer
    dimensions than the grid only those at coordinate 0 of the missing
    dimensions contribute (``gather_g``'s rule). A rank's owned range along a
    kept axis lands at its global indices, in two segments where a periodic
    rank's range wraps.

    float32 and float64 GPU tensors of any dense layout are read once by the
    HIP projection kernels (csrc/kernels/project_kernels.hip): at most two
    launches, no atomics, a number of workgroups, slices and an order of
    combination fixed by the box and the keep-set, so the bits are the same
    from run to run; the partials' workspace grows only (a call that must grow
    it cannot be captured: call once before capturing). Everything else takes
    torch on ``owned_view`` with the same semantics.
    """
    gg = _grid.global_grid()
    mean = op == "mean"
    if not mean and op not in _OPS:
        raise IGGError(f"project_g: op must be one of {sorted(_OPS) + ['mean']} (got {op!r}).")
    if not isinstance(A, torch.Tensor) or A.dim() < 1 or A.dim() > 3:
        raise IGGError(f"Fields must have 1 to 3 dimensions (got {A.dim() if isinstance(A, torch.Tensor) else A!r}).")
    keep = _keep_axes(A, keep)
    if mean and local:
        raise IGGError("project_g: the mean is over the global grid (no `local`).")
    rop = "sum" if mean else op
    B = _others((A,), other)[0] if rop in _TWO else None
    if rop not in _TWO and other is not None:
        raise IGGError(f"project_g: op {op!r} takes no `other`.")
    nd = A.dim()
    red = tuple(d for d in range(nd) if d not in keep)
    par = [(int(gg.nxyz[d]), int(gg.overlaps[d]), int(gg.dims[d]), int(gg.periods[d]), int(gg.coords[d]),
            int(A.shape[d])) for d in range(nd)]
    extent = [_extent(n, o, D, per, m) for n, o, D, per, _c, m in par]
    gshape = tuple(extent[d] for d in keep)
    if out is not None:
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != gshape or out.dtype != torch.float64
                or out.device != A.device or not out.is_contiguous()):
            raise IGGError(f"project_g: `out` must be a contiguous float64 tensor of shape {gshape} on {A.device}.")
        res = out
    else:
        res = torch.empty(gshape, dtype=torch.float64, device=A.device)
    # of the copies of a field with fewer dimensions than the grid one contributes (gather_g's rule)
    mine = all(int(gg.coords[d]) == 0 for d in range(nd, 3))
    ranges = owned_ranges(A) if mine else ((0, 0),) * nd
    segs = [_segments(*par[d]) if mine else [] for d in keep]  # (g0, g1, i0) per kept axis: one, or two at a wrap
    mine = mine and all(b > a for a, b in ranges)
    multi = not local and int(gg.nprocs) > 1
    maxt = rop in _MAX
    cells = res.numel()
    # across ranks the max-type ops travel as (value with NaN as -inf, NaN flag) under max
    travel = torch.empty((2,) + gshape, dtype=torch.float64, device=A.device) if (multi and maxt) else None
    dst = travel[0] if travel is not None else res
    if A.is_cuda and A.dtype in (torch.float32, torch.float64):
        native.project(_OPS[rop], A.data_ptr(), B.data_ptr() if B is not None else 0, list(A.shape),
                       list(A.stride()), list(B.stride()) if B is not None else [], [r[0] for r in ranges],
                       [r[1] for r in ranges], list(keep), A.element_size(), dst.data_ptr(),
                       dst.data_ptr() + 8 * cells if travel is not None else 0,
                       [s[0][0] if s else 0 for s in segs], list(gshape), list(dst.stride()),
                       torch.cuda.current_stream().cuda_stream)
    else:
        if travel is not None:
            travel[0].fill_(-math.inf)
            travel[1].zero_()
        else:
            res.fill_(0.0 if not maxt else math.inf if rop == "min" else -math.inf)
        if mine:
            v = _project_torch(rop, A, B, red, travel is not None)
            for combo in itertools.product(*segs):
                at = tuple(slice(g0, g1) for g0, g1, _i0 in combo)
                src = tuple(slice(i0 - ranges[d][0], i0 - ranges[d][0] + g1 - g0)
                            for d, (g0, g1, i0) in zip(keep, combo))
                if travel is not None:
                    nan = torch.isnan(v[src])
                    travel[0][at] = torch.where(nan, torch.full_like(v[src], -math.inf), v[src])
                    travel[1][at] = nan.double()
                else:
                    res[at] = v[src]
    if multi:
        if travel is not None:
            _allreduce(gg.comm, travel, "max")
            v = torch.where(travel[1] > 0, torch.full_like(travel[0], math.nan), travel[0])
            res.copy_(-v if rop == "min" else v)
        else:
            _allreduce(gg.comm, res, "sum")
    if mean:
        # (a tensor divisor: torch's GPU division by a Python scalar multiplies by its reciprocal)
        res.div_(torch.full_like(res, float(math.prod(extent[d] for d in red))))
    return res
