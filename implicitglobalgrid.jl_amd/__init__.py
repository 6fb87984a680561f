"""MI355X-native implicit global grid (capabilities of ImplicitGlobalGrid.jl).

Distributed stencil computing on regular, optionally staggered 1-D/2-D/3-D
grids: write a single-device solver on a *local* grid; ``init_global_grid``
builds a Cartesian process topology (one process per MI355X) and the *global*
grid follows implicitly; ``update_halo_`` exchanges one-plane halos (RCCL over
xGMI, HIP pack/unpack kernels); ``gather_`` assembles the global array on a
root rank.

Public API (reference names in parentheses, src/ImplicitGlobalGrid.jl:9-23):
``init_global_grid``, ``finalize_global_grid``, ``update_halo_``
(``update_halo!``), ``gather_`` (``gather!``), ``select_device``, ``nx_g``,
``ny_g``, ``nz_g``, ``x_g``, ``y_g``, ``z_g``, ``tic``, ``toc`` and
``get_global_grid``. Beyond the reference: reductions over the global grid in
which every global cell counts once (``reduce_g``, ``sum_g``, ``norm_g``,
``max_g``, ``mean_g``, ...; ops/reduce.py), ``project_g``, which reduces
over some axes and keeps the others (profiles, column maxima), and
``gather_g``, which assembles the true global field - whole, a box of it or
every n-th cell - from the owned cells (``indices_g``, ``selection_shape_g``;
parallel/gather_g.py), and its inverse ``scatter_g``, which fills the local
fields of all ranks from a global array on a root (``scatter_pieces``;
parallel/scatter_g.py); and ``accumulate_halo_``, the transpose of
``update_halo_``, which adds the halos into the cells of the ranks that own
them (parallel/accumulate.py), with the differentiable exchange
``igg.autograd.update_halo`` built on it; and ``sample_g``, the fields' values
at arbitrary points of the global grid, interpolated by the rank that owns
each point's cell, with ``Recorder`` for time series of them
(``sample_owner``, ``index_g``; parallel/sample_g.py), and its transpose
``spread_g``, point values added into the fields without atomics, with
``Source`` for a wavelet injected step by step (``spread_plan``,
``spread_targets``; parallel/spread_g.py) and ``igg.autograd.sample_g`` built
on it; and the diffusion step
transposed (``ops.stencil.diffusion3d_adjoint_``), with the differentiable step
``igg.autograd.diffusion3d`` and the model's backward time loop
``Diffusion3D.adjoint_run``; and the acoustic step transposed
(``ops.stencil.acoustic2d_adjoint_``), with ``igg.autograd.acoustic2d`` and
``Acoustic2D.adjoint_run``.
"""
from ._native import IGGError, PROC_NULL, native, native_path  # noqa: F401
from .parallel.grid import (  # noqa: F401
    GlobalGrid,
    finalize_global_grid,
    get_global_grid,
    global_grid,
    grid_is_initialized,
    init_global_grid,
)
from .parallel.device import select_device  # noqa: F401
from .parallel.halo import update_halo, update_halo_  # noqa: F401
from .parallel.accumulate import accumulate_halo_  # noqa: F401
from . import autograd  # noqa: F401
from .parallel.transport_select import select_transport  # noqa: F401
from .parallel.gather import gather, gather_, gather_async_  # noqa: F401
from .parallel.gather_g import gather_g, indices_g, selection_shape_g  # noqa: F401
from .parallel.scatter_g import scatter_g, scatter_pieces  # noqa: F401
from .parallel.sample_g import Recorder, index_g, sample_g, sample_owner  # noqa: F401
from .parallel.spread_g import Source, SpreadPlan, spread_g, spread_plan, spread_targets  # noqa: F401
from .utils.tools import coords_g, nx_g, ny_g, nz_g, tic, toc, x_g, y_g, z_g  # noqa: F401
from .utils.checkpoint import load_checkpoint, save_checkpoint  # noqa: F401
from .ops.reduce import (  # noqa: F401
    dot_g,
    max_g,
    maxabs_diff_g,
    maxabs_g,
    mean_g,
    min_g,
    norm_diff_g,
    norm_g,
    owned_ranges,
    owned_view,
    project_g,
    reduce_g,
    sum_g,
)

__version__ = "0.1.0"

__all__ = [
    "init_global_grid", "finalize_global_grid", "update_halo_", "update_halo", "gather_", "gather",
    "select_device", "nx_g", "ny_g", "nz_g", "x_g", "y_g", "z_g", "tic", "toc", "get_global_grid",
    "IGGError", "coords_g", "gather_async_", "save_checkpoint", "load_checkpoint", "select_transport",
    "owned_ranges", "owned_view", "reduce_g", "sum_g", "max_g", "min_g", "maxabs_g", "dot_g", "maxabs_diff_g",
    "norm_g", "norm_diff_g", "mean_g", "project_g", "gather_g", "indices_g", "selection_shape_g",
    "scatter_g", "scatter_pieces", "accumulate_halo_", "autograd", "sample_g", "sample_owner", "index_g", "Recorder",
    "spread_g", "spread_plan", "spread_targets", "SpreadPlan", "Source",
]
