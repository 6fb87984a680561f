"""3-D heat diffusion with Gaussian-anomaly initial conditions (the benchmark).

Reference application: examples/diffusion3D_multigpu_CuArrays_novis.jl (and its
CPU twin diffusion3D_multicpu_novis.jl): lam=1, cp_min=1, l=10 per axis, two
Gaussian anomalies in Cp and two in T built from x_g/y_g/z_g,
dt = min(dx^2,dy^2,dz^2)*cp_min/lam/8.1, per step: stencil update of the
interior then ``update_halo!(T)``.

MI355X design of a time step (``overlap=True`` and at least one neighbour):

  halo stream (high priority): boundary slabs of T2 (the planes update_halo
      sends) -> update_halo_(T2)  [pack -> RCCL -> unpack, x->y->z]
  compute stream:              interior of T2 (everything else)
  join, swap T <-> T2.
  (With the RCCL transport the exchange stays on the issuing stream and the
  interior goes to the forked one: RCCL captured on a forked stream crashes
  hipGraph capture, benchmarks/rccl_capture_repro.py.)

Both read T only; they write disjoint parts of T2, so the exchange hides behind
the interior update. Without neighbours (1 GPU, non-periodic) the step is one
fused kernel and update_halo_ is a no-op, as in the reference.

``fused=True`` (GPU, at least one neighbour; csrc/include/igg/fused.hpp): the
stencil kernel itself stores the send planes into the neighbours' IPC-mapped
arenas over xGMI while it sweeps, and reads its face halos from its own arena;
a 1-wave sync kernel is the whole exchange. The fields' halo planes are then
stale until ``sync_halo()`` (update_halo_ of T), which ``run``/``capture``
callers invoke before reading halos (gather, output). Interior values are
bitwise identical to the update_halo_ path.
"""
from __future__ import annotations

import os
import warnings

import torch

from .. import parallel  # noqa: F401
from .._native import IGGError
from ..ops import stencil
from ..parallel import grid as _grid
from ..parallel.halo import update_halo_
from ..utils import placement as _placement
from ..utils.fields import carve as _carve, ipc_limit, native_buffer  # noqa: F401
from ..utils.tools import coords_g, nx_g, ny_g, nz_g
from ._pingpong import (GRAPH_STEPS, THREESTEP_GRAPH_STEPS, TWOSTEP_GRAPH_STEPS, PingPongModel,  # noqa: F401
                        exchanging_dims, faster_pass, grid_sides, peer_mesh, two_step_env)

# Candidates re-timed by the autotune's ping-pong stage (_choose_variant).
PINGPONG_FRONT = 4
# Whole-line z-edge stores of the full-box steps (ops.stencil.diffusion3d_
# halo_z; the fused step on its z sides without a neighbour): T2's z halo gets
# T's values, which is a no-op at fixed boundaries (T2 = T.clone() at init,
# neither is ever changed there) and is rewritten by the exchange elsewhere.
# 1024^3 f32 -5.5..-6.8 %, 512^3 f64 up to -2.9 % per variant
# (profiles/r4_halo_z/). IGG_HALO_Z=0 restores partial-line edge stores.
HALO_Z = os.environ.get("IGG_HALO_Z", "1").strip() != "0"


def _rccl_transport() -> bool:
    from ..parallel import halo as H

    return H.transport_name() == "rccl"


class Diffusion3D(PingPongModel):
    """3-D heat diffusion with variable heat capacity on the local grid of the
    implicit global grid (examples/diffusion3D_multigpu_CuArrays_novis.jl):
    ``T2 = T + dt*lam/Cp * laplace(T)`` by one fused HIP kernel, then
    ``update_halo_(T2)`` (or the fused exchange, ``set_fused``), ping-pong T/T2.
    ``step``/``run`` advance, ``capture`` records hipGraphs, ``save``/``restore``
    checkpoint.

    Two-step pass (``two_step``; IGG_STENCIL_TWOSTEP=auto|0|1): where nothing
    looks at the field between steps and no halo is needed in between -
    ``run``/``capture`` on a GPU model whose grid has a halo width of at least
    2 in every dimension that ``update_halo_`` exchanges (a neighbour, a
    periodic self-exchange, loopback; a grid without any is the trivial case),
    not fused, not overlapped, no timer - pairs of steps run as one kernel pass
    that reads T and Cp once and writes the field two steps later
    (ops.stencil.diffusion3d_twostep_; bitwise the values of two single
    steps), followed by ONE ``update_halo_`` of two planes per side.
    ``step``/``local_step`` stay single steps. ``variant`` names the
    single-step kernel: assigning another one than the selection ran with
    switches the pass off until the original is assigned back.

    Quotient array (``Q``; IGG_STENCIL_QUOTIENT=auto|0|1): the pass may read
    ``Q = dt*lam/Cp`` where it reads ``Cp`` and then does not divide (the same
    bytes per pass, bitwise the same values). ``Cp``, ``dt`` and ``lam`` are
    constant over a time loop, so the model owns one further array of the
    fields' size (1 GiB at 512^3 float64; never checkpointed), builds it when
    the pass is selected and rebuilds it in place at the entry of
    ``run``/``capture`` when ``Cp`` (its storage or torch's version counter),
    ``dt`` or ``lam`` changed; after a write to ``Cp`` that torch cannot see
    (a raw pointer, another process) call ``mark_cp_modified()``. ``auto``
    keeps it where the set-up A/B measures the pass faster with it.

    Three-step pass (``three_step``; IGG_STENCIL_THREESTEP=auto|0|1): where
    the two-step pass runs with ``Q`` on a grid that exchanges nothing (a rank
    without neighbours) and a row fits one kernel tile (512 float64 / 1024
    float32 points), ``run``/``capture`` advance three steps per kernel pass
    (ops.stencil.diffusion3d_threestep_; bitwise the values of three single
    steps) and leave what does not fill a pass to the two-step pass and the
    single step. ``auto`` is considered only while IGG_STENCIL_TWOSTEP is
    ``auto`` too, and keeps the pass where the set-up A/B measures it faster
    per step than the selected two-step pass (``three_step_times``); ``1``
    selects it without timing wherever it can run - the two-step pass with
    ``Q`` that it rests on included, unless that is forced off. Grids that
    exchange (a halo three planes deep) are out of its scope.

    ``T2`` is the other ping-pong buffer: its boundary planes always equal
    ``T``'s fixed boundary values; its interior is the field of one step ago
    after a single step, of TWO steps ago after a two-step pass and of THREE
    after a three-step pass (it is rewritten by whatever runs next either
    way)."""

    _fields = ("T", "T2", "Cp")

    def __init__(self, *, dtype=torch.float64, device=None, lam: float = 1.0, cp_min: float = 1.0,
                 lx: float = 10.0, ly: float = 10.0, lz: float = 10.0, overlap: bool = False,
                 slab_width=None, variant=None, halo_variant=None, interior_rounds: int = 0,
                 halo_rounds: int = 0, reserve_cus: int = 0, field_memory: str = None):
        super().__init__()
        gg = _grid.global_grid()
        nx, ny, nz = (int(v) for v in gg.nxyz)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if gg.amdgpu_enabled else torch.device("cpu")
        self.device = torch.device(device)
        self.dtype = dtype
        self.lam, self.cp_min = lam, cp_min
        self.dx = lx / (nx_g() - 1)
        self.dy = ly / (ny_g() - 1)
        self.dz = lz / (nz_g() - 1)
        self.dt = min(self.dx ** 2, self.dy ** 2, self.dz ** 2) * cp_min / lam / 8.1
        self._variant = variant
        # Two-step pass: whether the selection kept it, its tiling (ops.stencil
        # TWOSTEP_FORMS) and grid rounds, the A/B's ms per step ("single" and
        # "t<form>@r<rounds>"), and the variant the selection ran with.
        self._two_step = False
        self._two_step_variant = None
        self.two_step_form = 0
        self.two_step_rounds = 0
        self.two_step_times = {}
        # Three-step pass: whether the selection kept it (it stands and falls
        # with the two-step selection and its variant), its tiling (ops.stencil
        # THREESTEP_FORMS) and grid rounds, and the A/B's ms per step ("two"
        # and "d<form>@r<rounds>").
        self._three_step = False
        self.three_step_form = 0
        self.three_step_rounds = 0
        self.three_step_times = {}
        # The pass's quotient array dt*lam/Cp (None: the pass reads Cp) and
        # what it was built from (Cp's storage and version, dt*lam).
        self.Q = None
        self._q_key = None
        self.rounds = 0  # grid residency rounds of the full-interior launch (0: library default)
        self.halo_z = HALO_Z  # whole-line z-edge stores of the full-interior launch (autotuned per variant)
        self.variant_times = None  # per-variant ms when autotuned (see _choose_variant)
        self.timer = None  # optional utils.trace.PhaseTimer (eager steps only)
        # Overlap tuning knobs: kernel variant / grid rounds of the boundary
        # slabs and grid rounds of the interior launch (see ops.stencil).
        self.halo_variant = halo_variant
        self.interior_rounds = interior_rounds
        self.halo_rounds = halo_rounds
        self.interior_first = False
        shape = (nx, ny, nz)
        probe = torch.empty(shape, device="meta")  # sizes only, for coords_g
        kw = dict(dtype=torch.float64, device=self.device)
        x = coords_g(0, self.dx, probe, **kw).view(-1, 1, 1)
        y = coords_g(1, self.dy, probe, **kw).view(1, -1, 1)
        z = coords_g(2, self.dz, probe, **kw).view(1, 1, -1)
        # field_memory (IGG_FIELD_MEMORY): "fine" (default: one native
        # fine-grained allocation) or "torch" (coarse-grained, torch's caching
        # allocator). The direct-z fused exchange stores into the neighbours'
        # T/T2 while their kernels run, which HIP defines for fine-grained
        # memory only (docs/COHERENCE.md); the plain sweep runs as fast on it
        # (profiles/r3_coherence/: 0.6222 vs 0.6263 ms/step).
        # One allocation with gaps between the three arrays: measured 1-3 %
        # faster than back-to-back 2 MiB-aligned tensors on MI355X
        # (profiles/r2_offsets/stencil_offsets.py: HBM channel placement). The
        # fields are allocated first and the initial conditions written into
        # them (no full-size temporary copies).
        self.field_memory = (field_memory or os.environ.get("IGG_FIELD_MEMORY", "fine")).strip().lower()
        if self.field_memory not in ("torch", "fine", "vmm"):
            raise ValueError(f"Diffusion3D: field_memory must be 'torch', 'fine' or 'vmm', got {self.field_memory!r}")
        if self.device.type == "cuda":
            # With neighbours in other processes T/T2 may be IPC-mapped (direct
            # z, gather_ pull): no allocation may reach the IPC size limit, so
            # a carve that would is split into one allocation per array. An
            # array that alone reaches it (1024^3 f32: 4 GiB) can never be IPC
            # mapped; with "fine" it then lives in HIP VMM memory (MemKind 4,
            # csrc/vmm.cpp), which gather_ maps through a file descriptor at
            # any size instead of staging it in chunks (round 6).
            kinds = {"torch": None, "fine": 1, "vmm": 4}
            self._field_kind = kinds[self.field_memory]
            spec = [torch.empty(shape, dtype=dtype, device="meta")] * 3
            multi = int(gg.nprocs) > 1
            big = multi and spec[0].numel() * spec[0].element_size() >= ipc_limit()

            def carve():
                return _carve(spec, gap=266240, kind=kinds[self.field_memory],
                              split_at=ipc_limit() if multi else None, device=self.device,
                              split_kind=4 if (big and self.field_memory == "fine") else None)

            (self.T, self.Cp, self.T2), self.placement = _placed_fields(carve, gg, spec[0], self.device)
            self._ipc_fields = self.field_memory == "fine" and not big  # direct z can map T/T2
        else:
            self.T, self.Cp, self.T2 = (torch.empty(shape, dtype=dtype) for _ in range(3))
            self.placement = None
        # Gaussian anomalies, evaluated in float64 a slab of x planes at a time
        # into the target dtype: the float64 temporaries of the whole field
        # (several x 8 bytes per point) would otherwise be the memory peak of a
        # 1024^3 rank - 8 ranks sharing one GPU ran out of memory here - while
        # every value is the same elementwise expression as before.
        slab = max(1, (1 << 24) // max(1, ny * nz))
        for x0 in range(0, nx, slab):
            xs = x[x0:x0 + slab]
            self.Cp[x0:x0 + slab] = (cp_min + 5 * torch.exp(-(xs - lx / 1.5) ** 2 - (y - ly / 2) ** 2 - (z - lz / 1.5) ** 2)
                                     + 5 * torch.exp(-(xs - lx / 3.0) ** 2 - (y - ly / 2) ** 2 - (z - lz / 1.5) ** 2))
            self.T[x0:x0 + slab] = (100 * torch.exp(-((xs - lx / 2) / 2) ** 2 - ((y - ly / 2) / 2) ** 2
                                                    - ((z - lz / 3.0) / 2) ** 2)
                                    + 50 * torch.exp(-((xs - lx / 2) / 2) ** 2 - ((y - ly / 2) / 2) ** 2
                                                     - ((z - lz / 1.5) / 2) ** 2))
        if _wide_grid() and exchanging_dims(3):
            # On a periodic grid the analytic values of T and Cp in the halo
            # planes are not the images of the interior they overlap. A single
            # step reads only T's plane 0 of them and the exchange rewrites what
            # it computes there; the two-step pass computes its intermediate
            # plane 1 from T's and Cp's own planes 0 .. 2, which must then be
            # what the neighbour holds. So both forms start from exchanged halos
            # (collective, like the variant autotune below; between the ranks of
            # a non-periodic grid the values already agree).
            update_halo_(self.T, self.Cp)
        self.T2.copy_(self.T)
        self.sides = sides = grid_sides(3)
        # (the overlapped step's slabs and the fused exchange move one plane per side)
        self.can_overlap = self.device.type == "cuda" and any(any(sd) for sd in sides) and not _wide_grid()
        self.inner = [stencil.inner_box(shape)]
        z_split = any(sides[2])
        if overlap and self.can_overlap and z_split and self.variant is None:
            self.variant = 11  # 128-point tiles: z-slabs stay one full tile wide
        if self.variant is None and self.device.type == "cuda":
            self.variant = _choose_variant(self)
        if slab_width is None:
            # A slab at every side with a neighbour, just wide enough to hold
            # the plane update_halo sends there (index ol-1 / n-ol) along dims
            # 0/1; along the contiguous dim 2 (where a thin slab would waste
            # whole cache lines per row) it is exactly one kernel tile wide, so
            # both the slab launch and the interior launch run full tiles.
            o = [int(v) for v in gg.overlaps]
            tile = max(1, int(stencil.native.diffusion3d_variant_tile(self.variant or 0)))
            slab_width = (max(1, o[0] - 1), max(1, o[1] - 1), max(o[2] - 1, tile - 1))
        self.slabs, self.interior = stencil.split_boundary(shape, sides, slab_width)
        if self.halo_variant is None and not z_split:
            self.halo_variant = 18  # x/y boundary planes: the one-row scalar kernel is fastest
        self.compute_stream = None
        self.halo_stream = None
        self._reserve_cus = reserve_cus
        self.overlap = False
        if overlap:
            self.set_overlap(True)
        # Fused halo exchange (set_fused): native FusedHalo, step counter (arena
        # half parity), whether the arena holds the halos of the current T.
        self.fused = False
        # Fused kernel: variant (tiling; one with a fused instantiation) and
        # send mode (0 stores as computed, 1 deferred one x step; +2 compiles the
        # z-edge exchange out when there is no z neighbour; +4 direct z: the z
        # faces go straight into the neighbours' next T, no z receive code; +8
        # peel: x-chunk waves sweep only x = 1 / n0-2 with the x exchange,
        # profiles/r2_peel/).
        self.fused_variant = 0
        self.fused_mode = 8
        self.fused_rounds = 3  # grid residency rounds (profiles/r1_fused/grid.log)
        self._fh = None
        self._fstep = 0
        self._fprimed = False
        # Entry barrier before the next fused step (neighbours store into this
        # rank's arena and, with direct z, its fields: their stores must not
        # overtake this rank's own earlier writes - a switch into fused mode, a
        # restore, external edits: mark_modified).
        self._fentry = True
        # Receive form of the last fused step (send-mode bits 4 / 64 / 16): where
        # the primed halos live (arena, T's z halo column) and how the step
        # synchronises. A step in another form re-primes first (_align_form).
        self._fform = None
        self._graph_parity = 0  # step parity and T's buffer when the graph was captured
        self._graph_T = 0
        _select_two_step(self)

    @property
    def variant(self):
        """The single-step kernel variant (ops.stencil)."""
        return self._variant

    @variant.setter
    def variant(self, v) -> None:
        self._variant = v

    @property
    def two_step(self) -> bool:
        """The two-step pass is selected and ``variant`` is still the one it
        was selected against (whether a given ``run`` uses it: ``_two_step_now``)."""
        return self._two_step and self._variant == self._two_step_variant

    @two_step.setter
    def two_step(self, flag: bool) -> None:
        self._two_step = bool(flag)
        self._two_step_variant = self._variant

    def _two_step_now(self) -> bool:
        """Eligibility of the two-step pass right now: selected, GPU, the
        plain step (not fused, not overlapped, no phase timer), every
        dimension update_halo_ exchanges on the grid as it is now (neighbour,
        periodic self-exchange, loopback) has a halo at least two planes deep,
        and the kernel has a form for the shape."""
        if not self.two_step or self.device.type != "cuda":
            return False
        if self.fused or self.overlap or self.timer is not None:
            return False
        return _pass_halo_ok() and stencil.twostep_ok(self.T, self.two_step_form)

    def _pass_key(self):
        return (self.two_step_form, self.two_step_rounds, self.Q is not None)

    @property
    def three_step(self) -> bool:
        """The three-step pass is selected, and so is the two-step pass it
        rests on (``variant`` unchanged since the selection; whether a given
        ``run`` uses it: ``_deep_key``)."""
        return self._three_step and self.two_step

    @three_step.setter
    def three_step(self, flag: bool) -> None:
        self._three_step = bool(flag)

    def _deep_key(self):
        """The three-step pass's setting while ``run``/``capture`` may use it
        right now, else None: selected, the two-step pass eligible and reading
        ``Q``, nothing exchanged on the grid as it is now, and the kernel has
        a form for the shape."""
        if not self.three_step or self.Q is None or not self._two_step_now():
            return None
        if exchanging_dims(3) or not stencil.threestep_ok(self.T, self.three_step_form):
            return None
        return (self.three_step_form, self.three_step_rounds)

    def _deep_pass(self) -> None:
        """Three time steps in one pass (callers checked ``_deep_key``): no
        exchange follows, the grid has none."""
        stencil.diffusion3d_threestep_(self.T2, self.T, self.Cp, Q=self.Q, lam=self.lam, dt=self.dt, dx=self.dx,
                                       dy=self.dy, dz=self.dz, form=self.three_step_form,
                                       rounds=self.three_step_rounds, halo_z=HALO_Z)
        self._swap()
        self._warm = True

    def _alloc_q(self) -> None:
        """The quotient array, in the fields' kind of memory (not yet built)."""
        meta = torch.empty(self.T.shape, dtype=self.dtype, device="meta")
        (self.Q,) = _carve([meta], gap=0, kind=self._field_kind, device=self.device)
        self._q_key = None

    def _refresh_q(self) -> None:
        """Rebuild ``Q`` in place if what it was built from changed (the buffer
        stays, so a captured graph that reads it stays valid)."""
        if self.Q is None:
            return
        key = (self.Cp.data_ptr(), self.Cp._version, self.dt * self.lam)
        if key != self._q_key:
            stencil.quotient_(self.Q, self.Cp, lam=self.lam, dt=self.dt)
            self._q_key = key

    def mark_cp_modified(self) -> None:
        """``Cp`` was written behind torch's back (a raw pointer, a kernel of
        another library): the next ``run``/``capture`` rebuilds ``Q``."""
        self._q_key = None

    def run(self, nt: int) -> None:
        self._refresh_q()
        super().run(nt)

    def capture(self, steps: int = None) -> None:
        self._refresh_q()
        super().capture(steps)

    run.__doc__ = PingPongModel.run.__doc__
    capture.__doc__ = PingPongModel.capture.__doc__

    def _q_current(self) -> bool:
        """``Q`` exists and was built from ``Cp``, ``dt`` and ``lam`` as they are."""
        return self.Q is not None and self._q_key == (self.Cp.data_ptr(), self.Cp._version, self.dt * self.lam)

    def adjoint_run(self, nt: int, g, out=None):
        """The transpose of ``run(nt)`` applied to ``g``: the gradient of
        ``<g, T after nt steps>`` with respect to the LOCAL array ``T`` that
        the steps started from.

        ``g`` has the shape, dtype and device of ``T`` and is not modified;
        the result is a new tensor, or ``out``. A step of the model is
        ``T <- H(S(T))`` - the stencil update ``S``, then ``update_halo_``
        (``H``) - so each of the ``nt`` adjoint steps is
        ``accumulate_halo_(g)`` (``Hᵀ``) followed by ``g' = Sᵀ g``
        (``ops.stencil.diffusion3d_adjoint_``), on two ping-pong buffers. ``S``
        is linear in ``T``: no forward state is stored or needed. ``run``
        leaves bitwise the values of single steps whichever pass it took, so
        this is the adjoint of ``run(nt)`` on every grid the model accepts. It
        uses the model's ``lam``, ``dt``, spacings and ``Cp``, and ``Q`` where
        the model keeps one that is current; it touches neither ``T`` and
        ``T2`` nor a captured graph. Collective like ``run``; it raises where
        ``accumulate_halo_`` would (a field with ``n < overlap + halowidth``
        in an exchanging dimension).

        The result is the gradient with respect to the LOCAL array: halo cells
        hold the part that belongs to the cell's owner on another rank. Where
        ``overlap == 2*halowidth`` in every exchanging dimension (the default
        grid), every cell a rank does not own is a halo cell, and one more
        ``accumulate_halo_(result)`` leaves the gradient with respect to the
        GLOBAL initial field in the owned cells (``gather_g`` assembles it).
        Wider overlaps need the transpose of ``scatter_g`` for that."""
        from ..parallel.accumulate import accumulate_halo_, check_accumulate

        nt = int(nt)
        if nt < 0:
            raise IGGError("adjoint_run: nt must be >= 0")
        for name, A in (("g", g), ("out", out)):
            if A is None:
                continue
            if not isinstance(A, torch.Tensor) or A.shape != self.T.shape or A.dtype != self.T.dtype \
                    or A.device != self.T.device:
                raise IGGError(f"adjoint_run: {name} must have T's shape {tuple(self.T.shape)}, dtype {self.T.dtype} "
                               f"and device {self.T.device}")
            if not A.is_contiguous():
                raise IGGError(f"adjoint_run: {name} must be C-contiguous")
        check_accumulate(g)
        if out is None:
            a = g.clone(memory_format=torch.contiguous_format)
        else:
            a = out
            if out.data_ptr() != g.data_ptr():
                out.copy_(g)
        if nt == 0:
            return a
        b = torch.empty_like(a)
        Q = self.Q if self._q_current() else None
        for _ in range(nt):
            accumulate_halo_(a)
            stencil.diffusion3d_adjoint_(b, a, self.Cp, Q=Q, lam=self.lam, dt=self.dt, dx=self.dx, dy=self.dy,
                                         dz=self.dz)
            a, b = b, a
        if out is not None and a is not out:
            out.copy_(a)
            return out
        return a

    def _swap(self) -> None:
        self.T, self.T2 = self.T2, self.T

    def residual(self) -> torch.Tensor:
        """``max|T - T2|`` over the global grid as a device scalar
        (``maxabs_diff_g``): right after a single ``step()`` the largest change
        of the step. It reads owned cells only, none of them a halo plane, so
        it is valid in fused mode without ``sync_halo()``. (After ``run`` the
        last pass may have been a two-step or three-step pass and ``T2`` two
        or three steps old: take one ``step()`` first, as ``run_until`` does.)"""
        from ..ops.reduce import maxabs_diff_g

        return maxabs_diff_g(self.T, self.T2)

    _residual = residual

    def _pass(self) -> None:
        """Two time steps in one pass (callers checked ``_two_step_now``), then
        the exchange of the two halo planes per side the next pass reads. The
        pass leaves planes 2 .. n-3 exact (the intermediate field's boundary
        planes keep T's values), which includes the send planes [2, 4) and
        [n-4, n-2); planes 0, 1, n-2, n-1 are what the exchange overwrites
        (next to a physical boundary plane 0 is fixed, so plane 1 is exact)."""
        stencil.diffusion3d_twostep_(self.T2, self.T, self.Cp, lam=self.lam, dt=self.dt, dx=self.dx, dy=self.dy,
                                     dz=self.dz, form=self.two_step_form, rounds=self.two_step_rounds,
                                     halo_z=HALO_Z, Q=self.Q)
        if exchanging_dims(3):
            update_halo_(self.T2)
        self._swap()
        self._warm = True

    @property
    def can_fuse(self) -> bool:
        """Fused halo exchange possible: GPU, a neighbour, overlap 2 where split,
        n2 a multiple of 4 (vector kernels)."""
        gg = _grid.global_grid()
        if self.device.type != "cuda" or not any(any(sd) for sd in self.sides) or _wide_grid():
            return False
        if any(any(self.sides[d]) and int(gg.overlaps[d]) != 2 for d in range(3)):
            return False
        if gg.nprocs > 1 and not gg.comm.one_node:  # IPC peer mappings: one node only
            return False
        return int(self.T.shape[2]) % 4 == 0 and int(self.T.shape[2]) >= 8

    def fused_available(self) -> bool:
        """Whether ``set_fused(True)`` would switch the fused exchange on (never
        on a grid with a halo width above 1: it moves one plane per side)."""
        return self.can_fuse

    def set_fused(self, flag: bool) -> bool:
        """Switch the fused halo exchange on/off (collective: every rank at the
        same point; the first switch-on creates the peer mesh). Switching off
        materialises the halos first. Returns the mode."""
        flag = bool(flag) and self.can_fuse
        if flag == self.fused:
            return flag
        if flag:
            if self._fh is None:
                mesh, nb = peer_mesh(3)
                self._fh = stencil.native.FusedHalo(mesh, list(self.T.shape), self.T.element_size(), nb)
                # Direct z sends (fused_mode bit 4) write into the neighbours'
                # T/T2 while their kernels run: defined for fine-grained fields
                # (docs/COHERENCE.md); torch-allocated fields only on one GPU.
                if getattr(self, "_ipc_fields", False) or _grid.global_grid().nprocs == 1:
                    try:
                        self._fh.set_fields(self.T.data_ptr(), self.T2.data_ptr())
                    except Exception as e:  # collective outcome: every rank gets here together
                        warnings.warn(f"Diffusion3D: direct z sends unavailable ({e})")
            if self.fused_mode & 4 and not self._fh.has_fields:
                self.fused_mode &= ~4
            if not stencil.native.diffusion3d_fused_variant_ok(int(self.fused_variant)):
                self.fused_variant = 0
            self.set_overlap(False)
            self._fprimed = False  # the field's halo planes are valid right now
            self._fentry = True
        else:
            self.sync_halo()
        self.fused = flag
        self.graph = None
        return flag

    def sync_halo(self) -> None:
        """Materialise the halo planes of T (fused mode leaves them stale):
        one update_halo_(T). Later fused steps read halos from T again."""
        if self.fused and self._fprimed:
            update_halo_(self.T)
            self._fprimed = False

    def mark_modified(self) -> None:
        """Declare that T/T2 were written outside the time loop: the next fused
        step first synchronises with the neighbours (collective) and reads its
        halos from T."""
        self._fprimed = False
        self._fentry = True

    def exchange_halos(self) -> None:
        """Make T's halo planes equal the neighbours' (update_halo_(T);
        collective) and mark the fields modified: after ``local_step`` calls
        the state is again one the time loop could have produced."""
        update_halo_(self.T)
        self.mark_modified()

    def close(self) -> None:
        """Release the fused exchange's peer mesh (collective: every rank)."""
        if self._fh is not None:
            if self.fused:
                self.sync_halo()
                self.fused = False
            torch.cuda.synchronize()
            self._fh.close()
            self._fh = None
            self.graph = None

    def set_overlap(self, flag: bool) -> bool:
        """Switch between the serial step and the boundary/interior overlapped
        step (needs a GPU model with at least one neighbour); returns the mode."""
        flag = bool(flag) and self.can_overlap
        if flag and self.halo_stream is None:
            if self._reserve_cus > 0:
                from ..utils.streams import cu_partition

                self.compute_stream, self.halo_stream = cu_partition(self._reserve_cus)
            else:
                _least, greatest = torch.cuda.Stream.priority_range()
                self.halo_stream = torch.cuda.Stream(device=self.device, priority=greatest)
        if flag != self.overlap:
            self.graph = None  # a captured schedule no longer matches
        self.overlap = flag
        return flag

    def _overlap_streams(self) -> int:
        """Concurrent streams of the overlapped step: the issuing stream and
        the forked halo stream, plus the CU-masked compute stream of
        ``reserve_cus`` on the put path (RCCL path: one side stream)."""
        if _rccl_transport():
            return 2
        return 3 if self.compute_stream is not None else 2

    def _kw(self, variant=None, rounds=None):
        return dict(lam=self.lam, dt=self.dt, dx=self.dx, dy=self.dy, dz=self.dz,
                    variant=self.variant if variant is None else variant,
                    rounds=self.rounds if rounds is None else rounds)

    @property
    def _fused_handle(self):
        return self._fh

    def _fused_step_mode(self) -> int:
        # direct z (bit 4) needs the registered field buffers; where they
        # could not be mapped (fields above the IPC limit) the same form runs
        # with the arena z exchange
        return self.fused_mode if self._fh.has_fields else self.fused_mode & ~4

    def _align_form(self) -> None:
        """Before a fused step: if the send mode's receive form changed since
        the last primed step, re-prime. A primed step reads its halos where the
        previous form's senders put them: the arena (arena z), T's z halo
        column (direct z, bit 4; z unpack, bit 64, written by the previous
        step's unpack copy) - a step of another form would read halos nobody
        wrote (switching 8 -> 72 read a stale z column). So the
        halos are materialised (update_halo_(T), collective: mode switches are
        collective) and the next step reads them from T behind an entry
        barrier (bit 16 changes how the neighbours' arrivals are counted)."""
        form = self._fused_step_mode() & (4 | 16 | 64)
        if self._fprimed and self._fform is not None and form != self._fform:
            self.sync_halo()
            self._fentry = True
        self._fform = form

    def _step(self) -> None:
        T, T2, Cp = self.T, self.T2, self.Cp
        if self.fused:
            rd2 = [1.0 / self.dx ** 2, 1.0 / self.dy ** 2, 1.0 / self.dz ** 2]
            s = torch.cuda.current_stream().cuda_stream
            self._align_form()  # (sync_halo leaves the buffer roles in place)
            mode = self._fused_step_mode()
            if self.timer is not None:
                with self.timer.phase("stencil+exchange"):
                    self._fh.step(T2.data_ptr(), T.data_ptr(), Cp.data_ptr(), rd2, self.dt * self.lam,
                                  self.fused_variant, self._fstep, self._fprimed, s, self.fused_rounds,
                                  mode, self._fentry, HALO_Z)
            else:
                self._fh.step(T2.data_ptr(), T.data_ptr(), Cp.data_ptr(), rd2, self.dt * self.lam,
                              self.fused_variant, self._fstep, self._fprimed, s, self.fused_rounds,
                              mode, self._fentry, HALO_Z)
            self._fentry = False
            self._fstep += 1
            self._fprimed = True
        elif self.overlap and _serial_overlap(self._overlap_streams()):
            # Fewer hardware queues per process than concurrent streams in the
            # overlapped step (GPU_MAX_HW_QUEUES=1, e.g. many ranks sharing a
            # GPU): the streams cannot all run concurrently, and a hipGraph
            # captured with the forked exchange crashed in replay with one
            # queue (profiles/r4_overlap_crash/). Same three parts in stream
            # order - identical results (disjoint writes), nothing lost.
            stencil.diffusion3d_(T2, T, Cp, boxes=self.slabs, **self._kw(self.halo_variant, self.halo_rounds))
            update_halo_(T2)
            stencil.diffusion3d_(T2, T, Cp, boxes=[self.interior], **self._kw(None, self.interior_rounds))
        elif self.overlap:
            # 1. boundary slabs on the compute stream (full bandwidth, nothing
            #    else running), 2. the halo exchange of T2 on the high-priority
            #    stream after an event, 3. the interior concurrently on the
            #    compute stream; slabs/interior/halo planes are disjoint.
            main = torch.cuda.current_stream()
            hs = self.halo_stream
            cs = self.compute_stream or main
            stencil.diffusion3d_(T2, T, Cp, boxes=self.slabs, **self._kw(self.halo_variant, self.halo_rounds))
            if _rccl_transport():
                # RCCL's p2p group must run on the stream the step was issued
                # on: captured on a stream forked from the capture origin it
                # crashes hipGraph capture (RCCL 2.26, SIGSEGV at the end of
                # the capture); on the origin, with the interior on a forked
                # stream running concurrently, it captures and replays
                # (benchmarks/rccl_capture_repro.py, profiles/r2_rccl_capture/).
                # So the roles swap: interior on the side stream, exchange here.
                side = cs if cs is not main else hs
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    stencil.diffusion3d_(T2, T, Cp, boxes=[self.interior], **self._kw(None, self.interior_rounds))
                update_halo_(T2)
                main.wait_stream(side)
            else:
                hs.wait_stream(main)
                if cs is not main:
                    cs.wait_stream(main)
                with torch.cuda.stream(hs):
                    update_halo_(T2)
                with torch.cuda.stream(cs):
                    stencil.diffusion3d_(T2, T, Cp, boxes=[self.interior], **self._kw(None, self.interior_rounds))
                main.wait_stream(hs)
                if cs is not main:
                    main.wait_stream(cs)
        elif self.timer is not None:
            with self.timer.phase("stencil"):
                stencil.diffusion3d_(T2, T, Cp, boxes=self.inner, halo_z=self.halo_z, **self._kw())
            with self.timer.phase("update_halo"):
                update_halo_(T2)
        else:
            # halo_z: T2's z halo gets T's values (whole-line z-edge stores):
            # at a physical boundary both hold the same fixed values, and
            # update_halo_(T2) right after rewrites every exchanged one
            stencil.diffusion3d_(T2, T, Cp, boxes=self.inner, halo_z=self.halo_z, **self._kw())
            update_halo_(T2)
        self._swap()
        self._warm = True

    def local_step(self) -> None:
        """One step of the LOCAL problem: what a rank without neighbours runs
        (the N = 1 run of the weak-scaling curve): the plain stencil with this
        model's variant, grid rounds and z-edge store form on the whole
        interior; update_halo_ with PROC_NULL neighbours is a no-op
        (reference: src/update_halo.jl:40-42, no neighbour -> nothing sent).
        Used by the bench's same-process efficiency E = t(local) / t(step).
        Leaves the halo planes unexchanged: timing only (callers that go on
        with real steps call ``exchange_halos`` afterwards)."""
        stencil.diffusion3d_(self.T2, self.T, self.Cp, boxes=self.inner, halo_z=self.halo_z, **self._kw())
        self._swap()

    def _capture_start(self) -> None:
        if not self._warm:
            self.step()
        if self.fused:
            self._align_form()  # no re-priming inside the capture
        if self.fused and not self._fprimed:
            self.step()  # captured fused steps read the arena: it must hold T's halos
        # The captured steps have their buffer roles baked in (T of the
        # capture is read first) and, fused, their arena halves too: they
        # assume a primed arena, no pending entry barrier and the step-counter
        # parity of the capture (an even number of steps: as it is now).
        self._graph_parity = self._fstep % 2
        self._graph_T = self.T.data_ptr()

    def _capture_cfg(self):
        """Fused mode and the fused kernel form a captured graph bakes in (a
        graph of another form is not replayed: the steps run eagerly until the
        next capture)."""
        return (self.fused_variant, self.fused_mode, self.fused_rounds) if self.fused else None

    def _replayed(self, k: int) -> None:
        if self.fused:
            self._fstep += k

    def _graph_ready(self) -> bool:
        if self.T.data_ptr() != self._graph_T:
            return False
        if self.fused:
            return self._fstep % 2 == self._graph_parity and self._fprimed and not self._fentry
        return True

    @property
    def a_eff_bytes(self) -> int:
        """A_eff = (2*D_u + D_k) * n_local * sizeof(T) with D_u = D_k = 1."""
        return 3 * self.T.numel() * self.T.element_size()


def _pass_halo_ok() -> bool:
    """The halo is deep enough for the two-step pass: at least two planes in
    every exchanging dimension (a dimension exchanges on every rank or on
    none, so all ranks agree)."""
    gg = _grid.global_grid()
    return all(int(gg.halowidths[d]) >= 2 for d in exchanging_dims(3))


def _wide_grid() -> bool:
    return any(int(w) > 1 for w in _grid.global_grid().halowidths)


def _select_two_step(m: "Diffusion3D") -> None:
    """Decide the two-step pass for this model (IGG_STENCIL_TWOSTEP): 0 off,
    1 on where eligible (form 0, library grid), auto (default): the chosen
    single-step kernel against every two-step form x GRID_ROUNDS in the time
    loop's ping-pong shape; the pass is kept only if its time PER STEP is
    below the single-step kernel's. On a grid that exchanges, a single step is
    kernel + update_halo_ and a pass is kernel + ONE update_halo_ for two
    steps; the times are summed over the ranks (every rank must make the same
    choice: one that exchanged every step would mismatch one that exchanges
    every two), and the timing itself is collective.

    The three-step pass (IGG_STENCIL_THREESTEP) is decided here as well, on
    top of a two-step pass that reads Q on a grid without exchange: 0 off, 1
    on wherever a form runs the shape, without any timing - the two-step
    selection is then made as with 1, and with Q, unless either is forced to
    0 -, auto: considered only while IGG_STENCIL_TWOSTEP is auto too
    (_select_three_step)."""
    env = two_step_env("IGG_STENCIL_TWOSTEP")
    qenv = two_step_env("IGG_STENCIL_QUOTIENT")
    denv = two_step_env("IGG_STENCIL_THREESTEP")
    m.two_step = False
    m.three_step = False
    m.Q = None
    if env == "0" or m.device.type != "cuda" or m.variant is None or not _pass_halo_ok():
        return
    forms = [f for f in stencil.TWOSTEP_FORMS if stencil.twostep_ok(m.T, f)]
    if not forms:
        return
    deep = [] if denv == "0" or qenv == "0" or exchanging_dims(3) else \
        [f for f in stencil.THREESTEP_FORMS if stencil.threestep_ok(m.T, f)]
    auto = env == "auto"
    if denv == "1" and deep:
        env = "1"
    if qenv != "0":
        # One more array of the fields' size; "auto" goes on without it where
        # it does not fit, "1" raises.
        try:
            m._alloc_q()
            m._refresh_q()
        except (RuntimeError, IGGError):
            m.Q = None
            if qenv == "1":
                raise
        gg = _grid.global_grid()
        if gg.nprocs > 1 and exchanging_dims(3):
            # the A/B below is collective over the same candidates: all ranks with Q or none
            import torch.distributed as dist

            have = torch.tensor([int(m.Q is not None)])
            dist.all_reduce(have, op=dist.ReduceOp.MIN, group=gg.comm.gloo)
            if not int(have[0]):
                m.Q = None
    if env == "1":
        m.two_step_form, m.two_step_rounds = forms[0], 0
        m.two_step = True
        if denv == "1" and deep and m.Q is not None:
            m.three_step_form, m.three_step_rounds = deep[0], 0
            m.three_step = True
        return
    rd2 = [1.0 / m.dx ** 2, 1.0 / m.dy ** 2, 1.0 / m.dz ** 2]
    boxes = [(list(b[0]), list(b[1])) for b in m.inner]
    # every pass candidate reading Cp and reading Q ("1": Q only), so that Q's
    # placement in memory is part of what is measured
    qs = [q for q in (False, True) if (q and m.Q is not None) or (not q and not (qenv == "1" and m.Q is not None))]
    cands = [(f, r, HALO_Z, q) for f in forms for r in stencil.GRID_ROUNDS for q in qs]
    exchanging = bool(exchanging_dims(3))
    single, t = stencil.time_twostep_pingpong(m.T2, m.T, m.Cp, rd2, m.dt * m.lam, boxes,
                                              (int(m.variant), int(m.rounds), bool(m.halo_z)), cands,
                                              exchange=update_halo_ if exchanging else None, Q=m.Q)
    gg = _grid.global_grid()
    if exchanging and gg.nprocs > 1:
        import torch.distributed as dist

        tot = torch.tensor([single] + [t[c] for c in cands], dtype=torch.float64)
        dist.all_reduce(tot, group=gg.comm.gloo)
        tot /= int(gg.nprocs)
        single, t = float(tot[0]), {c: float(x) for c, x in zip(cands, tot[1:])}
    best = faster_pass(m, single, t, lambda c: f"t{c[0]}{'q' if c[3] else ''}@r{c[1]}")
    if best is not None:
        m.two_step_form, m.two_step_rounds = int(best[0]), int(best[1])
        m.two_step = True
    if best is None or not best[3]:
        m.Q = None  # lost the A/B: the array is freed
    elif denv == "auto" and auto and deep:
        _select_three_step(m, rd2, best, deep)


def _select_three_step(m: "Diffusion3D", rd2, two, forms) -> None:
    """The A/B of the three-step pass: the selected two-step candidate ``two``
    (it reads Q) against every three-step form x GRID_ROUNDS, interleaved, in
    the time loop's ping-pong shape; the pass is kept only if its time PER
    STEP is below the two-step pass's. The ms per step go into
    ``m.three_step_times`` ("two" and "d<form>@r<rounds>"). No exchange and
    one rank's choice: the pass is considered only on a grid without any."""
    cands = [(f, r, HALO_Z) for f in forms for r in stencil.GRID_ROUNDS]
    t2, t = stencil.time_threestep_pingpong(m.T2, m.T, m.Cp, rd2, m.dt * m.lam, two[:3], cands, m.Q)
    m.three_step_times = {"two": round(t2, 5)}
    m.three_step_times.update({f"d{c[0]}@r{c[1]}": round(x, 5) for c, x in t.items()})
    best = min(t, key=t.get)
    if t[best] < t2:
        m.three_step_form, m.three_step_rounds = int(best[0]), int(best[1])
        m.three_step = True


def _hw_queues() -> int | None:
    """Hardware queues per process of the HIP runtime (GPU_MAX_HW_QUEUES,
    parsed as an integer: ' 01' is 1); None = the runtime's default (4)."""
    v = os.environ.get("GPU_MAX_HW_QUEUES", "").strip()
    try:
        return int(v) if v else None
    except ValueError:
        return None


def _serial_overlap(streams: int) -> bool:
    """Run the overlapped step's parts in stream order when the process has
    fewer hardware queues than the step has concurrent streams: they could
    not run concurrently anyway, and a captured fork in a one-queue process
    crashed the runtime's graph replay (profiles/r4_overlap_crash/: 2 side
    streams at GPU_MAX_HW_QUEUES=1; the full cell table is in its NOTES)."""
    q = _hw_queues()
    return q is not None and q < streams


def _placed_fields(carve, gg, meta: torch.Tensor, device):
    """(T, Cp, T2) from ``carve()``, the fastest of several candidate carves
    (utils/placement.py), and the probe's record (None without a probe)."""
    nbytes = meta.numel() * meta.element_size()
    k = _placement.candidate_count(gg, nbytes, 3 * nbytes, device)
    return _placement.placed(carve, k, lambda cands: _time_placements(cands, meta.dtype))


def _time_placements(cands, dtype, v=None, rounds: int = 3, halo_z: bool = False, steps: int = 6) -> list:
    """Median ms per ping-pong step of each (T, Cp, T2) candidate with a fixed
    plain variant (43 f64 / 14 f32 without whole-line z stores: separates fast
    from slow carves by 4.5-5 %, benchmarks/placement_probe.py). Values: T = 0,
    Cp = 1 (the model writes its initial conditions afterwards)."""
    if v is None:
        v = 43 if dtype == torch.float64 else 14
    if not stencil.native.diffusion3d_variant_compiled(v):
        v = stencil.compiled_variants()[0]
    for T, Cp, T2 in cands:
        T.zero_()
        T2.zero_()
        Cp.fill_(1)
    shape = list(cands[0][0].shape)
    boxes = [(list(b[0]), list(b[1])) for b in [stencil.inner_box(shape)]]
    s = torch.cuda.current_stream()
    es = cands[0][0].element_size()

    def launch(c, j):
        T, Cp, T2 = c
        dst, src = (T2, T) if j % 2 == 0 else (T, T2)
        stencil.native.diffusion3d(dst.data_ptr(), src.data_ptr(), Cp.data_ptr(), shape, [1.0, 1.0, 1.0], 1e-3,
                                   es, boxes, True, v, s.cuda_stream, rounds, halo_z)

    return _placement.time_candidates(cands, launch, steps=steps)


def _choose_variant(m: "Diffusion3D") -> int:
    """Kernel variant for this model: IGG_STENCIL_VARIANT if it is an integer,
    else the fastest of the shortlist timed on the model's own arrays, summed
    over all ranks so every rank runs the same kernel."""
    env = os.environ.get("IGG_STENCIL_VARIANT", "auto").strip().lower()
    if env != "auto":
        return int(env)
    rd2 = [1.0 / m.dx ** 2, 1.0 / m.dy ** 2, 1.0 / m.dz ** 2]
    boxes = [(list(b[0]), list(b[1])) for b in m.inner]
    gg = _grid.global_grid()

    def summed(t: dict):
        cands = sorted(t)
        tot = torch.tensor([t[c] for c in cands], dtype=torch.float64)
        if gg.nprocs > 1:
            import torch.distributed as dist

            dist.all_reduce(tot, group=gg.comm.gloo)
        return cands, tot

    # Stage 1: every (variant, rounds, z-edge store form) on fixed buffers
    # (T2 = f(T), cheap). The whole-line form (halo_z) wins for most tilings
    # and costs tiling 11 2.7 % (profiles/r4_halo_z/), so both are timed.
    forms = (True, False) if HALO_Z else (False,)
    t = stencil.time_variants(m.T2, m.T, m.Cp, rd2, m.dt * m.lam, boxes,
                              [(v, r, hz) for v in stencil.SHORTLIST for r in stencil.GRID_ROUNDS for hz in forms])
    cands, tot = summed(t)

    def key(v, r, hz):
        return f"{v}@r{r}" + ("/hz" if hz else "")

    m.variant_times = {key(*c): round(float(x) / max(1, int(gg.nprocs)), 5) for c, x in zip(cands, tot)}
    # Stage 2: the stage-1 front again, in the time loop's ping-pong shape and
    # with more launches: the minimum over ~44 noisy fixed-buffer timings is
    # biased low and the alternating buffers cost ~1 % (profiles/r2_gap/), so
    # the pick is made on what the run actually does.
    front = [cands[i] for i in torch.argsort(tot)[:PINGPONG_FRONT].tolist()]
    # 5 interleaved rounds of 20 steps, medians: the front differs by less
    # than the box noise of one sample (the round-4 picks varied run to run)
    t2 = stencil.time_variants_pingpong(m.T2, m.T, m.Cp, rd2, m.dt * m.lam, boxes, front, steps=20, rounds=5)
    cands2, tot2 = summed(t2)
    m.variant_times.update({key(*c) + "/pp": round(float(x) / max(1, int(gg.nprocs)), 5)
                            for c, x in zip(cands2, tot2)})
    v, r, hz = cands2[int(torch.argmin(tot2))]
    m.rounds = int(r)
    m.halo_z = bool(hz)
    return int(v)


def t_eff_gbs(model: Diffusion3D, t_it: float) -> float:
    return model.a_eff_bytes / t_it / 1e9


def run_diffusion3d(nx=128, ny=128, nz=128, nt=100, **kw):
    """Example driver mirroring diffusion3D_multicpu_novis.jl / _multigpu_ (novis)."""
    from ..parallel.grid import finalize_global_grid, init_global_grid
    from ..utils.tools import tic, toc

    init_global_grid(nx, ny, nz, quiet=kw.pop("quiet", False))
    m = Diffusion3D(**kw)
    tic()
    m.run(nt)
    t = toc()
    finalize_global_grid()
    return m, t
