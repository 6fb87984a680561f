"""2-D acoustic waves on a staggered grid: the staggered-field application.

BASELINE.json config "2-D staggered-grid solver 8192^2/GPU Float32 on 4
MI355X, 2x2 topology (staggered halo widths + mixed overlaps)". The reference
library has no such example; it is the canonical use of its staggered-array
support (fields one cell larger than the grid, ``ol(dim, A) = overlap +
size(A, dim) - n``: src/shared.jl:94, tools ``nx_g(A)``/``x_g(ix, dx, A)``:
src/tools.jl:3-107), as in ParallelStencil's acoustic examples.

Fields: P (nx, ny) at cell centres, Vx (nx+1, ny) on x-faces, Vy (nx, ny+1) on
y-faces. One time step = ONE fused HIP kernel (csrc/kernels/acoustic_kernels.hip:
P2 everywhere, then Vx2/Vy2 on inner faces from P2 recomputed in registers)
followed by ``update_halo_(Vx2, Vy2)`` (ol = 3 along the staggered dimension,
2 along the other: mixed overlaps in one call) and a buffer swap.

``set_fused(True)`` (GPU, a neighbour, overlap 2): the exchange moves into the
sweep (csrc/include/igg/acoustic.hpp FusedAcoustic): the kernel stores the
staggered boundary faces straight into the neighbours' next Vx2/Vy2 over xGMI
and one 1-wave sync kernel completes the step; every other halo value is
recomputed locally with the same arithmetic, so the fields are bitwise equal to
the update_halo_ path (tests/test_acoustic.py) - the communication is hidden
inside the HBM-bound sweep instead of following it.

Two-step pass (``two_step``; IGG_ACOUSTIC_TWOSTEP=auto|0|1): on a rank without
neighbours nobody looks at the fields between two steps (``update_halo_`` is a
no-op there), so ``run``/``capture`` advance pairs of steps with one kernel pass
(csrc/kernels/acoustic2_kernels.hip) that reads P, Vx, Vy once and writes the
fields two steps later, bitwise equal to two single steps.
"""
from __future__ import annotations

import math
import os

import torch

from .. import parallel  # noqa: F401
from .._native import IGGError, native
from ..ops import stencil as _stencil
from ..parallel import grid as _grid
from ..parallel.halo import update_halo_
from ..utils import placement as _placement
from ..utils.fields import carve, ipc_limit
from ..utils.tools import coords_g, nx_g, ny_g
from ._pingpong import PingPongModel, exchanging_dims, faster_pass, peer_mesh, two_step_env

# Chunk sizes (rows of x written per wave) the selection times the two-step
# pass with. A chunk re-reads two rows of lead-in (2/chunk more input), a
# short one puts more waves in flight: 4 .. 12 lie within a few per cent of
# each other at 8192^2 f32 and 4096^2 f64, 1 .. 2 and 64+ are slower
# (profiles/acoustic_twostep/NOTES.md).
TWOSTEP_CHUNKS = (4, 8, 12, 16, 32)


class Acoustic2D(PingPongModel):
    """2-D staggered acoustic wave propagation (pressure P at cell centres,
    velocities Vx/Vy on staggered faces: nx+1 / ny+1) with one fused HIP kernel
    per step and one ``update_halo_(Vx2, Vy2)`` (mixed overlaps); the 2-D
    staggered config of BASELINE.json.

    Two-step pass (``two_step``; IGG_ACOUSTIC_TWOSTEP=auto|0|1): in ``run`` and
    ``capture`` of a GPU model on a grid without any neighbour (no other rank,
    no periodic self-exchange, no loopback), not fused, pairs of steps run as
    one kernel pass that reads P, Vx, Vy once and writes the fields two steps
    later (ops.stencil.acoustic2d_twostep_; bitwise the values of two single
    steps). ``auto`` (default) times the single-step kernel against the pass
    with the chunks of ``TWOSTEP_CHUNKS`` on the model's own buffers and keeps
    the pass only if its time per step is lower (``two_step_times``,
    ``two_step_chunk``). ``step``/``local_step`` stay single steps.

    ``P2``/``Vx2``/``Vy2`` are the other ping-pong buffers: the state of one
    step ago after a single step and of TWO steps ago after a two-step pass
    (whatever runs next rewrites them either way)."""

    _fields = ("P", "Vx", "Vy", "P2", "Vx2", "Vy2")

    def __init__(self, *, dtype=torch.float32, device=None, K: float = 1.0, rho: float = 1.0,
                 lx: float = 10.0, ly: float = 10.0):
        super().__init__()
        gg = _grid.global_grid()
        nx, ny = int(gg.nxyz[0]), int(gg.nxyz[1])
        if int(gg.nxyz[2]) != 1:
            raise ValueError("Acoustic2D needs a 2-D grid (init_global_grid(nx, ny, 1))")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if gg.amdgpu_enabled else torch.device("cpu")
        self.device = torch.device(device)
        self.dtype = dtype
        self.nx, self.ny = nx, ny
        self.K, self.rho = K, rho
        self.dx = lx / (nx_g() - 1)
        self.dy = ly / (ny_g() - 1)
        self.dt = min(self.dx, self.dy) / math.sqrt(K / rho) / 4.1
        probe = torch.empty((nx, ny), device="meta")
        kw = dict(dtype=torch.float64, device=self.device)
        x = coords_g(0, self.dx, probe, **kw).view(-1, 1)
        y = coords_g(1, self.dy, probe, **kw).view(1, -1)
        P = torch.exp(-((x - lx / 2) ** 2) - (y - ly / 2) ** 2).to(dtype).contiguous()
        Vx = torch.zeros((nx + 1, ny), dtype=dtype, device=self.device)
        Vy = torch.zeros((nx, ny + 1), dtype=dtype, device=self.device)
        fields = [P, Vx, Vy, P.clone(), Vx.clone(), Vy.clone()]
        self.placement = None
        if self.device.type == "cuda" and os.environ.get("IGG_FIELD_MEMORY", "fine") != "torch":
            # One fine-grained allocation (the fused exchange stores into the
            # neighbours' Vx2/Vy2 while their kernels run: docs/COHERENCE.md),
            # the fastest of several candidates (utils/placement.py: 0.282 vs
            # 0.300 ms/step at 8192^2 between fast and slow carves).
            init = fields
            nbytes = P.numel() * P.element_size()
            k = _placement.candidate_count(gg, nbytes, sum(t.numel() * t.element_size() for t in init), self.device)
            # (with neighbours in other processes, which map the velocity
            # buffers, no allocation may reach the IPC size limit)
            split_at = ipc_limit() if int(gg.nprocs) > 1 else None
            fields, self.placement = _placement.placed(lambda: carve(init, kind=1, split_at=split_at), k,
                                                       self._time_placements)
            if self.placement is not None:  # the probe stepped the chosen carve: back to the initial state
                for dst, src in zip(fields, init):
                    dst.copy_(src)
        self.P, self.Vx, self.Vy, self.P2, self.Vx2, self.Vy2 = fields
        # P's halo cells, evaluated from the global coordinates above, equal
        # the neighbours' cells only up to rounding (periodic wrap of x_g);
        # one exchange makes them bitwise consistent, so every halo value the
        # step recomputes locally equals what update_halo_ would deliver (the
        # fused exchange relies on it: set_fused). P itself is never exchanged
        # again: P2 is recomputed everywhere from halo-consistent inputs.
        update_halo_(self.P)
        self._graph_P = 0  # P's buffer when the graph was captured
        self.fused = False
        self._fa = None  # native FusedAcoustic (set_fused)
        # The next fused step starts with an entry barrier: the neighbours'
        # remote stores must not overtake this rank's own writes to the fields
        # (switch into fused mode, restore, external edits: mark_modified).
        self._entry = True
        # Two-step pass: whether the selection kept it, its chunk (0: the
        # kernel's default) and the A/B's ms per step ("single", "c<chunk>").
        self.two_step = False
        self.two_step_chunk = 0
        self.two_step_times = {}
        _select_two_step(self)

    def _two_step_now(self) -> bool:
        """Eligibility of the two-step pass right now: selected, GPU, not
        fused, no neighbour of any kind in x or y on the grid as it is now,
        and the kernel takes the shape."""
        if not self.two_step or self.device.type != "cuda" or self.fused:
            return False
        return not exchanging_dims(2) and _stencil.acoustic2d_twostep_ok(self.P)

    def _pass_key(self):
        return int(self.two_step_chunk)

    def _swap(self) -> None:
        self.P, self.P2 = self.P2, self.P
        self.Vx, self.Vx2 = self.Vx2, self.Vx
        self.Vy, self.Vy2 = self.Vy2, self.Vy

    def _pass(self) -> None:
        """Two time steps in one pass (callers checked ``_two_step_now``: no
        exchange is due). One swap of the buffer roles."""
        s = torch.cuda.current_stream().cuda_stream
        native.acoustic2d_twostep(self.P2.data_ptr(), self.Vx2.data_ptr(), self.Vy2.data_ptr(), self.P.data_ptr(),
                                  self.Vx.data_ptr(), self.Vy.data_ptr(), self.nx, self.ny, self.dt * self.K,
                                  self.dt / self.rho, 1.0 / self.dx, 1.0 / self.dy, self.P.element_size(),
                                  int(self.two_step_chunk), s)
        self._swap()
        self._warm = True

    def _time_placements(self, cands) -> list:
        """ms per step of this model's kernel on each candidate carve
        (P, Vx, Vy, P2, Vx2, Vy2), ping-pong (utils/placement.py)."""

        def launch(c, j):
            a, b = (c[3:], c[:3]) if j % 2 == 0 else (c[:3], c[3:])
            self._update(*a, *b)

        return _placement.time_candidates(cands, launch)

    def _update(self, P2, Vx2, Vy2, P, Vx, Vy) -> None:
        dev = self.device.type == "cuda"
        s = torch.cuda.current_stream().cuda_stream if dev else 0
        native.acoustic2d(P2.data_ptr(), Vx2.data_ptr(), Vy2.data_ptr(), P.data_ptr(), Vx.data_ptr(), Vy.data_ptr(),
                          self.nx, self.ny, self.dt * self.K, self.dt / self.rho, 1.0 / self.dx, 1.0 / self.dy,
                          P.element_size(), dev, s)

    @property
    def can_fuse(self) -> bool:
        """Fused exchange possible: GPU, a neighbour in x or y, overlap 2 in
        both, the vector kernel's shape (ny % 16 B-vector width, >= 5x5)."""
        gg = _grid.global_grid()
        if self.device.type != "cuda" or not exchanging_dims(2):
            return False
        if int(gg.overlaps[0]) != 2 or int(gg.overlaps[1]) != 2:
            return False
        if gg.nprocs > 1 and not gg.comm.one_node:  # IPC peer mappings: one node only
            return False
        vj = 4 if self.P.element_size() == 4 else 2
        return self.ny % vj == 0 and self.nx >= 5 and self.ny >= 5

    def set_fused(self, flag: bool) -> bool:
        """Switch the fused halo exchange on/off (collective: every rank at the
        same point; the first switch-on maps the neighbours' fields)."""
        flag = bool(flag) and self.can_fuse
        if flag == self.fused:
            return flag
        if flag and self._fa is None:
            mesh, nb = peer_mesh(2)
            self._fa = native.FusedAcoustic(mesh, self.nx, self.ny, self.P.element_size(), nb)
            self._fa.set_fields(self.Vx.data_ptr(), self.Vx2.data_ptr(), self.Vy.data_ptr(), self.Vy2.data_ptr())
        self.fused = flag
        self._entry = True
        self.graph = None
        return flag

    def mark_modified(self) -> None:
        """Declare that the fields were written outside the time loop (e.g. a
        copy into P/Vx/Vy): the next fused step first synchronises with the
        neighbours, which store into this rank's fields (collective: every rank
        calls it at the same point)."""
        self._entry = True

    def sync_halo(self) -> None:
        """No-op: the fused step leaves every halo value as update_halo_ would
        (the API matches Diffusion3D's, whose fused step defers halo planes)."""

    @property
    def _fused_handle(self):
        return self._fa

    def close(self) -> None:
        """Release the fused exchange's peer mappings (collective: every rank)."""
        if self._fa is not None:
            torch.cuda.synchronize()
            self._fa.close()
            self._fa = None
            self.fused = False
            self.graph = None

    def _step(self) -> None:
        if self.fused:
            s = torch.cuda.current_stream().cuda_stream
            self._fa.step(self.P2.data_ptr(), self.Vx2.data_ptr(), self.Vy2.data_ptr(), self.P.data_ptr(),
                          self.Vx.data_ptr(), self.Vy.data_ptr(), self.nx, self.ny, self.dt * self.K,
                          self.dt / self.rho, 1.0 / self.dx, 1.0 / self.dy, self.P.element_size(), s,
                          self._entry)
            self._entry = False
        else:
            self._update(self.P2, self.Vx2, self.Vy2, self.P, self.Vx, self.Vy)
            update_halo_(self.Vx2, self.Vy2)
        self._swap()
        self._warm = True

    def local_step(self) -> None:
        """One step of the LOCAL problem (what a rank without neighbours runs:
        the staggered update, no exchange - update_halo_ with PROC_NULL
        neighbours is a no-op, reference src/update_halo.jl:40-42). Timing
        only (the bench's same-process efficiency, which restores the state
        afterwards). No halo exchange repairs the state it leaves: the
        staggered fields' overlap is 3 along their staggered dim, so one plane
        next to each halo is computed on both ranks (never exchanged) and
        drifts apart under local steps, and the fused step is bitwise equal to
        the update_halo_ path only from states where those copies agree."""
        self._update(self.P2, self.Vx2, self.Vy2, self.P, self.Vx, self.Vy)
        self._swap()

    def adjoint_run(self, nt: int, gP, gVx, gVy, out=None):
        """The transpose of ``run(nt)`` applied to ``(gP, gVx, gVy)``: the
        gradient of ``<gP, P> + <gVx, Vx> + <gVy, Vy>``, taken after ``nt``
        steps, with respect to the LOCAL arrays ``P``, ``Vx``, ``Vy`` that the
        steps started from. Returns ``(gP, gVx, gVy)`` as new tensors, or the
        three tensors of ``out``.

        The arguments have the shape, dtype and device of ``P``, ``Vx`` and
        ``Vy`` and are not modified. A step of the model is the staggered
        update ``S``, then ``update_halo_(Vx2, Vy2)`` (``H``), so each of the
        ``nt`` adjoint steps is ``accumulate_halo_(gVx, gVy)`` (``Hᵀ``)
        followed by ``Sᵀ`` (``ops.stencil.acoustic2d_adjoint_``), on two sets of
        ping-pong buffers; ``gP`` is never exchanged. ``S`` is linear: no
        forward state is stored or needed. The fused step and the two-step
        pass leave bitwise the values of single steps, so this is the adjoint
        of ``run(nt)`` on every grid the model accepts. It uses the model's
        ``dt``, ``K``, ``rho``, ``dx`` and ``dy`` as they are at the call and
        touches neither the model's six fields nor a captured graph.
        Collective like ``run``; it raises where ``accumulate_halo_`` would (a
        field with ``n < overlap + halowidth`` in an exchanging dimension, the
        loopback emulation).

        The result is the gradient with respect to the LOCAL arrays: cells a
        rank does not own hold the part that belongs to the cell's owner. For
        ``P`` on the default grid (``overlap == 2*halowidth``) every such cell
        is a halo cell, and one ``accumulate_halo_(gP)`` leaves the gradient
        with respect to the GLOBAL initial pressure in the owned cells
        (``gather_g`` assembles it). ``Vx`` and ``Vy`` have overlap 3 along
        their staggered dimension, so one copy of a face is neither owned nor
        halo: summing all copies of those fields needs the transpose of
        ``scatter_g``, which does not exist yet."""
        from ..parallel.accumulate import accumulate_halo_, check_accumulate

        nt = int(nt)
        if nt < 0:
            raise IGGError("adjoint_run: nt must be >= 0")
        like = (("P", self.P), ("Vx", self.Vx), ("Vy", self.Vy))
        gs = (gP, gVx, gVy)
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 3):
            raise IGGError("adjoint_run: out must be three tensors (gP, gVx, gVy)")
        for what, arrs in (("g", gs), ("out ", out)):
            if arrs is None:
                continue
            for (name, F), A in zip(like, arrs):
                if not isinstance(A, torch.Tensor) or A.shape != F.shape or A.dtype != F.dtype or A.device != F.device:
                    raise IGGError(f"adjoint_run: {what}{name} must have {name}'s shape {tuple(F.shape)}, dtype "
                                   f"{F.dtype} and device {F.device}")
                if not A.is_contiguous():
                    raise IGGError(f"adjoint_run: {what}{name} must be C-contiguous")
        if out is not None:
            for k, A in enumerate(out):
                if any(_stencil._overlaps(A, B) for B in tuple(out[k + 1:]) + tuple(g for j, g in enumerate(gs) if j != k)):
                    raise IGGError("adjoint_run: a tensor of out overlaps another one or another field's g")
        check_accumulate(gVx, gVy)
        if out is None:
            a = [g.clone(memory_format=torch.contiguous_format) for g in gs]
        else:
            a = list(out)
            for o, g in zip(a, gs):
                if o.data_ptr() != g.data_ptr():
                    o.copy_(g)
        if nt == 0:
            return tuple(a)
        b = [torch.empty_like(t) for t in a]
        for _ in range(nt):
            accumulate_halo_(a[1], a[2])
            _stencil.acoustic2d_adjoint_(*b, *a, dt=self.dt, K=self.K, rho=self.rho, dx=self.dx, dy=self.dy)
            a, b = b, a
        if out is not None and a[0] is not out[0]:
            for o, t in zip(out, a):
                o.copy_(t)
            return tuple(out)
        return tuple(a)

    def _capture_start(self) -> None:
        if not self._warm or (self.fused and self._entry):
            self.step()  # the graph holds steady-state steps only (no entry barrier)
        self._graph_P = self.P.data_ptr()

    def _graph_ready(self) -> bool:
        """The captured steps read the capture's P/Vx/Vy first and hold no
        entry barrier (``run`` realigns an odd step count and performs a
        pending barrier - mark_modified, restore - with eager steps)."""
        return self.P.data_ptr() == self._graph_P and not (self.fused and self._entry)

    @property
    def a_eff_bytes(self) -> int:
        """Each of P, Vx, Vy read once and written once per step. The two-step
        pass moves about half of that, so T_eff = a_eff_bytes / t_it can exceed
        the HBM bandwidth while it is on."""
        return 2 * (self.P.numel() + self.Vx.numel() + self.Vy.numel()) * self.P.element_size()


def _select_two_step(m: "Acoustic2D") -> None:
    """Decide the two-step pass for this model (IGG_ACOUSTIC_TWOSTEP): 0 off,
    1 on where eligible (the kernel's default chunk), auto (default): the
    single-step kernel against the pass with every chunk of TWOSTEP_CHUNKS, on
    the model's own six buffers in the time loop's ping-pong shape,
    interleaved rounds, medians; the pass is kept only if its time PER STEP is
    lower. The fields are put back into their initial state afterwards."""
    env = two_step_env("IGG_ACOUSTIC_TWOSTEP")
    m.two_step, m.two_step_chunk, m.two_step_times = False, 0, {}
    if env == "0" or m.device.type != "cuda" or exchanging_dims(2) or not _stencil.acoustic2d_twostep_ok(m.P):
        return
    if env == "1":
        m.two_step = True
        return
    a, b = (m.P, m.Vx, m.Vy), (m.P2, m.Vx2, m.Vy2)
    backup = [t.clone() for t in a + b]
    s = torch.cuda.current_stream().cuda_stream
    coef = (m.nx, m.ny, m.dt * m.K, m.dt / m.rho, 1.0 / m.dx, 1.0 / m.dy, m.P.element_size())

    def ptrs(dst, src):
        return [t.data_ptr() for t in dst + src]

    try:
        single, t = _stencil.time_acoustic_twostep_pingpong(
            a, b, lambda dst, src: native.acoustic2d(*ptrs(dst, src), *coef, True, s),
            lambda dst, src, c: native.acoustic2d_twostep(*ptrs(dst, src), *coef, int(c), s), TWOSTEP_CHUNKS)
    finally:
        for dst, src in zip(a + b, backup):
            dst.copy_(src)
        torch.cuda.synchronize()
        del backup
    best = faster_pass(m, single, t, lambda c: f"c{c}")
    if best is not None:
        m.two_step_chunk = int(best)
        m.two_step = True


def acoustic2d_reference(P, Vx, Vy, *, dt, K, rho, dx, dy):
    """Plain-PyTorch fp64 reference of one fused step (same update order)."""
    P, Vx, Vy = P.double(), Vx.double(), Vy.double()
    P2 = P - dt * K * ((Vx[1:, :] - Vx[:-1, :]) / dx + (Vy[:, 1:] - Vy[:, :-1]) / dy)
    Vx2, Vy2 = Vx.clone(), Vy.clone()
    Vx2[1:-1, :] = Vx[1:-1, :] - dt / rho * (P2[1:, :] - P2[:-1, :]) / dx
    Vy2[:, 1:-1] = Vy[:, 1:-1] - dt / rho * (P2[:, 1:] - P2[:, :-1]) / dy
    return P2, Vx2, Vy2
