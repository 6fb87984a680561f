"""Stencil operators backed by the native kernels (csrc/kernels/stencil_kernels.hip).

``diffusion3d_`` computes one explicit heat-diffusion update of the interior
(or of a list of boxes inside it) in a single fused pass:

    T2 = T + dt*lam/Cp * (d2T/dx2 + d2T/dy2 + d2T/dz2)

which is the five broadcast kernels of the reference example
(examples/diffusion3D_multigpu_CuArrays_novis.jl:42-46) fused, with no
temporaries. GPU tensors run the hand-written HIP kernel on the current stream;
CPU tensors run the threaded C++ host kernel.
"""
from __future__ import annotations

import contextlib
import os

import torch

from .._native import IGGError, native
from ..utils.timing import interleaved_medians

_autotune_cache: dict = {}


def variants() -> list[str]:
    """Names of every variant index (measurement-only ones included)."""
    return list(native.diffusion3d_variants())


def compiled_variants() -> list[int]:
    """Variant indices compiled in this build (``build.py --probes`` adds the
    measurement-only tilings of rounds 1-2)."""
    return [v for v in range(len(variants())) if native.diffusion3d_variant_compiled(v)]


# Every fused variant of the catalogue (csrc/include/igg/variants.hpp), of both build classes.
FUSED_VARIANTS = tuple(native.diffusion3d_fused_variants())


def compiled_fused_variants() -> list[int]:
    """Fused-exchange variants compiled in this build."""
    return [v for v in FUSED_VARIANTS if native.diffusion3d_fused_variant_ok(v)]


def _check(T2, T, Cp):
    for name, A in (("T2", T2), ("T", T), ("Cp", Cp)):
        if A.dim() != 3:
            raise IGGError(f"diffusion3d: {name} must be 3-D")
        if not A.is_contiguous():
            raise IGGError(f"diffusion3d: {name} must be C-contiguous")
        if A.shape != T.shape or A.dtype != T.dtype or A.device != T.device:
            raise IGGError("diffusion3d: T2, T and Cp must have identical shape, dtype and device")
    if T.dtype not in (torch.float32, torch.float64):
        raise IGGError("diffusion3d: only float32 and float64 are supported")
    if T2.data_ptr() == T.data_ptr():
        raise IGGError("diffusion3d: T2 must not alias T (use ping-pong buffers)")


def inner_box(shape) -> tuple:
    return ((1, 1, 1), tuple(int(s) - 1 for s in shape))


def _variant_for(T, boxes, rd2, dtlam, T2, Cp, stream) -> int:
    env = os.environ.get("IGG_STENCIL_VARIANT", "0").strip().lower()
    if env != "auto":
        return int(env)
    key = (tuple(T.shape), T.dtype, tuple(map(tuple, (b[0] for b in boxes))), tuple(map(tuple, (b[1] for b in boxes))))
    v = _autotune_cache.get(key)
    if v is None:
        v = autotune(T2, T, Cp, rd2, dtlam, boxes)
        _autotune_cache[key] = v
    return v


# The variants that won the autotune on some box in rounds 2-4 (the bench's
# 512^3 f64 / 1024^3 f32 configs, profiles/ and BENCH_r0*.json): 40, 24, 43,
# 11, 2 (f64), 14, 21, 26 (f32 and both). 21+: restrict-argument (fused-kernel)
# form; 40: lane-distributed z-segment edge loads at one workgroup per CU
# (profiles/r1_zl/); 43: full-row z tiles (profiles/r2_fullrow/). 0, 9, 23 and
# 25 never won a real config in rounds 2-4 (23/25 are --probes builds now).
# 44 (round 6): tiling 0 at 2 workgroups per CU (f32, profiles/r6_vsweep/).
SHORTLIST = (2, 11, 14, 21, 24, 26, 40, 43, 44)
# Grid residency rounds tried per variant by the model autotune: 1-4 measured
# best depending on the box and variant (profiles/r1_fused/grid.log,
# variant_sweep.log, r1_zl/: 1-2.5 %).
GRID_ROUNDS = (1, 2, 3, 4)


def _cand(c, halo_z: bool):
    """(variant, grid rounds, halo_z) of a candidate: a variant index, a
    (variant, rounds) pair or a (variant, rounds, halo_z) triple."""
    if isinstance(c, int):
        return c, 0, halo_z
    return (int(c[0]), int(c[1]), bool(c[2]) if len(c) > 2 else halo_z)


def _single_step_launcher(T, Cp, rd2, dtlam, boxes):
    """``launch((variant, grid rounds, halo_z), dst, src)``: one single-step
    kernel between buffers shaped like ``T`` on the current stream."""
    n, es, s = list(T.shape), T.element_size(), torch.cuda.current_stream().cuda_stream

    def launch(cand, dst, src):
        v, gr, hz = cand
        native.diffusion3d(dst.data_ptr(), src.data_ptr(), Cp.data_ptr(), n, rd2, dtlam, es, boxes, True, v, s, gr, hz)

    return launch


@contextlib.contextmanager
def _kept(T):
    """Save ``T`` and put it back on the way out, also when a launch raises."""
    backup = T.clone()
    try:
        yield
    finally:
        T.copy_(backup)
        torch.cuda.synchronize()
        del backup


def time_variants(T2, T, Cp, rd2, dtlam, boxes, candidates=None, reps: int = 5, rounds: int = 3,
                  halo_z: bool = False) -> dict:
    """Median-of-rounds time (ms) of each candidate on these arrays, interleaved
    (the update is pure: T2 = f(T, Cp), so T2 can be scribbled). A candidate is
    a variant index, a (variant, grid_rounds) pair (grid residency rounds of
    the launch, see diffusion3d_) or a (variant, grid_rounds, halo_z) triple
    (``halo_z`` applies to the others)."""
    cands = compiled_variants() if candidates is None else list(candidates)
    launch = _single_step_launcher(T, Cp, rd2, dtlam, boxes)

    def run(c, k):
        for _ in range(k):
            launch(_cand(c, halo_z), T2, T)

    return dict(zip(cands, interleaved_medians(cands, run, reps, rounds, warm=1)))  # warm: every code object once


def time_variants_pingpong(T2, T, Cp, rd2, dtlam, boxes, candidates, steps: int = 10, rounds: int = 3,
                           halo_z: bool = False) -> dict:
    """Like ``time_variants`` but in the time loop's shape: ``steps`` (even)
    launches alternating T2 = f(T) and T = f(T2) on the model's own two
    buffers (their HBM placement alternates exactly as in the run). T is saved
    and restored around the measurement; T2's interior is scribbled (it is
    overwritten by the next step anyway)."""
    cands = list(candidates)
    launch = _single_step_launcher(T, Cp, rd2, dtlam, boxes)

    def run(c, k):
        for j in range(k):
            launch(_cand(c, halo_z), *((T2, T) if j % 2 == 0 else (T, T2)))

    with _kept(T):
        return dict(zip(cands, interleaved_medians(cands, run, steps, rounds, warm=2)))


def autotune(T2, T, Cp, rd2, dtlam, boxes, reps: int = 5, candidates=None) -> int:
    """Fastest variant on these arrays (this process only)."""
    t = time_variants(T2, T, Cp, rd2, dtlam, boxes, candidates, reps)
    return min(t, key=t.get)


def diffusion3d_(T2, T, Cp, *, lam: float, dt: float, dx: float, dy: float, dz: float,
                 boxes=None, variant: int | None = None, stream: int | None = None, rounds: int = 0,
                 halo_z: bool = False) -> None:
    """One fused diffusion update of ``T2`` from ``T`` on ``boxes`` (default: whole interior).

    ``rounds`` sizes the grid of this launch: 0 = library default, k > 0 = k
    residency rounds (k x resident workgroups), k < 0 = |k| x 4096 workgroups.
    ``halo_z``: a box spanning the whole inner z range also writes ``T``'s values
    into ``T2``'s z halo elements (z = 0 and nz-1), so the z-edge stores are
    whole cache lines (5-7 % faster for 1024^3 f32, profiles/r4_halo_z/). Only
    where that is harmless: ``T2``'s z halo equals ``T``'s (fixed boundaries) or
    a halo update after the stencil rewrites it, and nothing writes ``T2``'s z
    halo concurrently. GPU only (the host kernel ignores it).
    """
    _check(T2, T, Cp)
    rd2 = [1.0 / (dx * dx), 1.0 / (dy * dy), 1.0 / (dz * dz)]
    dtlam = dt * lam
    if boxes is None:
        boxes = [inner_box(T.shape)]
    boxes = [(list(b[0]), list(b[1])) for b in boxes]
    dev = T.is_cuda
    if dev:
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        v = _variant_for(T, boxes, rd2, dtlam, T2, Cp, s) if variant is None else variant
    else:
        s, v = 0, 0
    native.diffusion3d(T2.data_ptr(), T.data_ptr(), Cp.data_ptr(), list(T.shape), rd2, dtlam,
                       T.element_size(), boxes, dev, v, s, rounds, bool(halo_z) and dev)


# Tilings of the two-step pass (csrc/kernels/stencil2_kernels.hip). They are
# not part of the variant index space: a variant names a single-step kernel.
TWOSTEP_FORMS = tuple(range(len(native.diffusion3d_twostep_forms())))


def twostep_ok(T, form: int = 0) -> bool:
    """Whether two-step form ``form`` can run on ``T`` (GPU, float32/float64,
    3-D contiguous, rows a multiple of the 16-byte vector)."""
    if not (T.is_cuda and T.dim() == 3 and T.is_contiguous() and T.dtype in (torch.float32, torch.float64)):
        return False
    return bool(native.diffusion3d_twostep_ok(list(T.shape), T.element_size(), int(form)))


def diffusion3d_twostep_(T2, T, Cp, *, lam: float, dt: float, dx: float, dy: float, dz: float,
                         form: int = 0, rounds: int = 0, halo_z: bool = False, stream: int | None = None,
                         Q=None) -> None:
    """Two diffusion updates in one pass over memory: afterwards ``T2`` holds,
    bitwise, what ``diffusion3d_(tmp, T, Cp)`` then ``diffusion3d_(T2, tmp, Cp)``
    on the whole interior leave, where ``tmp``'s boundary planes equal ``T``'s
    (fixed boundary values, no halo exchange between the two steps). ``T`` and
    ``Cp`` are only read; ``T2``'s boundary planes are not written (``halo_z``
    as in ``diffusion3d_``). GPU only; raises ``IGGError`` where ``twostep_ok``
    is false (callers then run two single steps).

    ``Q``: optionally the array ``quotient_`` left for this ``Cp`` and
    ``dt * lam`` (same shape, dtype and device as ``Cp``). The pass then reads
    it where it reads ``Cp`` and does not divide; the result is bitwise the
    same. Keeping ``Q`` current when ``Cp``, ``dt`` or ``lam`` change is the
    caller's business."""
    _check(T2, T, Cp)
    if not T.is_cuda:
        raise IGGError("diffusion3d_twostep: GPU tensors only (there is no host two-step kernel)")
    if not twostep_ok(T, form):
        raise IGGError(f"diffusion3d_twostep: form {form} cannot run shape {tuple(T.shape)} {T.dtype}")
    if Q is not None:
        _check_q(Q, Cp)
    rd2 = [1.0 / (dx * dx), 1.0 / (dy * dy), 1.0 / (dz * dz)]
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    native.diffusion3d_twostep(T2.data_ptr(), T.data_ptr(), Cp.data_ptr(), list(T.shape), rd2, dt * lam,
                               T.element_size(), int(form), s, int(rounds), bool(halo_z),
                               0 if Q is None else Q.data_ptr())


def _check_q(Q, Cp) -> None:
    if Q.shape != Cp.shape or Q.dtype != Cp.dtype or not Q.is_contiguous() or not Cp.is_contiguous():
        raise IGGError(f"quotient: Q {tuple(Q.shape)} {Q.dtype} must match Cp {tuple(Cp.shape)} {Cp.dtype}, "
                       "both C-contiguous")
    if not (Q.is_cuda and Q.device == Cp.device):
        raise IGGError("quotient: Q must be a GPU tensor on Cp's device")
    if Q.data_ptr() == Cp.data_ptr():
        raise IGGError("quotient: Q aliases Cp")


def quotient_(Q, Cp, *, lam: float, dt: float, stream: int | None = None) -> None:
    """``Q = dt*lam / Cp`` elementwise, by the division of the diffusion
    kernels: the optional input ``Q`` of ``diffusion3d_twostep_``. GPU only,
    float32 / float64."""
    if not Cp.is_cuda or Cp.dtype not in (torch.float32, torch.float64):
        raise IGGError("quotient: float32 / float64 GPU tensors only")
    _check_q(Q, Cp)
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    native.quotient(Q.data_ptr(), Cp.data_ptr(), Cp.numel(), dt * lam, Cp.element_size(), s)


def time_twostep_pingpong(T2, T, Cp, rd2, dtlam, boxes, single, candidates, steps: int = 20, rounds: int = 5,
                          exchange=None, Q=None) -> tuple:
    """Median ms PER STEP of the single-step candidate ``single`` (a
    (variant, rounds, halo_z) triple) and of each two-step candidate (form,
    rounds, halo_z) or (form, rounds, halo_z, use_q) - use_q: the pass reads
    the quotient array ``Q`` (``quotient_``) -, interleaved, in the time loop's ping-pong shape on the
    model's own two buffers (``steps`` a multiple of 4: an even number of
    passes). T is saved and restored; T2's interior is scribbled. With
    ``exchange`` (``update_halo_`` on a grid whose halo is two planes deep) it
    follows every kernel on the buffer just written, as in the time loop: one
    exchange per step against one per pass (collective: every rank runs the
    same candidates in the same order). Returns (single ms, {candidate: ms})."""
    n, es, s = list(T.shape), T.element_size(), torch.cuda.current_stream().cuda_stream
    launch = _single_step_launcher(T, Cp, rd2, dtlam, boxes)

    def run(c, k):
        for j in range(k if c is None else k // 2):
            dst, src = (T2, T) if j % 2 == 0 else (T, T2)
            if c is None:
                launch(single, dst, src)
            else:
                f, gr, hz = c[:3]
                q = Q if len(c) > 3 and c[3] else None
                native.diffusion3d_twostep(dst.data_ptr(), src.data_ptr(), Cp.data_ptr(), n, rd2, dtlam, es, f, s, gr,
                                           hz, 0 if q is None else q.data_ptr())
            if exchange is not None:
                exchange(dst)

    order = [None] + list(candidates)  # None: the single-step candidate
    with _kept(T):
        med = dict(zip(order, interleaved_medians(order, run, steps, rounds, warm=4)))
    return med.pop(None), med


# Tilings of the three-step pass (csrc/kernels/stencil3_kernels.hip): 0 = tiles
# of 8 rows that write 4, Q in registers; 1 = tiles of 10 rows that write 6, Q
# parked in LDS between the stages. Both span a row of 512 float64 / 1024
# float32 points and leave the same bits.
THREESTEP_FORMS = tuple(range(len(native.diffusion3d_threestep_forms())))


def threestep_ok(T, form: int = 0) -> bool:
    """Whether three-step form ``form`` can run on ``T``: what ``twostep_ok``
    asks, and rows no longer than the form's tile (512 float64 / 1024 float32
    points for forms 0 and 1). The pass also needs the quotient array."""
    if not (T.is_cuda and T.dim() == 3 and T.is_contiguous() and T.dtype in (torch.float32, torch.float64)):
        return False
    return bool(native.diffusion3d_threestep_ok(list(T.shape), T.element_size(), int(form)))


def diffusion3d_threestep_(T2, T, Cp, *, Q, lam: float, dt: float, dx: float, dy: float, dz: float,
                           form: int = 0, rounds: int = 0, halo_z: bool = False, stream: int | None = None) -> None:
    """Three diffusion updates in one pass over memory: afterwards ``T2``
    holds, bitwise, what three ``diffusion3d_`` calls ``T -> tmp1 -> tmp2 ->
    T2`` on the whole interior leave, where both ``tmp``'s boundary planes
    equal ``T``'s. The pass reads ``T`` and ``Q``, the array ``quotient_`` left
    for this ``Cp`` and ``dt * lam`` (required: it has no dividing form);
    ``Cp`` is only checked against. ``T2``'s boundary planes are not written
    (``halo_z`` as in ``diffusion3d_``). ``form`` picks the tiling
    (``THREESTEP_FORMS``), ``rounds`` the grid as in ``diffusion3d_``;
    ``native.diffusion3d_threestep_plan(shape, form, target)`` gives the tiles,
    planes per x chunk and workgroups of a launch that aims at ``target``
    workgroups. GPU only; raises ``IGGError``, before
    anything is written, where ``threestep_ok`` is false or ``Q`` is missing
    (callers then run the two-step pass or single steps)."""
    _check(T2, T, Cp)
    if not T.is_cuda:
        raise IGGError("diffusion3d_threestep: GPU tensors only (there is no host three-step kernel)")
    if Q is None:
        raise IGGError("diffusion3d_threestep: the pass reads the quotient array Q (quotient_)")
    if not threestep_ok(T, form):
        raise IGGError(f"diffusion3d_threestep: form {form} cannot run shape {tuple(T.shape)} {T.dtype}")
    _check_q(Q, Cp)
    if Q.data_ptr() in (T.data_ptr(), T2.data_ptr()):
        raise IGGError("diffusion3d_threestep: Q aliases a field")
    rd2 = [1.0 / (dx * dx), 1.0 / (dy * dy), 1.0 / (dz * dz)]
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    native.diffusion3d_threestep(T2.data_ptr(), T.data_ptr(), Q.data_ptr(), list(T.shape), rd2, dt * lam,
                                 T.element_size(), int(form), s, int(rounds), bool(halo_z))


def time_threestep_pingpong(T2, T, Cp, rd2, dtlam, two, candidates, Q, steps: int = 24, rounds: int = 5) -> tuple:
    """Median ms PER STEP of the two-step candidate ``two`` (form, rounds,
    halo_z; reading ``Q``) and of each three-step candidate (form, rounds,
    halo_z), interleaved, in the time loop's ping-pong shape on the model's own
    two buffers (``steps`` a multiple of 12: an even number of passes of
    either depth). No exchange: the three-step pass runs only on a grid that
    has none. T is saved and restored; T2's interior is scribbled. Returns
    (two-step ms, {candidate: ms})."""
    n, es, s = list(T.shape), T.element_size(), torch.cuda.current_stream().cuda_stream

    def run(c, k):
        for j in range(k // 2 if c is None else k // 3):
            dst, src = (T2, T) if j % 2 == 0 else (T, T2)
            if c is None:
                f, gr, hz = two[:3]
                native.diffusion3d_twostep(dst.data_ptr(), src.data_ptr(), Cp.data_ptr(), n, rd2, dtlam, es, f, s, gr,
                                           hz, Q.data_ptr())
            else:
                f, gr, hz = c[:3]
                native.diffusion3d_threestep(dst.data_ptr(), src.data_ptr(), Q.data_ptr(), n, rd2, dtlam, es, f, s, gr,
                                             hz)

    order = [None] + list(candidates)  # None: the two-step candidate
    with _kept(T):
        med = dict(zip(order, interleaved_medians(order, run, steps, rounds, warm=12)))
    return med.pop(None), med


def _acoustic_shapes_ok(P, Vx, Vy) -> bool:
    if P.dim() != 2:
        return False
    nx, ny = int(P.shape[0]), int(P.shape[1])
    return tuple(Vx.shape) == (nx + 1, ny) and tuple(Vy.shape) == (nx, ny + 1)


def acoustic2d_twostep_ok(P) -> bool:
    """Whether the two-step acoustic pass can run on pressure field ``P`` (GPU,
    float32/float64, 2-D contiguous (nx, ny), ny a multiple of the 16-byte
    vector and at least two vectors: the vector kernel's own rule)."""
    if not (P.is_cuda and P.dim() == 2 and P.is_contiguous() and P.dtype in (torch.float32, torch.float64)):
        return False
    return bool(native.acoustic2d_twostep_ok(int(P.shape[0]), int(P.shape[1]), P.element_size()))


def acoustic2d_twostep_(P2, Vx2, Vy2, P, Vx, Vy, *, dt: float, K: float, rho: float, dx: float, dy: float,
                        chunk: int = 0, stream: int | None = None) -> None:
    """Two acoustic time steps in one pass over memory
    (csrc/kernels/acoustic2_kernels.hip): afterwards ``P2``, ``Vx2``, ``Vy2``
    hold, bitwise, what two launches of the single-step kernel leave (ping-pong
    through a temporary, no halo exchange in between). Every element of the
    outputs is written; the boundary faces (Vx faces 0 / nx, Vy faces 0 / ny)
    keep their input values. ``P`` (nx, ny), ``Vx`` (nx+1, ny), ``Vy``
    (nx, ny+1) are only read. ``chunk``: rows of x written per wave (0: the
    kernel's default; each chunk re-reads two rows of lead-in). GPU only;
    raises ``IGGError`` without launching for CPU, non-contiguous, mis-shaped,
    mixed-dtype or aliasing tensors and where ``acoustic2d_twostep_ok`` is
    false."""
    ins, outs = (("P", P), ("Vx", Vx), ("Vy", Vy)), (("P2", P2), ("Vx2", Vx2), ("Vy2", Vy2))
    for name, A in ins + outs:
        if not A.is_cuda:
            raise IGGError(f"acoustic2d_twostep: {name} is not a GPU tensor (there is no host two-step kernel)")
        if not A.is_contiguous():
            raise IGGError(f"acoustic2d_twostep: {name} must be C-contiguous")
        if A.dtype != P.dtype or A.device != P.device:
            raise IGGError("acoustic2d_twostep: all six fields must have one dtype and device")
    if not (_acoustic_shapes_ok(P, Vx, Vy) and _acoustic_shapes_ok(P2, Vx2, Vy2) and P2.shape == P.shape):
        raise IGGError("acoustic2d_twostep: shapes must be P (nx, ny), Vx (nx+1, ny), Vy (nx, ny+1), inputs and "
                       f"outputs alike (got {[tuple(A.shape) for _n, A in ins + outs]})")
    if any(o.data_ptr() == i.data_ptr() for _n, o in outs for _m, i in ins):
        raise IGGError("acoustic2d_twostep: an output aliases an input (use ping-pong buffers)")
    if not acoustic2d_twostep_ok(P):
        raise IGGError(f"acoustic2d_twostep: cannot run shape {tuple(P.shape)} {P.dtype}")
    if int(chunk) < 0:
        raise IGGError(f"acoustic2d_twostep: chunk must be >= 0, got {chunk}")
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    native.acoustic2d_twostep(P2.data_ptr(), Vx2.data_ptr(), Vy2.data_ptr(), P.data_ptr(), Vx.data_ptr(),
                              Vy.data_ptr(), int(P.shape[0]), int(P.shape[1]), dt * K, dt / rho, 1.0 / dx, 1.0 / dy,
                              P.element_size(), int(chunk), s)


def time_acoustic_twostep_pingpong(a, b, launch_single, launch_pass, chunks, steps: int = 20,
                                   rounds: int = 5) -> tuple:
    """Median ms PER STEP of the single-step acoustic kernel and of the
    two-step pass with each chunk of ``chunks``, interleaved, in the time
    loop's ping-pong shape between the field triples ``a`` and ``b`` (``steps``
    a multiple of 4: an even number of passes). ``launch_single(dst, src)`` /
    ``launch_pass(dst, src, chunk)`` launch on the current stream. Both triples
    are scribbled (callers restore them). Returns (single ms, {chunk: ms})."""
    def run(c, k):
        for j in range(k if c is None else k // 2):
            dst, src = (b, a) if j % 2 == 0 else (a, b)
            if c is None:
                launch_single(dst, src)
            else:
                launch_pass(dst, src, c)

    order = [None] + list(chunks)  # None: the single-step kernel
    med = dict(zip(order, interleaved_medians(order, run, steps, rounds, warm=4)))
    return med.pop(None), med


def _overlaps(A, B) -> bool:
    """Whether the bytes of two dense tensors overlap (same device)."""
    if A.device != B.device or A.numel() == 0 or B.numel() == 0:
        return False
    a0, b0 = A.data_ptr(), B.data_ptr()
    return a0 < b0 + B.numel() * B.element_size() and b0 < a0 + A.numel() * A.element_size()


def diffusion3d_adjoint_(gT, g, Cp, *, lam: float, dt: float, dx: float, dy: float, dz: float,
                         Q=None, T=None, gCp=None, accumulate: bool = False, stream: int | None = None,
                         chunk: int = 0) -> None:
    """The transpose of one diffusion step, applied to ``g``.

    With ``S`` the step as the model's loop uses it - ``diffusion3d_`` on the
    whole interior into an array whose boundary cells hold ``T``'s - this
    writes ``gT = Sᵀ g`` (every cell of ``gT``, boundary cells included: they
    are copied by ``S``, so they keep their own ``g`` and receive from their
    interior neighbour, but send nothing through the stencil) and, where
    ``gCp`` is given, the derivative with respect to ``Cp``,
    ``gCp = -(dt*lam/Cp * g / Cp) * laplace(T)`` on interior cells and 0 on
    boundary cells. ``S`` is linear in ``T``, so ``gT`` needs no forward
    state; ``gCp`` needs the step's input ``T``.

    ``gT=None`` skips the first kernel. ``Q``: the array ``quotient_`` left
    for this ``Cp`` and ``dt*lam``; ``gT`` is then computed from it, ``Cp`` is
    not read for it, and the values are bitwise the same. ``accumulate=True``
    adds into ``gCp``'s interior cells and leaves its boundary cells alone.
    Boundary values of ``Cp`` and ``Q`` reach no result (``Cp == 0`` there is
    fine). An array with an extent below 3 has no interior: ``gT = g`` and
    ``gCp = 0``.

    CPU and GPU tensors, float32 / float64, 3-D and C-contiguous, all of one
    shape, dtype and device. GPU work is ordered on ``stream`` (default: the
    current stream) and can be captured in a hipGraph; the CPU path is the
    threaded host twin, which gives bitwise what the kernels give. ``chunk``:
    planes along x per workgroup (0: sized to the device). ``gT`` must not
    overlap ``g`` (the kernel reads neighbours) and ``gCp`` no other
    argument; every failed check raises ``IGGError`` before anything is
    written."""
    who = "diffusion3d_adjoint"
    named = [("g", g), ("gT", gT), ("Cp", Cp), ("Q", Q), ("T", T), ("gCp", gCp)]
    if g is None or Cp is None:
        raise IGGError(f"{who}: g and Cp are required")
    for name, A in named:
        if A is None:
            continue
        if not isinstance(A, torch.Tensor) or A.dim() != 3:
            raise IGGError(f"{who}: {name} must be a 3-D tensor")
        if A.shape != g.shape:
            raise IGGError(f"{who}: {name} has shape {tuple(A.shape)}, g has {tuple(g.shape)}")
        if A.dtype != g.dtype:
            raise IGGError(f"{who}: {name} has dtype {A.dtype}, g has {g.dtype}")
        if A.device != g.device:
            raise IGGError(f"{who}: {name} is on {A.device}, g is on {g.device}")
        if not A.is_contiguous():
            raise IGGError(f"{who}: {name} must be C-contiguous")
    if g.dtype not in (torch.float32, torch.float64):
        raise IGGError(f"{who}: g must be float32 or float64 (got {g.dtype})")
    if gCp is not None and T is None:
        raise IGGError(f"{who}: gCp needs T, the input of the forward step")
    if gT is not None and _overlaps(gT, g):
        raise IGGError(f"{who}: gT must not alias g (the kernel reads g's neighbours)")
    if gT is not None:
        for name, A in (("Cp", Cp), ("Q", Q), ("T", T)):
            if A is not None and _overlaps(gT, A):
                raise IGGError(f"{who}: gT must not alias {name}")
    if gCp is not None:
        for name, A in named[:5]:
            if A is not None and _overlaps(gCp, A):
                raise IGGError(f"{who}: gCp must not alias {name}")
    if int(chunk) < 0:
        raise IGGError(f"{who}: chunk must be >= 0")
    if gT is None and gCp is None:
        return
    rd2 = [1.0 / (dx * dx), 1.0 / (dy * dy), 1.0 / (dz * dz)]
    dev = g.is_cuda
    s = 0
    if dev:
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream

    def ptr(A):
        return 0 if A is None else A.data_ptr()

    native.diffusion3d_adjoint(ptr(gT), ptr(gCp), ptr(g), ptr(Cp), ptr(Q), ptr(T), list(g.shape), rd2, dt * lam,
                               g.element_size(), bool(accumulate), dev, s, int(chunk))


def _acoustic_step(P2, Vx2, Vy2, P, Vx, Vy, *, dt, K, rho, dx, dy) -> None:
    """The single acoustic step on checked, dense tensors (igg.autograd.acoustic2d's
    forward pass): the model's kernel, or its host twin, on the current stream."""
    fields = (P2, Vx2, Vy2, P, Vx, Vy)
    if not (_acoustic_shapes_ok(P, Vx, Vy) and _acoustic_shapes_ok(P2, Vx2, Vy2) and P2.shape == P.shape):
        raise IGGError("acoustic2d: shapes must be P (nx, ny), Vx (nx+1, ny), Vy (nx, ny+1) "
                       f"(got {[tuple(A.shape) for A in fields[3:]]})")
    if P.numel() == 0:
        raise IGGError("acoustic2d: needs nx >= 1 and ny >= 1")
    if P.dtype not in (torch.float32, torch.float64):
        raise IGGError(f"acoustic2d: the fields must be float32 or float64 (got {P.dtype})")
    if any(A.dtype != P.dtype or A.device != P.device or not A.is_contiguous() for A in fields):
        raise IGGError("acoustic2d: the fields must be C-contiguous and of one dtype and device")
    dev = P.is_cuda
    s = torch.cuda.current_stream().cuda_stream if dev else 0
    native.acoustic2d(*(A.data_ptr() for A in fields), int(P.shape[0]), int(P.shape[1]), dt * K, dt / rho, 1.0 / dx,
                      1.0 / dy, P.element_size(), dev, s)


def acoustic2d_adjoint_(gP, gVx, gVy, gP2, gVx2, gVy2, *, dt: float, K: float, rho: float, dx: float, dy: float,
                        chunk: int = 0, stream: int | None = None) -> None:
    """The transpose of one acoustic step, applied to ``(gP2, gVx2, gVy2)``.

    With ``S`` the staggered step ``(P, Vx, Vy) -> (P2, Vx2, Vy2)`` of
    ``Acoustic2D`` (boundary faces of ``Vx``/``Vy`` copied), this writes
    ``(gP, gVx, gVy) = Sᵀ (gP2, gVx2, gVy2)``, every element of the three
    outputs. With ``a = dt*K``, ``b = dt/rho``::

        wx = (b*gVx2)/dx on x-faces 1..nx-1, wy = (b*gVy2)/dy on y-faces 1..ny-1, else 0
        r  = gP2 + ((wx[i+1]-wx[i]) + (wy[j+1]-wy[j]))
        gP = r,  gVx = gVx2 + (a*(r[i]-r[i-1]))/dx,  gVy = gVy2 + (a*(r[j]-r[j-1]))/dy

    with ``r = 0`` outside the cells. ``S`` is linear, so no forward state is
    needed. Zeros are selected, never multiplied: what a boundary face of
    ``gVx2``/``gVy2`` holds (NaN, Inf) reaches that face of ``gVx``/``gVy`` and
    nothing else.

    Shapes as in the step: ``gP``/``gP2`` (nx, ny), ``gVx``/``gVx2``
    (nx+1, ny), ``gVy``/``gVy2`` (nx, ny+1), ``nx, ny >= 1``; CPU and GPU
    tensors, float32 / float64, C-contiguous, all of one dtype and device. GPU
    work is one kernel (csrc/kernels/acoustic_adj_kernels.hip: three arrays
    read, three written) ordered on ``stream`` (default: the current stream)
    and can be captured in a hipGraph; the CPU path is the threaded host twin,
    which gives bitwise what the kernel gives. ``chunk``: rows of x per wave
    (0: the kernel's default). No output may overlap an input or another
    output; every failed check raises ``IGGError`` before anything is
    written."""
    who = "acoustic2d_adjoint"
    outs = (("gP", gP), ("gVx", gVx), ("gVy", gVy))
    ins = (("gP2", gP2), ("gVx2", gVx2), ("gVy2", gVy2))
    for name, A in outs + ins:
        if not isinstance(A, torch.Tensor) or A.dim() != 2:
            raise IGGError(f"{who}: {name} must be a 2-D tensor")
    if not (_acoustic_shapes_ok(gP2, gVx2, gVy2) and _acoustic_shapes_ok(gP, gVx, gVy) and gP.shape == gP2.shape):
        raise IGGError(f"{who}: shapes must be gP (nx, ny), gVx (nx+1, ny), gVy (nx, ny+1), inputs and outputs "
                       f"alike (got {[tuple(A.shape) for _n, A in outs + ins]})")
    nx, ny = int(gP2.shape[0]), int(gP2.shape[1])
    if nx < 1 or ny < 1:
        raise IGGError(f"{who}: needs nx >= 1 and ny >= 1 (got {nx} x {ny})")
    for name, A in outs + ins:
        if A.dtype != gP2.dtype:
            raise IGGError(f"{who}: {name} has dtype {A.dtype}, gP2 has {gP2.dtype}")
        if A.device != gP2.device:
            raise IGGError(f"{who}: {name} is on {A.device}, gP2 is on {gP2.device}")
        if not A.is_contiguous():
            raise IGGError(f"{who}: {name} must be C-contiguous")
    if gP2.dtype not in (torch.float32, torch.float64):
        raise IGGError(f"{who}: the fields must be float32 or float64 (got {gP2.dtype})")
    for k, (name, A) in enumerate(outs):
        for other, B in outs[k + 1:] + ins:
            if _overlaps(A, B):
                raise IGGError(f"{who}: {name} must not overlap {other}")
    if int(chunk) < 0:
        raise IGGError(f"{who}: chunk must be >= 0")
    dev = gP2.is_cuda
    s = 0
    if dev:
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    native.acoustic2d_adjoint(gP.data_ptr(), gVx.data_ptr(), gVy.data_ptr(), gP2.data_ptr(), gVx2.data_ptr(),
                              gVy2.data_ptr(), nx, ny, dt * K, dt / rho, 1.0 / dx, 1.0 / dy, gP2.element_size(),
                              dev, s, int(chunk))


def diffusion3d_reference(T, Cp, *, lam, dt, dx, dy, dz) -> torch.Tensor:
    """Plain-PyTorch (fp64) reference of the reference example's 5 broadcasts."""
    T = T.double()
    Cp = Cp.double()
    qx = -lam * (T[1:, 1:-1, 1:-1] - T[:-1, 1:-1, 1:-1]) / dx
    qy = -lam * (T[1:-1, 1:, 1:-1] - T[1:-1, :-1, 1:-1]) / dy
    qz = -lam * (T[1:-1, 1:-1, 1:] - T[1:-1, 1:-1, :-1]) / dz
    dTedt = 1.0 / Cp[1:-1, 1:-1, 1:-1] * (
        -(qx[1:] - qx[:-1]) / dx - (qy[:, 1:] - qy[:, :-1]) / dy - (qz[:, :, 1:] - qz[:, :, :-1]) / dz)
    out = T.clone()
    out[1:-1, 1:-1, 1:-1] = T[1:-1, 1:-1, 1:-1] + dt * dTedt
    return out


def split_boundary(shape, active, widths):
    """Boundary slabs + interior box of the inner region (see csrc/stencil_host.cpp).

    ``active[d]`` is a bool (both sides) or a (left, right) pair of bools.
    """
    act = [[bool(a), bool(a)] if isinstance(a, (bool, int)) else [bool(a[0]), bool(a[1])] for a in active]
    slabs, interior = native.split_boundary(list(shape), act, list(widths))
    return slabs, interior
