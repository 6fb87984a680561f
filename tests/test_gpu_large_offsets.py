"""Every kernel family on fields whose offsets pass 2^31 and 2^32: plane and
row bases, flattened indices, tile counts and byte offsets that the few-MiB
shapes of the other GPU tests never reach.

No reference of a 17 GB field is computed. A big field is PERIODIC along its
long axis with the period ``P = 7`` planes, with values distinct at every cell
of one period. Every kernel here is translation invariant along that axis, so
``k`` planes away from the fixed ends its output has the same period:

* whole array: ``out[k+P : n-k] == out[k : n-k-P]`` in one ``torch.equal`` of
  two views (``aperiodic_cells``). Every interior cell takes part; a load or a
  store whose address wrapped or was truncated anywhere breaks it;
* anchor: the first ``P + k`` and the last ``P + k`` planes equal, bitwise, the
  same kernel's output on a small field (``4P + 2k`` planes, plus the few that
  give its end the big field's phase) holding the same periodic data; for the
  single-step kernels they are also held against the fp64 references, at the
  tolerances, constants and value ranges of tests/test_gpu_stencil.py and
  tests/test_acoustic.py;
* stores: the output starts as NaN with the boundary copied from the input;
  afterwards no NaN is left, the boundary equals the input's, and the 1 MiB of
  NaN on either side of every array (same allocation) is untouched;
* inputs: still periodic, their first period still the block they were tiled
  from, which is every cell of them.

No aliasing hides a wrap. A truncation moves an address by 2^31 or 2^32
elements or bytes. ``P`` has the odd factor 7, so no such shift is a multiple
of ``7 * plane``: it lands on a cell of another phase or position, whose value
differs because a period's values are distinct. ``test_helper_...`` asserts
that arithmetic for every shape of this file, on the CPU.

Shapes (the smallest at which the offsets can go wrong; ``n0`` = the planes that
reach the threshold, rounded up, plus 16):

    L31/f32  (174779, 12, 1024) f32   > 2^31 elements, 8.6 GB: passes 2^31
             elements and 2^31, 2^32, 2^33 bytes     (2^31 / 12288 = 174762.7)
    L31/f64  (349542, 12,  512) f64   > 2^31 elements, 17.2 GB (2^31 / 6144 = 349525.3)
    L32/f32  (349542, 12, 1024) f32   > 2^32 elements, 17.2 GB (2^32 / 12288 = 349525.3)
    FAT      (4, 524287, 1024)  f32   plane of 2^31 - 4096 bytes, the largest
             the two- and three-step passes accept; periodic along y
    A31/f32  nx = 2097168, ny = 1024  nx * ny > 2^31, six arrays of 8.6 GB
    A30/f64  nx = 1048592, ny = 1024  nx * ny > 2^30: passes 2^33 bytes

Rows of 1024 f32 / 512 f64 are what the three-step tile spans; 12 rows are more
than one y tile of every pass and leave a partial last tile (two-step tiles
advance by 6 or 14 rows, three-step tiles by 4).

Each test allocates its arrays itself (at most 68 GiB) and returns them; it
skips only where the device has less free memory than it needs. The cases
that repeat a sibling in the other dtype or at the next threshold are ``slow``
(``IGG_TEST_SLOW=1``); measured times and memory: profiles/large_offsets/NOTES.md.

Not here: the fused exchange, the put arenas and multi-rank runs (their fields
are bounded by the 2^31 check of csrc/fused.cpp and by the IPC limit), and the
roofline probes.
"""
import math
import time

import pytest
import torch

import igg
from igg._native import native
from igg.ops import stencil

gpu_test = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAN = float("nan")
P = 7                # period, in planes of the long axis
GUARD = 1 << 20      # bytes of NaN before and after every big array
GIB = 1 << 30

L31_F32 = ((174779, 12, 1024), F32)
L31_F64 = ((349542, 12, 512), F64)
L32_F32 = ((349542, 12, 1024), F32)
FAT = ((4, 524287, 1024), F32)
A31_F32 = ((2097168, 1024), F32)
A30_F64 = ((1048592, 1024), F64)
LONG = {"L31/f32": L31_F32, "L31/f64": L31_F64, "L32/f32": L32_F32}
ACOUSTIC = {"A31/f32": A31_F32, "A30/f64": A30_F64}

# constants, value ranges and tolerances of tests/test_gpu_stencil.py and tests/test_acoustic.py
KW = dict(lam=1.0, dt=0.01, dx=0.3, dy=0.25, dz=0.2)
TOL = {F64: 1e-12, F32: 1e-5}
AKW = dict(dt=0.01, K=1.3, rho=0.8, dx=0.1, dy=0.07)
ATOL = {F64: 1e-13, F32: 2e-6}


def _es(dtype):
    return torch.empty(0, dtype=dtype).element_size()


# ------------------------------------------------------------------ the helpers
def aperiodic_cells(out, k, axis=0, lo=None, hi=None, period=P):
    """Cells of ``out[lo+period : hi]`` along ``axis`` (``lo = k``, ``hi = n - k``
    unless given) that differ from the cell one period before them: 0 where the
    range is periodic. NaN differs from everything."""
    n = out.shape[axis]
    lo = k if lo is None else lo
    hi = n - k if hi is None else hi
    m = hi - lo - period
    assert m > 0, (n, lo, hi)
    a, b = out.narrow(axis, lo + period, m), out.narrow(axis, lo, m)
    if torch.equal(a, b):
        return 0
    return int((a != b).sum())


def cell_identity(f, shape, axis):
    """What decides the value of the cell at flat index ``f`` of a field that
    is periodic along ``axis``: its place in the period and across it."""
    idx = []
    for n in reversed(shape):
        idx.append(f % n)
        f //= n
    idx = idx[::-1]
    idx[axis] %= P
    return tuple(idx)


def wrap_shifts(es):
    """The element shifts of an address truncated to 31 or 32 bits, counted in
    elements or in bytes."""
    return sorted({1 << 31, 1 << 32, (1 << 31) // es, (1 << 32) // es})


def no_wrap_aliases(shape, es, axis):
    """No shift of ``wrap_shifts`` maps a cell onto one of the same value."""
    total = math.prod(shape)
    cells = (0, 1, shape[-1], total // 2 + 12345, total - 1)
    for s in wrap_shifts(es):
        if axis == 0:
            assert s % (P * math.prod(shape[1:])) != 0, (shape, s)
        for f in cells:
            for g in (f + s, f - s):
                if 0 <= g < total:
                    assert cell_identity(g, shape, axis) != cell_identity(f, shape, axis), (shape, s, f)
    return True


def small_extent(n, k):
    """Extent of the anchor field: ``4P + 2k``, plus what gives its far end the
    phase of the big field's."""
    base = 4 * P + 2 * k
    return base + (n - base) % P


_blocks = {}


def block(shape, seed, lo=0.0):
    """One period on the host (f64): ``lo + i / n`` over a permutation ``i`` of the
    cells, so distinct at every cell also after the conversion to f32."""
    key = (tuple(shape), seed, lo)
    if key not in _blocks:
        n = math.prod(shape)
        assert n < 1 << 22  # i / n + lo < 2 differ by more than an f32 ulp
        g = torch.Generator().manual_seed(seed)
        _blocks[key] = (torch.randperm(n, generator=g).to(F64) / n + lo).reshape(tuple(shape))
    return _blocks[key]


def tile_(A, blk, axis=0):
    """Fill ``A`` with ``blk`` repeated along ``axis``."""
    n, p = A.shape[axis], blk.shape[axis]
    q, r = divmod(n, p)
    if q:
        shp = list(A.shape)
        shp[axis:axis + 1] = [q, p]
        A.narrow(axis, 0, q * p).view(shp).copy_(blk.unsqueeze(axis))
    if r:
        A.narrow(axis, q * p, r).copy_(blk.narrow(axis, 0, r))
    return A


class Guarded:
    """An array with GUARD bytes of NaN before and after it in one allocation."""

    def __init__(self, shape, dtype, device):
        self.g, self.n = GUARD // _es(dtype), math.prod(shape)
        self.buf = torch.empty(self.n + 2 * self.g, dtype=dtype, device=device)
        self.buf[:self.g] = NAN
        self.buf[self.g + self.n:] = NAN
        self.a = self.buf[self.g:self.g + self.n].view(tuple(shape))

    def intact(self):
        return bool(torch.isnan(self.buf[:self.g]).all()) and bool(torch.isnan(self.buf[self.g + self.n:]).all())


def canary_(dst, src):
    """NaN inside, ``src``'s boundary planes, rows and columns around it."""
    dst.fill_(NAN)
    for d in range(dst.dim()):
        for i in (0, -1):
            dst.select(d, i).copy_(src.select(d, i))
    return dst


def boundary_equal(a, b):
    return all(torch.equal(a.select(d, i), b.select(d, i)) for d in range(a.dim()) for i in (0, -1))


def still_tiled(A, blk, axis=0):
    """``A`` is, cell for cell, the array ``tile_`` made of ``blk``."""
    return aperiodic_cells(A, 0, axis) == 0 and torch.equal(A.narrow(axis, 0, P), blk)


def need_gib(gib):
    """Skip where the device has less free memory than the test's need + 4 GiB."""
    free = torch.cuda.mem_get_info()[0]
    if free < (gib + 4) * GIB:
        pytest.skip(f"needs {gib} GiB + 4 GiB of device memory, {free / GIB:.1f} GiB are free")


def gib_of(shape, dtype, arrays):
    """GiB of ``arrays`` big arrays plus one byte per element for torch's masks."""
    n = math.prod(shape)
    return math.ceil((arrays * n * _es(dtype) + 2 * n) / GIB) + 1


@pytest.fixture
def big(request):
    """Holds a test's big arrays; drops them and returns their memory whatever
    the test does. Prints the test's wall time and peak device memory."""
    hold = {}
    cuda = torch.cuda.is_available()
    if cuda:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    try:
        yield hold
    finally:
        hold.clear()
        if cuda:
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() / GIB
            torch.cuda.empty_cache()
            print(f"LARGE {request.node.name}: {time.perf_counter() - t0:.2f} s, peak {peak:.1f} GiB")


# --------------------------------------------------- the helper itself, on the CPU
def test_helper_reports_one_wrong_cell_and_no_shape_aliases():
    """The whole-array check bites: one cell of a periodic array changed past a
    chosen offset is reported, at any place of the checked range; and for every
    shape of this file no 2^31 / 2^32 shift lands on a cell of the same value."""
    shape = (5 * P + 3, 3, 8)
    out = tile_(torch.empty(shape, dtype=F32), block((P, 3, 8), 1).to(F32))
    assert aperiodic_cells(out, 0) == 0 and aperiodic_cells(out, 2) == 0
    assert still_tiled(out, block((P, 3, 8), 1).to(F32))
    for at in ((2, 0, 0), (2 * P + 1, 1, 5), (shape[0] - 3, 2, 7)):
        bad = out.clone()
        bad[at] = out[(at[0] + 1) % P, at[1], at[2]]  # the value of the neighbouring phase: a load one plane off
        assert bad[at] != out[at]
        assert aperiodic_cells(bad, 2) in (1, 2), at  # it differs from the cell before and the cell after it
        bad[at] = NAN  # a cell never stored
        assert aperiodic_cells(bad, 2) in (1, 2), at
    bad = out.clone()
    bad[1, 1, 1] += 1  # inside the k planes next to the end: not the helper's business
    assert aperiodic_cells(bad, 2) == 0 and aperiodic_cells(bad, 0) == 1
    # along the middle axis, as the fat plane is checked
    fat = tile_(torch.empty((4, 4 * P + 1, 8), dtype=F32), block((4, P, 8), 2).to(F32), axis=1)
    assert aperiodic_cells(fat, 3, axis=1) == 0
    fat[2, 2 * P, 3] = fat[2, 2 * P + 1, 3]
    assert aperiodic_cells(fat, 3, axis=1) == 2
    # the shapes: thresholds passed by 16 planes, phases of the anchors, no aliases
    for (shape, dtype), thr in ((L31_F32, 1 << 31), (L31_F64, 1 << 31), (L32_F32, 1 << 32)):
        plane = shape[1] * shape[2]
        assert shape[0] == -(-thr // plane) + 16 and math.prod(shape) >= thr + 16 * plane
        assert shape[2] * _es(dtype) == 4096 and shape[2] % (16 // _es(dtype)) == 0
        assert no_wrap_aliases(shape, _es(dtype), 0)
        for k in (0, 1, 2, 3):
            s = small_extent(shape[0], k)
            assert 4 * P + 2 * k <= s < 5 * P + 2 * k and (shape[0] - s) % P == 0
    assert math.prod(L31_F32[0]) * 4 > 1 << 33 and math.prod(L31_F64[0]) * 8 > 1 << 34
    for (shape, dtype), thr in ((A31_F32, 1 << 31), (A30_F64, 1 << 30)):
        assert shape[0] == thr // shape[1] + 16 and shape[0] * shape[1] * _es(dtype) > 1 << 33
        for rows, cols in ((shape[0], shape[1]), (shape[0] + 1, shape[1]), (shape[0], shape[1] + 1)):
            assert no_wrap_aliases((rows, cols), _es(dtype), 0)
    shape, dtype = FAT
    assert shape[1] * shape[2] * 4 == (1 << 31) - 4096 and (shape[1] + 1) * shape[2] * 4 == 1 << 31
    assert no_wrap_aliases(shape, 4, 1)
    assert (shape[1] - small_extent(shape[1], 3)) % P == 0


# --------------------------------------------------------- diffusion, 3-D fields
def _run_diffusion(gpu, big, case, k, launch, axis=0, arrays=3, with_q=False, ref64=False):
    """One pass of ``launch(T2, T, Cp, Q)`` over the big field of ``case`` and
    over its anchor field, and every check of the module docstring. ``k``: the
    time steps of the pass."""
    shape, dtype = case
    need_gib(gib_of(shape, dtype, arrays))
    pshape = list(shape)
    pshape[axis] = P
    bT = block(pshape, 1).to(dtype).to(gpu)           # T in [0, 1)
    bC = block(pshape, 2, lo=1.0).to(dtype).to(gpu)   # Cp in [1, 2)
    sshape = list(shape)
    sshape[axis] = small_extent(shape[axis], k)
    S = tile_(torch.empty(sshape, dtype=dtype, device=gpu), bT, axis)
    SC = tile_(torch.empty(sshape, dtype=dtype, device=gpu), bC, axis)
    SQ, bQ = None, None
    if with_q:  # the quotient array is tiled from the small one: nothing here rests on quotient_ at large offsets
        SQ = torch.empty_like(SC)
        stencil.quotient_(SQ, SC, lam=KW["lam"], dt=KW["dt"])
        bQ = SQ.narrow(axis, 0, P).clone()
    S2 = canary_(torch.empty_like(S), S)
    launch(S2, S, SC, SQ)
    torch.cuda.synchronize()
    assert not torch.isnan(S2).any()

    T = big["T"] = Guarded(shape, dtype, gpu)
    Cp = big["Cp"] = Guarded(shape, dtype, gpu)
    T2 = big["T2"] = Guarded(shape, dtype, gpu)
    tile_(T.a, bT, axis)
    tile_(Cp.a, bC, axis)
    Q = None
    if with_q:
        Q = big["Q"] = Guarded(shape, dtype, gpu)
        tile_(Q.a, bQ, axis)
    canary_(T2.a, T.a)
    launch(T2.a, T.a, Cp.a, Q.a if with_q else None)
    torch.cuda.synchronize()
    out = T2.a
    # stores
    assert not torch.isnan(out).any(), "a cell was never stored"
    assert boundary_equal(out, T.a), "a boundary cell was written"
    assert all(G.intact() for G in big.values()), "a guard band was written"
    # the whole array
    bad = aperiodic_cells(out, k, axis)
    print(case, "k", k, "cells off the period:", bad)
    assert bad == 0
    # the anchor
    m = P + k
    n, ns = shape[axis], sshape[axis]
    for name, at, ats in (("head", 0, 0), ("tail", n - m, ns - m)):
        got, want = out.narrow(axis, at, m), S2.narrow(axis, ats, m)
        assert torch.equal(got, want), (name, (got != want).nonzero()[:8].tolist())
    if ref64:
        ref = stencil.diffusion3d_reference(S.cpu(), SC.cpu(), **KW)
        for name, at, ats in (("head", 0, 0), ("tail", n - m, ns - m)):
            err = (out.narrow(axis, at, m).double().cpu() - ref.narrow(axis, ats, m)).abs().max().item()
            print(case, name, "against the fp64 reference:", err)
            assert err < TOL[dtype], (name, err)
    # the inputs
    assert still_tiled(T.a, bT, axis) and still_tiled(Cp.a, bC, axis)
    assert Q is None or still_tiled(Q.a, bQ, axis)


MODEL_VARIANT = 11  # the variant the model pins where it overlaps, and the suite's IGG_STENCIL_VARIANT
RESTRICT = 26 if 26 in stencil.compiled_variants() else max(v for v in stencil.compiled_variants() if v >= 21)


def _cases(rows, redundant):
    """``slow`` (IGG_TEST_SLOW=1 runs them) on the rows that repeat a sibling
    in another dtype or at the next threshold: the single-GPU tests were past
    their 300 s before this file (profiles/large_offsets/NOTES.md)."""
    return [pytest.param(*r, marks=pytest.mark.slow) if r[0] in redundant else r for r in rows]


# (shape, variant, rounds, halo_z, boxes)
SINGLE = [("L31/f32", v, 0, False, False) for v in stencil.compiled_variants()]
SINGLE += [("L31/f32", MODEL_VARIANT, 3, False, False)]
SINGLE += [(s, v, 0, False, False) for s in ("L31/f64", "L32/f32") for v in (0, 11, RESTRICT)]
SINGLE += [("L31/f32", MODEL_VARIANT, 0, True, False), ("L31/f64", MODEL_VARIANT, 0, True, False)]
SINGLE += [("L31/f32", MODEL_VARIANT, 0, False, True)]
SINGLE = _cases(SINGLE, ("L31/f64", "L32/f32"))


@gpu_test
@pytest.mark.parametrize("shape,variant,rounds,halo_z,boxes", SINGLE)
def test_single_step(gpu, big, shape, variant, rounds, halo_z, boxes):
    """``diffusion3d_``: every compiled variant. ``boxes``: the slabs and the
    interior of ``split_boundary`` in one call, which together are the inner
    box; the far x slab's origin is itself past 2^31 elements."""
    def launch(T2, T, Cp, Q):
        bx = None
        if boxes:
            slabs, interior = stencil.split_boundary(T.shape, [(1, 1)] * 3, (3, 2, 64))
            bx = [b for b in list(slabs) + [interior] if all(h > l for l, h in zip(b[0], b[1]))]
            assert len(bx) == 7 and max(b[0][0] for b in bx) == T.shape[0] - 4
        stencil.diffusion3d_(T2, T, Cp, variant=variant, rounds=rounds, halo_z=halo_z, boxes=bx, **KW)

    _run_diffusion(gpu, big, LONG[shape], 1, launch, ref64=True)


@gpu_test
@pytest.mark.parametrize("shape", ["L32/f32", "L31/f64"])
def test_quotient(gpu, big, shape):
    """``quotient_``: every element written, the output periodic from the first
    plane to the last, both ends bitwise those of the small run."""
    shp, dtype = LONG[shape]
    need_gib(gib_of(shp, dtype, 2))
    bC = block((P,) + shp[1:], 2, lo=1.0).to(dtype).to(gpu)
    sshape = (small_extent(shp[0], 0),) + shp[1:]
    SC = tile_(torch.empty(sshape, dtype=dtype, device=gpu), bC)
    SQ = torch.full_like(SC, NAN)
    stencil.quotient_(SQ, SC, lam=1.3, dt=0.004)
    Cp = big["Cp"] = Guarded(shp, dtype, gpu)
    Q = big["Q"] = Guarded(shp, dtype, gpu)
    tile_(Cp.a, bC)
    Q.a.fill_(NAN)
    stencil.quotient_(Q.a, Cp.a, lam=1.3, dt=0.004)
    torch.cuda.synchronize()
    assert not torch.isnan(SQ).any() and not torch.isnan(Q.a).any()
    assert Q.intact() and Cp.intact()
    assert aperiodic_cells(Q.a, 0) == 0
    assert torch.equal(Q.a[:P], SQ[:P]) and torch.equal(Q.a[-P:], SQ[-P:])
    assert still_tiled(Cp.a, bC)


def _fat_refused(gpu):
    """One more vector of rows makes the plane 2^31 bytes: refused by the
    predicates, which need no memory of that shape (nothing is launched)."""
    n0, n1, n2 = FAT[0]
    for form in stencil.TWOSTEP_FORMS:
        assert native.diffusion3d_twostep_ok([n0, n1, n2], 4, form)
        assert not native.diffusion3d_twostep_ok([n0, n1 + 1, n2], 4, form)
    for form in stencil.THREESTEP_FORMS:
        assert native.diffusion3d_threestep_ok([n0, n1, n2], 4, form)
        assert not native.diffusion3d_threestep_ok([n0, n1 + 1, n2], 4, form)


# (shape, form, with Q)
TWOSTEP = [("L31/f32", f, q) for f in stencil.TWOSTEP_FORMS for q in (False, True)]
TWOSTEP += [("L31/f64", f, True) for f in stencil.TWOSTEP_FORMS]  # at 512-point rows the model may pick any form
TWOSTEP += [("FAT", 0, True), ("FAT", 0, False)]
TWOSTEP = _cases(TWOSTEP, ("L31/f64",))


@gpu_test
@pytest.mark.parametrize("shape,form,with_q", TWOSTEP)
def test_twostep(gpu, big, shape, form, with_q):
    case, axis = (FAT, 1) if shape == "FAT" else (LONG[shape], 0)
    if shape == "FAT":
        _fat_refused(gpu)

    def launch(T2, T, Cp, Q):
        assert stencil.twostep_ok(T, form)
        stencil.diffusion3d_twostep_(T2, T, Cp, form=form, Q=Q, **KW)

    _run_diffusion(gpu, big, case, 2, launch, axis=axis, arrays=3 + with_q, with_q=with_q)


THREESTEP = [(s, hz, r) for s in ("L31/f32", "L31/f64", "L32/f32", "FAT") for hz in (False, True) for r in (0, -1)]
THREESTEP = _cases(THREESTEP, ("L31/f64",))


@gpu_test
@pytest.mark.parametrize("shape,halo_z,rounds", THREESTEP)
def test_threestep(gpu, big, shape, halo_z, rounds):
    """rounds -1: a 4096-workgroup target, so many x chunks with four-position
    lead-ins, their origins on both sides of every threshold."""
    case, axis = (FAT, 1) if shape == "FAT" else (LONG[shape], 0)
    if shape == "FAT":
        _fat_refused(gpu)

    def launch(T2, T, Cp, Q):
        assert stencil.threestep_ok(T, 0)
        stencil.diffusion3d_threestep_(T2, T, Cp, Q=Q, form=0, rounds=rounds, halo_z=halo_z, **KW)

    _run_diffusion(gpu, big, case, 3, launch, axis=axis, arrays=4, with_q=True)


# ------------------------------------------------------------- acoustic, 2-D fields
# (shape, kernel, chunk): kernel 0, 1, 2 = the single-step variants, "pass" = the two-step pass
ACOUSTIC_CASES = [("A31/f32", v, 0) for v in (0, 1, 2)] + [("A31/f32", "pass", c) for c in (4, 8, 0)]
ACOUSTIC_CASES += [("A30/f64", 2, 0), ("A30/f64", "pass", 0)]


def _acoustic_launch(kernel, chunk, dst, src):
    nx, ny = src[0].shape
    if kernel == "pass":
        assert stencil.acoustic2d_twostep_ok(src[0])
        stencil.acoustic2d_twostep_(*dst, *src, chunk=chunk, **AKW)
        return
    native.acoustic2d_set_variant(kernel)
    try:
        native.acoustic2d(*(t.data_ptr() for t in dst + src), nx, ny, AKW["dt"] * AKW["K"], AKW["dt"] / AKW["rho"],
                          1.0 / AKW["dx"], 1.0 / AKW["dy"], src[0].element_size(), True,
                          torch.cuda.current_stream().cuda_stream)
    finally:
        native.acoustic2d_set_variant(2)


@gpu_test
@pytest.mark.parametrize("shape,kernel,chunk", ACOUSTIC_CASES)
def test_acoustic(gpu, big, shape, kernel, chunk):
    """Periodic along x, rows as planes. After ``k`` steps the rows that no
    fixed x face has reached are: P and Vy (nx rows) ``[k-1, nx-k+1)``, Vx
    (nx+1 rows; faces 0 and nx are fixed) ``[k, nx+1-k)``."""
    from igg.models.acoustic2d import acoustic2d_reference

    (nx, ny), dtype = ACOUSTIC[shape]
    k = 2 if kernel == "pass" else 1
    need_gib(math.ceil((6 * nx * (ny + 1) * _es(dtype) + 2 * nx * ny) / GIB) + 1)
    shapes = lambda n: ((n, ny), (n + 1, ny), (n, ny + 1))
    blocks = [block((P, s[1]), 3 + i).to(dtype).to(gpu) for i, s in enumerate(shapes(nx))]
    nxs = small_extent(nx, k)
    src_s = tuple(tile_(torch.empty(s, dtype=dtype, device=gpu), b) for s, b in zip(shapes(nxs), blocks))
    out_s = tuple(torch.full_like(t, NAN) for t in src_s)
    _acoustic_launch(kernel, chunk, out_s, src_s)
    torch.cuda.synchronize()
    assert not any(torch.isnan(t).any() for t in out_s)

    names = ("P", "Vx", "Vy")
    src = [Guarded(s, dtype, gpu) for s in shapes(nx)]
    out = [Guarded(s, dtype, gpu) for s in shapes(nx)]
    big.update({"in" + n: g for n, g in zip(names, src)})
    big.update({"out" + n: g for n, g in zip(names, out)})
    for g, b in zip(src, blocks):
        tile_(g.a, b)
    for g in out:
        g.a.fill_(NAN)  # every element of the outputs is written
    _acoustic_launch(kernel, chunk, tuple(g.a for g in out), tuple(g.a for g in src))
    torch.cuda.synchronize()
    o = [g.a for g in out]
    for name, t in zip(names, o):
        assert not torch.isnan(t).any(), name
    assert all(g.intact() for g in big.values()), "a guard band was written"
    # the boundary faces keep their input values
    assert torch.equal(o[1][0], src[1].a[0]) and torch.equal(o[1][-1], src[1].a[-1])
    assert torch.equal(o[2][:, 0], src[2].a[:, 0]) and torch.equal(o[2][:, -1], src[2].a[:, -1])
    valid = {"P": (k - 1, nx - k + 1), "Vx": (k, nx + 1 - k), "Vy": (k - 1, nx - k + 1)}
    for name, t in zip(names, o):
        bad = aperiodic_cells(t, k, lo=valid[name][0], hi=valid[name][1])
        print(shape, kernel, chunk, name, "cells off the period:", bad)
        assert bad == 0, name
    m = P + k
    for name, t, ts in zip(names, o, out_s):
        assert torch.equal(t[:m], ts[:m]), (name, "head")
        assert torch.equal(t[-m:], ts[-m:]), (name, "tail")
    if k == 1:
        ref = acoustic2d_reference(*(t.cpu() for t in src_s), **AKW)
        for name, t, r in zip(names, o, ref):
            err = max((t[:m].double().cpu() - r[:m]).abs().max().item(),
                      (t[-m:].double().cpu() - r[-m:]).abs().max().item())
            print(shape, kernel, name, "against the fp64 reference:", err)
            assert err < ATOL[dtype], (name, err)
    for g, b in zip(src, blocks):
        assert still_tiled(g.a, b)


# ------------------------------------------------------------------- reductions
def int_block(shape, seed):
    """One period of integers of [0, 1024) on the host (int64): sums of 2^32 +
    16 planes of their squares stay below 2^53, so every sum is exact in f64
    in any order."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1024, tuple(shape), generator=g)


def phase_counts(a, b):
    """How many planes ``i`` of ``[a, b)`` have ``i % P == p``, per ``p``."""
    return [len(range(a + (p - a) % P, b, P)) for p in range(P)]


GRIDS = {"whole": dict(), "periodic": dict(periodx=1, periody=1, periodz=1, overlapx=3, overlapy=3, overlapz=3)}


def _grid_field(gpu, big, name, case, blk):
    """A field of the initialised grid tiled from ``blk``, NaN in every cell
    this rank does not own; and its owned ranges."""
    shape, dtype = case
    G = big[name] = Guarded(shape, dtype, gpu)
    tile_(G.a, blk.to(dtype).to(gpu))
    rng = igg.owned_ranges(G.a)
    for d, (a, b) in enumerate(rng):
        G.a.narrow(d, 0, a).fill_(NAN)
        G.a.narrow(d, b, shape[d] - b).fill_(NAN)
    return G, rng


@gpu_test
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("shape", ["L32/f32", "L31/f64"])
def test_reduce_g(gpu, big, shape, grid):
    """Exact values from the period and the cell counts, in Python integers.
    "periodic": one rank, periodic in all dimensions with overlap 3, owns
    ``[1, n-2)``: rows start at odd elements and end short, and every cell it
    does not own is NaN here. "whole": the owned box is the array."""
    case = LONG[shape]
    (n0, n1, n2), dtype = case
    need_gib(gib_of(case[0], dtype, 2))
    igg.init_global_grid(n0, n1, n2, quiet=True, init_MPI=False, **GRIDS[grid])
    bA, bB = int_block((P, n1, n2), 1), int_block((P, n1, n2), 2)
    A, rng = _grid_field(gpu, big, "A", case, bA)
    B, _ = _grid_field(gpu, big, "B", case, bB)
    (a0, b0), (a1, b1), (a2, b2) = rng
    assert rng == (((1, n0 - 2), (1, n1 - 2), (1, n2 - 2)) if grid == "periodic" else ((0, n0), (0, n1), (0, n2)))
    cells = (b0 - a0) * (b1 - a1) * (b2 - a2)
    # "whole": a box of more than 2^32 (L32) / 2^31 elements; "periodic": fewer cells, whose offsets still pass it
    thr = 1 << 32 if shape == "L32/f32" else 1 << 31
    assert (cells if grid == "whole" else (b0 - 1) * n1 * n2) > thr
    plan = native.reduce_plan(list(A.a.shape), list(A.a.stride()), [a0, a1, a2], [b0, b1, b2], A.a.element_size(),
                              A.a.data_ptr())
    assert plan["total"] == cells and plan["path"] == ("rows" if grid == "periodic" else "flat"), plan
    cnt = phase_counts(a0, b0)
    oA, oB = bA[:, a1:b1, a2:b2], bB[:, a1:b1, a2:b2]
    per_phase = lambda t: [int(t[p].sum()) for p in range(P)]
    total = lambda t: sum(c * s for c, s in zip(cnt, per_phase(t)))
    want = {"sum": total(oA), "sumsq": total(oA * oA), "dot": total(oA * oB), "sumsq_diff": total((oA - oB) ** 2)}
    assert max(want.values()) < 1 << 53

    def twice(f):
        x, y = f().item(), f().item()
        assert math.isnan(x) == math.isnan(y) and (math.isnan(x) or x == y), "two runs differ"
        return x

    assert twice(lambda: igg.reduce_g("sum", A.a)) == want["sum"]
    assert twice(lambda: igg.reduce_g("dot", A.a, other=B.a)) == want["dot"]
    assert twice(lambda: igg.norm_g(A.a)) == math.sqrt(want["sumsq"])
    assert twice(lambda: igg.norm_diff_g(A.a, B.a)) == math.sqrt(want["sumsq_diff"])
    # extremes in the last owned plane, past every threshold; one just outside the owned box must not count
    last = b0 - 1
    old_hi, old_lo = int(A.a[last, a1, a2 + 1].item()), int(A.a[last, b1 - 1, b2 - 1].item())
    A.a[last, a1, a2 + 1] = 5000.0
    A.a[last, b1 - 1, b2 - 1] = -6000.0
    if grid == "periodic":
        A.a[b0, a1, a2 + 1] = 9999.0
        A.a[last, b1, b2 - 1] = -9999.0
    assert twice(lambda: igg.reduce_g("max", A.a)) == 5000.0
    assert twice(lambda: igg.reduce_g("min", A.a)) == -6000.0
    assert twice(lambda: igg.reduce_g("maxabs", A.a)) == 6000.0
    assert twice(lambda: igg.reduce_g("sum", A.a)) == want["sum"] - old_hi - old_lo + 5000 - 6000
    # a NaN in an unowned plane ("periodic": all of them hold one) reaches nothing; one in the last owned plane does
    A.a[last, a1 + 1, b2 - 2] = NAN
    for op in ("sum", "max", "min", "maxabs", "sumsq"):
        assert math.isnan(twice(lambda: igg.reduce_g(op, A.a))), op
    assert math.isnan(twice(lambda: igg.reduce_g("dot", B.a, other=A.a)))
    assert A.intact() and B.intact()
    torch.cuda.synchronize()
    native.reduce_free_workspace()
    igg.finalize_global_grid(finalize_MPI=False)


@gpu_test
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("shape", ["L31/f32", "L31/f64"])
def test_project_g(gpu, big, shape, grid):
    """Exact projections from the period. On one rank a periodic dimension's
    global index is the local one minus 1 (the first cell is a halo cell), so
    the owned range ``[1, n-2)`` fills the whole global extent ``n - 3`` in
    order; a non-periodic dimension's is the local one."""
    case = LONG[shape]
    (n0, n1, n2), dtype = case
    need_gib(gib_of(case[0], dtype, 1) + 4)
    igg.init_global_grid(n0, n1, n2, quiet=True, init_MPI=False, **GRIDS[grid])
    bA = int_block((P, n1, n2), 3)
    A, rng = _grid_field(gpu, big, "A", case, bA)
    (a0, b0), (a1, b1), (a2, b2) = rng
    lo, hi = [a0, a1, a2], [b0, b1, b2]
    for keep in ((0,), (2,), (0, 2), (1,)):
        p = native.project_plan(list(A.a.shape), list(A.a.stride()), lo, hi, list(keep), A.a.element_size(),
                                A.a.data_ptr())
        # vector loads with 64-bit indices: the combination only a span of 2^31 elements reaches
        assert p["vec"] == 16 // A.a.element_size() and p["index_bits"] == 64, (keep, p)
    o = bA[:, a1:b1, a2:b2].to(F64).to(gpu)                     # the period's owned rows and columns
    phase = (torch.arange(a0, b0, device=gpu) % P)              # of every owned plane
    cnt = torch.tensor(phase_counts(a0, b0), dtype=F64, device=gpu)
    ext = (b0 - a0, b1 - a1, b2 - a2)
    weighted = lambda t: (t * cnt.view(P, *([1] * (t.dim() - 1)))).sum(0)  # integers below 2^53: exact
    want = {
        ((0,), "sum"): o.sum((1, 2))[phase], ((0,), "max"): o.amax((1, 2))[phase],
        ((2,), "sum"): weighted(o.sum(1)), ((2,), "max"): o.amax((0, 1)),
        ((0, 2), "sum"): o.sum(1)[phase], ((0, 2), "max"): o.amax(1)[phase],
        ((1,), "sum"): weighted(o.sum(2)), ((1,), "max"): o.amax((0, 2)),
    }
    assert min(phase_counts(a0, b0)) > 0  # every phase is owned: the maxima over x are the period's
    for keep in ((0,), (2,), (0, 2), (1,)):
        red = math.prod(ext[d] for d in range(3) if d not in keep)
        for op in ("sum", "max", "mean"):
            got = igg.project_g(op, A.a, keep)
            w = want[(keep, "sum" if op == "mean" else op)]
            if op == "mean":
                w = w / torch.full_like(w, float(red))
            assert got.shape == tuple(ext[d] for d in keep) and got.dtype == F64
            assert torch.equal(got, w), (keep, op, (got != w).nonzero()[:8].tolist())
            assert torch.equal(got, igg.project_g(op, A.a, keep)), "two runs differ"
            del got, w
    # a NaN in the last owned plane makes NaN exactly the cells whose line or plane holds it
    A.a[b0 - 1, a1 + 1, a2 + 2] = NAN
    got = igg.project_g("sum", A.a, (0,))
    assert torch.isnan(got[-1]) and not torch.isnan(got[:-1]).any()
    got = igg.project_g("max", A.a, (2,))
    assert torch.isnan(got[2]) and int(torch.isnan(got).sum()) == 1
    assert A.intact()
    del got, want, o, phase
    torch.cuda.synchronize()
    native.project_free_workspace()
    igg.finalize_global_grid(finalize_MPI=False)


# --------------------------------------------------- select_convert and gather_g
def _select_job(gpu, src, dst, c, S, T, src_off, dst_off, seed, path, bits):
    """One descriptor over the f64 buffer ``src`` and the f32 buffer ``dst``
    (both NaN): plants integers of [-1024, 1024] at the lattice. Returns the
    descriptor and a check of the destination lattice."""
    plan = native.select_plan(list(c), list(S), list(T))
    assert plan["path"] == path and plan["index_bits"] == bits, plan
    span = lambda st: sum((n - 1) * s for n, s in zip(c, st)) + 1
    assert src_off + span(S) <= src.numel() and dst_off + span(T) <= dst.numel()  # in bounds before anything runs
    g = torch.Generator().manual_seed(seed)
    vals = torch.randint(-1024, 1025, tuple(c), generator=g).to(F64).to(gpu)
    src.as_strided(list(c), list(S), src_off).copy_(vals)
    desc = (src.data_ptr() + 8 * src_off, dst.data_ptr() + 4 * dst_off, list(c), list(S), list(T))

    def check():
        got = dst.as_strided(list(c), list(T), dst_off)
        assert torch.equal(got, vals.float()), (path, bits, (got != vals.float()).nonzero()[:8].tolist())
        return math.prod(c)

    return desc, check


@gpu_test
def test_select_convert_wide_source(gpu, big):
    """``select_convert_kernel<uint64_t>``: small lattices whose source span
    passes 2^31 elements, on the rows path and (a permuted layout) on the
    element path, each alone and in one launch with a narrow job, which the
    64-bit kernel then runs as well. Everything else of the destinations stays
    NaN."""
    n = (1 << 31) + (1 << 23)
    need_gib(math.ceil(n * 8 / GIB) + 3)
    src = big["src"] = torch.full((n,), NAN, dtype=F64, device=gpu)
    c = (3, 5, 67)
    S_rows = ((1 << 30) + 12345, 1031, 1)   # 2 * S0 > 2^31; rows start at odd and even elements
    S_elem = (1031, 1, 32537632)            # the inner axis has the long stride: 66 * S2 = 2^31 + 64
    S_narrow = (5 * 71, 71, 1)
    Td = (5 * 69, 69, 1)
    launches = []
    for jobs in (["rows"], ["elem"], ["narrow", "rows"], ["elem", "narrow"]):
        dst = torch.full((len(jobs) * 4096,), NAN, dtype=F32, device=gpu)
        descs, checks = [], []
        for i, kind in enumerate(jobs):
            S, path, bits = {"rows": (S_rows, "rows", 64), "elem": (S_elem, "element", 64),
                             "narrow": (S_narrow, "rows", 32)}[kind]
            # the sources of one launch lie apart: rows from 1, elem from 2^20 + 1, narrow past 2^31
            off = {"rows": 1, "elem": (1 << 20) + 1, "narrow": (1 << 31) + 4099}[kind]
            d, chk = _select_job(gpu, src, dst, c, S, Td, off, 4096 * i + 3, 10 * len(launches) + i, path, bits)
            descs.append(d)
            checks.append(chk)
        native.select_convert(descs, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert sum(chk() for chk in checks) == int((~torch.isnan(dst)).sum()), jobs
        launches.append(jobs)


@gpu_test
def test_select_convert_wide_destination(gpu, big):
    """A job whose destination span passes 2^31 elements (the source is small)."""
    n = (1 << 31) + (1 << 20)
    need_gib(math.ceil(n * 4 / GIB) + 4)
    dst = big["dst"] = torch.full((n,), NAN, dtype=F32, device=gpu)
    src = torch.full((1 << 16,), NAN, dtype=F64, device=gpu)
    c = (3, 5, 67)
    for S, T, path in (((5 * 71, 71, 1), ((1 << 30) + 77, 69, 1), "rows"),
                       ((1, 3, 15), ((1 << 30) + 77, 69, 1), "element")):
        dst.fill_(NAN)
        src.fill_(NAN)
        d, chk = _select_job(gpu, src, dst, c, S, T, 1, 3, 7, path, 64)
        native.select_convert([d], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert chk() == int((~torch.isnan(dst)).sum()), path


@gpu_test
def test_gather_g_plane_of_a_wide_field(gpu, big):
    """A y plane of the L31/f64 field, converted (the 64-bit lattice kernel, as
    ``gather_g`` plans it) and plain (the byte mover), against torch indexing."""
    (n0, n1, n2), dtype = L31_F64
    need_gib(gib_of((n0, n1, n2), dtype, 1) + 4)
    igg.init_global_grid(n0, n1, n2, quiet=True, init_MPI=False)
    A = big["A"] = Guarded((n0, n1, n2), dtype, gpu)
    bA = block((P, n1, n2), 5).to(gpu)
    tile_(A.a, bA)
    j = 5
    st = list(A.a.stride())
    assert native.select_plan([n0, 1, n2], st, [n2, n2, 1])["index_bits"] == 64
    for dt in (torch.float32, None):
        odt = dt or dtype
        out = torch.full(igg.selection_shape_g(A.a, (None, j, None)), NAN, dtype=odt, device=gpu)
        assert out.shape == (n0, 1, n2)
        igg.gather_g(A.a, out, box=(None, j, None), dtype=dt)
        torch.cuda.synchronize()
        want = A.a[:, j:j + 1, :].to(odt)
        assert torch.equal(out, want), (dt, (out != want).nonzero()[:8].tolist())
        assert aperiodic_cells(out, 0) == 0  # and the plane is periodic from end to end
        del out, want
    assert A.intact() and still_tiled(A.a, bA)
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------------------ update_halo_
@gpu_test
@pytest.mark.parametrize("pack", ["kernel", "memcpy2d"])
@pytest.mark.parametrize("mode", ["sequential", "onephase"])
@pytest.mark.parametrize("overlap,width", [(2, 1), (4, 2)])
def test_update_halo(gpu, big, overlap, width, mode, pack):
    """One rank, periodic in all three dimensions: the halo planes ``[0, w)``
    receive the planes ``[n-o, n-o+w)`` and ``[n-w, n)`` the planes ``[o-w, o)``.
    The halo starts as NaN. Afterwards each received face equals the torch
    slice copy of its send face, taken before the exchange, on the cells that
    are no halo of another dimension (whose values the edges carry on), and,
    everywhere, the send face as it is now; everything else is untouched."""
    from igg.parallel import halo as H

    (n0, n1, n2), dtype = L31_F32
    need_gib(gib_of((n0, n1, n2), dtype, 1) + 3)
    o, w = overlap, width
    igg.init_global_grid(n0, n1, n2, periodx=1, periody=1, periodz=1, overlapx=o, overlapy=o, overlapz=o,
                         halowidthx=w, halowidthy=w, halowidthz=w, quiet=True, init_MPI=False)
    H.set_halo_mode(mode)
    H.set_pack_mode(pack)
    A = big["A"] = Guarded((n0, n1, n2), dtype, gpu)
    bA = block((P, n1, n2), 6).to(dtype).to(gpu)
    tile_(A.a, bA)
    n = (n0, n1, n2)
    inner = lambda d: tuple(slice(None) if e == d else slice(w, n[e] - w) for e in range(3))
    pairs = []  # (dimension, received planes, planes sent to them)
    for d in range(3):
        pairs += [(d, (0, w), (n[d] - o, n[d] - o + w)), (d, (n[d] - w, n[d]), (o - w, o))]
    sent = [A.a.narrow(d, s[0], w)[inner(d)].clone() for d, _r, s in pairs]
    for d in range(3):
        A.a.narrow(d, 0, w).fill_(NAN)
        A.a.narrow(d, n[d] - w, w).fill_(NAN)
    igg.update_halo_(A.a)
    torch.cuda.synchronize()
    assert not torch.isnan(A.a).any(), "a halo cell was not received"
    for (d, r, s), before in zip(pairs, sent):
        got = A.a.narrow(d, r[0], w)
        assert torch.equal(got[inner(d)], before), (d, r, "against the send face before the exchange")
        assert torch.equal(got, A.a.narrow(d, s[0], w)), (d, r, "against the send face now")
    # the interior is untouched: periodic, and its first period is the block's
    core = A.a[w:n0 - w, w:n1 - w, w:n2 - w]
    assert aperiodic_cells(core, 0) == 0
    first = (torch.arange(w, w + P, device=gpu) % P)
    assert torch.equal(core[:P], bA[first][:, w:n1 - w, w:n2 - w])
    assert A.intact()
    igg.finalize_global_grid(finalize_MPI=False)
