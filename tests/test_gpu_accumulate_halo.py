"""The accumulation kernels (accum3d_batch_kernel, csrc/kernels/accum_kernels.hip)
at descriptor level and accumulate_halo_ on the GPU (parallel/accumulate.py).

Kernel tests, in the manner of tests/test_gpu_scatter_g.py: the source box is
carved out of a NaN buffer, the destination box out of a buffer filled with a
sentinel, with NaN / the sentinel between the rows too. ``native.host_accum3d``
does the same descriptors on host copies of both buffers, and BOTH whole
allocations are compared with the host's bit for bit: a stray store, a lane one
element off, a cleared cell too many or a load that let a neighbour's NaN in
shows up. Values are random non-integers with infinities, signed zeros and
subnormals among them: the GPU's add must be the host's add.
"""
import numpy as np
import pytest
import torch

import igg
from igg._native import native
from tests.test_accumulate_halo_cpu import run_accumulate_ranks

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -7777.0
PAD = 64  # elements around a carved box: the buffers' bases stay 256-B aligned
DTYPES = {"float64": torch.float64, "float32": torch.float32}
INT = {torch.float64: torch.int64, torch.float32: torch.int32}


def _span(c, s):
    return sum((n - 1) * k for n, k in zip(c, s)) + 1


def _values(c, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    v = (torch.randn(tuple(c), generator=g, dtype=torch.float64) * 8).to(dtype)
    flat = v.view(-1)
    tiny = torch.finfo(dtype).tiny
    special = [0.0, -0.0, float("inf"), -float("inf"), tiny / 4, -tiny / 8, tiny, torch.finfo(dtype).max, 1.0 / 3.0]
    k = min(len(special), flat.numel())
    flat[:k] = torch.tensor(special[:k], dtype=dtype)
    return v


class Job:
    """One descriptor with its buffers on the host and on the device."""

    def __init__(self, gpu, c, S, T, op, dtype="float64", src_off=0, dst_off=0, seed=1):
        self.c, self.S, self.T, self.op, self.dtype = list(c), list(S), list(T), op, dtype
        dt = DTYPES[dtype]
        eb = torch.empty(0, dtype=dt).element_size()
        self.so, self.do = PAD + src_off, PAD + dst_off
        self.hsrc = torch.full((self.so + _span(c, S) + PAD,), NAN, dtype=dt)
        self.hsrc.as_strided(self.c, self.S, self.so).copy_(_values(c, dt, seed))
        self.hdst = torch.full((self.do + _span(c, T) + PAD,), SENTINEL, dtype=dt)
        self.hdst.as_strided(self.c, self.T, self.do).copy_(_values(c, dt, seed + 1000).flip(0))
        self.src, self.dst = self.hsrc.to(gpu), self.hdst.to(gpu)
        self.box = self.c + self.S + self.T
        self.ptrs = (self.src.data_ptr() + eb * self.so, self.dst.data_ptr() + eb * self.do)
        self.hptrs = (self.hsrc.data_ptr() + eb * self.so, self.hdst.data_ptr() + eb * self.do)
        self.plan = native.accum3d_plan(self.box, self.ptrs, dtype)

    def check(self, tag=""):
        it = INT[DTYPES[self.dtype]]
        for name, got, want in (("dst", self.dst.cpu(), self.hdst), ("src", self.src.cpu(), self.hsrc)):
            if not torch.equal(got.view(it), want.view(it)):
                bad = (got.view(it) != want.view(it)).nonzero().flatten()[:6]
                off = self.do if name == "dst" else self.so
                raise AssertionError(f"{tag} {self.op} {self.dtype} c={self.c} S={self.S} T={self.T}: {name} differs "
                                     f"at {[int(b) - off for b in bad]}: got {got[bad].tolist()}, "
                                     f"want {want[bad].tolist()}")
        if self.op in ("take", "add_take"):  # exact zeros: +0, never -0
            left = self.src.cpu().as_strided(self.c, self.S, self.so)
            assert (left.view(it) == 0).all(), f"{tag}: the taken cells are not all +0"


def _launch(*jobs):
    assert len({j.dtype for j in jobs}) == 1
    native.host_accum3d([j.box for j in jobs], [j.hptrs for j in jobs], [j.op for j in jobs], jobs[0].dtype)
    native.accum3d([j.box for j in jobs], [j.ptrs for j in jobs], [j.op for j in jobs], jobs[0].dtype,
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _run(gpu, c, S, T, op, path, vec=None, **kw):
    j = Job(gpu, c, S, T, op, **kw)
    assert j.plan["path"] == path, j.plan
    if vec is not None:
        assert j.plan["vec_bytes"] == vec, j.plan
    _launch(j)
    j.check(path)
    return j


OPS = ("add", "take", "add_take")
ROW_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1027)


# ------------------------------------------------------- rows: flat and chunk
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", ROW_LENGTHS)
def test_rows_at_every_residue_with_odd_pitches(gpu, n, dtype):
    """3 x 5 rows of n in pitches that are no multiple of 16 bytes, the box
    starting at every 16-byte residue on both sides: short rows go one element
    per lane (flat), long ones by row chunks - by element, since no two rows
    are aligned alike."""
    per16 = 2 if dtype == "float64" else 4
    ps, pt = (n + 2) | 1, (n + 4) | 1
    path = "flat" if n < 64 else "chunk"
    k = 0
    for rs in range(per16):
        for rd in range(per16):
            _run(gpu, (3, 5, n), (5 * ps + 2, ps, 1), (5 * pt + 3, pt, 1), OPS[k % 3], path, vec=0, dtype=dtype,
                 src_off=rs, dst_off=rd, seed=n + 8 * rs + rd)
            k += 1


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", ROW_LENGTHS[9:])
def test_aligned_rows_move_16_bytes_per_lane(gpu, n, dtype):
    """Pitches of a multiple of 16 bytes and aligned bases: 16-byte accesses,
    the row's last n mod (2 or 4) elements one by one; one misaligned side
    turns them off."""
    per16 = 2 if dtype == "float64" else 4
    ps, pt = (n + 2 * per16) // per16 * per16, (n + 4 * per16) // per16 * per16
    for k, op in enumerate(OPS + ("zero",)):
        _run(gpu, (3, 5, n), (5 * ps, ps, 1), (6 * pt, pt, 1), op, "chunk", vec=16, dtype=dtype, seed=n + k)
    _run(gpu, (3, 5, n), (5 * ps, ps, 1), (6 * pt, pt, 1), "add", "chunk", vec=0, dtype=dtype, src_off=1)
    _run(gpu, (3, 5, n), (5 * ps, ps, 1), (6 * pt, pt, 1), "take", "chunk", vec=0, dtype=dtype, dst_off=1)


def test_a_contiguous_slab_is_zeroed_in_long_aligned_rows(gpu):
    for dtype in DTYPES:
        j = Job(gpu, (4, 6, 70), (420, 70, 1), (420, 70, 1), "zero", dtype=dtype)
        # a Zero descriptor carries its slab on both sides
        j.ptrs = (j.dst.data_ptr() + j.dst.element_size() * j.do,) * 2
        j.hptrs = (j.hdst.data_ptr() + j.hdst.element_size() * j.do,) * 2
        j.plan = native.accum3d_plan(j.box, j.ptrs, dtype)
        assert j.plan["path"] == "chunk" and j.plan["box"][:3] == (1, 4, 6 * 70) and j.plan["vec_bytes"] == 16
        _launch(j)
        j.check("zero")
        assert (j.dst[j.do:j.do + 1680].cpu().view(INT[DTYPES[dtype]]) == 0).all()


# ------------------------------------------------------------ the z-slab shape
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("w", [1, 2])
def test_z_slab_of_a_c_ordered_field_takes_the_gather_path(gpu, w, dtype):
    """37 x 130 rows of w elements, 70 apart, against their packed image: one
    row per lane, 8 outer indices per lane (37 = 32 + 5: a partial group), 130
    rows = two full waves and a partial one. A row is one access where both
    sides are aligned to it."""
    eb = 8 if dtype == "float64" else 4
    no, nm = 37, 130
    field, packed = (nm * 70, 70, 1), (nm * w, w, 1)
    vec = w * eb if w > 1 else 0  # (a row of one element is an element access whichever way)
    _run(gpu, (no, nm, w), field, packed, "take", "gather", vec=vec, dtype=dtype)          # halo slab -> message
    _run(gpu, (no, nm, w), packed, field, "add", "gather", vec=vec, dtype=dtype, seed=2)   # message -> send slab
    _run(gpu, (no, nm, w), field, field, "add_take", "gather", vec=vec, dtype=dtype, seed=3)  # self-periodic
    if w == 2:
        # the slab starts at an odd element: rows are not aligned to their size, a lane goes by element
        _run(gpu, (no, nm, w), field, packed, "take", "gather", vec=0, dtype=dtype, src_off=1, seed=4)
        _run(gpu, (no, nm, w), packed, field, "add", "gather", vec=0, dtype=dtype, dst_off=1, seed=5)


# ------------------------------------------------------------ permuted strides
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_permuted_strides(gpu, dtype):
    n0, n1, n2 = 7, 9, 13
    dense = (n1 * n2, n2, 1)
    for k, op in enumerate(OPS):
        _run(gpu, (n0, n1, n2), (1, n0, n0 * n1), dense, op, "flat", dtype=dtype, seed=k)            # a permuted source
        _run(gpu, (n0, n1, n2), dense, (1, n0 + 3, (n0 + 3) * (n1 + 2)), op, "flat", dtype=dtype,    # a box in a
             src_off=1, dst_off=1, seed=k + 3)                                                    # permuted array
    # long strided rows: chunks by element, 5 x 70 rows of 66
    c = (5, 70, 66)
    _run(gpu, c, (1, 5, 350), (70 * 66, 66, 1), "take", "chunk", vec=0, dtype=dtype)
    _run(gpu, c, (70 * 66, 66, 1), (1, 5, 350), "add", "chunk", vec=0, dtype=dtype)
    # a one-plane face across the fastest axis: long strided rows become one row per lane
    _run(gpu, (1, 40, 100), (0, 100 * 70, 70), (0, 100, 1), "take", "gather", vec=0, dtype=dtype)


# -------------------------------------------------------------------- batches
def test_more_descriptors_than_one_launch_takes(gpu):
    assert native.MAX_BATCH == 32
    for dtype in DTYPES:
        jobs = [Job(gpu, (2, 3, 5 + 9 * k), (3 * 340, 340, 1), (3 * 337, 337, 1), ("add", "take", "add_take")[k % 3],
                    dtype=dtype, src_off=k & 3, dst_off=k & 1, seed=k) for k in range(33)]
        jobs.append(Job(gpu, (4, 0, 9), (90, 9, 1), (90, 9, 1), "add", dtype=dtype))  # empty
        jobs.append(Job(gpu, (1, 1, 1), (0, 0, 1), (0, 0, 1), "add_take", dtype=dtype, src_off=1))
        assert {j.plan["path"] for j in jobs} == {"flat", "chunk"} and jobs[33].plan["blocks"] == 0
        _launch(*jobs)
        for k, j in enumerate(jobs):
            j.check(f"job {k}")


def test_bad_descriptors_are_refused(gpu):
    j = Job(gpu, (2, 3, 9), (27, 9, 1), (27, 9, 1), "add")
    stream = torch.cuda.current_stream().cuda_stream
    s, d = j.ptrs
    for ptrs, op, dtype in (((s + 4, d), "add", "float64"), ((0, d), "add", "float64"), ((s, d), "sub", "float64"),
                            ((s, d), "add", "int32"), ((s, d), "add", "float16")):
        with pytest.raises(igg.IGGError):
            native.accum3d([j.box], [ptrs], [op], dtype, stream)
    torch.cuda.synchronize()
    assert torch.equal(j.dst.cpu().view(torch.int64), j.hdst.view(torch.int64))


# ------------------------------------------- one rank, periodic: GPU against CPU
def _fields(shapes, dtype, layouts=None, seed=0):
    out = []
    for k, s in enumerate(shapes):
        g = torch.Generator().manual_seed(seed + k)
        t = torch.randn(s, generator=g, dtype=torch.float64).to(dtype)
        perm = (layouts or {}).get(k)
        if perm is not None:  # the same values, stored with the axes in another order
            inv = [perm.index(d) for d in range(3)]
            t = t.permute(perm).contiguous().permute(inv)
            assert t.shape == torch.Size(s) and not t.is_contiguous()
        out.append(t)
    return out


def _same_bits(a, b):
    it = INT[a.dtype]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,overlap,width,shapes,layouts", [
    ((16, 12, 70), 2, 1, [(16, 12, 70)], None),
    ((16, 12, 70), 2, 1, [(16, 12, 70)], {0: (2, 1, 0)}),     # x fastest
    ((16, 12, 70), 2, 1, [(16, 12, 70)], {0: (0, 2, 1)}),     # y fastest
    ((3, 4, 70), 2, 1, [(3, 4, 70)], None),                   # the send slabs in x are one plane: two launches
    ((16, 12, 70), 4, 2, [(16, 12, 70)], None),               # width 2
    ((16, 12, 70), 2, 1, [(17, 12, 70)], None),               # a staggered field
    ((16, 12, 70), 2, 1, [(16, 12, 70), (17, 12, 70), (16, 13, 71)], {2: (2, 1, 0)}),  # three fields in one call
    ((70, 66, 130), 4, 2, [(70, 66, 130), (70, 67, 130)], None),  # long enough for the chunk and gather paths
])
def test_one_periodic_rank_gpu_against_cpu_bitwise(gpu, n, overlap, width, shapes, layouts, dtype):
    igg.init_global_grid(*n, periodx=1, periody=1, periodz=1, overlapx=overlap, overlapy=overlap, overlapz=overlap,
                         halowidthx=width, halowidthy=width, halowidthz=width, quiet=True, init_MPI=False)
    C = _fields(shapes, dtype, layouts)
    Gp = [c.to(gpu) for c in C]
    for c, g in zip(C, Gp):
        assert g.stride() == c.stride()
    for rep in range(2):  # the second call starts from zero halos and changes the send slabs no more
        igg.accumulate_halo_(*C)
        igg.accumulate_halo_(*Gp)
        for k, (c, g) in enumerate(zip(C, Gp)):
            assert _same_bits(g.cpu(), c), f"call {rep}, field {k} {shapes[k]}: {int((g.cpu() != c).sum())} cells differ"
    igg.finalize_global_grid(finalize_MPI=False)


def test_a_captured_call_replays(gpu):
    """One eager call, then a capture; two replays equal two eager calls."""
    from igg.parallel import halo as HL

    igg.init_global_grid(16, 12, 70, periodx=1, periody=1, periodz=1, quiet=True, init_MPI=False)
    a0, b0 = _fields([(16, 12, 70), (17, 12, 70)], torch.float64, seed=5)
    A, B = a0.to(gpu), b0.to(gpu)
    igg.accumulate_halo_(A, B)  # eager: the buffers exist
    A.copy_(a0)
    B.copy_(b0)
    # keep a deposit in the halos between the replays: the second one has something to move
    graph = HL.capture_graph(lambda: (igg.accumulate_halo_(A, B), A.add_(1.0), B.add_(1.0)), "accumulate_halo_")
    A.copy_(a0)
    B.copy_(b0)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    Ea, Eb = a0.to(gpu), b0.to(gpu)
    for _ in range(2):
        igg.accumulate_halo_(Ea, Eb)
        Ea.add_(1.0)
        Eb.add_(1.0)
    assert _same_bits(A, Ea) and _same_bits(B, Eb)
    Ca, Cb = a0.clone(), b0.clone()
    for _ in range(2):
        igg.accumulate_halo_(Ca, Cb)
        Ca.add_(1.0)
        Cb.add_(1.0)
    assert _same_bits(A.cpu(), Ca) and _same_bits(B.cpu(), Cb)
    igg.finalize_global_grid(finalize_MPI=False)


def test_gpu_dtype_and_loopback_are_refused(gpu):
    igg.init_global_grid(16, 12, 70, periodx=1, periody=1, periodz=1, quiet=True, init_MPI=False)
    for dt in (torch.float16, torch.int32, torch.complex64):
        A = torch.ones(16, 12, 70, dtype=dt, device=gpu)
        with pytest.raises(igg.IGGError, match="GPU fields must be float32 or float64"):
            igg.accumulate_halo_(A)
        assert (A == 1).all()
    igg.finalize_global_grid(finalize_MPI=False)
    from igg.parallel import halo as HL

    igg.init_global_grid(16, 12, 70, periodx=1, periody=1, periodz=1, quiet=True, init_MPI=False)
    HL.enable_loopback()
    A = torch.ones(16, 12, 70, dtype=torch.float64, device=gpu)
    with pytest.raises(igg.IGGError, match="loopback emulation has no transposed exchange"):
        igg.accumulate_halo_(A)
    assert (A == 1).all()
    igg.finalize_global_grid(finalize_MPI=False)


def test_autograd_on_the_gpu(gpu):
    igg.init_global_grid(16, 12, 70, periodx=1, periody=1, periodz=1, quiet=True, init_MPI=False)
    c, a = _fields([(16, 12, 70), (16, 12, 70)], torch.float64, seed=9)
    c = c.to(gpu)
    A = a.to(gpu).requires_grad_(True)
    (c * igg.autograd.update_halo(A)).sum().backward()
    want = c.clone()
    igg.accumulate_halo_(want)
    assert _same_bits(A.grad, want)
    igg.finalize_global_grid(finalize_MPI=False)


# ------------------------------------------------------- ranks sharing device 0
@pytest.mark.parametrize("nprocs,dtype,args", [
    (2, "float64", (2, 1, 1, 0, 2, 1)),
    (4, "float32", (2, 1, 2, 5, 4, 2)),   # periodic x and z, overlap 4, width 2: both neighbours are one peer
    (8, "float64", (2, 2, 2, 0, 2, 1)),
])
def test_multi_rank_on_one_device(gpu, nprocs, dtype, args):
    # ranks share one GPU: RCCL cannot, the messages are staged through the host
    run_accumulate_ranks(nprocs, "accumulate", "gpu", dtype, *args, timeout=120,
                         env_extra={"IGG_TRANSPORT": "staged"})


@pytest.mark.multigpu
def test_two_ranks_on_two_devices_over_rccl(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: one rank per device over RCCL")
    run_accumulate_ranks(2, "accumulate", "mgpu", "float64", 2, 1, 1, 0, 2, 1, timeout=150,
                         env_extra={"IGG_TRANSPORT": "rccl"})
