"""Oracle and case tables for the batched copy kernels (``native.copy2d`` /
``native.copy3d``; csrc/kernels/copy_kernels.hip, csrc/copy_plan.cpp).

The oracle is plain index arithmetic: for every ``(o, m, i)`` of a box it sets
``dst[o*dso + m*dsm + i*dsi] = src[o*sso + m*ssm + i*ssi]`` on ``uint8`` arrays
viewed with the element size. It knows nothing of the launcher's rewrite of a
box (``normalized``), of paths or of vector rows; the tests compare the WHOLE
destination allocation with it, byte for byte, so a moved value and a byte that
must not have been touched weigh the same.

A box is the 9-tuple ``(n_outer, n_mid, n_inner, src_so, src_sm, src_si,
dst_so, dst_sm, dst_si)`` of ``native.copy3d`` or the 6-tuple ``(n_outer,
n_inner, src_so, src_si, dst_so, dst_si)`` of ``native.copy2d``; strides are
in elements. No test functions live here (tests/test_copy_descriptors.py,
tests/test_gpu_copy_descriptors.py).
"""
from __future__ import annotations

from dataclasses import dataclass, field as _dc_field

import numpy as np

ELEM_BYTES = (1, 2, 4, 8, 16)
BASES = (0, 1, 3)   # elements between the start of an allocation slot and the region
GUARD = 64          # elements after every region that nothing may touch
SLOT_ALIGN = 16     # slots start at multiples of 16 elements: `base` alone sets the alignment
MAX_BATCH = 32      # regions per launch (igg/copy.hpp)


# ------------------------------------------------------------------- boxes
def box9(box):
    """A 2-D box as the 3-extent box that enumerates the same elements."""
    if len(box) == 9:
        return tuple(int(v) for v in box)
    no, ni, sso, ssi, dso, dsi = (int(v) for v in box)
    return (1, no, ni, 0, sso, ssi, 0, dso, dsi)


def offsets(box):
    """(source offsets, destination offsets) of every element of the box, in
    elements from the region's base; ``(o, m, i)`` order."""
    no, nm, ni, sso, ssm, ssi, dso, dsm, dsi = box9(box)
    if min(no, nm, ni) <= 0:
        e = np.zeros(0, dtype=np.int64)
        return e, e
    o = np.arange(no, dtype=np.int64)[:, None, None]
    m = np.arange(nm, dtype=np.int64)[None, :, None]
    i = np.arange(ni, dtype=np.int64)[None, None, :]
    return (o * sso + m * ssm + i * ssi).ravel(), (o * dso + m * dsm + i * dsi).ravel()


def span(offs):
    """Elements an allocation needs after the base to hold these offsets."""
    return int(offs.max()) + 1 if offs.size else 0


# ------------------------------------------------------------------ oracle
def apply(copies, elem_bytes, src_bytes, dst_bytes):
    """The destination allocation after the call. ``copies`` is a list of
    ``(src_off, dst_off, box, inplace)``: element offsets of the region bases
    into ``src_bytes`` / ``dst_bytes`` (``inplace``: the source is read from the
    destination allocation too). The inputs are not modified.

    Asserts what makes a batch independent of the order in which its elements
    move: every index lies inside its allocation, the destination element sets
    of the call are pairwise disjoint, and no destination element is a source
    element of the same call."""
    eb = int(elem_bytes)
    assert src_bytes.dtype == np.uint8 and dst_bytes.dtype == np.uint8
    assert src_bytes.size % eb == 0 and dst_bytes.size % eb == 0
    src = src_bytes.reshape(-1, eb)
    before = dst_bytes.reshape(-1, eb)
    out = before.copy()
    all_d, all_s_in_dst = [], []
    for src_off, dst_off, box, inplace in copies:
        so, do = offsets(box)
        if so.size == 0:
            continue
        so, do = so + int(src_off), do + int(dst_off)
        from_ = before if inplace else src
        assert so.min() >= 0 and so.max() < from_.shape[0], "source index outside its allocation"
        assert do.min() >= 0 and do.max() < out.shape[0], "destination index outside its allocation"
        out[do] = from_[so]
        all_d.append(do)
        if inplace:
            all_s_in_dst.append(so)
    if all_d:
        d = np.concatenate(all_d)
        assert np.unique(d).size == d.size, "destination elements of one call overlap"
        if all_s_in_dst:
            assert np.intersect1d(d, np.concatenate(all_s_in_dst)).size == 0, \
                "a destination element is a source element of the same call"
    return out.reshape(-1)


def pattern(n_elems, elem_bytes, first=0):
    """Source values: element k holds ``k*2654435761 mod 2^(8*eb)`` (little
    endian); 1-byte elements ``(k*97 + 13) mod 251``, so that neighbours in every
    direction differ."""
    k = np.arange(first, first + n_elems, dtype=np.uint64)
    if elem_bytes == 1:
        return ((k * np.uint64(97) + np.uint64(13)) % np.uint64(251)).astype(np.uint8)
    v = k * np.uint64(2654435761)  # < 2^64 for k < 2^32: the value itself, no wrap
    assert n_elems + first < 2 ** 32
    out = np.zeros((n_elems, elem_bytes), dtype=np.uint8)
    le = v.astype("<u8").view(np.uint8).reshape(n_elems, 8)
    out[:, :min(8, elem_bytes)] = le[:, :min(8, elem_bytes)]
    return out.reshape(-1)


# ------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    name: str
    family: str
    box: tuple               # 9-tuple (copy3d) or 6-tuple (copy2d)
    src_off: int = 0         # region base, elements after the slot start
    dst_off: int = 0
    src_span: int = 0        # elements of the source object (0: what the box reaches)
    dst_span: int = 0
    inplace: bool = False    # source and destination in one object (dst allocation)
    path: str | None = None  # path of the kernel the case is named for
    vec: dict = _dc_field(default_factory=dict, hash=False, compare=False)  # elem_bytes -> vec_bytes at base 0

    @property
    def is3d(self):
        return len(self.box) == 9

    def spans(self):
        so, do = offsets(self.box)
        return (max(self.src_span, self.src_off + span(so)), max(self.dst_span, self.dst_off + span(do)))


def field_strides(shape, order=None, pad=0):
    """Strides (elements) of a field of ``shape`` stored in memory order
    ``order`` (slowest dimension first; default C order), every row of the
    fastest dimension followed by ``pad`` unused elements. Returns (strides,
    elements of the allocation)."""
    order = tuple(order) if order is not None else tuple(range(len(shape)))
    st = [0] * len(shape)
    acc = 1
    for k, d in enumerate(reversed(order)):
        st[d] = acc
        acc *= shape[d] + (pad if k == 0 else 0)
    return tuple(st), acc


def field_slab(shape, dim, lo, w, order=None, pad=0):
    """Boxes of the slab ``lo <= index[dim] < lo + w`` of a field: its pack
    (field -> packed buffer), its unpack (packed buffer -> field) and its
    in-place move to the receive slab at the far end of ``dim`` (the
    self-periodic exchange). The extents are ordered by decreasing stride, as
    region_face (csrc/halo.cpp) orders them; the packed image has the region's
    memory order. Returns ``{"pack"|"unpack"|"move": dict(box, src_off,
    dst_off, src_span, dst_span, inplace)}``."""
    st, total = field_strides(shape, order, pad)
    ext = [w if d == dim else shape[d] for d in range(3)]
    dims = sorted(range(3), key=lambda d: (-st[d], d))
    n = tuple(ext[d] for d in dims)
    fs = tuple(st[d] for d in dims)
    ps = (n[1] * n[2], n[2], 1)
    packed = n[0] * n[1] * n[2]
    off = lo * st[dim]
    lo2 = shape[dim] - w if lo + w <= shape[dim] - w else 0
    assert lo2 + w <= lo or lo + w <= lo2, "the move's slabs overlap"
    return {
        "pack": dict(box=n + fs + ps, src_off=off, dst_off=0, src_span=total, dst_span=packed, inplace=False),
        "unpack": dict(box=n + ps + fs, src_off=0, dst_off=off, src_span=packed, dst_span=total, inplace=False),
        "move": dict(box=n + fs + fs, src_off=off, dst_off=lo2 * st[dim], src_span=0, dst_span=total, inplace=True),
    }


def _slab_cases(name, family, path, vec, shape, dim, w, lo=None, order=None, pad=0, layouts=("pack", "unpack", "move")):
    if lo is None:
        lo = min(w, shape[dim] - 2 * w)
    s = field_slab(shape, dim, lo, w, order, pad)
    return [Case(name=f"{name}/{k}", family=family, path=path, vec=dict(vec), **s[k]) for k in layouts]


def _direct(name, family, path, vec, box, swap=False):
    """A box given by its extents and strides; ``swap`` exchanges the sides."""
    b = tuple(box)
    if swap:
        b = b[:3] + b[6:9] + b[3:6]
    return Case(name=name, family=family, path=path, vec=dict(vec), box=b)


def _packed(n):
    return (n[1] * n[2], n[2], 1)


F = (12, 67, 131)  # the odd field: 67 rows (no multiple of 4 * GROWS), odd row stride
FS, _ = field_strides(F)


def cases3d():
    """Named copy3d cases, by family. The path in each case is the one the
    case is named for; native.copy3d_plan is asserted against it."""
    c = []
    # --- flat
    c += _slab_cases("flat:slab(5,6,7)z2", "flat", "flat", {}, (5, 6, 7), 2, 2)
    c += [_direct("flat:box(1,5,51)pad60", "flat", "flat", {}, (1, 5, 51, 300, 60, 1) + _packed((1, 5, 51)))]  # 255
    c += [_direct("flat:box(1,8,32)pad40", "flat", "flat", {}, (1, 8, 32, 320, 40, 1) + _packed((1, 8, 32)))]  # 256
    # (257 is prime: no flat box has 257 elements; the first size past one block)
    c += [_direct("flat:box(2,3,43)pad", "flat", "flat", {}, (2, 3, 43, 200, 50, 1) + _packed((2, 3, 43)))]  # 258
    c += [_direct("flat:corner(3,3,3)", "flat", "flat", {}, (3, 3, 3) + FS + _packed((3, 3, 3)))]
    # --- gather, vector rows
    c += _slab_cases("vec:slab(9,10,70)z2", "gather_vec", "gather", {2: 4, 4: 8, 8: 16}, (9, 10, 70), 2, 2)
    c += _slab_cases("vec:slab(9,10,72)z4@4", "gather_vec", "gather", {1: 4, 2: 8, 4: 16}, (9, 10, 72), 2, 4, lo=4)
    c += _slab_cases("vec:slab(9,10,72)z8@8", "gather_vec", "gather", {1: 8, 2: 16}, (9, 10, 72), 2, 8, lo=8)
    c += _slab_cases("vec:slab(5,16,64)z16@16", "gather_vec", "gather", {1: 16}, (5, 16, 64), 2, 16, lo=16)
    c += [_direct("vec:rows_of_1(70,1,1)", "gather_vec", "gather", {4: 4, 8: 8, 16: 16}, (70, 1, 1, 5, 1, 1, 1, 1, 1))]
    # --- gather, scalar rows (the vector test must fail)
    c += _slab_cases("scalar:slab(12,67,131)z2", "gather_scalar", "gather", {}, F, 2, 2)
    c += _slab_cases("scalar:slab(9,10,72)z4@1", "gather_scalar", "gather", {}, (9, 10, 72), 2, 4, lo=1)
    c += _slab_cases("scalar:slab(9,10,70)z3", "gather_scalar", "gather", {}, (9, 10, 70), 2, 3)
    c += _slab_cases("scalar:slab(12,67,131)z1", "gather_scalar", "gather", {}, F, 2, 1)
    c += [_direct("scalar:row(1,1,257)si3", "gather_scalar", "gather", {}, (1, 1, 257, 800, 800, 3, 257, 257, 1))]
    # --- gather, n_outer kept
    for shp in ((31, 64, 10), (32, 65, 10), (33, 65, 10)):
        c += _slab_cases(f"outer:slab{shp}z2".replace(" ", ""), "gather_outer", "gather", {2: 4, 4: 8, 8: 16}, shp, 2, 2)
    c += _slab_cases("outer:slab(12,67,131)[1,2,0]x2", "gather_outer", "gather", {2: 4, 4: 8, 8: 16}, F, 0, 2,
                     order=(1, 2, 0))
    # --- chunk
    c += _slab_cases("chunk:slab(12,67,131)y2", "chunk", "chunk", {}, F, 1, 2)
    c += _slab_cases("chunk:slab(12,67,131)x2", "chunk", "chunk", {}, F, 0, 2)
    for n2, pad in ((1023, 1), (1025, 7), (2049, 3)):
        c += _slab_cases(f"chunk:slab(4,3,{n2})x2pad{pad}", "chunk", "chunk", {}, (4, 3, n2), 0, 2, pad=pad)
    c += [_direct("chunk:box(3,5,1025)", "chunk", "chunk", {},
                  (3, 5, 1025, 5 * 1100 + 17, 1100, 1) + _packed((3, 5, 1025)))]
    c += [_direct("chunk:box(3,5,130)si2", "chunk", "chunk", {}, (3, 5, 130, 5 * 300 + 7, 300, 2) + _packed((3, 5, 130)))]
    c += [_direct("chunk:edge(2,2,131)", "chunk", "chunk", {}, (2, 2, 131) + FS + _packed((2, 2, 131)))]
    # --- layouts: the permuted memory orders of the odd field
    c += _slab_cases("layout:(12,67,131)[1,2,0]z2", "layouts", "gather", {}, F, 2, 2, order=(1, 2, 0))
    c += _slab_cases("layout:(12,67,131)[1,2,0]y3", "layouts", "chunk", {}, F, 1, 3, order=(1, 2, 0))
    c += _slab_cases("layout:(12,67,131)[2,0,1]z2", "layouts", "chunk", {}, F, 2, 2, order=(2, 0, 1))
    c += _slab_cases("layout:(12,67,131)[2,0,1]y3", "layouts", "gather", {}, F, 1, 3, order=(2, 0, 1))
    # the direct boxes also with the sides exchanged (packed source)
    c += [_direct(k.name + "/swapped", k.family, k.path, k.vec, k.box, swap=True)
          for k in list(c) if "/" not in k.name]
    return c


FAMILIES3D = ("flat", "gather_vec", "gather_scalar", "gather_outer", "chunk", "layouts")


def _path2d(n_inner, strided):
    return "flat" if n_inner < 64 else ("gather" if strided else "chunk")


def cases2d():
    """Named copy2d cases: every one as given (pack: the strided or padded
    side is the source where only one side is) and with the sides exchanged."""
    c = []
    for ni in (1, 63, 64, 65, 127, 129):
        for no in (1, 31, 32, 33, 65):
            # inner stride 3 / 2, rows 5 / 2 elements apart from the next
            s_str, s_den = (ni * 3 + 5, 3), (ni + 2, 1)
            d_str, d_den = (ni * 2 + 1, 2), (ni, 1)
            for kind, s, d in (("src", s_str, d_den), ("dst", s_den, d_str), ("both", s_str, d_str)):
                fam = "2d_" + _path2d(ni, True)
                c.append(Case(name=f"2d:{kind}-strided({no},{ni})", family=fam, path=_path2d(ni, True),
                              box=(no, ni) + s + d))
    for ni in (64, 1023, 1024, 1025, 2500):
        c.append(Case(name=f"2d:rows(3,{ni})padded", family="2d_chunk", path="chunk",
                      box=(3, ni, ni + 5, 1, ni, 1)))
    c += [Case(name=k.name + "/swapped", family=k.family, path=k.path,
               box=k.box[:2] + k.box[4:6] + k.box[2:4]) for k in list(c)]
    return c


FAMILIES2D = ("2d_flat", "2d_gather", "2d_chunk")


def family(name):
    table = cases2d() if name.startswith("2d_") else cases3d()
    out = [k for k in table if k.family == name]
    assert out, name
    return out


def batch70():
    """One call of 70 copy3d boxes cycling through every path (three launches:
    32 + 32 + 6), with empty boxes at positions 0, 31, 32 and 69."""
    pool = [k for k in cases3d() if k.name in (
        "flat:slab(5,6,7)z2/pack", "vec:slab(9,10,70)z2/pack", "chunk:box(3,5,130)si2", "scalar:slab(9,10,70)z3/unpack",
        "flat:corner(3,3,3)", "outer:slab(31,64,10)z2/move", "chunk:edge(2,2,131)", "vec:rows_of_1(70,1,1)",
        "scalar:row(1,1,257)si3", "chunk:slab(4,3,1023)x2pad1/unpack", "vec:slab(9,10,72)z4@4/move")]
    assert len(pool) == 11
    out = []
    for k in range(70):
        if k in (0, 31, 32, 69):
            z = [(0, 5, 7), (4, 0, 7), (4, 5, 0), (0, 0, 0)][len([e for e in out if e.path is None])]
            out.append(Case(name=f"empty{k}", family="batch", path=None, box=z + (35, 7, 1, 35, 7, 1)))
        else:
            p = pool[k % len(pool)]
            out.append(Case(name=f"{k}:{p.name}", family="batch", path=p.path, vec=p.vec, box=p.box, src_off=p.src_off,
                            dst_off=p.dst_off, src_span=p.src_span, dst_span=p.dst_span, inplace=p.inplace))
    return out


def batch70_2d():
    """The same for copy2d."""
    pool = [k for k in cases2d() if k.name in (
        "2d:src-strided(31,63)", "2d:dst-strided(33,65)", "2d:rows(3,1025)padded", "2d:both-strided(65,129)",
        "2d:rows(3,64)padded/swapped", "2d:src-strided(1,1)", "2d:both-strided(32,64)/swapped")]
    assert len(pool) == 7
    out = []
    for k in range(70):
        if k in (0, 31, 32, 69):
            out.append(Case(name=f"empty{k}", family="batch", path=None, box=((0, 9) if k % 2 else (9, 0)) + (9, 1, 9, 1)))
        else:
            p = pool[k % len(pool)]
            out.append(Case(name=f"{k}:{p.name}", family="batch", path=p.path, box=p.box))
    return out


# ------------------------------------------------------------------- arena
def _round_up(v, a):
    return (v + a - 1) // a * a


class Arena:
    """One source and one destination allocation that hold every case of a
    list, each in a slot of its own: the region's object starts ``base``
    elements into the slot and at least GUARD untouched elements follow it.
    The source holds ``pattern``; the destination seeded random bytes, except
    the objects of in-place cases, which hold the pattern too."""

    def __init__(self, cases, elem_bytes, base, seed=1234):
        self.cases, self.eb, self.base = list(cases), int(elem_bytes), int(base)
        s_cur = d_cur = 0
        self.copies = []
        inplace_objs = []
        for k in self.cases:
            ss, ds = k.spans()
            s0, d0 = s_cur + base, d_cur + base
            if k.inplace:
                self.copies.append((d0 + k.src_off, d0 + k.dst_off, k.box, True))
                inplace_objs.append((d0, ds))
            else:
                self.copies.append((s0 + k.src_off, d0 + k.dst_off, k.box, False))
                s_cur = _round_up(s0 + ss + GUARD, SLOT_ALIGN)
            d_cur = _round_up(d0 + ds + GUARD, SLOT_ALIGN)
        self.n_src, self.n_dst = max(s_cur, SLOT_ALIGN), max(d_cur, SLOT_ALIGN)
        self.src = pattern(self.n_src, self.eb)
        rng = np.random.default_rng(seed + 16 * self.eb + base)
        self.dst = rng.integers(0, 256, self.n_dst * self.eb, dtype=np.uint8)
        for d0, ds in inplace_objs:
            self.dst[d0 * self.eb:(d0 + ds) * self.eb] = pattern(ds, self.eb, first=d0)
        self._want = None

    def expected(self, copies=None):
        if copies is not None:
            return apply(copies, self.eb, self.src, self.dst)
        if self._want is None:
            self._want = apply(self.copies, self.eb, self.src, self.dst)
            self._want.setflags(write=False)
        return self._want

    def pointers(self, k, src_ptr, dst_ptr):
        """(source, destination) addresses of region k for allocations at these addresses."""
        so, do, _box, inplace = self.copies[k]
        return ((dst_ptr if inplace else src_ptr) + so * self.eb, dst_ptr + do * self.eb)

    def args3d(self, src_ptr, dst_ptr, which=None):
        """(boxes, ptrs) of native.copy3d for the listed regions (default all)."""
        which = range(len(self.cases)) if which is None else which
        return ([list(box9(self.copies[k][2])) for k in which], [self.pointers(k, src_ptr, dst_ptr) for k in which])

    def args2d(self, src_ptr, dst_ptr, which=None):
        which = range(len(self.cases)) if which is None else which
        return [self.pointers(k, src_ptr, dst_ptr) + tuple(self.copies[k][2]) for k in which]


def first_difference(got, want, elem_bytes):
    """None when the allocations are equal byte for byte, else a description
    of the first differing element."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.size != want.size:
        return f"sizes differ: {got.size} != {want.size}"
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    e = int(bad[0]) // elem_bytes
    sl = slice(e * elem_bytes, (e + 1) * elem_bytes)
    return (f"{np.unique(bad // elem_bytes).size} elements differ; first at element {e}: got "
            f"{bytes(got[sl]).hex()}, want {bytes(want[sl]).hex()}")


def aligned_buffer(data, align=256):
    """A copy of the bytes in a numpy buffer whose address is a multiple of ``align``."""
    raw = np.empty(data.size + align, dtype=np.uint8)
    off = (-raw.ctypes.data) % align
    out = raw[off:off + data.size]
    out[:] = data
    return out
