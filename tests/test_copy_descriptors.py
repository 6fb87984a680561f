"""Copy descriptors, CPU tier: the host-side plan of the batched copy kernels
(csrc/copy_plan.cpp through native.copy2d_plan / copy3d_plan) and the host
copies, against the index-arithmetic oracle of tests/copy_oracle.py. The GPU
tier (tests/test_gpu_copy_descriptors.py) runs the same tables through the
kernels."""
import numpy as np
import pytest

from igg._native import native
from tests import copy_oracle as O

FAKE_SRC, FAKE_DST = 1 << 30, 1 << 31  # the plan computes with addresses, it never reads them


def _plan(case_box, ptrs, eb):
    if len(case_box) == 9:
        return native.copy3d_plan(list(case_box), ptrs, eb)
    return native.copy2d_plan(tuple(ptrs) + tuple(case_box), eb)


def _pairs(box):
    """Sorted (source offset, destination offset) pairs of a box."""
    s, d = O.offsets(box)
    p = np.stack([s, d], axis=1)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def _random_boxes(n=300, seed=2024):
    """Boxes with extents 1-80 whose sides are regions of dense, padded or
    permuted fields (each side drawn on its own), n_inner sometimes 1; with
    element size and (fake) base addresses of every alignment."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ext = [int(v) for v in rng.integers(1, 81, 3)]
        r = rng.random()
        if r < 0.25:
            ext[2] = 1
        elif r < 0.35:
            ext[1] = 1
        elif r < 0.5:
            ext[2] = int(rng.choice([2, 3, 4, 8, 16]))  # short rows: the vector candidates

        def side():
            kind = rng.integers(0, 4)
            field = [e + int(rng.integers(0, 3)) * int(kind != 0) for e in ext]  # the box is a region of a field
            order = tuple(int(v) for v in rng.permutation(3)) if kind == 3 else (0, 1, 2)
            pad = int(rng.integers(1, 9)) if kind == 2 else 0
            st, _total = O.field_strides(field, order, pad)
            return st

        eb = int(rng.choice(O.ELEM_BYTES))
        step = 1
        if rng.random() < 0.35:
            # candidates for vector rows: 64-80 rows of 4, 8 or 16 bytes in a
            # field whose row pitch is mostly, not always, a multiple of the
            # row; bases mostly, not always, a multiple of it
            ext[1] = int(rng.integers(64, 81))
            ext[2] = step = int(rng.choice([v for v in (4, 8, 16) if v >= eb])) // eb

            def side():  # noqa: F811
                row = ext[2] * int(rng.integers(1, 5)) + int(rng.random() < 0.15)
                return (ext[1] * row + row * int(rng.integers(0, 3)), row, 1)

        ss, ds = side(), side()
        ptrs = tuple(p + int(rng.integers(0, 32)) * eb * (step if rng.random() < 0.7 else 1)
                     for p in (FAKE_SRC, FAKE_DST))
        out.append((tuple(ext) + ss + ds, ptrs, eb))
    return out


RANDOM = _random_boxes()


def _named(eb, base=0):
    """(case, box, ptrs) of every named case of both kernels in its arena slot."""
    out = []
    for table in (O.cases3d(), O.cases2d()):
        a = O.Arena(table, eb, base)
        out += [(c, c.box, a.pointers(k, FAKE_SRC, FAKE_DST)) for k, c in enumerate(a.cases)]
    return out


# ------------------------------------------------------------ normalisation
def test_normalisation_preserves_the_copy_named_cases():
    for c, box, ptrs in _named(4):
        p = _plan(box, ptrs, 4)
        assert np.array_equal(_pairs(p["box"]), _pairs(box)), (c.name, p)


def test_normalisation_preserves_the_copy_random_boxes():
    assert len(RANDOM) == 300
    seen = set()
    for box, ptrs, eb in RANDOM:
        p = native.copy3d_plan(list(box), ptrs, eb)
        assert np.array_equal(_pairs(p["box"]), _pairs(box)), (box, p)
        seen.add(p["path"])
    assert seen == {"flat", "gather", "chunk"}  # the random boxes are not all of one kind


def test_normalised_box_keeps_outer_only_with_rows():
    """What the kernel's decode relies on: n_outer > 1 only with n_mid > 1."""
    for box, ptrs, eb in RANDOM:
        no, nm = native.copy3d_plan(list(box), ptrs, eb)["box"][:2]
        assert no == 1 or nm > 1, box


# --------------------------------------------------------------------- plan
def test_named_cases_take_the_path_they_are_named_for():
    for eb in O.ELEM_BYTES:
        for c, box, ptrs in _named(eb):
            p = _plan(box, ptrs, eb)
            assert p["path"] == c.path, (eb, c.name, p)
            assert p["vec_bytes"] == c.vec.get(eb, 0), (eb, c.name, p)


def test_every_path_and_vector_width_is_reached():
    """Asserted over the tables, so that a later change of a threshold cannot
    quietly leave a path of either kernel without a case."""
    paths3, paths2, pairs = set(), set(), set()
    for eb in O.ELEM_BYTES:
        for c, box, ptrs in _named(eb):
            p = _plan(box, ptrs, eb)
            (paths3 if c.is3d else paths2).add(p["path"])
            if p["vec_bytes"]:
                assert c.is3d and p["path"] == "gather"
                pairs.add((eb, p["vec_bytes"]))
    assert paths3 == {"flat", "gather", "chunk"}
    assert paths2 == {"flat", "gather", "chunk"}
    want = {(eb, v) for v in (4, 8, 16) for eb in O.ELEM_BYTES if v >= eb}
    assert len(want) == 12 and pairs == want, sorted(want - pairs)
    # shapes of the gather and chunk decodes the slab exchange does not produce
    kept = [native.copy3d_plan(list(c.box), (FAKE_SRC, FAKE_DST), 4) for c in O.cases3d()]
    assert any(p["path"] == "chunk" and p["box"][0] > 1 and p["box"][1] > 1 for p in kept)
    assert any(p["path"] == "chunk" and p["box"][5] != 1 for p in kept)          # strided chunk
    assert any(p["path"] == "gather" and p["box"][2] == 1 and p["vec_bytes"] for p in kept)  # rows of 1
    assert {p["box"][0] for p in kept if p["path"] == "gather"} >= {31, 32, 33}


def _row_addresses(box, ptr, eb, side):
    no, nm = box[0], box[1]
    so, sm = box[3 + 3 * side], box[4 + 3 * side]
    o = np.arange(no, dtype=np.int64)[:, None]
    m = np.arange(nm, dtype=np.int64)[None, :]
    return ptr + (o * so + m * sm).ravel() * eb


def _check_vec(p, ptrs, eb, what):
    v = p["vec_bytes"]
    assert v in (0, 4, 8, 16), what
    if v:
        box = p["box"]
        assert p["path"] == "gather" and box[2] * eb == v and box[5] == 1 and box[8] == 1, what
        for side in (0, 1):
            assert not np.any(_row_addresses(box, ptrs[side], eb, side) % v), (what, "misaligned row", side)


def test_vector_rows_are_never_misaligned():
    nvec = nrej = 0
    for box, ptrs, eb in RANDOM:
        p = native.copy3d_plan(list(box), ptrs, eb)
        _check_vec(p, ptrs, eb, box)
        nvec += bool(p["vec_bytes"])
        nrej += p["path"] == "gather" and p["box"][2] * eb in (4, 8, 16) and not p["vec_bytes"]
    assert nvec >= 20 and nrej >= 20, (nvec, nrej)  # the property is exercised both ways, not vacuous
    # the named cases at every base: an odd base must switch the vector rows off
    for eb in O.ELEM_BYTES:
        for base in O.BASES:
            for c, box, ptrs in _named(eb, base):
                if c.is3d:
                    _check_vec(_plan(box, ptrs, eb), ptrs, eb, (c.name, eb, base))


def test_a_misaligned_base_switches_vector_rows_off():
    box = list(O.field_slab((9, 10, 72), 2, 4, 4)["pack"]["box"])
    assert native.copy3d_plan(box, (FAKE_SRC, FAKE_DST), 4)["vec_bytes"] == 16
    for ds, dd in ((4, 0), (0, 8), (12, 12)):
        assert native.copy3d_plan(box, (FAKE_SRC + ds, FAKE_DST + dd), 4)["vec_bytes"] == 0


def _blocks(p, is3d):
    b = p["box"]
    cdiv = lambda a, d: -(-a // d)  # noqa: E731
    if is3d:
        no, nm, ni = b[:3]
        return {"flat": cdiv(no * nm * ni, 256), "gather": cdiv(nm, 64) * cdiv(no, 32),
                "chunk": no * nm * cdiv(ni, 1024)}[p["path"]]
    no, ni = b[:2]
    return {"flat": cdiv(no * ni, 256), "gather": cdiv(ni, 64) * cdiv(no, 32), "chunk": no * cdiv(ni, 1024)}[p["path"]]


def test_blocks_match_the_formula_of_the_path():
    for eb in (1, 16):
        for c, box, ptrs in _named(eb):
            p = _plan(box, ptrs, eb)
            assert p["blocks"] == _blocks(p, c.is3d) and p["blocks"] > 0, (c.name, p)
    for box, ptrs, eb in RANDOM:
        p = native.copy3d_plan(list(box), ptrs, eb)
        assert p["blocks"] == _blocks(p, True) and p["blocks"] > 0, (box, p)
    for c in O.batch70() + O.batch70_2d():
        if c.path is None:
            assert _plan(c.box, (FAKE_SRC, FAKE_DST), 4)["blocks"] == 0, c.name


# --------------------------------------------------------------- host copies
def _run_host(arena, which=None):
    src, dst = O.aligned_buffer(arena.src), O.aligned_buffer(arena.dst)
    if arena.cases[0].is3d or any(c.is3d for c in arena.cases):
        boxes, ptrs = arena.args3d(src.ctypes.data, dst.ctypes.data, which)
        native.copy3d(boxes, ptrs, arena.eb, False)
    else:
        native.copy2d(arena.args2d(src.ctypes.data, dst.ctypes.data, which), arena.eb, False)
    assert np.array_equal(src, arena.src), "a host copy wrote into the source allocation"
    return dst


@pytest.mark.parametrize("fam", O.FAMILIES3D + O.FAMILIES2D)
def test_host_copies_match_the_oracle(fam):
    """One call per case (so no case depends on another), all cases of a
    family in one pair of allocations, compared whole."""
    for eb in O.ELEM_BYTES:
        a = O.Arena(O.family(fam), eb, base=1)
        src, dst = O.aligned_buffer(a.src), O.aligned_buffer(a.dst)
        for k in range(len(a.cases)):
            if a.cases[k].is3d:
                native.copy3d(*a.args3d(src.ctypes.data, dst.ctypes.data, [k]), eb, False)
            else:
                native.copy2d(a.args2d(src.ctypes.data, dst.ctypes.data, [k]), eb, False)
        assert O.first_difference(dst, a.expected(), eb) is None, (fam, eb, O.first_difference(dst, a.expected(), eb))


def test_host_copy_above_the_thread_threshold():
    """Regions of more than THREADCOPY_THRESHOLD (32 KiB) bytes take the threaded split."""
    # (host_copy3d threads each of its n_outer planes by the plane's own size)
    big3 = O.Case(name="big3", family="big", **O.field_slab((3, 3000, 40), 2, 4, 4)["pack"])
    big2 = O.Case(name="big2", family="big", box=(700, 65, 65 * 3 + 5, 3, 65, 1))
    assert big3.box[1] * big3.box[2] * 4 >= 32768 and big2.box[0] * big2.box[1] >= 32768
    for eb in O.ELEM_BYTES:
        for case in (big3, big2):
            a = O.Arena([case], eb, base=3)
            dst = _run_host(a)
            assert O.first_difference(dst, a.expected(), eb) is None, (case.name, eb)


@pytest.mark.parametrize("maker", [O.batch70, O.batch70_2d])
def test_host_batch_of_70_with_empty_boxes(maker):
    for eb in (1, 8, 16):
        a = O.Arena(maker(), eb, base=0)
        assert len(a.cases) == 70 and [k for k, c in enumerate(a.cases) if c.path is None] == [0, 31, 32, 69]
        dst = _run_host(a)
        assert O.first_difference(dst, a.expected(), eb) is None, eb


# ---------------------------------------------------------- harness self-test
def _one(box, **kw):
    return O.Arena([O.Case(name="t", family="t", box=tuple(box), **kw)], 4, base=1)


def test_comparison_fails_for_a_wrong_copy():
    """A comparator that cannot fail proves nothing: a short row, a stride off
    by one and a flipped guard byte must each be seen."""
    s = O.field_slab((9, 10, 70), 2, 2, 2)["pack"]
    a = _one(**s)
    good = a.expected()
    assert O.first_difference(good.copy(), good, 4) is None
    so, do, box, inplace = a.copies[0]
    short = box[:2] + (box[2] - 1,) + box[3:]
    assert O.first_difference(a.expected([(so, do, short, inplace)]), good, 4) is not None
    compared = 0
    for k in (3, 4, 6, 7):  # an outer or mid stride of either side, one element off
        off = tuple(v + (1 if j == k else 0) for j, v in enumerate(box))
        try:
            wrong = a.expected([(so, do, off, inplace)])
        except AssertionError:
            continue  # the oracle's own input checks caught it (overlapping destination)
        assert O.first_difference(wrong, good, 4) is not None, k
        compared += 1
    assert compared >= 2
    flipped = good.copy()
    guard = (do + O.span(O.offsets(box)[1]) + 5) * 4  # inside the guard zone after the region
    flipped[guard] ^= 1
    assert "1 elements differ" in O.first_difference(flipped, good, 4)
    # and through the host copy: the same wrong boxes, run for real
    src, dst = O.aligned_buffer(a.src), O.aligned_buffer(a.dst)
    native.copy3d([list(short)], [a.pointers(0, src.ctypes.data, dst.ctypes.data)], 4, False)
    assert O.first_difference(dst, good, 4) is not None


def test_oracle_rejects_order_dependent_batches():
    a = _one(**O.field_slab((9, 10, 70), 2, 2, 2)["move"])
    so, do, box, inplace = a.copies[0]
    with pytest.raises(AssertionError, match="source element"):
        a.expected([(so, so + 1, box, True)])  # destination slab overlaps the source slab
    with pytest.raises(AssertionError, match="overlap"):
        a.expected([(so, do, box, True), (so, do + 1, box, True)])
    with pytest.raises(AssertionError, match="outside"):
        a.expected([(so, a.n_dst, box, True)])


def test_pattern_distinguishes_neighbours():
    for eb in O.ELEM_BYTES:
        p = O.pattern(70000, eb).reshape(-1, eb)
        v = p[:, :min(eb, 8)].copy().view({1: "u1", 2: "<u2", 4: "<u4"}.get(eb, "<u8")).ravel()
        for step in (1, 2, 7, 70, 131, 8777):  # element, row and plane neighbours of the tables' fields
            assert not np.any(v[step:] == v[:-step]), (eb, step)
