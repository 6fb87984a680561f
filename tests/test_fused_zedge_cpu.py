"""The z-edge lane rule of the fused diffusion kernels (csrc/include/igg/zedge.hpp)
over its whole space, without a device.

A wave keeps the z-face values of its rows one per lane: low-edge row r in lane
r; high-edge row r in lane 32 + r (readlane form) or in lane zh - r (DPP form,
fused variant 48). ``native.fused_zedge_lane`` is the rule for one lane's
source and destination as zedge.hpp states it (the kernel takes the side and
row of a DPP lane's destination from the same functions and spells the rest
out; tests/test_gpu_fused_z_edges.py holds the kernel to it). Here every (form,
RY, nv, zh, sides) the launch admits is enumerated and each side's lanes must
map one-to-one onto the rows 0..nv-1, at the promised lanes. The rule the
kernel had before (the row offset taken from the low edge whenever the lane
also held a low-edge row) is evaluated once as well: it swaps rows exactly
where arithmetic says it must.
"""
import itertools

import pytest

from igg.ops import stencil

native = stencil.native
lane_rule = native.fused_zedge_lane
SIDES = list(itertools.product([False, True], repeat=4))  # (in_lo, in_hi, out_lo, out_hi)


def _admitted(dpp, ry, zh, sides):
    in_lo, in_hi, out_lo, out_hi = sides
    if not dpp:
        return True  # the readlane form also runs a wave that holds both edges
    # one z edge per wave, and the high edge's rows inside the edge lane's DPP row
    one_edge = not ((in_lo or out_lo) and (in_hi or out_hi))
    return one_edge and native.fused_zedge_dpp_rows_fit(zh, ry)


def _promised(dpp, side, zh, r):
    if side == 0:
        return r
    return zh - r if dpp else 32 + r


def _old_rule(dpp, lane, zh, nv, out_lo, out_hi):
    """(dst, dst_row) as fused_impl.hpp computed them before zedge.hpp."""
    rl = lane & 31
    rh = zh - lane if dpp else rl
    lo = lane < 32 and rl < nv
    hi = (0 <= rh < nv) if dpp else (lane >= 32 and rl < nv)
    row = rh if (hi and not lo) else rl
    dst = 0 if (lo and out_lo) else (1 if (hi and out_hi) else -1)
    return dst, (row if dst >= 0 else 0)


def _check_side(lanes, active, side, dpp, zh, nv, what):
    """lanes: {lane: row} of the lanes that take `side`."""
    bad = []
    if not active:
        if lanes:
            bad.append(f"{what} side {side} inactive but lanes {sorted(lanes)} take it")
        return bad
    want = {_promised(dpp, side, zh, r): r for r in range(nv)}
    if lanes != want:
        diff = {l: (lanes.get(l), want.get(l)) for l in sorted(set(lanes) | set(want)) if lanes.get(l) != want.get(l)}
        bad.append(f"{what} side {side}: lane -> (row, promised row) {diff}")
    return bad


def _case(rule_dst, dpp, zh, nv, sides):
    """Failures of one wave; rule_dst(lane) -> (dst, dst_row) lets the old rule stand in."""
    in_lo, in_hi, out_lo, out_hi = sides
    src = {0: {}, 1: {}}
    dst = {0: {}, 1: {}}
    bad = []
    for lane in range(64):
        lo, hi, rl, rh, s, srow, _d, _drow = lane_rule(dpp, lane, zh, nv, *sides)
        d, drow = rule_dst(lane)
        assert s in (-1, 0, 1) and d in (-1, 0, 1)  # at most one source, one destination
        for side, row, table in ((s, srow, src), (d, drow, dst)):
            if side >= 0:
                if not 0 <= row < nv:
                    bad.append(f"lane {lane}: row {row} outside [0, {nv})")
                table[side][lane] = row
        # the lane classes themselves
        assert lo == (lane < nv) and rl == lane % 32
        assert hi == (0 <= _promised(dpp, 1, zh, 0) - lane < nv if dpp else 32 <= lane < 32 + nv)
        if hi:
            assert _promised(dpp, 1, zh, rh) == lane
    bad += _check_side(src[0], in_lo, 0, dpp, zh, nv, "receive")
    bad += _check_side(src[1], in_hi, 1, dpp, zh, nv, "receive")
    bad += _check_side(dst[0], out_lo, 0, dpp, zh, nv, "send")
    bad += _check_side(dst[1], out_hi, 1, dpp, zh, nv, "send")
    return bad


def _space():
    for dpp in (False, True):
        for ry in (4, 8):
            for nv in range(1, ry + 1):
                for zh in range(64):
                    for sides in SIDES:
                        if _admitted(dpp, ry, zh, sides):
                            yield dpp, ry, nv, zh, sides


def test_launch_predicates():
    """zh on the host, one wave with both edges, and the DPP guard."""
    for vz in (2, 4):
        for n2 in range(2 * vz, 3 * 64 * vz + 1, vz):
            zh = native.fused_zedge_zh(n2, vz)
            assert zh == ((n2 - vz) % (64 * vz)) // vz and 0 <= zh < 64
            assert native.fused_zedge_one_wave(n2, vz) == (n2 <= 65 * vz)
            for ry in (4, 8):
                assert native.fused_zedge_dpp_rows_fit(zh, ry) == (zh % 16 >= ry - 1)
                assert native.fused_zedge_dpp_ok(n2, vz, ry) == (n2 > 65 * vz and zh % 16 >= ry - 1)
    assert not native.fused_zedge_dpp_rows_fit(63, 17)  # a 16-lane DPP row holds at most 16 rows


def test_every_side_maps_lanes_one_to_one_onto_rows():
    n = 0
    failures = []
    for dpp, ry, nv, zh, sides in _space():
        n += 1
        bad = _case(lambda lane: lane_rule(dpp, lane, zh, nv, *sides)[6:8], dpp, zh, nv, sides)
        if bad:
            failures.append((dpp, ry, nv, zh, sides, bad[:2]))
    # readlane: 4 + 8 (RY, nv) pairs x 64 zh x 16 side sets; DPP: the admitted zh x 7 one-edge side sets
    assert n == 12 * 64 * 16 + 7 * (4 * 13 * 4 + 8 * 9 * 4)
    assert not failures, f"{len(failures)} waves, first: {failures[:3]}"


def test_old_rule_swaps_rows_where_derived():
    """The rule before zedge.hpp fails this file's check exactly where a DPP
    wave sends high only and some lane L < nv also holds high row zh - L != L."""
    got = set()
    for dpp, ry, nv, zh, sides in _space():
        bad = _case(lambda lane: _old_rule(dpp, lane, zh, nv, sides[2], sides[3]), dpp, zh, nv, sides)
        if bad:
            assert dpp and sides[2:] == (False, True), (dpp, ry, nv, zh, sides, bad[:2])
            got.add((ry, nv, zh))
    want = {(ry, nv, zh) for ry in (4, 8) for nv in range(1, ry + 1) for zh in range(64)
            if zh % 16 >= ry - 1 and any(0 <= zh - L < nv and zh - L != L for L in range(nv))}
    assert got == want
    # variant 48's tiling (RY = 8), full waves: zh 7..13 swap rows L and zh - L, zh = 14 does not
    assert sorted(zh for ry, nv, zh in got if ry == 8 and nv == 8) == list(range(7, 14))
    assert sorted((nv, zh) for ry, nv, zh in got if ry == 8 and nv < 8) == [
        (5, 7), (6, 7), (6, 8), (6, 9), (7, 7), (7, 8), (7, 9), (7, 10), (7, 11)]
    # what is stored where: lane L keeps row zh - L's value and the old offset was row L's
    for zh in range(7, 14):
        for L in range(8):
            if 0 <= zh - L < 8:
                assert _old_rule(True, L, zh, 8, False, True) == (1, L)
                assert lane_rule(True, L, zh, 8, False, False, False, True)[6:8] == (1, zh - L)


@pytest.mark.parametrize("v", stencil.compiled_fused_variants())
def test_fused_tile_query(v):
    by, ry, vz, bz, dpp = native.diffusion3d_fused_tile(v)
    assert by * bz == 4 and ry in (4, 8) and vz in (2, 4) and bz in (1, 2)
    assert dpp == (v == 48)
    if v < 21 and v in stencil.compiled_variants():  # a plain vector variant's id: the same z tile
        assert native.diffusion3d_variant_tile(v) == 64 * vz * bz
