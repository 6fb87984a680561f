"""What the diffusion variant catalogue (csrc/include/igg/variants.hpp) must
say, as literal values: every variant computes bitwise the same field, so a
mis-routed index shows in no other test. One table for the default build and
one for a ``build.py --probes`` build."""
import pytest

import igg
from igg.ops import stencil

IGGError = igg.IGGError
native = stencil.native
PROBES = bool(native.probes_build())

NAMES = [
    "v4_by4_ry4_nt", "s_by4_ry8", "v2_by4_ry4_pf_nt", "v4_by4_ry4", "v4_by4_ry4_pf_nt", "v4_by4_ry2_nt",
    "v8_by4_ry2_nt", "v4_by2_ry4_nt", "v4_by8_ry2_nt", "v4_by4_ry8_nt", "v8_by2_ry2_nt", "v2_by4_ry8_nt",
    "v4_bz2_by8_ry4_nt", "v4_bz2_by4_ry4_nt", "v4_bz2_by2_ry8_nt", "v2_bz2_by4_ry8_nt", "v4_bz2_by8_ry2_nt",
    "v2_bz4_by4_ry4_nt", "s_by4_ry1", "v2_by4_ry1_nt", "v4_by4_ry2",
    "hx_v4_by4_ry4_nt", "hx_v2_by4_ry4_pf_nt", "hx_v4_by4_ry8_nt", "hx_v2_by4_ry8_nt", "hx_v4_bz2_by2_ry8_nt",
    "hx_v2_by2_ry8_nt", "hx_v2_by4_ry6_nt", "hx_v2_by4_ry8_pf_nt", "hx_v2_by4_ry4_nt", "hx_v4_by4_ry2_nt",
    "hx_v2_by8_ry4_nt",
    "hx_v2_by4_ry8_nt_ntc", "hx_v4_by4_ry4_nt_ntc", "hx_v4_by4_ry8_nt_ntc", "hx_v4_bz2_by2_ry8_nt_ntc",
    "hx_v2_by4_ry8_nt_zl", "hx_v4_by4_ry8_nt_zl", "hx_v2_by2_ry8_nt_zl", "hx_v4_by4_ry4_nt_zl",
    "hx_v2_by4_ry8_nt_zl_occ1", "hx_v2_by4_ry10_nt_zl_occ1", "hx_v2_by4_ry12_nt_zl_occ1",
    "hx_v2_bz4_by2_ry8_nt", "hx_v4_by4_ry4_nt_occ2",
]

# z width of a workgroup tile; 21+: of the variant's fallback for other boxes (the same in both builds)
TILES = [
    256, 64, 128, 256, 256, 256, 512, 256, 256, 256, 512, 128, 512, 512, 512, 256, 512, 512, 64, 128, 256,  # 0..20
    256, 128, 256, 128, 512,            # 21..25: fallbacks 0, 2, 9, 11, 14
    128, 128, 128, 128, 256, 128,       # 26..31: 11, 11, 11, 2, 5, 11
    128, 256, 256, 512,                 # 32..35: 11, 0, 9, 14
    128, 256, 128, 256, 128, 128, 128,  # 36..42: 11, 9, 11, 0, 11, 11, 11
    128, 256,                           # 43, 44: 11, 0
]

COMPILED = {
    False: [0, 1, 2, 5, 9, 11, 14, 18, 21, 24, 26, 40, 43, 44],
    True: list(range(45)),
}

# (BY, RY, VZ, BZ, dpp)
_FUSED_CORE = {
    0: (4, 4, 4, 1, False), 50: (4, 4, 4, 1, False),
    40: (4, 8, 2, 1, False), 42: (4, 8, 2, 1, False),
    9: (4, 8, 4, 1, False), 48: (4, 8, 4, 1, True),
    14: (2, 8, 4, 2, False), 44: (2, 8, 4, 2, False),
}
FUSED = {
    False: _FUSED_CORE,
    True: {**_FUSED_CORE, 2: (4, 4, 2, 1, False), 11: (4, 8, 2, 1, False), 41: (4, 8, 2, 1, False),
           45: (4, 4, 4, 1, False)},
}


def test_names():
    assert len(NAMES) == 45
    assert list(native.diffusion3d_variants()) == NAMES
    assert stencil.variants() == NAMES


def test_compiled():
    assert [v for v in range(-2, 50) if native.diffusion3d_variant_compiled(v)] == COMPILED[PROBES]
    assert stencil.compiled_variants() == COMPILED[PROBES]


def test_tiles():
    assert [native.diffusion3d_variant_tile(v) for v in range(45)] == TILES
    # the default build's variants, as tabulated for the reader
    assert {v: TILES[v] for v in COMPILED[False]} == {0: 256, 1: 64, 2: 128, 5: 256, 9: 256, 11: 128, 14: 512, 18: 64,
                                                      21: 256, 24: 128, 26: 128, 40: 128, 43: 128, 44: 256}
    for v in (-7, -1, 45, 46, 100, 611):
        assert native.diffusion3d_variant_tile(v) == 0


def test_fused_ok():
    assert [v for v in range(-1, 64) if native.diffusion3d_fused_variant_ok(v)] == sorted(FUSED[PROBES])


def test_fused_variant_list():
    # every fused index of either build, whether this build compiles it or not
    assert tuple(stencil.FUSED_VARIANTS) == (0, 2, 9, 11, 14, 40, 41, 42, 44, 45, 48, 50)
    assert stencil.compiled_fused_variants() == sorted(FUSED[PROBES])


def test_fused_tiles():
    assert {v: tuple(native.diffusion3d_fused_tile(v)) for v in FUSED[PROBES]} == FUSED[PROBES]


@pytest.mark.parametrize("v", [-1, 1, 5, 18, 21, 24, 43, 47, 49, 51, 63, 150] + ([] if PROBES else [2, 11, 41, 45]))
def test_fused_tile_raises(v):
    assert not native.diffusion3d_fused_variant_ok(v)
    with pytest.raises(IGGError, match="no fused instantiation"):
        native.diffusion3d_fused_tile(v)
