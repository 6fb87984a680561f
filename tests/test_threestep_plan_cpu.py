"""The launch plan of the three-step pass (tiles along dim 1, planes per x
chunk, workgroups) as host arithmetic, without a device: the headline shape
gets the grids the forms were designed for, and for any shape the tiles and
chunks cover every inner row and plane exactly once."""
import pytest

from igg.ops import stencil

plan = stencil.native.diffusion3d_threestep_plan
WRITTEN = {0: 4, 1: 6}  # rows a tile of the form writes (its by * ry - 4)


def test_forms_and_their_names():
    names = list(stencil.native.diffusion3d_threestep_forms())
    assert names[:2] == ["t3_by2_ry4_bz4", "t3_by2_ry5_bz4_qlds"]
    assert stencil.THREESTEP_FORMS == tuple(range(len(names)))


def test_headline_shape_at_one_residency_round():
    # 256 CUs, one workgroup each: 510 inner rows and planes
    assert plan([512, 512, 512], 1, 256) == (85, 170, 255)  # 85 x 6 rows, 3 x 170 planes: nothing partial
    assert plan([512, 512, 512], 0, 256) == (128, 255, 256)


def _covered(n, form, target):
    tiles, ch, nblk = plan(list(n), form, target)
    tys = WRITTEN[form]
    rows = [0] * n[1]
    for ty in range(tiles):  # a tile writes rows ty * tys + 1 .. + tys, those inside the array
        for y in range(ty * tys + 1, min(ty * tys + 1 + tys, n[1] - 1)):
            rows[y] += 1
    assert ch >= 1 and nblk % tiles == 0
    planes = [0] * n[0]
    for cx in range(nblk // tiles):  # a chunk writes planes 1 + cx * ch .. + ch, those inside the array
        xs = 1 + cx * ch
        assert xs < n[0] - 1, "an empty chunk"
        for x in range(xs, min(xs + ch, n[0] - 1)):
            planes[x] += 1
    return rows, planes, ch


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("target", [1, 7, 256, 1024, 4096])
@pytest.mark.parametrize("n", [(3, 3, 4), (4, 9, 8), (5, 8, 8), (9, 14, 32), (16, 33, 64), (70, 20, 64), (11, 7, 4),
                               (37, 101, 16), (513, 515, 8)])
def test_every_inner_row_and_plane_is_covered_once(n, form, target):
    rows, planes, ch = _covered(n, form, target)
    assert rows == [0] + [1] * (n[1] - 2) + [0]
    assert planes == [0] + [1] * (n[0] - 2) + [0]
    # a chunk pays a four-position lead-in: none is shorter than 8 planes unless the whole range is
    assert ch >= min(8, n[0] - 2)


def test_plan_rejects_an_unknown_form_and_tiny_shapes():
    with pytest.raises(Exception):
        plan([16, 16, 16], len(stencil.THREESTEP_FORMS), 256)
    with pytest.raises(Exception):
        plan([2, 16, 16], 0, 256)
