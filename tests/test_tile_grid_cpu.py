"""CPU: every case of tests/tile_grid_cases.py still exercises what its row of the table says -- checked on the oracle's
lists, so that a change of the scene generator or of a builder shows here and not as a GPU test that quietly stopped
testing its limit."""
import numpy as np
import pytest

import tile_grid_cases as tg


def test_the_table_is_the_grids_it_names():
    want = {"t1024": (1024, 1), "t1025": (1025, 2), "t4097": (4097, 5), "t8281": (8281, 9), "t16383": (16383, 16),
            "t16384": (16384, 16), "t16384_strip": (16384, 16), "t16385": (16385, 17), "t16512": (16512, 17),
            "t16400_strip": (16400, 17), "t65792": (65792, 65)}
    assert set(want) == set(tg.GRIDS)
    for name, (ntx, nty, W, H, L, N, _) in tg.GRIDS.items():
        T = ntx * nty
        assert (T, tg.per_of(T)) == want[name], name
        assert ((W + 15) // 16, (H + 15) // 16) == (ntx, nty), name
        ragged = name == "t16383"
        assert ((W % 16 != 0) and (H % 16 != 0)) == ragged, name
    assert 16383 % 8 == 7
    assert [tg.tile_bits(t) for t in (1, 2, 3, 4, 5, 16384, 16385, 65536, 65537, 65792)] == [1, 1, 2, 2, 3, 14, 15, 16, 17, 17]
    assert tg.BIN_MAX_TILES // tg.BIN_THREADS == 16
    assert [tg.longest_empty_run(x) for x in ([1, 1], [0], [1, 0, 0, 2, 0], [0, 0, 0, 1])] == [0, 1, 2, 3]


@pytest.mark.parametrize("name,kind", tg.CASES)
def test_case_preconditions(scene, orc, name, kind):
    L = tg.GRIDS[name][4]
    params, cam = tg.grid_scene(scene, name, kind)
    ref = tg.oracle_forward(orc, scene, params, cam, L)
    fig = tg.check_preconditions(name, kind, ref)
    print(f"{name} {kind}: {fig}")
    assert np.isfinite(ref["image"]).all()
    n = np.asarray(ref["n"])
    assert n.max() > 0
    if kind == "long":  # some pixel's chain runs deep into the long list: the split has boundaries to get wrong
        assert n.max() > 2 * 496


def test_small_long_view_has_a_list_to_split(scene, orc):
    params, cam = tg.small_long_scene(scene)
    ref = tg.oracle_forward(orc, scene, params, cam, 1)
    lens = np.diff(ref["ranges"])
    assert lens.max() > tg.SEG_SPLIT_MIN and len(lens) == 920


def test_the_8281_tile_grid_puts_its_heavy_tile_in_the_partly_live_slots():
    t, per_xcd = tg.check_hot_tile_is_in_the_partial_slots("t8281")
    assert (t, per_xcd) == (90 * 91 + 87, 1036)  # run 7, offset 1025
    assert ("t8281", "skewed") in tg.CASES and ("t8281", "long") in tg.CASES


@pytest.mark.parametrize("name", tg.EMPTY_TAIL_GRIDS)
def test_empty_tail_scenes(scene, orc, name):
    L = tg.GRIDS[name][4]
    full = tg.oracle_forward(orc, scene, *tg.grid_scene(scene, name), L)
    ref = tg.oracle_forward(orc, scene, *tg.empty_tail_scene(scene, name), L)
    tg.check_empty_tail(name, ref, full)


def test_absgrad_scene(scene, orc):
    params, cam = tg.absgrad_scene(scene)
    assert len(params["xyz"]) == tg.ABSGRAD_GAUSSIANS
    tg.check_absgrad_scene(tg.oracle_forward(orc, scene, params, cam, tg.GRIDS["t16512"][4]))


@pytest.mark.parametrize("ntx,nty,empty_tail", tg.BAND_GRIDS)
def test_binning_operator_scenes(orc, ntx, nty, empty_tail):
    uv, xyz, radius = tg.band_scene(ntx, nty, empty_tail)
    _, ranges, cap = orc.get_sorted_gaussian_list(uv, xyz, radius, ntx, nty)
    tg.check_band_scene(ntx, nty, empty_tail, ranges)
    assert cap >= ranges[-1] > 0
