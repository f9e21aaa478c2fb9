"""CPU: the inputs of tests/test_hip_post_variants.py really reach what that file is about -- checked with numpy and the oracle alone, so
that the GPU tests cannot pass vacuously.  The expectation table must name the twelve instantiations launch_post can reach:
k_post<4|8|16|32, 0|1> and k_post_dma<16|32, 0|1>.  k_post_dma<4|8, .> are compiled but unreachable: post_use_dma requires R >= 16."""
import numpy as np
import pytest

import _post_variants as pv
from oracle import emap_oracle as eo

IDS = [pv.case_key(*c) for c in pv.CASES]


@pytest.fixture(scope="module")
def states():
    return {c: pv.state(c[0], c[1], pv.case_seed(*c)) for c in pv.CASES}


@pytest.mark.parametrize("case", pv.CASES, ids=IDS)
def test_every_tile_height_meets_sparse_and_dense_windows(case, states):
    """a tile searches on bit masks when more than 3/4 of its (R + 6) x 70 window are holes, and probes anti-diagonals otherwise"""
    C, d = case
    e = states[case]
    mask = e[2] + e[6]
    for R in pv.TILE_ROWS:
        full = (R + 6) * (pv.PT_C + 6)
        counts = pv.window_holes(mask, R)
        if d <= pv.SPARSE_MAX_D:        # the bit-mask search is switched off above d = 15 by design (the kernels' `sparse` condition): nothing to reach there
            assert any(4 * n > 3 * full for n in counts), (case, R, counts)
        assert any(0 < n and 4 * n <= 3 * full for n in counts), (case, R, counts)


@pytest.mark.parametrize("case", pv.CASES, ids=IDS)
def test_dilation_fills_holes_and_leaves_the_unreachable_ones(case, states):
    C, d = case
    e = states[case]
    mask = e[2] + e[6]
    dil, _ = eo.dilate_plane(C, d, e[5], mask)
    holes = mask < 0.5
    assert int((holes & (dil != e[5])).sum()) >= 100
    r0, c0, s = pv.hole_rectangle(C, d)
    assert s == 2 * d + 8 and r0 >= 1 and c0 >= 1 and r0 + s <= C - 1 and c0 + s <= C - 1
    assert not (e[2][r0:r0 + s, c0:c0 + s].any() or e[6][r0:r0 + s, c0:c0 + s].any())
    rc, cc = r0 + s // 2, c0 + s // 2                       # the square's centre: its (2d + 1)^2 window holds no source and leaves no row
    assert rc - d >= r0 and rc + d < r0 + s and cc - d >= c0 and cc + d < c0 + s
    assert holes[rc, cc] and dil[rc, cc] == e[5][rc, cc]
    if C - 1 - C // 2 >= s:                                  # (everywhere but at (66, 20): inside the dense half)
        assert c0 >= C // 2


def test_the_state_has_what_the_cases_are_about(states):
    for (C, d), e in states.items():
        assert e.shape == (7, C, C) and e.dtype == np.float32
        assert e[2][0].all() and e[2][:, C - 1].all()                                  # valid border cells
        assert 0.25 < e[2][1:, :4].mean() < 0.75 and 0.25 < e[2][1:, C - 4:C - 1].mean() < 0.75       # busy edge columns
        assert np.array_equal(e, pv.state(C, d, pv.case_seed(C, d)))                   # the child and the parent build the same state


def test_the_expectation_names_every_reachable_instantiation():
    import test_hip_post_variants as tv
    want = {"k_post<%d, %d>" % (r, s) for r in (4, 8, 16, 32) for s in (0, 1)} | {"k_post_dma<%d, %d>" % (r, s) for r in (16, 32) for s in (0, 1)}
    assert tv.reachable_instantiations() == want
    assert set(tv.VARIANTS) == set(tv.EXPECTED)
    for v in tv.VARIANTS:
        assert set(tv.EXPECTED[v]) == {d for _, d in pv.CASES}


def _interior_tiles(C, d, R):
    """tiles whose staged region (halo 3 + d) keeps rows and columns within [1, C - 2]: k_post's interior staging, no wrap"""
    n = 0
    for tr in range(0, C, R):
        for tc in range(0, C, pv.PT_C):
            r0, c0 = tr - 3 - d, tc - 3 - d
            n += r0 >= 1 and r0 + R + 6 + 2 * d - 1 <= C - 2 and c0 >= 1 and c0 + pv.PT_C + 6 + 2 * d - 1 <= C - 2
    return n


def test_interior_tiles_exist_at_202_and_not_at_66():
    assert _interior_tiles(202, 3, 32) >= 1
    for R in pv.TILE_ROWS:
        assert _interior_tiles(202, 3, R) >= 1
        for d in (1, 3, 20):
            assert _interior_tiles(66, d, R) == 0
