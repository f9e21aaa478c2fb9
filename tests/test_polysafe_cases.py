"""CPU: the case table of the safety-polygon service on the device (tests/_polysafe_cases.py) -- every case has the property it is named
for, under the NumPy model of the verdict; the GPU tests (test_hip_polygon_safety.py) run the same cases against the device."""
import numpy as np
import pytest

import _polysafe_cases as pc


@pytest.fixture(scope="module")
def built():
    return {name: pc.build(name) for name in pc.CASES}


def _model(b):
    C, center, world, clipped, mask, trav, valid, table = b
    return pc.model(mask, trav, valid, table)


def test_the_threshold_cases_stand_on_both_sides_of_max_unsafe_n(built):
    at, over = _model(built["threshold_at"]), _model(built["threshold_over"])
    assert at["n_risky"] == pc.MAX_UNSAFE_N and over["n_risky"] == pc.MAX_UNSAFE_N + 1
    assert at["is_safe"] is True and over["is_safe"] is False
    assert at["max_risk"] == over["max_risk"] <= 1.0 - pc.SAFE_MIN_THRESH          # the count alone decides


def test_the_ragged_box_is_no_multiple_of_the_tile_and_spans_several_tiles(built):
    r0, c0, nrows, ncols, tiles = built["ragged"][7]
    assert nrows % pc.TILE and ncols % pc.TILE
    assert max(t[0] for t in tiles) >= 1 and max(t[1] for t in tiles) >= 1 and len(tiles) == (max(t[0] for t in tiles) + 1) * (max(t[1] for t in tiles) + 1)
    assert _model(built["ragged"])["ring"] is not None


def test_the_cut_box_straddles_the_physical_wrap(built):
    C, move = pc.CASES["cut"][0], pc.CASES["cut"][1]
    r0, c0, nrows, ncols, _ = built["cut"][7]
    # move_to by d cells from the origin: physical = (logical + d) % C, so the wrap lies between the logical indices C - 1 - d and C - d
    assert r0 <= C - 1 - move[0] < C - move[0] <= r0 + nrows - 1
    assert c0 <= C - 1 - move[1] < C - move[1] <= c0 + ncols - 1
    m = _model(built["cut"])
    assert m["n_risky"] == 9 and m["n_inside"] > 100


@pytest.mark.parametrize("name, n", [("hull_0", 0), ("hull_1", 1), ("hull_2", 2), ("hull_4_collinear", 4)])
def test_the_degenerate_hull_cases_have_no_ring(built, name, n):
    m = _model(built[name])
    cells = np.argwhere(m["too_risky"])
    assert m["n_risky"] == n == len(cells) and m["ring"] is None
    if n == 4:
        assert len(set(cells[:, 1])) == 1 and len(set(cells[:, 0])) == 4          # one column, four rows: one extreme per row
    if n == 2:
        assert len(set(cells[:, 0])) == 1                                         # one row: its two extremes


def test_the_nan_and_poison_cases_give_a_nan_maximum(built):
    for name in ("nan_inside", "poison"):
        m = _model(built[name])
        assert np.isnan(m["max_risk"]) and np.isnan(m["mean_risk"]) and m["is_safe"] is False, name
    C, center, world, clipped, mask, trav, valid, table = built["poison"]
    bad = np.argwhere(~np.isfinite(trav))
    assert len(bad) == 1 and mask[tuple(bad[0])] == 0 and valid[tuple(bad[0])] > 0.5
    C, center, world, clipped, mask, trav, valid, table = built["no_poison"]
    bad = np.argwhere(~np.isfinite(trav))
    assert len(bad) == 1 and mask[tuple(bad[0])] == 0 and valid[tuple(bad[0])] < 0.5
    assert np.isfinite(_model(built["no_poison"])["max_risk"])


def test_the_border_box_is_cut_to_the_interior(built):
    C, center, world, clipped, mask, trav, valid, (r0, c0, nrows, ncols, tiles) = built["border"]
    assert (r0, c0, nrows, ncols) == (1, 1, C - 2, C - 2)
    assert mask[0].any() and mask[-1].any() and mask[:, 0].any() and mask[:, -1].any()      # the polygon itself covers the border


def test_every_case_has_unknown_cells_inside(built):
    for name, b in built.items():
        m = _model(b)
        assert m["n_known"] < m["n_inside"], name


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_the_work_table_covers_the_mask(built, name):
    C, center, world, clipped, mask, trav, valid, (r0, c0, nrows, ncols, tiles) = built[name]
    covered = np.zeros((C, C), bool)
    for tr, tc in tiles:
        rr, cc = r0 + tr * pc.TILE, c0 + tc * pc.TILE
        covered[rr:min(rr + pc.TILE, r0 + nrows), cc:min(cc + pc.TILE, c0 + ncols)] = True
    assert tiles == sorted(tiles) and mask[1:-1, 1:-1].sum() > 0
    inner = np.zeros((C, C), bool); inner[1:-1, 1:-1] = True
    assert not ((mask > 0) & inner & ~covered).any()
    assert not covered[0].any() and not covered[-1].any() and not covered[:, 0].any() and not covered[:, -1].any()


def test_the_kernel_order_sum_is_a_sum():
    C, center, world, clipped, mask, trav, valid, table = pc.build("ragged")
    inside = np.zeros((C, C), bool); inside[1:-1, 1:-1] = mask[1:-1, 1:-1] > 0
    got = pc.kernel_order_sum(trav, inside, table)
    want = float(trav[inside].astype(np.float64).sum())
    assert abs(got - want) <= inside.sum() * 2.0 ** -53 * want
