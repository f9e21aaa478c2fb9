"""CPU: the inputs of tests/test_hip_ray_variants.py really reach what that file is about -- checked with numpy and the oracle alone, so
that the GPU tests cannot pass vacuously: the ray pass changes the map in every case, its effects reach the far edges of the reach
window on every side that lies inside the map, the corner and outside cases lose a good part of their cloud beyond the map's edge, the
two threshold cases have exactly the threshold's point counts, the literal window table is sane, and the expectation table names every
instantiation of k_rays the variant table lists."""
import numpy as np
import pytest

import _ray_variants as rv
from oracle import emap_oracle as eo

RAY_PLANES = [0, 1, 2, 5, 6]      # (not plane 3: the traversability filter's flat-index row wrap carries differences to the far edge of the map)
MIN_CELLS = 500                   # cells the ray pass must change
REACH = 50                        # max_ray_length / resolution of the windowed cases
MIN_REACH = 44                    # a changed cell at least this far from the sensor cell, on every side with REACH cells of map


@pytest.fixture(scope="module")
def runs(weights):
    """case key -> (oracle with the ray pass, oracle without): computed once, read-only"""
    done = {}

    def get(key):
        if key not in done:
            eo.set_threads(8)
            try:
                done[key] = (rv.oracle_run(rv.case_of(key), weights, True), rv.oracle_run(rv.case_of(key), weights, False))
            finally:
                eo.set_threads(1)
        return done[key]

    return get


def _sensor_cell(case, axis):
    return int(np.floor(np.float32(case["t"][axis]) / rv.RES + case["C"] / 2))


@pytest.mark.parametrize("key", rv.KEYS)
def test_the_ray_pass_changes_the_map_up_to_the_windows_edges(key, runs):
    case = rv.case_of(key)
    on, off = runs(key)
    assert all(v > 0 for v in on[3]) and off[3] == [0, 0]
    diff = np.zeros((case["C"], case["C"]), bool)
    for k in RAY_PLANES:
        diff |= on[0][k].view(np.uint32) != off[0][k].view(np.uint32)
    n = int(diff.sum())
    rows, cols = np.nonzero(diff)
    print("%s: %d cells differ, visits %r" % (key, n, on[3]))
    assert n >= MIN_CELLS
    if case["mrl"] != REACH * rv.RES:
        return                                            # (whole128: rays longer than the map, no window to reach the edges of)
    sides = 0
    for axis, where in ((0, rows), (1, cols)):
        s = _sensor_cell(case, axis)
        for sign in (-1, 1):
            if not 0 <= s + sign * REACH <= case["C"] - 1:
                continue
            far = int((sign * (where - s)).max())
            print("%s: axis %d side %+d: farthest changed cell %d cells from the sensor cell" % (key, axis, sign, far))
            assert far >= MIN_REACH, (key, axis, sign, far)
            sides += 1
    assert sides >= (3 if key == "outside" else 1), (key, sides)      # (outside: the row side inside the map and both column sides)


@pytest.mark.parametrize("key", ["corner_a", "corner_b", "outside", "fp32_corner", "stats384"])
def test_corner_and_outside_cases_lose_points_beyond_the_map(key):
    case = rv.case_of(key)
    R, t0, clouds = rv.case_inputs(case)
    orc = eo.OracleMap(eo.make_params(rv.case_config(case, eo.YAML), cell_n=case["C"], mode=case["mode"]))
    for p in clouds:
        _, valid, inside = orc.point_index(p, R, t0)
        assert int((inside == 0).sum()) >= 0.1 * case["N"], (key, int((inside == 0).sum()))
        assert int(((inside != 0) & (valid != 0)).sum()) >= 0.1 * case["N"], key           # ... and a good part still lands inside


def test_point_counts_sit_on_both_sides_of_the_threshold():
    for case in rv.CASES:
        clouds = rv.case_inputs(case)[2]
        assert all(p.shape == (case["N"], 3) and p.dtype == np.float32 for p in clouds)
        if case["key"] == "n131071":
            assert case["N"] == 131071
        elif case["key"] == "n131072":
            assert case["N"] == 131072
        else:
            assert case["N"] >= 131072
    assert rv.SMALL_CLOUD_KEY == "n131071"


def test_inputs_are_deterministic_and_distinct():
    seen = set()
    for case in rv.CASES:
        a, b = rv.case_inputs(case), rv.case_inputs(case)
        assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
        assert not np.array_equal(a[2][0], a[2][1])
        seen.add(rv.case_seed(case))
    assert len(seen) == len(rv.CASES) == len(set(rv.KEYS)) == 17


def test_the_window_table_is_sane():
    for case in rv.CASES:
        C, w = case["C"], case["window"]
        wpr32 = ((C + 63) // 64) * 2                       # 32-bit words per bitmap row
        if w is None:
            continue
        r0, nr, w0, wpr = w
        assert 0 <= r0 and nr >= 1 and r0 + nr <= C, case
        assert 0 <= w0 and wpr >= 4 and w0 + wpr <= wpr32, case
        assert w0 % 4 == 0 and wpr % 4 == 0, case
        assert nr * wpr < C * wpr32, case
    by = {c["key"]: c["window"] for c in rv.CASES}
    assert by["piece_lo"][2] != by["piece_lo-1"][2] and by["piece_lo"][2] == 4 and by["piece_lo-1"][2] == 0
    assert by["refused300"] is None and by["whole128"] is None and by["n131071"] is None
    assert sum(w is not None for w in by.values()) == 14


def test_the_expectation_names_every_reachable_instantiation():
    import test_hip_ray_variants as tv
    want = {"k_rays<0, %s, %d, false, 512, %s, 1>" % (s, i, l) for s in ("false", "true") for i in (2, 1) for l in ("true", "false")}
    want |= {"k_rays<1, false, 0, false, 512, %s, 1>" % l for l in ("true", "false")}
    want |= {"k_rays<0, false, %d, false, 256, false, 4>" % i for i in (2, 1)}
    assert tv.reachable_instantiations() == want and len(want) == 12
    assert set(tv.VARIANTS) == set(tv.IDX) == set(tv.LMAP)
    for v in tv.VARIANTS:
        assert len(tv.IDX[v]) == len(rv.CASES)
        for key in rv.KEYS:
            names = tv.expected_names(v, key)
            assert len(names) == (2 if v == "default" and key != rv.SMALL_CLOUD_KEY else 1), (v, key, names)
    # the hooked variants together pin each of the twelve with a single legal name (the unhooked child may run either place)
    single = {n for v in tv.VARIANTS if v != "default" for k in rv.KEYS for n in tv.expected_names(v, k)}
    assert single == want
