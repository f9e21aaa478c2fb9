"""CPU: the camera case table (tests/_cam_cases.py) reaches every branch of the camera path, every walk ends within a budget, and
ElevationMap's camera_cell equals the reference's uint32 expression wherever that one is non-negative.  Oracle and NumPy only."""
import threading
import time

import numpy as np
import pytest

import _cam_cases as cc
import _fixtures as fx
from elevation_mapping_cupy_amd.elevation_mapping import CAM_CELL_MAX, camera_cell
from oracle import emap_oracle as eo

BUDGET_S = 5.0        # per case; the longest walk of the table is ~100 cells for each of <= 9604 cells: milliseconds


def _params(c):
    return eo.make_params(dict(eo.YAML, enable_visibility_cleanup=False), cell_n=c["C"], mode=c["mode"])


def _run_with_budget(c, emap=None, tol="case"):
    """the oracle's call in a thread (ctypes releases the GIL): a walk that does not end fails the case instead of the session"""
    box = {}

    def work():
        try:
            box["out"] = cc.oracle_run(eo, _params(c), c, emap, tol)
        except BaseException as e:      # noqa: BLE001
            box["err"] = e
    th = threading.Thread(target=work, daemon=True)
    t0 = time.perf_counter()
    th.start(); th.join(BUDGET_S)
    assert not th.is_alive(), "%s: the oracle's walk did not end within %.0f s" % (c["name"], BUDGET_S)
    if "err" in box:
        raise box["err"]
    return box["out"], time.perf_counter() - t0


@pytest.fixture(scope="module")
def table():
    out = {}
    for c in cc.cases():
        emap = cc.camera_map(c["C"])
        (uv, va, inputs), dt = _run_with_budget(c)
        cls, counts = cc.classify(c, emap, uv, va, inputs)
        out[c["name"]] = dict(case=c, emap=emap, uv=uv, valid=va, inputs=inputs, cls=cls, counts=counts, seconds=dt)
    return out


def test_every_case_ends_within_its_budget_and_camera_cells_are_integers(table):
    for name, r in table.items():
        _, x1, y1, _, _, _, _ = r["inputs"]
        assert r["seconds"] < BUDGET_S, name
        assert float(x1) == int(x1) and float(y1) == int(y1) and max(abs(x1), abs(y1)) <= CAM_CELL_MAX, name
    neg = [n for n, r in table.items() if r["inputs"][1] < 0 or r["inputs"][2] < 0]
    assert {"negative_x", "negative_y", "negative_xy", "negative_x_level"} <= set(neg)
    high = [n for n, r in table.items() if r["inputs"][1] >= r["case"]["C"] or r["inputs"][2] >= r["case"]["C"]]
    assert {"beyond_x", "beyond_y", "beyond_xy"} <= set(high)
    assert table["negative_x"]["inputs"][1] == -10 and table["negative_xy"]["inputs"][2] == -6       # toward zero, not floor


def test_every_cell_class_is_reached(table, capsys):
    best = {n: (0, None) for n in cc.CLASSES}
    for name, r in table.items():
        for n in cc.CLASSES:
            if r["counts"][n] > best[n][0]:
                best[n] = (r["counts"][n], name)
    with capsys.disabled():
        print()
        for name, r in table.items():
            print("  %-18s %s" % (name, " ".join("%s=%d" % (n, r["counts"][n]) for n in cc.CLASSES)))
    for n in cc.CLASSES:
        if n == "own-cell":
            continue
        assert best[n][0] >= 5, "class %s: at most %d cells (%s)" % (n, best[n][0], best[n][1])
    assert table["own_cell"]["counts"]["own-cell"] == 1 and table["down"]["counts"]["own-cell"] == 1
    assert all(r["counts"]["own-cell"] <= 1 for r in table.values())
    # per case: what the case is in the table for
    for d in ("", "_radtan"):
        lw, nr = table["low_wall" + d]["counts"], table["narrow" + d]["counts"]
        assert lw["behind"] >= 98 * 30 and lw["occluded"] >= 100 and lw["visible"] >= 100 and lw["off-bottom"] >= 5
        assert lw["off-left"] >= 5 and lw["off-right"] >= 5
        assert all(nr[b] >= 5 for b in ("off-left", "off-right", "off-top", "off-bottom")) and nr["visible"] >= 50
        assert table["down" + d]["counts"]["visible"] >= 500 and table["down_seam" + d]["counts"]["visible"] >= 500
    for n in ("beyond_x", "beyond_y", "beyond_xy", "negative_x", "negative_y", "negative_xy", "negative_x_level"):
        assert table[n]["counts"]["walk-leaves-map"] >= 50 and table[n]["counts"]["visible"] == 0, n


def test_the_wall_occludes_a_known_set_and_half_valid_cells_occlude_without_being_projected(table):
    r = table["low_wall"]
    c, emap, va, cls = r["case"], r["emap"], r["valid"], r["cls"]
    C = c["C"]
    wx = C // 2 + C // 5
    half = emap[2] == cc.HALF
    assert half.sum() >= 5 and (cls[half] == cc.CLASSES.index("unknown")).all() and not r["uv"][:, half].any()    # `!= 1`: not projected
    # flat terrain behind a 0.6 m wall seen from 0.4 m: every projected cell straight behind the wall is occluded
    behind_wall = np.zeros((C, C), bool); behind_wall[wx + 2:, C // 2 - 5:C // 2 + 5] = True
    behind_wall &= emap[2] == 1
    assert behind_wall.sum() >= 100 and not va[behind_wall].any()
    assert (cls[behind_wall] == cc.CLASSES.index("occluded")).all()
    # `!= 0` in the walk: with the half-valid wall cells made unknown, cells behind them become visible
    no_half = emap.copy(); no_half[2][half] = 0.0
    (uv2, va2, _), _ = _run_with_budget(c, no_half)
    assert np.array_equal(uv2, r["uv"]) and ((va2 == 1) & (va == 0)).sum() >= 5 and not ((va2 == 0) & (va == 1)).any()
    # unknown cells hold garbage above every line of sight: nothing may be occluded by them (the map without them occludes the same)
    flat = emap.copy(); flat[0][emap[2] == 0] = -5.0
    (_, va3, _), _ = _run_with_budget(c, flat)
    assert np.array_equal(va3, va)


def test_the_tolerance_changes_the_occluded_set(table):
    v0, v10, v50 = (table[n]["valid"] for n in ("low_wall_tol0", "low_wall", "low_wall_tol05"))
    assert np.array_equal(table["low_wall_tol0"]["uv"], table["low_wall"]["uv"])
    assert not np.array_equal(v0, v10) and not np.array_equal(v10, v50)
    assert not (v0 & ~v10).any() and not (v10 & ~v50).any()            # a larger tolerance only ever shows more
    assert (v50 & ~v0).sum() >= 50
    # the default of the optional argument is the reference's 0.10
    (_, vd, _), _ = _run_with_budget(table["low_wall"]["case"], tol=0.10)
    assert np.array_equal(vd, v10)


def test_modes_and_the_map_centre_do_not_change_the_correspondence(table):
    assert np.array_equal(table["low_wall_fp32"]["valid"], table["low_wall"]["valid"])
    assert np.array_equal(table["low_wall_fp32"]["uv"], table["low_wall"]["uv"])
    assert np.array_equal(table["low_wall_seam"]["valid"].sum() > 100, True)


def _walk(emap, x0, y0, x1, y1, z1, tol, max_steps):
    """the occlusion walk of one projected cell in plain Python (float32 where the kernel uses float32); None = it did not end"""
    f32, C = np.float32, emap.shape[1]
    xs, ys, z0 = x0, y0, emap[0, x0, y0]
    dist = lambda a, b, c, d: np.sqrt(f32(a - c) * f32(a - c) + f32(b - d) * f32(b - d), dtype=f32)      # noqa: E731
    total, dz = dist(x0, y0, int(x1), int(y1)), f32(z1) - z0
    dx, sx, dy, sy = abs(int(x1) - x0), (1 if x0 < x1 else -1), -abs(int(y1) - y0), (1 if y0 < y1 else -1)
    err = dx + dy
    for _ in range(max_steps):
        if x0 == x1 and y0 == y1:
            return True
        if 0 <= x0 < C and 0 <= y0 < C and emap[2, x0, y0] != 0:
            ray = z0 + f32(dist(xs, ys, x0, y0) / total * dz)
            if float(emap[0, x0, y0]) - tol > float(ray):
                return False
        e2 = 2 * err
        if e2 >= dy:
            if x0 == x1:
                return True
            err += dy; x0 += sx
        if e2 <= dx:
            if y0 == y1:
                return True
            err += dx; y0 += sy
    return None


@pytest.mark.parametrize("name", ["negative_xy", "negative_x", "beyond_y", "own_cell", "narrow_radtan"])
def test_the_walk_in_plain_python_agrees_and_ends_within_its_length(table, name):
    """every walk of the small cases, camera cell inside, beyond the high side and on the low side (negative index), ends within
    |dx| + |dy| + 1 steps and decides what the oracle decides, at the default tolerance and at 0"""
    r = table[name]
    c, emap, (_, x1, y1, z1, _, _, _) = r["case"], r["emap"], r["inputs"]
    for tol, va in ((0.10, r["valid"]), (0.0, _run_with_budget(c, tol=0.0)[0][1])):
        n = 0
        for x0, y0 in np.argwhere(r["cls"] >= cc.CLASSES.index("occluded")):
            got = _walk(emap, int(x0), int(y0), int(x1), int(y1), z1, tol, abs(int(x1) - x0) + abs(int(y1) - y0) + 1)
            assert got is not None and got == bool(va[x0, y0]), (name, tol, x0, y0, got)
            n += 1
        assert n >= 100


# ---- camera_cell -------------------------------------------------------------------------------------------------------------------
def _poses():
    rng = np.random.default_rng(11)
    for k in range(400):
        C = (34, 66, 98, 202, 2002)[k % 5]
        R = fx.rot(*rng.uniform(-3, 3, 3)).astype(np.float32)
        cam = rng.uniform(-1.5, 1.5, 3) * C * 0.04 * (0.5 if k % 3 else 1.0)
        center = (rng.uniform(-2, 2, 3) * (k % 2)).astype(np.float32)
        t = (-R.astype(np.float64) @ (cam + center)).astype(np.float32)
        yield C, center, R, t


def test_camera_cell_equals_the_uint32_expression_wherever_that_is_non_negative():
    n_same = n_neg = 0
    for C, center, R, t in _poses():
        t_cam_map = -R.T @ t - center
        s = [(C / 2) + (t_cam_map[a] / 0.04) for a in (0, 1)]
        x1, y1, z1 = camera_cell(center, C, 0.04, R, t)
        assert x1.dtype == np.float32 and y1.dtype == np.float32 and z1.dtype == np.float32
        K = np.eye(3, dtype=np.float32)
        for a, mine in ((0, x1), (1, y1)):
            if s[a] > -1:                                    # (-1, 0) truncates to 0 under either cast
                ref = np.float32(np.uint32(s[a]))
                assert mine.tobytes() == ref.tobytes() or (mine == 0 and ref == 0), (C, a, s[a], mine, ref)
                n_same += 1
            else:
                assert mine == np.float32(int(s[a])) and mine < 0 and mine == np.trunc(s[a]), (C, a, s[a], mine)
                n_neg += 1
        if s[0] >= 0 and s[1] >= 0:
            _, fx1, fy1, fz1 = fx.camera_inputs(center, C, 0.04, K, R, t)
            assert (fx1.tobytes(), fy1.tobytes(), np.float32(fz1).tobytes()) == (x1.tobytes(), y1.tobytes(), z1.tobytes())
    assert n_same >= 300 and n_neg >= 100


@pytest.mark.parametrize("bad", ["nan", "inf", "far", "far_negative", "nan_z"])
def test_camera_cell_refuses_what_the_walk_cannot_reach(bad):
    R = np.eye(3, dtype=np.float32)
    cam = {"nan": [np.nan, 0, 1], "inf": [0, np.inf, 1], "far": [(CAM_CELL_MAX + 1) * 0.04, 0, 1],
           "far_negative": [0, -(CAM_CELL_MAX + 2 + 17) * 0.04, 1], "nan_z": [0, 0, np.nan]}[bad]
    with pytest.raises(ValueError):
        camera_cell(np.zeros(3, np.float32), 34, 0.04, R, -np.asarray(cam, np.float32))
    with pytest.raises(ValueError):      # the oracle refuses the same cells the C ABI refuses
        eo.image_correspondence(eo.make_params(eo.YAML, cell_n=34), cc.camera_map(34), 3.5 if bad == "nan" else 4294967296.0, 1.0, 1.0,
                                np.zeros(12, np.float32), np.eye(3, dtype=np.float32).ravel(), np.zeros(5, np.float32), 8, 8,
                                np.zeros(3, np.float32))


def test_camera_cell_accepts_the_cap_itself():
    R = np.eye(3, dtype=np.float32)
    x1, y1, _ = camera_cell(np.zeros(3, np.float32), 0, 1.0, R, -np.array([CAM_CELL_MAX, -CAM_CELL_MAX, 1], np.float32))
    assert (x1, y1) == (CAM_CELL_MAX, -CAM_CELL_MAX)
