"""CPU: the point-cloud output's contract without a device.  The NumPy model of tests/_cloud_out_cases.py against a per-cell loop that
restates grid_map's iterator; the field rules; grid_cell_positions against hand values; every ValueError the context-free helpers can
reach; the arrow arithmetic; and the sentinel condition over the GPU tests' case table: no comparison there is vacuously equal.
grid_map is absent offline: all of this is a RESTATEMENT, not pinned by a compiled reference."""
import numpy as np
import pytest

import _cloud_out_cases as cc
from elevation_mapping_cupy_amd.elevation_mapping import _cloud_compact, grid_cell_positions, normal_arrow_markers, point_cloud_descriptor


def _planes(M, seed):
    rng = np.random.default_rng(seed)
    names = ["variance", "elevation", "color", "normal_x", "normal_y", "normal_z", "upper_bound"]
    planes = [rng.uniform(-1.0, 1.0, (M, M)).astype(np.float32) for _ in names]
    planes[1][rng.random((M, M)) < 0.4] = np.nan                                # elevation: the point layer
    planes[1][0, M - 1] = np.inf
    planes[0][rng.random((M, M)) < 0.2] = cc.NAN_PAYLOAD                        # another field: NaN bits travel
    planes[6][rng.random((M, M)) < 0.3] = np.nan                                # a basic layer of its own
    planes[2] = rng.integers(0, 2 ** 24, (M, M)).astype(np.uint32).view(np.float32)      # colour bits
    for k in (3, 4, 5):
        planes[k] *= np.float32(0.12)                                           # norms around 0.1
    planes[3][1, 2] = np.nan
    return names, planes


@pytest.mark.parametrize("M", [5, 33])
def test_the_model_is_the_iterator_cell_by_cell(M):
    names, planes = _planes(M, M)
    xs, ys = (a.astype(np.float32) for a in grid_cell_positions((0.3, -0.7), 0.1, M))
    for kw in (dict(basic=["elevation"]), dict(basic=[]), dict(basic=["elevation", "upper_bound"]), dict(basic=["upper_bound"], hidden=["upper_bound"]),
               dict(basic=["elevation"], index=True), dict(basic=["elevation"], index=True, normal_min=0.1), dict(basic=[], normal_min=0.05)):
        fm, rm = cc.model_cloud(planes, names, "elevation", xs=xs, ys=ys, **kw)
        fl, rl = cc.loop_cloud(planes, names, "elevation", xs=xs, ys=ys, **kw)
        assert fm == fl and cc.same_words(rm, rl), kw
        assert 0 < rm.shape[0] < M * M
    f, r = cc.model_cloud(planes, names, "elevation", ["elevation"], xs, ys)
    assert np.isnan(r[:, f.index("variance")]).any() and (r[np.isnan(r[:, 0]), 0].view(np.uint32) == 0x7FC12345).all()      # emitted with its NaN bits


def test_the_package_host_route_agrees_with_the_model():
    M = 33
    names, planes = _planes(M, 3)
    xs, ys = (a.astype(np.float32) for a in grid_cell_positions((0.3, -0.7), 0.1, M))
    by_name = dict(zip(names, planes))
    emit = [n for n in names if n != "upper_bound"]
    rec = _cloud_compact(by_name, emit, "elevation", ["elevation", "upper_bound"], xs, ys, index=True, normals=names[3:6], normal_min=0.1)
    _, want = cc.model_cloud(planes, names, "elevation", ["elevation", "upper_bound"], xs, ys, index=True, normal_min=0.1, hidden=["upper_bound"])
    assert cc.same_words(rec, want) and 0 < rec.shape[0] < M * M


def test_field_rules():
    f, step = point_cloud_descriptor(["elevation"], "elevation")
    assert [(x.name, x.offset, x.datatype, x.count) for x in f] == [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1)] and step == 12
    f, step = point_cloud_descriptor(["variance", "elevation", "color", "normal_x"], "elevation")      # the point layer in the middle, colour -> rgb
    assert [x.name for x in f] == ["variance", "x", "y", "z", "rgb", "normal_x"] and [x.offset for x in f] == [0, 4, 8, 12, 16, 20] and step == 24
    assert cc.field_names(["variance", "elevation", "color", "normal_x"], "elevation") == [x.name for x in f]
    assert cc.field_names(["upper_bound", "elevation"], "elevation", hidden=["upper_bound"], index=True) == ["x", "y", "z", "index"]      # a hidden basic layer
    for bad in (dict(layers=[], point_layer="elevation"), dict(layers=["variance"], point_layer="elevation"), dict(layers=["elevation", "elevation"], point_layer="elevation")):
        with pytest.raises(ValueError):
            point_cloud_descriptor(**bad)


def test_cell_positions_by_hand():
    """M = 32, res = 0.1: L = 3.2, the first cell's centre lies at p + 1.55, each next one 0.1 below"""
    xs, ys = grid_cell_positions((0.0, 0.0), 0.1, 32)
    off = 0.5 * (32 * 0.1) - 0.5 * 0.1
    assert xs.dtype == np.float64 and xs.shape == (32,) and xs[0] == off == ys[0] and abs(off - 1.55) < 1e-15
    assert xs[1] == off + 0.1 * -1.0 and xs[31] == off + 0.1 * -31.0 and abs(xs[31] + 1.55) < 1e-14 and (xs == ys).all()
    assert (np.diff(xs) < 0).all()                                              # i counts down from the upper edge
    res = float(np.float32(0.04)); p = (float(np.float32(12.3456)), float(np.float32(-7.001)))      # an off-origin float32 centre, a float32 resolution widened
    xs, ys = grid_cell_positions(p, res, 32)
    lx, ly = cc.positions_loop(p, res, 32)
    assert cc.same_words(xs, lx) and cc.same_words(ys, ly)
    assert xs[0] == (p[0] + (0.5 * (32 * res) - 0.5 * res)) + res * -0.0 and ys[5] == (p[1] + (0.5 * (32 * res) - 0.5 * res)) + res * -5.0
    assert abs(xs[0] - (12.3456 + 15.5 * 0.04)) < 1e-5 and abs(ys[31] - (-7.001 - 15.5 * 0.04)) < 1e-5
    for bad in (dict(center_xy=(0.0, float("nan")), resolution=0.1, M=4), dict(center_xy=(0.0, 0.0), resolution=0.0, M=4), dict(center_xy=(0.0, 0.0), resolution=0.1, M=0),
                dict(center_xy=(0.0, 0.0), resolution=float("inf"), M=4), dict(center_xy=(0.0, 0.0, 0.0), resolution=0.1, M=4)):
        with pytest.raises(ValueError):
            grid_cell_positions(**bad)


def test_arrow_arithmetic_against_a_loop():
    M = 9
    rng = np.random.default_rng(2)
    elev = rng.uniform(-1, 1, (M, M)).astype(np.float32)
    elev[rng.random((M, M)) < 0.3] = np.nan
    n = [rng.uniform(-0.7, 0.7, (M, M)).astype(np.float32) for _ in range(3)]
    elev[0, :4] = 0.5
    below, above = np.float32(0.1) - np.float32(1e-8), np.float32(0.1) + np.float32(1e-8)
    assert float(below) < 0.1 < float(above)
    for k, v in enumerate((below, above, np.float32(np.nan), np.float32(0.0))):      # a normal just below / above 0.1 along z, a NaN normal, a zero normal
        n[0][0, k], n[1][0, k], n[2][0, k] = 0.0, 0.0, v
    xs, ys = grid_cell_positions((float(np.float32(1.7)), float(np.float32(-0.3))), float(np.float32(0.04)), M)
    ids, st, en = cc.model_arrows(elev, n[0], n[1], n[2], xs, ys)
    lids, lst, len_ = cc.loop_arrows(elev, n[0], n[1], n[2], xs, ys)
    assert (ids == lids).all() and cc.same_words(st, lst) and cc.same_words(en, len_) and 0 < ids.size < M * M
    assert 0 not in ids and 1 in ids and 2 in ids and 3 not in ids            # lin = j * M + i with j = 0: below skipped, above kept, NaN kept, zero skipped
    k = int(np.nonzero(ids == 1)[0][0])
    assert st[k, 0] == xs[1] and st[k, 1] == ys[0] and st[k, 2] == float(elev[0, 1]) and en[k, 2] == st[k, 2] + float(above) * 0.1
    assert np.isnan(en[int(np.nonzero(ids == 2)[0][0]), 2])
    arr = normal_arrow_markers(type("A", (), dict(ids=ids, starts=st, ends=en))(), frame_id="map", stamp=3.0)
    mk = arr.markers[k]
    assert len(arr.markers) == ids.size and (mk.ns, mk.id, mk.type, mk.action) == ("normal", 1, 0, 0) and mk.header.frame_id == "map"
    assert (mk.scale.x, mk.scale.y, mk.scale.z) == (0.01, 0.01, 0.01) and (mk.color.r, mk.color.g, mk.color.b, mk.color.a) == (0.0, 1.0, 0.0, 1.0)
    assert mk.pose.orientation.w == 1.0 and (mk.points[0].x, mk.points[1].z) == (st[k, 0], en[k, 2])


@pytest.mark.parametrize("C", cc.SIZES)
def test_no_gpu_comparison_is_vacuous(C):
    """in every case but "none valid" the model emits at least one point, and it skips at least one cell in every case but "all valid" (which skips none)"""
    M = C - 2
    xs, ys = (a.astype(np.float32) for a in grid_cell_positions((0.0, 0.0), 0.1, M))
    for name in cc.all_cases(M):
        p = cc.published_planes(M, name, center_z=0.05)
        basic = ["elevation", "variance"] if name == "tested layer NaN" else ["elevation"]
        _, rec = cc.model_cloud([p["elevation"], p["variance"]], ["elevation", "variance"], "elevation", basic, xs, ys)
        n = rec.shape[0]
        assert (n == 0) == (name == "none valid"), (name, n)
        assert (n == M * M) == (name == "all valid"), (name, n)
        plain = cc.model_cloud([cc.published_planes(M, "checkerboard", 0.05)[k] for k in ("elevation", "variance")], ["elevation", "variance"], "elevation", ["elevation"], xs, ys)[1]
        if name == "other field NaN":
            assert n == plain.shape[0] and np.isnan(rec[:, 3]).any()           # emitted, NaN bits in the other field
        if name in ("+inf elevation", "tested layer NaN"):
            assert 0 < n < plain.shape[0]                                       # those cells are skipped


def test_the_largest_size_passes_the_scans_single_trip():
    assert cc.mask_words(cc.SIZES[-2] - 2) < cc.SCAN_TRIP < cc.mask_words(cc.SIZES[-1] - 2)
    assert (cc.SIZES[-2] - 2 + 31) // 32 == 9 and cc.SIZES[-2] - 2 > 256
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc", "emap_launch.h")).read()
    assert "#define EM_CLOUD_SCAN_BLOCK 1024" in src and "#define EM_CLOUD_SCAN_TRIP (4 * EM_CLOUD_SCAN_BLOCK)" in src
