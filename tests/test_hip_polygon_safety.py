"""GPU: the safety-polygon service on the device (emap_polygon_safety; ElevationMap.get_polygons_traversability and the device route
of get_polygon_traversability) against the host route on the SAME context: is_safe, area, vertex count, the counts and the maximum are
identical, the ring is the same cyclic sequence, and the mean lies within the bound of two float64 summations of the same terms from the
model's float64 mean (tests/_polysafe_cases.py).  Maps of 66^2, 130^2 and 258^2 cells dressed with set_layer_raw; one 530^2 map for the
call behind a frame whose stencil pass is pending (maps up to 512^2 never defer it)."""
import ctypes as ct
import os

import numpy as np
import pytest

import _fixtures as fx
import _polysafe_cases as pc
from _util import make_parameter
from test_hip_services import POLYGONS
from test_polygon_safety_abi import _call

pytestmark = pytest.mark.gpu


def _map(C, weights, plugin_file=None):
    from elevation_mapping_cupy_amd.elevation_mapping import ElevationMap
    p = make_parameter({}, C, "reference_fp16", weights)
    p.safe_thresh, p.safe_min_thresh, p.max_unsafe_n = pc.SAFE_THRESH, pc.SAFE_MIN_THRESH, pc.MAX_UNSAFE_N
    if plugin_file is not None:
        p.plugin_config_file = str(plugin_file)
    return ElevationMap(p)


@pytest.fixture(scope="module")
def maps(weights):
    made = {}

    def get(C):
        if C not in made:
            made[C] = _map(C, weights)
        return made[C]
    return get


def _dress(hip, trav, valid):
    hip.set_layer_raw("traversability", trav)
    hip.set_layer_raw("is_valid", valid)


def _same_f32(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def _same_ring(a, b):
    """the same vertices in the same order, whichever comes first"""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or not (np.array_equal(a[0], a[-1]) and np.array_equal(b[0], b[-1])):
        return False
    a, b = a[:-1], b[:-1]
    return any(np.array_equal(np.roll(a, k, axis=0), b) for k in range(len(a)))


def _check(hip, poly, layer=None, route="device"):
    """both routes on this context for one polygon; returns the device route's verdict and the model"""
    res = np.zeros(3)
    n_host = hip._polygon_traversability_host(poly, res, layer)
    ring_host, counts, mask = hip.untraversable_polygon, hip._host_counts, hip.mask.copy()
    out, rings = hip.get_polygons_traversability([poly], layer)
    assert hip.last_polygon_route == route
    assert np.array_equal(hip.mask, mask)        # built when it is read: no mask came back from the device
    v = out[0]
    print("host", res, counts, "device", v)
    assert bool(v["is_safe"]) == bool(res[0]) and v["area"] == res[2]
    assert (0 if rings[0] is None else rings[0].shape[0]) == n_host
    assert v["n_inside"] == int(mask[1:-1, 1:-1].sum())
    assert v["n_known"] == counts[0] and v["n_risky"] == counts[1]
    assert _same_f32(v["max_risk"], counts[2]), (v["max_risk"], counts[2])
    assert _same_ring(rings[0], ring_host), (rings[0], ring_host)
    name = hip.param.checker_layer if layer is None else layer
    m = pc.model(mask, np.asarray(hip.get_layer(name), np.float32), hip.get_layer_raw("is_valid"),
                 pc.work_table(hip.cell_n, hip._clip_polygon(np.asarray(poly, np.float64)), hip.center),
                 hip.param.max_unsafe_n, hip.param.safe_thresh, hip.param.safe_min_thresh)
    from elevation_mapping_cupy_amd.elevation_mapping import _shoelace_area
    in_map = _shoelace_area(hip._clip_polygon(np.asarray(poly, np.float64))) >= 0.001      # (a polygon clipped to nothing is unsafe whatever it holds)
    assert m["n_inside"] == v["n_inside"] and m["n_risky"] == v["n_risky"] and (m["is_safe"] and in_map) == bool(v["is_safe"])
    if np.isnan(m["mean_risk"]):
        assert np.isnan(v["mean_risk"]) and np.isnan(res[1])
    else:                                    # two float64 summations of the same n_inside terms
        d = abs(float(v["mean_risk"]) - m["mean_risk"])
        print("mean: device %.17g model %.17g host %.17g" % (v["mean_risk"], m["mean_risk"], res[1]))
        assert d * m["sum_valid"] <= 2 * m["n_inside"] * 2.0 ** -53 * m["abs_risk"]
        assert abs(res[1] - m["mean_risk"]) <= 1e-5 * max(1.0, abs(m["mean_risk"]))      # (the host route's float32 sum: the same quantity)
    return v, rings[0], m


@pytest.mark.parametrize("name", [n for n in sorted(pc.CASES) if pc.CASES[n][1] is None and pc.CASES[n][4]])
def test_cases_against_the_host_route(name, maps):
    C, center, world, clipped, mask, trav, valid, table = pc.build(name)
    hip = maps(C)
    _dress(hip, trav, valid)
    v, ring, m = _check(hip, world)
    want = pc.model(mask, trav, valid, table)      # the case's own planes and the oracle's mask: the property it is named for, on the device
    assert v["n_inside"] == want["n_inside"] and v["n_risky"] == want["n_risky"] and bool(v["is_safe"]) == want["is_safe"]
    assert _same_f32(v["max_risk"], want["max_risk"])
    assert (ring is None) == (want["ring"] is None)
    assert v["n_known"] < v["n_inside"]            # unknown cells inside
    res = np.zeros(3)
    n = hip.get_polygon_traversability(world, res)
    assert hip.last_polygon_route == "device" and bool(res[0]) == bool(v["is_safe"]) and res[2] == v["area"] and n == (0 if ring is None else ring.shape[0])
    assert _same_f32(np.float32(res[1]), np.float32(v["mean_risk"]))
    assert np.array_equal(hip.mask, hip.polygon_mask(hip._clip_polygon(world)))      # built when it is read


@pytest.mark.parametrize("k", range(len(POLYGONS) + 1))
@pytest.mark.parametrize("C", [66, 130])
def test_service_polygons_against_the_host_route(k, C, maps):
    """convex, concave, sub-cell, larger than the map, and one outside the map"""
    hip = maps(C)
    trav, valid = pc.base_planes(C, seed=3)
    trav[::5, ::3] = pc.RISKY
    _dress(hip, trav, valid)
    poly = POLYGONS[k].astype(np.float64) if k < len(POLYGONS) else np.array([[90.0, 90.0], [91.0, 90.0], [91.0, 91.0], [90.0, 91.0]])
    v, ring, m = _check(hip, poly)
    if k == len(POLYGONS):
        assert not v["is_safe"]


def test_the_border_box_is_cut_to_the_interior(maps):
    """a box that reaches rows and columns 0 and C-1 (no clipping: straight into the entry point's wrapper) counts rows and columns 1 .. C-2"""
    C, center, world, clipped, mask, trav, valid, table = pc.build("border")
    hip = maps(C)
    _dress(hip, trav, valid)
    with hip.map_lock:
        verdicts, cells = hip._polygons_device([clipped], (0, 3))
    v, m = verdicts[0], pc.model(mask, trav, valid, table)
    assert (v.row_begin, v.n_rows, v.col_begin, v.n_cols) == (1, C - 2, 1, C - 2)
    assert v.n_inside == m["n_inside"] == (C - 2) ** 2 and v.n_risky == m["n_risky"] == 12 and v.sum_valid == m["n_known"]
    assert _same_f32(v.max_risk, m["max_risk"]) and v.sum_risk == m["sum_risk"]      # the model sums in the kernels' order: the same bits
    got = set(map(tuple, cells[0]))
    risky = np.argwhere(m["too_risky"])
    want = set()
    for r in set(risky[:, 0]):
        cs = risky[risky[:, 0] == r][:, 1]
        want |= {(r, cs.min()), (r, cs.max())}
    assert got == want


@pytest.mark.parametrize("layer", ["traversability", "sem"])
def test_the_circular_origin_cuts_the_box(layer, weights):
    """one real frame, then a move_to that puts the physical wrap inside the polygon's box: a map layer and a semantic layer"""
    C, center, world, clipped, mask, trav, valid, table = pc.build("cut")
    hip = _map(C, weights)
    if layer == "sem":
        hip.semantic_map.add_layer("sem")
    R, t = fx.POSES["identity"]
    hip.input_pointcloud(fx.cloud(C, 20000, 0), ["x", "y", "z"], R, t.copy(), 0.0, 0.0)
    hip.move_to(center.astype(np.float64), np.eye(3))
    assert np.array_equal(hip.center[:2], center[:2])
    v0, _, _ = _check(hip, world, "traversability")      # the frame's own planes
    assert v0["n_inside"] > 100
    _dress(hip, trav, valid)
    if layer == "sem":
        hip.semantic_map.set_layer("sem", trav)
        hip.set_layer_raw("traversability", np.full((C, C), 0.75, np.float32))
    v, ring, m = _check(hip, world, layer)
    want = pc.model(mask, trav, valid, table)
    assert v["n_inside"] == want["n_inside"] and v["n_risky"] == want["n_risky"] == 9 and ring is not None


PLUGIN_YAML = """
min_filter:
  enable: True
  fill_nan: False
  is_height_layer: False
  layer_name: "min_filter"
  extra_params:
    dilation_size: 1
    iteration_n: 30
"""


def test_a_plugin_checker_layer_on_both_routes(weights, tmp_path, monkeypatch):
    cfg = tmp_path / "plugins.yaml"
    cfg.write_text(PLUGIN_YAML)
    C = 66
    hip = _map(C, weights, cfg)
    rng = np.random.RandomState(5)
    hip.set_layer_raw("elevation", rng.rand(C, C).astype(np.float32))      # risk = 1 - min-filtered elevation: 0 .. 1
    hip.set_layer_raw("is_valid", (rng.rand(C, C) > 0.2).astype(np.float32))
    hip.param.checker_layer = "min_filter"
    v, ring, m = _check(hip, pc.QUAD)
    assert hip.last_polygon_route == "device" and v["n_risky"] > 0
    res = np.zeros(3)
    n = hip.get_polygon_traversability(pc.QUAD, res)
    assert hip.last_polygon_route == "device" and bool(res[0]) == bool(v["is_safe"])
    monkeypatch.setenv("EMAP_PLUGIN_RESIDENT", "0")                          # the same plugin on its host route: the service follows it
    res_h = np.zeros(3)
    n_h = hip.get_polygon_traversability(pc.QUAD, res_h)
    assert hip.last_polygon_route == "host" and n_h == n and res_h[0] == res[0] and res_h[2] == res[2] and abs(res_h[1] - res[1]) < 1e-6
    out, rings = hip.get_polygons_traversability([pc.QUAD])
    assert hip.last_polygon_route == "host" and out["n_risky"][0] == v["n_risky"] and out["n_inside"][0] == v["n_inside"]
    monkeypatch.delenv("EMAP_PLUGIN_RESIDENT")
    monkeypatch.setenv("EMAP_POLYGON_RESIDENT", "0")                         # the knob of the service itself
    hip.get_polygon_traversability(pc.QUAD, res_h)
    assert hip.last_polygon_route == "host"
    monkeypatch.delenv("EMAP_POLYGON_RESIDENT")
    hip.param.checker_layer = "no_such_layer"                                # an unknown layer: the host route, which fails as it always did
    with pytest.raises(IndexError):                                          # (get_layer returns None: a 0-dimensional plane)
        hip.get_polygon_traversability(pc.QUAD, res_h)
    assert hip.last_polygon_route == "host"
    hip.param.checker_layer = "traversability"
    hip.get_polygon_traversability(np.concatenate([pc.QUAD] * 65), res_h)    # 260 vertices
    assert hip.last_polygon_route == "host"


def _batch_polygons(n, seed):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        c, s = rng.uniform(-1.8, 1.8, 2), rng.uniform(0.05, 0.9, 2)
        out.append(c + np.array([[-s[0], -s[1]], [s[0], -s[1] * 0.7], [s[0] * 0.8, s[1]], [-s[0] * 0.6, s[1] * 0.9]]))
    return out


def _raw(hip, polys):
    with hip.map_lock:
        verdicts, cells = hip._polygons_device([hip._clip_polygon(np.asarray(p, np.float64)) for p in polys], (0, 3))
    return [bytes(v) for v in verdicts], cells


@pytest.mark.parametrize("n", [1, 2, 37])
def test_a_batch_equals_the_single_calls(n, maps):
    C = 130
    hip = maps(C)
    trav, valid = pc.base_planes(C, seed=11)
    trav[::4, ::7] = pc.RISKY
    _dress(hip, trav, valid)
    polys = _batch_polygons(n, 2)
    out, rings = hip.get_polygons_traversability(polys)
    assert hip.last_polygon_route == "device" and out.shape == (n,)
    raw, cells = _raw(hip, polys)
    for k, p in enumerate(polys):
        one, ring = hip.get_polygons_traversability([p])
        assert one[0].tobytes() == out[k].tobytes()
        assert (ring[0] is None and rings[k] is None) or np.array_equal(ring[0], rings[k])
        raw1, cells1 = _raw(hip, [p])
        assert raw1[0] == raw[k] and np.array_equal(cells1[0], cells[k])
    assert out["n_inside"].min() > 0 and out["n_risky"].max() > 0


def test_batch_position_and_repetition_change_no_byte(maps):
    C = 130
    hip = maps(C)
    trav, valid = pc.base_planes(C, seed=12)
    trav[::3, ::5] = pc.RISKY
    _dress(hip, trav, valid)
    a, b = _batch_polygons(2, 9)
    raw, cells = _raw(hip, [a, b, a, b, b])
    assert raw[0] == raw[2] and raw[1] == raw[3] == raw[4] and raw[0] != raw[1]
    assert np.array_equal(cells[0], cells[2]) and np.array_equal(cells[1], cells[4])
    raw2, cells2 = _raw(hip, [a, b, a, b, b])
    assert raw2 == raw and all(np.array_equal(x, y) for x, y in zip(cells, cells2))


def _fused(hip):
    v = ct.c_uint32(0)
    hip._chk(hip._lib.emap_post_fused_launches(hip._ctx, ct.byref(v)))
    return int(v.value)


def test_a_call_behind_a_pending_stencil_pass_sees_the_settled_traversability(weights, monkeypatch):
    """two binned whole-map frames back to back: the second ran the first's stencil pass in its own launch (the counter proves that this
    map defers), so its own pass is pending when the service is called"""
    C = 530
    R, t = fx.POSES["identity"]
    poly = np.array([[-3.0, -2.0], [4.0, -3.0], [3.0, 4.0], [-2.0, 3.0]])

    def run(defer):
        if not defer:
            monkeypatch.setenv("EMAP_POST_DEFER", "0")
        hip = _map(C, weights)
        hip.set_scatter_mode("binned")
        hip.bind_points(fx.cloud(C, 60000, 0))      # once: an upload is a call into the library and would launch the pending pass
        for _ in (0, 1):
            hip.update_map_with_kernel(None, [], R, t.copy(), 0.0, 0.0, want_stats=False)
        monkeypatch.delenv("EMAP_POST_DEFER", raising=False)
        return hip

    a = run(True)
    assert _fused(a) == 1
    out, rings = a.get_polygons_traversability([poly])      # the first call into the library after the frame
    assert a.last_polygon_route == "device"
    b = run(False)
    assert _fused(b) == 0
    trav = b.get_layer_raw("traversability")
    res = np.zeros(3)
    n = b._polygon_traversability_host(poly, res)
    assert np.array_equal(a.get_layer_raw("traversability").view(np.uint32), trav.view(np.uint32))
    v = out[0]
    assert bool(v["is_safe"]) == bool(res[0]) and (v["n_known"], v["n_risky"]) == b._host_counts[:2] and _same_f32(v["max_risk"], b._host_counts[2])
    assert v["n_inside"] == int(b.mask[1:-1, 1:-1].sum())
    assert v["n_known"] > 1000 and abs(v["mean_risk"] - res[1]) < 1e-5
    assert _same_ring(rings[0], b.untraversable_polygon)


def test_refusals_with_a_context(maps, weights):
    from elevation_mapping_cupy_amd import _lib
    from elevation_mapping_cupy_amd.elevation_mapping import ElevationMap
    hip = maps(66)
    lib = hip._lib
    why = lambda: lib.emap_last_error(hip._ctx).decode()
    assert _call(lib, hip._ctx) == 0                                          # the helper's call is a good one
    for kw, word in [(dict(xy=False), "null"), (dict(verdicts=False), "null"), (dict(ext=False), "null"), (dict(begin=None), "null"), (dict(ext_begin=None), "null"),
                     (dict(n=0), "n_polygons"), (dict(n=_lib.POLY_MAX_BATCH + 1, begin=tuple(range(_lib.POLY_MAX_BATCH + 2)), ext_begin=(0,) * (_lib.POLY_MAX_BATCH + 2)), "n_polygons"),
                     (dict(begin=(0, 0)), "at least 1 vertex"), (dict(begin=(0, 257)), "at most 256"), (dict(n=2, begin=(0, 4, 2), ext_begin=(0, 64, 128)), "increase"),
                     (dict(begin=(1, 4)), "vertex_begin[0]"), (dict(kind=2), "layer_kind"), (dict(kind=0, index=7), "0 .. 6"), (dict(kind=1, index=0), "semantic"),
                     (dict(kind=3, index=0), "not reserved"), (dict(ext_begin=(0, 0)), "room")]:
        assert _call(lib, hip._ctx, **kw) == -1 and word in why(), (kw, why())
    p = make_parameter({}, 66, "reference_fp16", weights)
    strip = ElevationMap(p, strip=(0, 33, 0))
    assert _call(lib, strip._ctx) == -1 and "single-strip" in lib.emap_last_error(strip._ctx).decode()
    with pytest.raises(_lib.EmapError):
        strip.get_polygons_traversability([pc.QUAD])
