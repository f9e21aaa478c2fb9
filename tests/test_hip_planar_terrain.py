"""GPU: the planar terrain on the device (emap_planar_terrain / csrc/emap_terrain.hip; ElevationMap.get_planar_terrain).  The yardstick is
the whole-map door on the same context and state, get_grid_map_layers(order="rows") of the source layer, fed to the host model
(elevation_mapping_cupy_amd/planar_terrain.py, checked on the CPU by tests/test_planar_terrain_cases.py): the labels, n_labels, the
float normals and the eight float planes (uint32 views) and every field of the plane records (uint64 views of the doubles) compared bit
for bit.  The start state is that of tests/_grid_cases.py (the circular origin off zero, a shift pending); scenes are written in
published index space with set_layer_raw.  No test provokes a fault: every refusal happens before a launch.  Reference:
GridMapPreprocessing.cpp:14-39, Postprocessing.cpp:14-146."""
import ctypes as ct

import numpy as np
import pytest

import _grid_cases as gc
import _plane_seg_cases as pc
import _planar_terrain_cases as tc
import _plug_cases as plug
from elevation_mapping_cupy_amd import planar_terrain as pt

pytestmark = pytest.mark.gpu
POISON = 0x5A5A5A5A
_maps = {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_shared_maps():
    yield
    for m in _maps.values():
        m.close()
    _maps.clear()


def _shared(C):
    if C not in _maps:
        _maps[C] = gc.start(C)
    return _maps[C]


def _frame(m):
    from elevation_mapping_cupy_amd.elevation_mapping import grid_cell_positions
    res = float(np.float32(m.resolution))
    xs, ys = grid_cell_positions((float(m.center[0]), float(m.center[1])), res, m.cell_n - 2)
    return res, (float(xs[0]), float(ys[0]))


def _write(m, h):
    """heights in published index space; NaN: the cell is not valid (the published elevation is NaN there)"""
    C = m.cell_n
    valid = ~np.isnan(h)
    m.set_layer_raw("elevation", pc.logical_plane(np.where(valid, h, np.float32(0.0)), C))
    m.set_layer_raw("is_valid", pc.logical_plane(valid, C))


def _check(m, over, pre, post, layer="elevation", what=""):
    """one call against the model on the yardstick's plane"""
    _, planes = m.get_grid_map_layers([layer])
    res, origin = _frame(m)
    P = pc.params(**over)
    want = pt.terrain(planes[0], res, origin, pre, post, **P)
    got = m.get_planar_terrain(layer, preprocess=pre, postprocess=post, intermediates=True, normals=True, **P)
    assert m.last_planar_terrain_route == "device", what
    assert got.origin_xy == origin and got.resolution == res
    assert got.n_labels == want.n_labels, (what, got.n_labels, want.n_labels)
    assert (got.labels == want.labels).all(), "%s: %d labels differ" % (what, int((got.labels != want.labels).sum()))
    assert tc.same_words(got.normals, want.normals), "%s: normals" % what
    assert len(got.planes) == len(want.planes), (what, len(got.planes), len(want.planes))
    for f in ("label", "n_points", "needs_refinement", "n_left_out", "support", "normal"):
        assert tc.same_words(got.planes[f], want.planes[f]), (what, f, got.planes[f], want.planes[f])
    for n in pt.PLANES:
        a, b = getattr(got, n), getattr(want, n)
        assert tc.same_words(a, b), "%s: %s, %d words differ (first at %s)" % (what, n, int((a.view(np.uint32) != b.view(np.uint32)).sum()),
                                                                               np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:1].tolist())
    return want, got


@pytest.mark.parametrize("C", tc.SIZES)
def test_every_scene_with_the_reference_defaults(C):
    """postprocess=None at 4 cm: kd = 11, kb = 7, kg = 3, offset 1, 2 cm; without and with the preprocessing"""
    m = _shared(C)
    res, _ = _frame(m)
    assert pt.check(C - 2, res, tc.PRE, None)[2] == (11, 7, 3)
    for name, (h, over) in tc.scenes(C - 2).items():
        _write(m, h)
        raw = _check(m, over, None, None, what="%s at %d" % (name, C))[1]
        pre = _check(m, over, tc.PRE, None, what="%s at %d, preprocessed" % (name, C))[1]
        if name == "no planar cell":
            assert np.isnan(raw.smooth_planar).all() and raw.n_labels == 0      # (the median flattens the rough checker: not so with it)
        if name == "all NaN":
            assert np.isnan(pre.elevation).all() and np.isnan(pre.elevation_before_postprocess).all()
        if name == "hole":
            assert np.isnan(raw.elevation_before_postprocess).any() and not np.isnan(pre.elevation_before_postprocess).any()


@pytest.mark.parametrize("name", sorted(tc.parameter_sets(tc.RES)))
def test_every_parameter_set(name):
    """kernels of 1 and 31 cells, the Gaussian past its fixed tables, the median's sizes and repeats, the dilation's offsets, the lifts"""
    for C in tc.SIZES:
        m = _shared(C)
        res, _ = _frame(m)
        pre, post = tc.parameter_sets(res)[name]
        for scene in tc.SWEEP_SCENES:
            h, over = tc.scenes(C - 2)[scene]
            _write(m, h)
            _check(m, over, pre, post, what="%s on %s at %d" % (name, scene, C))


def test_the_large_map_once():
    """M = 363: 12 x 12 tiles with a ragged edge, 4118 mask words"""
    m = _shared(tc.BIG)
    for name in tc.BIG_SCENES:
        h, over = tc.scenes(tc.BIG - 2)[name]
        _write(m, h)
        _check(m, over, tc.PRE, None, what="%s at %d" % (name, tc.BIG))


def test_without_preprocessing_the_segmentation_is_get_plane_segmentations():
    m = _shared(67)
    for name in ("pieces", "hills", "bridge"):
        h, over = tc.scenes(65)[name]
        _write(m, h)
        P = pc.params(**over)
        a = m.get_plane_segmentation(normals=True, **P)
        b = m.get_planar_terrain(normals=True, postprocess=dict(extracted_planes_height_offset=0.0), **P)
        assert a.n_labels == b.n_labels and a.labels.tobytes() == b.labels.tobytes() and a.normals.tobytes() == b.normals.tobytes() and a.planes.tobytes() == b.planes.tobytes(), name
        assert not hasattr(b, "elevationWithNaN") and tc.same_words(b.plane_classification, (a.labels > 0).astype(np.float32))
        _, planes = m.get_grid_map_layers(["elevation"])
        assert tc.same_words(b.elevation_before_postprocess, planes[0])


def test_a_second_call_after_the_map_changed_and_the_host_route(monkeypatch):
    def run(m):
        r = m.get_planar_terrain(preprocess={}, intermediates=True, normals=True, connectivity=8)
        return b"".join(getattr(r, n).tobytes() for n in pt.PLANES) + r.labels.tobytes() + r.normals.tobytes() + r.planes.tobytes() + np.int64(r.n_labels).tobytes()
    m = _shared(67)
    _write(m, tc.hole(65))
    first = run(m)
    _write(m, np.full((65, 65), np.nan, np.float32))
    empty = run(m)
    _write(m, tc.hole(65))
    assert run(m) == first and empty != first                 # the context's buffers are reused: nothing of the call before is left
    monkeypatch.setenv("EMAP_TERRAIN_RESIDENT", "0")
    assert run(m) == first and m.last_planar_terrain_route == "host"


def test_the_start_state_and_a_plugin_layer_as_the_source(tmp_path):
    cfg = tmp_path / "plugins.yaml"
    cfg.write_text(plug.yaml_of([plug._entry("smooth_filter", "smooth", fill_nan=True, height=True, input_layer_name="elevation"), plug.CORE[2]]))
    m = gc.start(67, plugin_file=cfg)
    try:
        want, _ = _check(m, {}, tc.PRE, None, what="start state")      # the relief of tests/_grid_cases.py as it lies after the move
        assert 0 < int(want.plane_classification.sum()) < 65 * 65
        _write(m, tc.scenes(65)["terraces"][0])
        _check(m, {}, None, None, layer="smooth", what="a resident plugin plane")
        assert m.last_plugin_route == {"smooth": "device"}
        with pytest.raises(ValueError, match="host route"):
            m.get_planar_terrain("inpaint")
        with pytest.raises(ValueError):
            m.get_planar_terrain("ghost")
    finally:
        m.close()


# ---- the raw call: planes that were not asked for, refusals ---------------------------------------------------------------------------------
def _raw(m, null=(), capacity=64, plane_over=None, **over):
    from elevation_mapping_cupy_amd import _lib
    M = m.cell_n - 2
    res, origin = _frame(m)
    src = _lib.EmapGridLayerEx(0, 0, 0, 0)
    pv = dict(kernel_size=3, planarity_opening_filter=0, min_number_points_per_label=4, connectivity=4, use_only_above_for_upper_bound=0, reserved=0,
              center_z=float(m.center[2]), reserved_f=0.0, resolution=res, origin_x=origin[0], origin_y=origin[1], plane_patch_error_threshold=0.02,
              cos_local_plane_inclination=0.8, cos_plane_inclination=0.85, global_plane_fit_distance_error_threshold=0.025, cos_global_plane_fit_angle=0.9)
    pv.update(plane_over or {})
    P = _lib.EmapPlaneParams(**pv)
    tv = dict(preprocess=1, median_kernel_size=3, median_repeats=1, nonplanar_horizontal_offset=1, want=255, reserved=0, smoothing_dilation_size=5 * res,
              smoothing_box_kernel_size=3 * res, smoothing_gauss_kernel_size=res, extracted_planes_height_offset=0.0, nonplanar_height_offset=0.02)
    tv.update(over)
    Q = _lib.EmapTerrainParams(**tv)
    labels, normals = np.full(M * M, POISON, np.uint32), np.full(3 * M * M, POISON, np.uint32)
    rec = np.full(capacity * 64 + 64, 0x5A, np.uint8)
    planes = np.full((8, M * M), POISON, np.uint32)
    O = _lib.EmapTerrainPlanes()
    for k in range(8):
        if "plane %d" % k not in null:
            O.plane[k] = planes[k].ctypes.data_as(ct.POINTER(ct.c_float))
    n_labels, n_planes = ct.c_int32(-7), ct.c_int64(-7)
    rc = m._lib.emap_planar_terrain(m._ctx, None if "source" in null else ct.byref(src), None if "params" in null else ct.byref(P), None if "terrain" in null else ct.byref(Q),
                                    None if "labels" in null else labels.ctypes.data_as(ct.POINTER(ct.c_int32)), normals.ctypes.data_as(ct.POINTER(ct.c_float)),
                                    None if "planes" in null else rec.ctypes.data_as(ct.POINTER(_lib.EmapPlaneRecord)), capacity, None if "n_labels" in null else ct.byref(n_labels),
                                    None if "n_planes" in null else ct.byref(n_planes), None if "out" in null else ct.byref(O))
    untouched = bool((labels == POISON).all() and (normals == POISON).all() and (rec == 0x5A).all() and (planes == POISON).all() and n_labels.value == -7 and n_planes.value == -7)
    return rc, untouched, planes


def test_planes_that_were_not_asked_for_keep_their_poison():
    m = _shared(67)
    _write(m, tc.hole(65))
    rc, _, every = _raw(m)
    assert rc == 0 and not (every == POISON).all(axis=1).any()
    for want in (1, 2 | 8, 4 | 128, 16 | 32 | 64, 0):
        rc, _, planes = _raw(m, want=want)
        assert rc == 0
        for k in range(8):
            if (want >> k) & 1:
                assert (planes[k] == every[k]).all(), (want, k)
            else:
                assert (planes[k] == POISON).all(), (want, k)
    rc, _, planes = _raw(m, want=2, null=("plane 0", "plane 7"))      # a plane that is not wanted needs no buffer
    assert rc == 0 and (planes[1] == every[1]).all()


def test_every_refusal_leaves_the_outputs_and_the_map_as_they_were():
    m = gc.start(34)
    try:
        _write(m, tc.scenes(32)["terraces"][0])
        res, _ = _frame(m)
        state = lambda: m.elevation_map.tobytes() + m.normal_map.tobytes()      # noqa: E731
        s0 = state()
        nan, inf = float("nan"), float("inf")
        cases = {
            "null source": dict(null=("source",)), "null params": dict(null=("params",)), "null terrain": dict(null=("terrain",)), "null labels": dict(null=("labels",)),
            "null planes": dict(null=("planes",)), "null n_labels": dict(null=("n_labels",)), "null n_planes": dict(null=("n_planes",)), "null out": dict(null=("out",)),
            "a wanted plane without a buffer": dict(null=("plane 3",)), "unknown plane": dict(want=256), "preprocess 2": dict(preprocess=2),
            "even median": dict(median_kernel_size=4), "median 2": dict(median_kernel_size=2), "9 repeats": dict(median_repeats=9), "-1 repeats": dict(median_repeats=-1),
            "offset 16": dict(nonplanar_horizontal_offset=16), "offset -1": dict(nonplanar_horizontal_offset=-1),
            "closing of 33 cells": dict(smoothing_dilation_size=16 * res), "box of 33 cells": dict(smoothing_box_kernel_size=16 * res), "Gaussian of 33 cells": dict(smoothing_gauss_kernel_size=16 * res),
            "negative size": dict(smoothing_box_kernel_size=-res), "size NaN": dict(smoothing_dilation_size=nan), "size inf": dict(smoothing_gauss_kernel_size=inf),
            "offset NaN": dict(nonplanar_height_offset=nan), "offset inf": dict(extracted_planes_height_offset=inf), "negative capacity": dict(capacity=-1),
            "kernel 4 (segmentation)": dict(plane_over=dict(kernel_size=4)), "connectivity 6": dict(plane_over=dict(connectivity=6)), "resolution 0": dict(plane_over=dict(resolution=0.0)),
        }
        for what, kw in cases.items():
            rc, untouched, _ = _raw(m, **kw)
            assert rc == -1 and untouched, what
            assert b"emap_planar_terrain" in m._lib.emap_last_error(m._ctx), what
        assert state() == s0
        assert _raw(m)[0] == 0 and _raw(m, smoothing_dilation_size=15 * res, smoothing_box_kernel_size=15 * res, nonplanar_horizontal_offset=15)[0] == 0      # 31 cells fit 32
        for kw in (dict(preprocess={"kernelSize": 4}), dict(preprocess={"numberOfRepeats": 9}), dict(preprocess={"resolution": 0.05}),
                   dict(postprocess={"nonplanar_horizontal_offset": 16}), dict(postprocess={"smoothing_dilation_size": 16 * res}), dict(kernel_size=4)):
            with pytest.raises(ValueError):
                m.get_planar_terrain(**kw)
        assert state() == s0
    finally:
        m.close()


def test_a_kernel_larger_than_the_map_and_a_strip_context_are_refused():
    from elevation_mapping_cupy_amd._lib import EmapError
    m = gc.start(12)                                           # M = 10: the default closing of 11 cells does not fit
    try:
        res, _ = _frame(m)
        rc, untouched, _ = _raw(m)
        assert rc == -1 and untouched and b"map's side" in m._lib.emap_last_error(m._ctx)
        with pytest.raises(ValueError):
            m.get_planar_terrain()
        assert _raw(m, smoothing_dilation_size=4 * res)[0] == 0      # 9 cells do
    finally:
        m.close()
    m = gc.start(34, strip=(0, 17, 0))
    try:
        rc, untouched, _ = _raw(m)
        assert rc == -1 and untouched and b"single-strip" in m._lib.emap_last_error(m._ctx)
        with pytest.raises(EmapError):
            m.get_planar_terrain()
    finally:
        m.close()
