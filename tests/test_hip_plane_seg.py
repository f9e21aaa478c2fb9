"""GPU: the plane segmentation on the device (emap_plane_segmentation / csrc/emap_planeseg.hip; ElevationMap.get_plane_segmentation).
The yardstick is the whole-map door on the same context and state, get_grid_map_layers(order="rows") of the source layer, fed to the
tests' model (tests/_plane_seg_cases.py, checked on the CPU by tests/test_plane_seg_cases.py): labels, n_labels, the planar bits, the
float normals (uint32 views) and every field of the plane records (uint64 views of the doubles) compared bit for bit; the tail of the
label buffer keeps its poison.  The planar bits are read off a second call whose plane inclination limit rejects nothing: there a
cell is planar exactly if its label is not 0.  The start state is that of tests/_grid_cases.py: the circular origin is off zero, a
shift is pending, the normals lie at an older origin; scenes are written in published index space with set_layer_raw.  No test
provokes a fault: every refusal happens before a launch.  Reference: SlidingWindowPlaneExtractor.cpp:49-77, :115-220, :277-300."""
import ctypes as ct

import numpy as np
import pytest

import _grid_cases as gc
import _plane_seg_cases as pc
import _plug_cases as plug

pytestmark = pytest.mark.gpu
POISON = np.int32(-0x5A5A5A5B)
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


def _same_words(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    w = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(w) == b.view(w)).all())


def _check(m, over, layer="elevation", what=""):
    """one call against the model on the yardstick's plane"""
    M = m.cell_n - 2
    _, planes = m.get_grid_map_layers([layer])
    res, origin = _frame(m)
    want = pc.model(planes[0], over, resolution=res, origin=origin)
    P = pc.params(**over)
    buf = np.full(M * M + 64, POISON, np.int32)
    got = m.get_plane_segmentation(layer, normals=True, out=buf[:M * M].reshape(M, M), **P)
    assert m.last_plane_segmentation_route == "device", what
    assert (buf[M * M:] == POISON).all(), "%s: written past the labels" % what
    assert got.labels.ctypes.data == buf.ctypes.data and got.origin_xy == origin and got.resolution == res
    assert got.n_labels == want.n_labels, (what, got.n_labels, want.n_labels)
    assert (got.labels == want.labels).all(), "%s: %d labels differ" % (what, int((got.labels != want.labels).sum()))
    assert _same_words(got.normals, want.normals), "%s: %d normal words differ" % (what, int((got.normals.view(np.uint32) != want.normals.view(np.uint32)).sum()))
    assert len(got.planes) == len(want.planes), (what, len(got.planes), len(want.planes))
    for f in ("label", "n_points", "needs_refinement", "n_left_out", "support", "normal"):
        assert _same_words(got.planes[f], want.planes[f]), (what, f, got.planes[f], want.planes[f])
    every = m.get_plane_segmentation(layer, **dict(P, plane_inclination_threshold_degrees=89.9))
    assert ((every.labels > 0) == want.planar).all(), "%s: planar bits" % what
    assert every.normals is None
    return want


@pytest.mark.parametrize("C", pc.SIZES)
def test_every_scene(C):
    """C = 365: M = 363, 4118 bit words -- past the 4096 words the numbering scan's one workgroup takes in a single trip"""
    m = _shared(C)
    M = C - 2
    for name, (h, over, props) in pc.scenes(M).items():
        if C == pc.SIZES[-1] and name not in pc.BIG_SCENES:
            continue
        _write(m, h)
        want = _check(m, over, what="%s at %d" % (name, C))
        if "n_labels" in props:
            assert want.n_labels == props["n_labels"], name                     # the scene is what it claims, on the device's own plane
        if "n_planes" in props:
            assert len(want.planes) == props["n_planes"], name
        if "needs" in props:
            assert want.planes["needs_refinement"].tolist() == props["needs"], name


def test_the_start_state_itself():
    """the relief of tests/_grid_cases.py as it lies in the map after the move: the walk's origin handling, not a designed scene"""
    m = gc.start(67)
    try:
        want = _check(m, {}, what="start state")
        assert 0 < int(want.planar.sum()) < 65 * 65
        _check(m, dict(connectivity=8, kernel_size=5, planarity_opening_filter=2), what="start state, 8 / 5 / 2")
    finally:
        m.close()


def test_a_plugin_layer_as_the_source_and_the_host_route_refusal(tmp_path):
    cfg = tmp_path / "plugins.yaml"
    cfg.write_text(plug.yaml_of([plug._entry("smooth_filter", "smooth", fill_nan=True, height=True, input_layer_name="elevation"), plug.CORE[2]]))
    m = gc.start(67, plugin_file=cfg)
    try:
        h, over, _ = pc.scenes(65)["terraces"]
        _write(m, h)
        want = _check(m, over, layer="smooth", what="a resident plugin plane")
        assert m.last_plugin_route == {"smooth": "device"} and want.n_labels >= 2
        labels = np.full((65, 65), POISON, np.int32)
        with pytest.raises(ValueError, match="host route"):
            m.get_plane_segmentation("inpaint", out=labels)
        assert (labels == POISON).all()
        with pytest.raises(ValueError):
            m.get_plane_segmentation("ghost")
    finally:
        m.close()


def test_two_calls_two_contexts_and_the_host_route_agree(monkeypatch):
    def run(m):
        r = m.get_plane_segmentation(normals=True, connectivity=8)
        return r.labels.tobytes() + r.normals.tobytes() + r.planes.tobytes() + np.int64(r.n_labels).tobytes()
    a, b = gc.start(67), gc.start(67)
    try:
        for name in ("elevation", "is_valid"):                                  # the second context holds the same planes
            b.set_layer_raw(name, a.get_layer_raw(name))
        first = run(a)
        assert run(a) == first and run(b) == first
        monkeypatch.setenv("EMAP_PLANES_RESIDENT", "0")
        assert run(a) == first and a.last_plane_segmentation_route == "host"
    finally:
        a.close(); b.close()


def test_the_record_buffer_grows_and_a_short_one_is_left_alone():
    """more labels with a plane than the wrapper's first buffer holds: 2 x 2 blocks four cells apart"""
    m = _shared(365)
    M = 363
    P = np.zeros((M, M), bool)
    for a in (0, 1):
        for b in (0, 1):
            P[2 + a:M - 3:6, 2 + b:M - 3:6] = True
    _write(m, pc.carve(P))
    want = _check(m, {}, what="many planes")
    assert len(want.planes) > 256
    n_planes, rec = _raw(m, capacity=16)[1:]
    assert n_planes == len(want.planes) and (rec.view(np.uint8) == 0x5A).all()


# ---- refusals: before anything is launched or copied ---------------------------------------------------------------------------------------
def _raw(m, capacity=8, null=(), source=(0, 0, 0), **over):
    from elevation_mapping_cupy_amd import _lib
    M = m.cell_n - 2
    res, origin = _frame(m)
    src = _lib.EmapGridLayerEx(source[0], source[1], 0, source[2])
    vals = dict(kernel_size=3, planarity_opening_filter=0, min_number_points_per_label=4, connectivity=4, use_only_above_for_upper_bound=0, reserved=0,
                center_z=float(m.center[2]), reserved_f=0.0, resolution=res, origin_x=origin[0], origin_y=origin[1], plane_patch_error_threshold=0.02,
                cos_local_plane_inclination=0.8, cos_plane_inclination=0.85, global_plane_fit_distance_error_threshold=0.025, cos_global_plane_fit_angle=0.9)
    vals.update(over)
    P = _lib.EmapPlaneParams(**vals)
    labels, normals = np.full(M * M, POISON, np.int32), np.full(3 * M * M, 0x5A5A5A5A, np.uint32)
    rec = np.full(max(capacity, 1) * 64 + 64, 0x5A, np.uint8)
    n_labels, n_planes = ct.c_int32(-7), ct.c_int64(-7)
    rc = m._lib.emap_plane_segmentation(m._ctx, None if "source" in null else ct.byref(src), None if "params" in null else ct.byref(P),
                                        None if "labels" in null else labels.ctypes.data_as(ct.POINTER(ct.c_int32)),
                                        normals.ctypes.data_as(ct.POINTER(ct.c_float)), None if "planes" in null else rec.ctypes.data_as(ct.POINTER(_lib.EmapPlaneRecord)),
                                        capacity, None if "n_labels" in null else ct.byref(n_labels), None if "n_planes" in null else ct.byref(n_planes))
    untouched = (labels == POISON).all() and (normals == 0x5A5A5A5A).all() and (rec == 0x5A).all() and n_labels.value == -7 and n_planes.value == -7
    return (rc, untouched) if rc and n_planes.value == -7 else (rc, n_planes.value, rec)


def test_every_refusal_leaves_the_outputs_and_the_map_as_they_were():
    m = gc.start(34)
    try:
        _write(m, pc.scenes(32)["flat"][0])
        state = lambda: m.elevation_map.tobytes() + m.normal_map.tobytes()      # noqa: E731
        s0 = state()
        nan, inf = float("nan"), float("inf")
        cases = {
            "null source": dict(null=("source",)), "null params": dict(null=("params",)), "null labels": dict(null=("labels",)), "null planes": dict(null=("planes",)),
            "null n_labels": dict(null=("n_labels",)), "null n_planes": dict(null=("n_planes",)),
            "kernel 4": dict(kernel_size=4), "kernel 1": dict(kernel_size=1), "kernel 9": dict(kernel_size=9), "connectivity 6": dict(connectivity=6),
            "opening -1": dict(planarity_opening_filter=-1), "opening 9": dict(planarity_opening_filter=9), "negative min points": dict(min_number_points_per_label=-1),
            "threshold 0": dict(plane_patch_error_threshold=0.0), "threshold NaN": dict(plane_patch_error_threshold=nan), "distance -1": dict(global_plane_fit_distance_error_threshold=-1.0),
            "resolution 0": dict(resolution=0.0), "resolution inf": dict(resolution=inf), "cosine 1.5": dict(cos_plane_inclination=1.5), "cosine NaN": dict(cos_local_plane_inclination=nan),
            "angle cosine -2": dict(cos_global_plane_fit_angle=-2.0), "origin NaN": dict(origin_x=nan), "center_z inf": dict(center_z=inf), "negative capacity": dict(capacity=-1),
            "kind 4": dict(source=(4, 0, 0)), "built-in 9": dict(source=(0, 9, 0)), "plugin plane not reserved": dict(source=(3, 0, 0)), "flags on a cell layer": dict(source=(0, 0, 1)),
        }
        for what, kw in cases.items():
            assert _raw(m, **kw) == (-1, True), what
            assert b"emap_plane_segmentation" in m._lib.emap_last_error(m._ctx), what
        assert state() == s0
        rc, n_planes, rec = _raw(m, capacity=0)                                 # too few records: the count comes back, no record is written
        assert rc == -1 and n_planes >= 1 and (rec == 0x5A).all()
        rc, n2, rec = _raw(m, capacity=n_planes + 3)
        assert (rc, n2) == (0, n_planes) and not (rec[:64 * n_planes] == 0x5A).all() and (rec[64 * n_planes:] == 0x5A).all()      # the records' tail keeps its poison
        assert state() == s0
    finally:
        m.close()


def test_a_strip_context_is_refused():
    from elevation_mapping_cupy_amd._lib import EmapError
    m = gc.start(34, strip=(0, 17, 0))
    try:
        assert _raw(m) == (-1, True) and b"single-strip" in m._lib.emap_last_error(m._ctx)
        with pytest.raises(EmapError):
            m.get_plane_segmentation()
    finally:
        m.close()
