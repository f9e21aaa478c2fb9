"""GPU: the point-cloud output on the device (emap_publish_point_cloud / k_cloud_count, k_cloud_scan, k_cloud_write, csrc/emap_cloudout.hip;
ElevationMap.get_point_cloud_message, get_point_cloud, get_normal_arrows).  The yardstick is the whole-map door on the same context and
state, get_grid_map_layers(order="message"), fed to the tests' own NumPy model (tests/_cloud_out_cases.py): uint32 views compared bit
for bit, NaN bits included; n, point_step, row_step and the fields exactly.  The start state is that of tests/_grid_cases.py: the
circular origin is off zero, a shift is pending, the normals lie at an older origin.  No test provokes a fault: every refusal happens
before a launch.  Reference: elevation_mapping_ros.cpp:501-505, :751-809 (grid_map restated, not pinned by a compiled reference)."""
import ctypes as ct

import numpy as np
import pytest

import _cloud_out_cases as cc
import _fixtures as fx
import _grid_cases as gc
import _plug_cases as pc

pytestmark = pytest.mark.gpu
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


def _positions(m):
    from elevation_mapping_cupy_amd.elevation_mapping import grid_cell_positions
    return grid_cell_positions((float(m.center[0]), float(m.center[1])), float(np.float32(m.resolution)), m.cell_n - 2)


def _check(m, layers, point_layer="elevation", basic=None, normal_color=False, route="device", what=""):
    """one get_point_cloud_message call against the model on the yardstick's planes; the buffer's tail keeps its poison"""
    M = m.cell_n - 2
    basic_eff = (["elevation"] if "elevation" in layers else []) if basic is None else list(basic)
    asked = list(layers) + [b for b in basic_eff if b not in layers]
    all_names, planes = m.get_grid_map_layers(asked, order="message", normal_color=normal_color)
    hidden = [n for n in all_names if n not in layers and not (normal_color and n in ("normal_x", "normal_y", "normal_z", "color"))]
    xs, ys = (a.astype(np.float32) for a in _positions(m))
    want_fields, want = cc.model_cloud(planes, all_names, point_layer, [b for b in basic_eff if b in all_names], xs, ys, hidden=hidden)
    n, step = want.shape[0], 4 * len(want_fields)
    buf = np.full(M * M * step + 64, cc.POISON & 0xFF, np.uint8)
    msg = m.get_point_cloud_message(layers, point_layer, basic, frame_id="odom", stamp=2.5, normal_color=normal_color, out=buf[:M * M * step])
    assert m.last_point_cloud_route == route, what
    assert [(f.name, f.offset, f.datatype, f.count) for f in msg.fields] == [(nm, 4 * k, 7, 1) for k, nm in enumerate(want_fields)], what
    assert (msg.width, msg.height, msg.point_step, msg.row_step, msg.is_dense, msg.is_bigendian) == (n, 1, step, n * step, False, False), (what, msg.width, n)
    assert msg.header.frame_id == "odom" and msg.header.stamp == 2.5
    assert msg.data.dtype == np.uint8 and msg.data.size == n * step and (n == 0 or msg.data.ctypes.data == buf.ctypes.data)
    assert (buf[n * step:] == cc.POISON & 0xFF).all(), "%s: written past n * point_step" % what
    got = msg.data.view(np.uint32).reshape(n, len(want_fields))
    bad = got != want.view(np.uint32)
    if bad.any():
        k = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d words differ, first at point %d field %s: %#x vs %#x" % (what, int(bad.sum()), bad.size, k[0], want_fields[k[1]], got[k[0], k[1]], want.view(np.uint32)[k[0], k[1]]))
    return want_fields, want


def _write_case(m, name):
    """a validity pattern or extra case in the published index space, written with set_layer_raw"""
    C = m.cell_n
    valid, h, v = cc.case_state(C - 2, name)
    m.set_layer_raw("elevation", cc.logical_plane(h, C))
    m.set_layer_raw("variance", cc.logical_plane(v, C))
    m.set_layer_raw("is_valid", cc.logical_plane(valid, C))
    return valid, h


# ---- 1. every validity pattern at every size -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", cc.SIZES)
def test_every_validity_pattern(C):
    """C = 355: M = 353, 4236 mask words -- past the 4096 words the scan's one workgroup takes in a single trip (cc.SIZES)"""
    m = gc.start(C)
    try:
        M = C - 2
        for name in cc.all_cases(M):
            valid, h = _write_case(m, name)
            basic = ["elevation", "variance"] if name == "tested layer NaN" else None
            fields, want = _check(m, ["elevation", "variance"], basic=basic, what="%s at %d" % (name, C))
            n = want.shape[0]
            assert fields == ["x", "y", "z", "variance"]
            assert (n == 0) == (name == "none valid") and (n == M * M) == (name == "all valid"), (name, n)      # the sentinel condition, on the device's own planes
            if name in cc.validity_patterns(M):
                assert n == int(valid.sum()), name
            if name == "other field NaN":
                assert (want[:, 3].view(np.uint32) == 0x7FC12345).any()
            if name in ("+inf elevation", "tested layer NaN"):
                assert 0 < n < int(valid.sum())
            _check(m, ["elevation"], what="%s at %d, elevation alone" % (name, C))
    finally:
        m.close()


# ---- 2. layer lists on the start state -------------------------------------------------------------------------------------------------------
LISTS = {
    "hot": ("variance", "elevation"), "cold": ("upper_bound", "time", "is_upper_bound"), "both": ("time", "traversability", "variance", "elevation"),
    "semantic": ("elevation", "rgb", "s1"), "point layer not first": ("s0", "variance", "elevation", "rgb", "upper_bound"),
}


@pytest.mark.parametrize("C", (34, 67))
def test_layer_lists_on_the_start_state(C):
    m = _shared(C)
    for name, layers in LISTS.items():
        point = "elevation" if "elevation" in layers else "upper_bound"
        fields, want = _check(m, list(layers) + ["ghost"], point_layer=point, what=name)      # a name that does not exist is dropped
        assert 0 < want.shape[0] < (C - 2) ** 2, name
    for only_above in (True, False):
        m.param.use_only_above_for_upper_bound = only_above
        try:
            _check(m, ["upper_bound", "elevation"], what="only_above %s" % only_above)
        finally:
            m.param.use_only_above_for_upper_bound = False
    fields, _ = _check(m, ["elevation", "variance"], normal_color=True, what="normal colour")
    assert fields == ["x", "y", "z", "variance", "normal_x", "normal_y", "normal_z", "rgb"]
    fields, want = _check(m, ["elevation", "variance"], basic=["elevation", "traversability"], what="a hidden basic layer")
    assert fields == ["x", "y", "z", "variance"]
    _, plain = _check(m, ["elevation", "variance"], what="plain")
    assert 0 < want.shape[0] <= plain.shape[0]                                  # (cells whose traversability is NaN are skipped; the patterns above pin a tested layer that does skip)
    fields, _ = _check(m, ["variance", "elevation"], basic=[], what="no basic layer")
    assert fields == ["variance", "x", "y", "z"]
    names, arr = m.get_point_cloud(["elevation", "rgb"])
    assert names == ["x", "y", "z", "rgb"] and arr.dtype == np.float32 and arr.shape == (plain.shape[0], 4) and cc.same_words(arr[:, :3], plain[:, :3])
    with pytest.raises(ValueError):
        m.get_point_cloud_message(["variance"], "elevation")
    with pytest.raises(ValueError):
        m.get_point_cloud_message(["variance", "ghost"], "ghost")


@pytest.mark.parametrize("C", (34, 67))
def test_a_device_plugin_and_a_host_route_plugin(C, tmp_path):
    cfg = tmp_path / "plugins.yaml"
    cfg.write_text(pc.yaml_of([pc.CORE[0], pc.CORE[2]]))                       # min_filter (a device op), inpainting with method "telea" (the host route)
    m = gc.start(C, plugin_file=cfg)
    try:
        assert m.plugin_manager.layer_names == ["min_filter", "inpaint"]
        fields, dev = _check(m, ["elevation", "min_filter", "rgb"], what="a device plugin")
        assert fields == ["x", "y", "z", "min_filter", "rgb"] and m.last_plugin_route == {"min_filter": "device"}
        _check(m, ["min_filter", "elevation"], point_layer="min_filter", basic=["min_filter"], what="a plugin plane as the point layer")
        fields, host = _check(m, ["elevation", "min_filter", "inpaint"], route="host", what="a host-route plugin")      # the whole call takes the host route
        assert m.last_plugin_route == {"min_filter": "device", "inpaint": "host"}
        assert cc.same_words(host[:, :4], dev[:, :4])
    finally:
        m.close()


PUB = [pc._entry("smooth_filter", "pub_%d%d" % (f, h), fill_nan=f, height=h, input_layer_name="elevation") for f in (0, 1) for h in (0, 1)]      # fill_nan x is_height_layer
PUB_CASES = {      # layers, point layer, basic layers
    "plain and ADD_Z, no cell layer": (["pub_01", "pub_00"], "pub_01", ["pub_01"]),
    "FILL_NAN where no half is asked for": (["pub_11", "pub_10"], "pub_11", ["pub_11"]),
    "FILL_NAN beside the hot half": (["elevation", "pub_10", "pub_11"], "elevation", None),
    "FILL_NAN beside the cold half only": (["upper_bound", "time", "pub_10"], "upper_bound", ["upper_bound", "pub_10"]),
}


@pytest.mark.parametrize("C", (10, 67))
def test_plugin_planes_with_every_flag_beside_each_half_of_a_cell(C, tmp_path):
    """the branches of the plugin-plane entry, tested and emitted: no flag, ADD_Z, and FILL_NAN taking is_valid from the hot half it adds,
    from a hot half that is loaded anyway, and from cold.w when only the cold half is"""
    cfg = tmp_path / "plugins.yaml"
    cfg.write_text(pc.yaml_of(PUB))
    m = gc.start(C, plugin_file=cfg)
    try:
        counts = {}
        for what, (layers, point, basic) in PUB_CASES.items():
            _, want = _check(m, layers, point_layer=point, basic=basic, what=what)
            assert set(m.last_plugin_route.values()) == {"device"}, what
            counts[what] = want.shape[0]
        assert 0 < counts["FILL_NAN where no half is asked for"] < counts["plain and ADD_Z, no cell layer"]      # the fill does skip cells
    finally:
        m.close()


# ---- 3. arrows ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (10, 35, 67))
def test_the_normal_arrows(C, monkeypatch):
    m = gc.start(C)
    try:
        M = C - 2
        nrm = (gc.normal_pattern(C) * np.float32(0.2)).astype(np.float32)      # lengths on both sides of 0.1
        nrm[:, 2, 3] = 0.0; nrm[2, 2, 3] = np.float32(0.1) - np.float32(1e-8)  # just below
        nrm[:, 3, 2] = 0.0; nrm[2, 3, 2] = np.float32(0.1) + np.float32(1e-8)  # just above
        nrm[0, 4, 4] = np.nan                                                   # a NaN normal is not skipped
        m.normal_map = nrm
        valid = np.ones((M, M), bool); valid[::3, 1::2] = False
        m.set_layer_raw("is_valid", cc.logical_plane(valid, C))
        m.set_layer_raw("elevation", cc.logical_plane(cc.heights(M), C))
        names, planes = m.get_grid_map_layers(["elevation"], order="message", normal_color=True)
        assert names[:4] == ["elevation", "normal_x", "normal_y", "normal_z"]
        xs, ys = _positions(m)
        for scale, min_norm in ((0.1, 0.1), (0.25, 0.05), (0.1, 0.0)):
            ids, st, en = cc.model_arrows(planes[0], planes[1], planes[2], planes[3], xs, ys, scale, min_norm)
            a = m.get_normal_arrows(scale, min_norm)
            assert m.last_point_cloud_route == "device"
            assert a.ids.dtype == np.int32 and (a.ids == ids).all() and cc.same_words(a.starts, st) and cc.same_words(a.ends, en), (scale, min_norm)
            assert 0 < ids.size < M * M
        kept = set(ids.tolist())
        nan_cells = np.argwhere(np.isnan(planes[1]) & np.isfinite(planes[0]))
        assert len(nan_cells) and all(int(j * M + i) in kept for j, i in nan_cells)
        ids, st, en = cc.model_arrows(planes[0], planes[1], planes[2], planes[3], xs, ys)
        short = np.isfinite(planes[0]) & (np.sqrt(sum(p.astype(np.float64) ** 2 for p in planes[1:4])) < 0.1)
        assert short.any() and ids.size == int((np.isfinite(planes[0]) & ~short).sum())
        monkeypatch.setenv("EMAP_CLOUD_RESIDENT", "0")
        b = m.get_normal_arrows()
        assert m.last_point_cloud_route == "host" and (b.ids == ids).all() and cc.same_words(b.starts, st) and cc.same_words(b.ends, en)
        with pytest.raises(ValueError):
            m.get_normal_arrows(min_norm=float("nan"))
    finally:
        m.close()


# ---- 4. behaviour -------------------------------------------------------------------------------------------------------------------------------
def test_an_out_that_is_too_small_raises_and_is_left_untouched(monkeypatch):
    m = _shared(67)
    msg = m.get_point_cloud_message(["elevation", "rgb"])
    n = msg.width
    assert n > 4 and msg.data.size == n * 16
    for route in ("device", "host"):
        if route == "host":
            monkeypatch.setenv("EMAP_CLOUD_RESIDENT", "0")
        small = np.full((n - 1) * 16 + 7, 0x5A, np.uint8)
        with pytest.raises(ValueError):
            m.get_point_cloud_message(["elevation", "rgb"], out=small)
        assert (small == 0x5A).all() and m.last_point_cloud_route == route
        exact = np.zeros(n * 4, np.float32)                                     # a float32 buffer of exactly the size
        again = m.get_point_cloud_message(["elevation", "rgb"], out=exact)
        assert again.width == n and (again.data == msg.data).all() and again.data.ctypes.data == exact.ctypes.data
    with pytest.raises(ValueError):
        m.get_point_cloud_message(["elevation"], out=np.zeros(8, np.float64))


def test_two_calls_around_a_frame_without_a_sync_and_two_runs_agree():
    C = 67
    m = gc.start(C)
    try:
        layers = ["elevation", "variance", "time", "rgb"]
        R, t = fx.POSES["identity"]
        a1 = m.get_point_cloud_message(layers).data.copy()
        a2 = m.get_point_cloud_message(layers).data.copy()
        assert a1.tobytes() == a2.tobytes()                                     # two runs on one state agree byte for byte
        _, before = _check(m, layers, what="before")
        m.input_pointcloud(gc.semantic_frame(C, 3000, 7), gc.CHANNELS, R, t.copy() + m.center, 0.0, 0.0)
        b = m.get_point_cloud_message(layers).data.copy()                       # no sync in between
        _, after = _check(m, layers, what="after")
        assert a1.tobytes() == before.tobytes() and b.tobytes() == after.tobytes() and a1.tobytes() != b.tobytes()
    finally:
        m.close()


def test_the_host_route_gives_the_same_bits(monkeypatch):
    m = _shared(67)
    layers = ["variance", "elevation", "rgb", "traversability"]
    dev = m.get_point_cloud_message(layers, normal_color=True)
    assert m.last_point_cloud_route == "device"
    monkeypatch.setenv("EMAP_CLOUD_RESIDENT", "0")
    host = m.get_point_cloud_message(layers, normal_color=True)
    assert m.last_point_cloud_route == "host"
    assert [f.name for f in dev.fields] == [f.name for f in host.fields] and dev.width == host.width > 0 and dev.data.tobytes() == host.data.tobytes()
    _check(m, layers, normal_color=True, route="host", what="host route against the model")


def test_the_buffers_grow_and_are_kept():
    """a larger list after a smaller one, and back: the context's buffers grew once and still answer right"""
    m = _shared(67)
    for layers in (["elevation"], ["elevation", "variance", "time", "rgb", "s0", "s1"], ["elevation"]):
        _check(m, layers, what="growth")


# ---- 5. refusals: before anything is uploaded, launched or copied ------------------------------------------------------------------------
def _raw(m, entries, out, capacity=None, call_flags=0, normal_min=0.1, n_fields=None, null=()):
    from elevation_mapping_cupy_amd import _lib
    table = (_lib.EmapCloudField * max(1, len(entries)))()
    for g, (kind, index, flags, cf) in zip(table, entries):
        g.kind, g.index, g.flags, g.cloud_flags = kind, index, flags, cf
    M = m.cell_n - 2
    pos = np.zeros(M, np.float32)
    n, step = ct.c_int64(-7), ct.c_int32(-7)
    rc = m._lib.emap_publish_point_cloud(m._ctx, None if "fields" in null else table, len(entries) if n_fields is None else n_fields, ct.c_float(0.5), 0,
                                         None if "xs" in null else _lib.f32p(pos), None if "ys" in null else _lib.f32p(pos), ct.c_double(normal_min), call_flags,
                                         None if "out" in null else out.ctypes.data_as(ct.POINTER(ct.c_uint8)), out.size // 64 if capacity is None else capacity,
                                         None if "n" in null else ct.byref(n), None if "step" in null else ct.byref(step))
    return rc, n.value, step.value


def test_every_refusal_leaves_the_buffer_and_the_map_as_they_were():
    C = 34
    m = gc.start(C)
    try:
        M = C - 2
        n_sem = len(m.semantic_map.layer_names)
        state = lambda: m.elevation_map.tobytes() + m.normal_map.tobytes() + m.semantic_map.semantic_map.tobytes()      # noqa: E731
        s0 = state()
        P, T, H = 1, 2, 4
        good = [(0, 0, 0, P | T), (1, 0, 0, 0)]
        out = np.full(M * M * 64, 0x5A, np.uint8)
        cases = {
            "null table": dict(null=("fields",)), "null x": dict(null=("xs",)), "null y": dict(null=("ys",)), "null out": dict(null=("out",)),
            "null n_points": dict(null=("n",)), "null point_step": dict(null=("step",)),
            "no entry": dict(entries=[]), "negative entry count": dict(n_fields=-1), "33 entries": dict(entries=[good[0]] + [(1, 0, 0, 0)] * 32),
            "kind 4": dict(entries=[good[0], (4, 0, 0, 0)]), "kind -1": dict(entries=[good[0], (-1, 0, 0, 0)]),
            "built-in 9": dict(entries=[good[0], (0, 9, 0, 0)]), "built-in -1": dict(entries=[good[0], (0, -1, 0, 0)]),
            "semantic beyond": dict(entries=[good[0], (1, n_sem, 0, 0)]), "semantic -1": dict(entries=[good[0], (1, -1, 0, 0)]),
            "plugin plane not reserved": dict(entries=[good[0], (3, 0, 0, 0)]), "flags on a cell layer": dict(entries=[good[0], (0, 1, 1, 0)]),
            "no POINT": dict(entries=[(0, 0, 0, T), good[1]]), "two POINT": dict(entries=[good[0], (0, 4, 0, P)]),
            "HIDDEN without TEST": dict(entries=[good[0], (0, 1, 0, H)]), "HIDDEN POINT": dict(entries=[(0, 0, 0, P | T | H), good[1]]),
            "unknown cloud flag": dict(entries=[good[0], (0, 1, 0, 32)]), "unknown call flag": dict(call_flags=1),
            "negative capacity": dict(capacity=-1),
            "NaN normal_min": dict(call_flags=8, normal_min=float("nan")), "infinite normal_min": dict(call_flags=8, normal_min=float("inf")),
        }
        for what, kw in cases.items():
            kw = dict(dict(entries=good), **kw)
            assert _raw(m, out=out, **kw) == (-1, -7, -7), what
            assert b"emap_publish_point_cloud" in m._lib.emap_last_error(m._ctx), what
            assert (out == 0x5A).all(), what
        assert state() == s0
        rc, n, step = _raw(m, good, out, capacity=3)                            # more points than the capacity: the count comes back, nothing is written
        assert rc == -1 and n > 3 and step == 16 and (out == 0x5A).all()
        rc, n2, step = _raw(m, good, out, normal_min=float("nan"))              # (a NaN bound without NORMAL_MIN is not read) the good call goes through
        assert (rc, n2, step) == (0, n, 16) and not (out[:n * 16] == 0x5A).all() and (out[n * 16:] == 0x5A).all()
        assert state() == s0
    finally:
        m.close()


def test_a_strip_context_is_refused():
    from elevation_mapping_cupy_amd._lib import EmapError
    C = 34
    m = gc.start(C, strip=(0, 17, 0))
    try:
        out = np.full(64 * 32 * 32, 0x5A, np.uint8)
        assert _raw(m, [(0, 0, 0, 1)], out) == (-1, -7, -7)
        assert b"single-strip" in m._lib.emap_last_error(m._ctx)
        assert (out == 0x5A).all()
        with pytest.raises(EmapError):
            m.get_point_cloud_message()
        with pytest.raises(EmapError):
            m.get_normal_arrows()
    finally:
        m.close()
