"""GPU: the submap service on the device (emap_publish_grid_windows / k_grid_windows, csrc/emap_submap.hip; ElevationMap.get_submap_layers,
get_submap_messages).  The yardstick is the whole-map door on the same context and state: get_grid_map_layers(order="rows"), sliced
[k, i0:i0+ni, j0:j0+nj] -- for "message" order the slice's transpose stored contiguous.  Bit for bit on uint32 views, NaN with NaN,
every layer; the device FeaturesPca included (its reductions are order-fixed: two runs on one state agree).  The start state is that of
tests/_grid_cases.py: the circular origin is off zero, a shift is pending, the normals lie at an older origin.  No test provokes a
fault: every refusal happens before a launch.  Reference: elevation_mapping_ros.cpp:507-553."""
import ctypes as ct
import os

import numpy as np
import pytest

import _fixtures as fx
import _grid_cases as gc
import _plug_cases as pc
import _submap_cases as sc

pytestmark = pytest.mark.gpu
_maps = {}
ALL_LAYERS = gc.BUILTINS[:6] + ("s0", "s1", "c0", "rgb")
LISTS = {"hot": gc.HOT_ONLY, "cold": gc.COLD_ONLY, "both": gc.BOTH_HALVES, "semantic": gc.SEMANTIC, "mixed": gc.MIXED}


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


def _poisoned(total, tail=16):
    return np.full(total + tail, gc.POISON, np.uint32).view(np.float32)


def _check(m, windows, names, order, normal_color=False, what=""):
    """one get_submap_layers call against the slices of the yardstick; the buffer's tail keeps its poison"""
    want_names, full = m.get_grid_map_layers(list(names), order="rows", normal_color=normal_color)
    total = sc.packed_size(windows, len(want_names))
    buf = _poisoned(total)
    got_names, views = m.get_submap_layers(windows, list(names), out=buf[:total], order=order, normal_color=normal_color)
    assert got_names == want_names and len(views) == len(windows) and m.last_submap_route == "device", what
    assert (buf[total:].view(np.uint32) == gc.POISON).all(), "%s: written past the end" % what
    want = sc.pack_slices(full, windows, order)
    ok = gc.same_bits(buf[:total], want)
    if not ok.all():
        i = int(np.argwhere(~ok)[0][0])
        raise AssertionError("%s (%s): %d of %d values differ bitwise, first at float %d: %r vs %r" % (what, order, int((~ok).sum()), ok.size, i, buf[i], want[i]))
    for v, (i0, j0, ni, nj) in zip(views, windows):
        assert v.shape == ((len(want_names), ni, nj) if order == "rows" else (len(want_names), nj, ni)) and v.base is not None
        s = full[:, i0:i0 + ni, j0:j0 + nj]
        assert gc.same_bits(v, s if order == "rows" else s.transpose(0, 2, 1)).all(), what
    return got_names, views


# ---- 0. the yardstick can tell a missing flip, a transpose, a shifted window or a missing NaN fill -------------------------------------
@pytest.mark.parametrize("C", gc.SIZES)
def test_the_yardstick_is_not_symmetric_and_mixes_nan_with_finite_cells(C):
    m = _shared(C)
    names, full = m.get_grid_map_layers(list(gc.BUILTINS[:6]) + ["s0", "s1", "c0", "rgb"], order="rows", normal_color=True)
    assert names == list(ALL_LAYERS) + ["normal_x", "normal_y", "normal_z", "color"]
    for n, r in zip(names, full):
        for what, other in (("transpose", r.T), ("row flip", r[::-1]), ("column flip", r[:, ::-1]), ("both flips", r[::-1, ::-1])):
            assert not gc.same_bits(r, other).all(), (n, what)
    e = full[0]
    mixed = [w for w in sc.all_windows(C - 2) if w[2] * w[3] > 1 and np.isnan(e[w[0]:w[0] + w[2], w[1]:w[1] + w[3]]).any()
             and np.isfinite(e[w[0]:w[0] + w[2], w[1]:w[1] + w[3]]).any()]
    assert mixed, "no multi-cell window holds both NaN and finite elevation"


# ---- 1. every window set, every layer kind -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", gc.ORDERS)
@pytest.mark.parametrize("C", gc.SIZES)
def test_every_window_set_as_a_batch_of_its_own(C, order):
    """one window (the whole map), the nine of the partition, overlapping and repeated windows, 64 windows, and the shapes that only a
    swapped ni / nj or a tile edge can break -- all ten cell and semantic layers plus the normals and their colour"""
    m = _shared(C)
    for name, ws in sc.window_sets(C - 2).items():
        _check(m, ws, ALL_LAYERS, order, normal_color=True, what="%s at %d" % (name, C))


@pytest.mark.parametrize("order", gc.ORDERS)
@pytest.mark.parametrize("C", gc.SIZES)
def test_each_built_in_layer_alone(C, order):
    m = _shared(C)
    ws = sc.all_windows(C - 2)
    for n in gc.BUILTINS[:6]:
        _check(m, ws, [n], order, what=n)
    for n in gc.BUILTINS[6:]:                                                  # the normal planes are layers of a list only with the switch: the raw table
        _raw_layer(m, ws, (0, gc.BUILTINS.index(n)), n, order)


def _raw_layer(m, windows, entry, yard_name, order):
    out = np.zeros((m.cell_n - 2, m.cell_n - 2), np.float32)
    m.get_map_with_name_ref(yard_name, out)
    total = sc.packed_size(windows, 1)
    buf = _poisoned(total)
    assert _raw(m, [entry + (0, 0)], windows, buf[:total], order=gc.ORDERS.index(order)) == 0
    assert gc.same_bits(buf[:total], sc.pack_slices(out[None], windows, order)).all(), yard_name
    assert (buf[total:].view(np.uint32) == gc.POISON).all()


@pytest.mark.parametrize("only_above", [False, True])
@pytest.mark.parametrize("names", sorted(LISTS))
@pytest.mark.parametrize("order", gc.ORDERS)
@pytest.mark.parametrize("C", gc.SIZES)
def test_lists_that_need_one_half_of_a_cell_or_both_and_semantic_layers(C, order, names, only_above):
    m = _shared(C)
    m.param.use_only_above_for_upper_bound = only_above
    try:
        _check(m, sc.all_windows(C - 2), LISTS[names] + ("ghost",), order, what=names)      # a name that does not exist is dropped
    finally:
        m.param.use_only_above_for_upper_bound = False


@pytest.mark.parametrize("order", gc.ORDERS)
@pytest.mark.parametrize("C", gc.SIZES)
def test_the_normal_colour_alone_and_with_the_normals(C, order):
    m = gc.start(C)
    try:
        m.normal_map = gc.normal_pattern(C)
        ws = sc.all_windows(C - 2)
        nref = []
        for n in ("normal_x", "normal_y", "normal_z"):
            nref.append(np.zeros((C - 2, C - 2), np.float32))
            m.get_map_with_name_ref(n, nref[-1])
        want = gc.normal_color(*nref)
        if C >= 34:
            assert len(np.unique(want.view(np.uint32))) > 50
        total = sc.packed_size(ws, 1)
        buf = _poisoned(total)
        assert _raw(m, [(2, 0, 0, 0)], ws, buf[:total], order=gc.ORDERS.index(order)) == 0
        assert gc.same_bits(buf[:total], sc.pack_slices(want[None], ws, order)).all()
        names, _ = _check(m, ws, ["elevation", "normal_y"], order, normal_color=True, what="colour with the normals")
        assert names == ["elevation", "normal_x", "normal_y", "normal_z", "color"]
        names, _ = m.get_submap_layers(ws, ["normal_x", "color", "elevation"], order=order)      # without the switch neither exists
        assert names == ["elevation"]
    finally:
        m.close()


# ---- 2. plugin layers: once per call, device planes read by the window launch, host planes sliced on the host --------------------------
@pytest.mark.parametrize("order", gc.ORDERS)
@pytest.mark.parametrize("C", gc.SIZES)
def test_a_device_plugin_and_a_host_route_plugin_in_one_list(C, order, tmp_path):
    cfg = tmp_path / "plugins.yaml"
    cfg.write_text(pc.yaml_of([pc.CORE[0], pc.CORE[2]]))                       # min_filter (a device op), inpainting with method "telea" (the host route)
    m = gc.start(C, plugin_file=cfg)
    try:
        assert m.plugin_manager.layer_names == ["min_filter", "inpaint"]
        layers = ["elevation", "inpaint", "min_filter", "rgb", "is_valid"]      # is_valid: a plane of the map that is not published
        names, views = _check(m, sc.all_windows(C - 2), layers, order, what="plugins")
        assert names == ["elevation", "inpaint", "min_filter", "rgb"]
        assert m.last_plugin_route == {"inpaint": "host", "min_filter": "device"}
        whole = views[0]                                                        # the first window of the batch is the whole map
        assert np.isfinite(whole[2]).sum() > np.isfinite(whole[0]).sum()       # the plugin did fill cells
        _check(m, sc.window_sets(C - 2)["partition"], ["min_filter"], order, what="a device plugin alone")      # FILL_NAN off, ADD_Z on, no cell layer
        assert m.last_plugin_route == {"min_filter": "device"}
    finally:
        m.close()


PUB = [pc._entry("smooth_filter", "pub_%d%d" % (f, h), fill_nan=f, height=h, input_layer_name="elevation") for f in (0, 1) for h in (0, 1)]      # fill_nan x is_height_layer
PUB_LISTS = {"plain and ADD_Z, no cell layer": ["pub_00", "pub_01"], "FILL_NAN where no half is asked for": ["pub_10", "pub_11"],
             "FILL_NAN beside the hot half": ["elevation", "pub_10", "pub_11"], "FILL_NAN beside the cold half only": ["time", "pub_10", "upper_bound", "pub_11"]}


@pytest.mark.parametrize("order", gc.ORDERS)
@pytest.mark.parametrize("C", (10, 67))
def test_plugin_planes_with_every_flag_beside_each_half_of_a_cell(C, order, tmp_path):
    """the branches of the plugin-plane entry: no flag, ADD_Z, and FILL_NAN taking is_valid from the hot half it adds, from a hot half
    that is loaded anyway, and from cold.w when only the cold half is"""
    cfg = tmp_path / "plugins.yaml"
    cfg.write_text(pc.yaml_of(PUB))
    m = gc.start(C, plugin_file=cfg)
    try:
        for what, layers in PUB_LISTS.items():
            names, views = _check(m, sc.all_windows(C - 2), layers, order, what=what)
            assert names == layers and set(m.last_plugin_route.values()) == {"device"}, what
            if "pub_10" in names:
                whole = views[0][names.index("pub_10")]                         # the first window of the batch is the whole map
                assert np.isnan(whole).any() and np.isfinite(whole).any(), what
    finally:
        m.close()


def test_the_plugins_run_once_per_call_not_once_per_window(tmp_path):
    C = 34
    cfg = tmp_path / "plugins.yaml"
    cfg.write_text(pc.yaml_of([pc.CORE[0], pc.CORE[2]]))
    m = gc.start(C, plugin_file=cfg)
    try:
        calls = []
        pm = m.plugin_manager
        run_plan, host_step = pm.run_plan, m._plugin_host_step
        pm.run_plan = lambda *a, **k: (calls.append("plan"), run_plan(*a, **k))[1]
        m._plugin_host_step = lambda n: (calls.append(n), host_step(n))[1]
        m.get_submap_layers(sc.window_sets(C - 2)["partition"], ["min_filter", "inpaint"])
        assert calls == ["plan", "inpaint"]
    finally:
        m.close()


def test_features_pca_on_the_device_agrees_with_itself(tmp_path):
    C = 34
    cfg = tmp_path / "plugins.yaml"
    cfg.write_text(pc.yaml_of([pc._entry("features_pca", "pca", process_layer_names=["^s0$", "^s1$", "^c0$"])]))
    m = gc.start(C, plugin_file=cfg)
    try:
        for order in gc.ORDERS:
            _check(m, sc.window_sets(C - 2)["partition"], ["pca", "elevation"], order, what="pca")
            assert m.last_plugin_route == {"pca": "device"}
    finally:
        m.close()


# ---- 3. the messages ------------------------------------------------------------------------------------------------------------------------
def test_the_messages_of_a_batch_with_a_failed_request_beside_good_ones():
    from elevation_mapping_cupy_amd.elevation_mapping import submap_geometry
    C = 67
    m = _shared(C)
    M, res = C - 2, float(np.float32(m.resolution))
    cx, cy = float(m.center[0]), float(m.center[1])
    assert cx != 0 and cy != 0
    half = M * res / 2
    requests = [((cx + 7.3 * res, cy - 3.6 * res), (9.2 * res, 20.6 * res)),   # interior, ni != nj; every corner lies strictly inside a cell
                ((cx + half + 3.3 * res, cy), (2.2 * res, 2.2 * res)),         # its centre lies outside the map
                ((cx + half - 1.4 * res, cy - half + 2.6 * res), (8.4 * res, 8.4 * res))]      # clipped by a corner
    layers = ["elevation", "ghost", "traversability", "rgb"]
    answers = m.get_submap_messages(requests, layers, frame_id="odom", stamp=12.5)
    assert [ok for _, ok in answers] == [True, False, True]
    _, full = m.get_grid_map_layers(layers, order="rows")
    bad = answers[1][0]
    assert bad.layers == [] and bad.data == [] and bad.index_in_submap is None and bad.header.frame_id == "odom"
    first = None
    for (msg, ok), (p, ln) in zip(answers, requests):
        if not ok:
            continue
        i0, j0, ni, nj, sub_pos, sub_len, inside = submap_geometry((cx, cy), M * res, res, M, p, ln)
        assert msg.layers == ["elevation", "traversability", "rgb"] and msg.basic_layers == ["elevation"]
        assert msg.header is msg.info.header and msg.header.frame_id == "odom" and msg.header.stamp == 12.5
        assert msg.info.resolution == m.resolution and (msg.info.length_x, msg.info.length_y) == tuple(sub_len) == (ni * res, nj * res)
        q, o = msg.info.pose.position, msg.info.pose.orientation
        assert (q.x, q.y, q.z) == (sub_pos[0], sub_pos[1], 0.0) and (o.x, o.y, o.z, o.w) == (0.0, 0.0, 0.0, 1.0)
        assert msg.outer_start_index == 0 and msg.inner_start_index == 0 and msg.index_in_submap == tuple(inside)
        for k, d in enumerate(msg.data):
            assert [(x.label, x.size, x.stride) for x in d.layout.dim] == [("column_index", nj, ni * nj), ("row_index", ni, ni)] and d.layout.data_offset == 0
            assert d.data.dtype == np.float32 and d.data.shape == (ni * nj,) and d.data.flags["C_CONTIGUOUS"]
            first = d.data.ctypes.data if first is None else first
            want = full[k, i0:i0 + ni, j0:j0 + nj]
            i, j = inside                                                       # the requested cell through the layout's strides
            assert gc.same_bits(d.data[j * d.layout.dim[1].stride + i], want[i, j]).all()
            assert gc.same_bits(d.data.reshape(nj, ni), want.T).all()
    good = [a[0] for a in answers if a[1]]
    sizes = [len(g.layers) * g.data[0].data.size for g in good]
    assert good[1].data[0].data.ctypes.data == first + 4 * sizes[0]             # ONE buffer: the second window starts where the first ends
    assert good[0].info.length_x != good[0].info.length_y                       # ni != nj
    w1 = submap_geometry((cx, cy), M * res, res, M, *requests[2])
    assert w1[0] == 0 and w1[1] + w1[3] == M                                    # the corner request was clipped
    one, ok = m.get_submap_message(requests[0][0], requests[0][1], layers)
    assert ok and gc.same_bits(one.data[0].data, good[0].data[0].data).all()
    every, ok = m.get_submap_message(requests[0][0], requests[0][1])            # no layer list: every layer the map publishes
    assert ok and every.layers == list(ALL_LAYERS) and every.basic_layers == ["elevation"]
    none, ok = m.get_submap_message(*requests[1])
    assert not ok and none.layers == []


def test_two_calls_around_a_frame_without_a_sync():
    C = 67
    m = gc.start(C)
    try:
        layers = ["elevation", "variance", "time", "rgb"]
        ws = sc.window_sets(C - 2)["partition"]
        R, t = fx.POSES["identity"]
        _, before = m.get_grid_map_layers(layers, order="rows")
        _, a = m.get_submap_layers(ws, layers, order="message")
        m.input_pointcloud(gc.semantic_frame(C, 3000, 7), gc.CHANNELS, R, t.copy() + m.center, 0.0, 0.0)
        _, b = m.get_submap_layers(ws, layers, order="message")
        _, after = m.get_grid_map_layers(layers, order="rows")
        for k, n in enumerate(layers):
            assert not gc.same_bits(before[k], after[k]).all(), n
        for va, vb, (i0, j0, ni, nj) in zip(a, b, ws):
            assert gc.same_bits(va, before[:, i0:i0 + ni, j0:j0 + nj].transpose(0, 2, 1)).all()
            assert gc.same_bits(vb, after[:, i0:i0 + ni, j0:j0 + nj].transpose(0, 2, 1)).all()
    finally:
        m.close()


@pytest.mark.parametrize("order", gc.ORDERS)
def test_the_host_route_gives_the_same_bits(order, tmp_path, monkeypatch):
    C = 67
    cfg = tmp_path / "plugins.yaml"
    cfg.write_text(pc.yaml_of([pc.CORE[0], pc.CORE[2]]))
    m = gc.start(C, plugin_file=cfg)
    try:
        ws = sc.all_windows(C - 2)
        layers = ["elevation", "inpaint", "min_filter", "rgb", "traversability"]
        names, dev = m.get_submap_layers(ws, layers, order=order, normal_color=True)
        assert m.last_submap_route == "device"
        monkeypatch.setenv("EMAP_SUBMAP_RESIDENT", "0")
        names_h, host = m.get_submap_layers(ws, layers, order=order, normal_color=True)
        assert m.last_submap_route == "host" and names_h == names
        for d, h in zip(dev, host):
            assert d.shape == h.shape and gc.same_bits(d, h).all()
        assert gc.same_bits(dev[0].base, host[0].base).all()                    # the packed buffers as a whole
    finally:
        m.close()


# ---- 4. refusals: before anything is uploaded, launched or copied ------------------------------------------------------------------------
def _raw(m, entries, windows, out, order=0, n_layers=None, n_windows=None, host_floats=None, null_table=False, null_windows=False, null_out=False):
    from elevation_mapping_cupy_amd import _lib
    table = (_lib.EmapGridLayerEx * max(1, len(entries)))()
    for g, (kind, index, slot, flags) in zip(table, entries):
        g.kind, g.index, g.slot, g.flags = kind, index, slot, flags
    wt = (_lib.EmapGridWindow * max(1, len(windows)))()
    for g, (i0, j0, ni, nj) in zip(wt, windows):
        g.i0, g.j0, g.ni, g.nj = i0, j0, ni, nj
    return m._lib.emap_publish_grid_windows(m._ctx, None if null_table else table, len(entries) if n_layers is None else n_layers, order, ct.c_float(0.5), 0,
                                            None if null_windows else wt, len(windows) if n_windows is None else n_windows,
                                            None if null_out else _lib.f32p(out), out.size if host_floats is None else host_floats)


def test_every_refusal_leaves_the_buffer_and_the_map_as_they_were():
    C = 34
    m = gc.start(C)
    try:
        M = C - 2
        n_sem = len(m.semantic_map.layer_names)
        state = lambda: m.elevation_map.tobytes() + m.normal_map.tobytes() + m.semantic_map.semantic_map.tobytes()      # noqa: E731
        s0 = state()
        good, wins = [(0, 0, 0, 0), (1, 0, 1, 0)], [(1, 2, 3, 4), (0, 0, 2, 2)]
        out = np.full(2 * (12 + 4), gc.POISON, np.uint32).view(np.float32)
        cases = {
            "null table": dict(null_table=True), "null windows": dict(null_windows=True), "null out": dict(null_out=True),
            "no layer": dict(entries=[]), "negative layer count": dict(n_layers=-1), "33 layers": dict(entries=[(1, 0, 0, 0)] * 33, host_floats=33 * 16),
            "no window": dict(windows=[], host_floats=0), "negative window count": dict(n_windows=-1),
            "65 windows": dict(windows=[(0, 0, 1, 1)] * 65, host_floats=2 * 65),
            "kind 4": dict(entries=[(4, 0, 0, 0)] + good[1:]), "kind -1": dict(entries=[(-1, 0, 0, 0)] + good[1:]),
            "order 2": dict(order=2), "order -1": dict(order=-1),
            "built-in 9": dict(entries=[(0, 9, 0, 0)] + good[1:]), "built-in -1": dict(entries=[good[0], (0, -1, 1, 0)]),
            "semantic beyond": dict(entries=[good[0], (1, n_sem, 1, 0)]), "semantic -1": dict(entries=[good[0], (1, -1, 1, 0)]),
            "plugin plane not reserved": dict(entries=[good[0], (3, 0, 1, 0)]), "flags on a cell layer": dict(entries=[(0, 0, 0, 1), good[1]]),
            "one row past the bottom": dict(windows=[(M - 2, 2, 3, 4), wins[1]]), "one column past the right": dict(windows=[(1, M - 3, 3, 4), wins[1]]),
            "one row before the top": dict(windows=[(-1, 2, 3, 4), wins[1]]), "one column before the left": dict(windows=[(1, -1, 3, 4), wins[1]]),
            "a window beyond int": dict(windows=[(2 ** 31 - 2, 2, 3, 4), wins[1]]),
            "no rows": dict(windows=[(1, 2, 0, 4), wins[1]], host_floats=8), "no columns": dict(windows=[(1, 2, 3, 0), wins[1]], host_floats=8),
            "negative rows": dict(windows=[(1, 2, -3, 4), wins[1]]),
            "too few floats": dict(host_floats=31), "too many floats": dict(host_floats=33), "no floats": dict(host_floats=0),
        }
        for what, kw in cases.items():
            kw = dict(dict(entries=good, windows=wins), **kw)
            assert _raw(m, out=out, **kw) == -1, what
            assert b"emap_publish_grid_windows" in m._lib.emap_last_error(m._ctx) or what == "null ctx", what
            assert (out.view(np.uint32) == gc.POISON).all(), what
        assert state() == s0
        assert _raw(m, good, wins, out) == 0                                    # and the good call does go through afterwards
        assert not (out.view(np.uint32) == gc.POISON).any()
        with pytest.raises(ValueError):
            m.get_submap_layers([(0, 0, M + 1, 1)], ["elevation"])
        with pytest.raises(ValueError):
            m.get_submap_layers([(0, 0, 1, 1)], ["elevation"], order="columns")
        with pytest.raises(ValueError):
            m.get_submap_layers([(0, 0, 2, 2)], ["elevation"], out=np.zeros(5, np.float32))
    finally:
        m.close()


def test_a_strip_context_is_refused():
    from elevation_mapping_cupy_amd._lib import EmapError
    C = 34
    m = gc.start(C, strip=(0, 17, 0))
    try:
        out = np.full(4, gc.POISON, np.uint32).view(np.float32)
        assert _raw(m, [(0, 0, 0, 0)], [(0, 0, 2, 2)], out) == -1
        assert b"single-strip" in m._lib.emap_last_error(m._ctx)
        assert (out.view(np.uint32) == gc.POISON).all()
        with pytest.raises(EmapError):
            m.get_submap_layers([(0, 0, 2, 2)], ["elevation"])
        with pytest.raises(EmapError):
            m.get_submap_messages([((0.0, 0.0), (0.1, 0.1))])
    finally:
        m.close()


@pytest.mark.parametrize("order", gc.ORDERS)
def test_more_than_64_windows_go_in_groups(order):
    """76 windows: two ABI calls, the second group's planes follow the first's in the one packed buffer"""
    C = 67
    m = _shared(C)
    sets = sc.window_sets(C - 2)
    ws = sets["sixty-four"] + sets["overlapping and repeated"] + sets["partition"]
    assert len(ws) == 76
    _check(m, ws, ("elevation", "rgb", "time"), order, what="76 windows")


def test_the_buffers_grow_once_and_are_kept():
    """the second call of a size allocates nothing: a larger batch after a smaller one still answers right (the context's buffers grew)"""
    C = 67
    m = _shared(C)
    for ws in (sc.window_sets(C - 2)["single cells"], sc.window_sets(C - 2)["whole"], sc.window_sets(C - 2)["single cells"]):
        _check(m, ws, ("elevation", "rgb"), "message", what="growth")
