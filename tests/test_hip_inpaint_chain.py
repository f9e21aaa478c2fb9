"""GPU: the Inpainting plugin's method "telea_fronts" as an op of the plugin chain (EMAP_PLUGIN_INPAINT_FRONTS; csrc/emap_inpaint_chain.hip,
the device-side core of csrc/emap_inpaint_fronts.hip, csrc/emap_api_plugchain.hip).  No tolerance anywhere: every comparison is on uint32
views with NaN equal to NaN.  The yardstick is the plugin's HOST route of the same method -- get_map_with_name_ref / PluginManager with
EMAP_PLUGIN_RESIDENT unset -- taken from a TWIN map in the same state (tests/_plug_cases.py, tests/_inpaint_chain_cases.py).  Next to the
published layer (border stripped) the RAW planes are compared: the cells farthest from a known one lie in the border.  Maps of cell_n
10, 34, 67, 100: one partial fronts tile, then 2, 3 and 4 tiles of 30 per axis at the default 16 fronts per launch."""
import os

import numpy as np
import pytest

import _fixtures as fx
import _grid_cases as gc
import _inpaint_chain_cases as ic
import _plug_cases as pc
import _variant_children as vc
from conftest import ROOT

pytestmark = pytest.mark.gpu
_pairs, _refs = {}, {}
CONFIGS = {"ops": ic.ops_config(), "core": ic.CORE_FRONTS}


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """pair(C, config, case) -> (map, twin): built once per module, for the tests that do not change the map"""
    def get(C, cfg, case):
        key = (C, cfg, case)
        if key not in _pairs:
            _pairs[key] = ic.twins(C, CONFIGS[cfg], tmp_path_factory.mktemp("inp") / ("%s_%d.yaml" % (cfg, C)), case)
        return _pairs[key]
    yield get
    for m, t in _pairs.values():
        m.close(); t.close()
    _pairs.clear(); _refs.clear()


def _ref(m, name):
    out = np.zeros((m.cell_n - 2, m.cell_n - 2), np.float32)
    m.get_map_with_name_ref(name, out)
    return out


def _yardstick(pair, C, cfg, case):
    """the twin's host route for every plugin layer of the configuration, once: name -> (published layer, raw plane)"""
    key = (C, cfg, case)
    if key not in _refs:
        twin = pair(*key)[1]
        _refs[key] = {}
        for n in twin.plugin_manager.layer_names:
            pub = _ref(twin, n)
            raw = twin.plugin_manager.host_layer(n).copy()
            pub.setflags(write=False); raw.setflags(write=False)
            _refs[key][n] = (pub, raw)
            assert twin.plugin_manager.plugins[twin.plugin_manager.layer_names.index(n)].fronts_run is not None      # the host route waited
    return _refs[key]


def _check(got, ref, order, what):
    want = ref if order == "rows" else gc.message_plane(ref)
    assert got.shape == want.shape and got.dtype == np.float32, what
    ok = gc.same_bits(got, want)
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s (%s): %d of %d values differ bitwise, first at %s: %r vs %r" % (what, order, int((~ok).sum()), ok.size, i, got[i], want[i]))


def _raw(m, name):
    """the resident plane as the device left it (one download)"""
    assert m.plugin_manager._newer[m.plugin_manager.layer_names.index(name)] == "device", name
    return m.plugin_manager.host_layer(name).copy()


def _frame(m, C, seed):
    R, t = fx.POSES["identity"]
    m.input_pointcloud(gc.semantic_frame(C, 3000, seed), gc.CHANNELS, R, t.copy() + m.center, 0.0, 0.0)


# ---- 1. the op alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ic.HOLED)
@pytest.mark.parametrize("C", ic.SIZES)
def test_the_op_alone_against_the_twin(pair, C, case):
    m = pair(C, "ops", case)[0]
    refs = _yardstick(pair, C, "ops", case)
    for order in pc.ORDERS:
        for n in ic.PUBLISHED:                                         # fill_nan x is_height_layer
            names, got = m.get_grid_map_layers([n], order=order)
            assert names == [n] and m.last_plugin_route == {n: "device"}, n
            _check(got[0], refs[n][0], order, "%s at %d, %s" % (n, C, case))
            _check(_raw(m, n), refs[n][1], "rows", "raw plane of %s at %d, %s" % (n, C, case))
    assert m.plugin_manager.plugins[0].fronts_run is None              # the device route does not wait for the largest front
    pub, raw = refs["inp_00"]
    assert not gc.same_bits(raw, m.get_layer_raw(0)).all()             # the plane is not the elevation
    assert np.isnan(refs["inp_10"][0]).any() and np.isfinite(refs["inp_10"][0]).any() and not np.isnan(pub).any()
    assert not gc.same_bits(refs["inp_01"][0], pub).all() and not gc.same_bits(pub, pub.T).all()


@pytest.mark.parametrize("case", ic.HOLED)
@pytest.mark.parametrize("C", ic.SIZES)
def test_the_plane_does_not_depend_on_the_fronts_per_launch(pair, C, case):
    m = pair(C, "ops", case)[0]
    refs = _yardstick(pair, C, "ops", case)
    for n in ic.STEP_LAYERS:                                           # i0 = 0, 1, 4, 16
        _, got = m.get_grid_map_layers([n])
        assert m.last_plugin_route == {n: "device"}
        _check(got[0], refs[n][0], "rows", "%s at %d, %s" % (n, C, case))
        _check(_raw(m, n), refs[n][1], "rows", "raw plane of %s at %d, %s" % (n, C, case))
        _check(refs[n][1], refs["inp_01"][1], "rows", "the yardstick of %s against that of i0 = 0" % n)


# ---- 2. degenerate states -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ic.DEGENERATE)
@pytest.mark.parametrize("C", ic.SIZES)
def test_degenerate_states_equal_the_host_route(pair, C, case):
    m, t = pair(C, "ops", case)
    refs = _yardstick(pair, C, "ops", case)
    lst = ic.PUBLISHED + ["inp_s4"]
    for order in pc.ORDERS:
        names, got = m.get_grid_map_layers(lst, order=order)           # five inpaint ops in one chain
        assert names == lst and set(m.last_plugin_route.values()) == {"device"}
        for k, n in enumerate(lst):
            _check(got[k], refs[n][0], order, "%s at %d, %s" % (n, C, case))
    for n in lst:
        _check(m.plugin_manager.host_layer(n), refs[n][1], "rows", "raw plane of %s at %d, %s" % (n, C, case))
    raw = refs["inp_00"][1]
    if case == "constant":
        assert np.unique(raw).size == 1 and raw[0, 0] == np.float32(0.25)
    else:                                                              # no valid cell / every cell valid: the elevation as it is
        assert gc.same_bits(raw, t.get_layer_raw(0)).all()
        assert (t.get_layer_raw(2) >= 0.5).all() == (case == "all_valid") and (t.get_layer_raw(2) >= 0.5).any() == (case == "all_valid")


# ---- 3. the geometric bound -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps_layer", ic.STEP_LAYERS)
def test_one_known_cell_in_a_corner_needs_the_last_launch(pair, steps_layer):
    """max d = 66 = rows + cols - 2 at cell_n 34: fronts 65 and 66 (three border cells around the far corner) belong to the last launch of
    ceil(66 / S) alone; the span is 1 here, so a cell left at its input value de-quantises to another float than a filled one"""
    C = 34
    m = pair(C, "ops", "corner")[0]
    refs = _yardstick(pair, C, "ops", "corner")
    _, got = m.get_grid_map_layers([steps_layer])
    _check(got[0], refs[steps_layer][0], "rows", steps_layer)
    raw = _raw(m, steps_layer)
    _check(raw, refs[steps_layer][1], "rows", "raw plane of " + steps_layer)
    assert raw[0, C - 1] != m.get_layer_raw(0)[0, C - 1]               # the far corner was filled (tests/test_inpaint_chain_cases.py: a launch less leaves its input)


# ---- 4. lists -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (34, 67))
def test_two_inpaint_ops_in_one_chain(pair, C):
    m = pair(C, "ops", "block")[0]
    refs = _yardstick(pair, C, "ops", "block")
    for lst in (["inp_s4", "inp_01"], ["inp_10", "inp_s1", "inp_s16"]):
        names, got = m.get_grid_map_layers(lst, order="message")
        assert names == lst and m.last_plugin_route == {n: "device" for n in lst}
        for k, n in enumerate(lst):
            _check(got[k], refs[n][0], "message", n)
            _check(_raw(m, n), refs[n][1], "rows", "raw plane of " + n)


@pytest.mark.parametrize("order", pc.ORDERS)
@pytest.mark.parametrize("C", ic.SIZES)
def test_the_shipped_filter_publisher_with_telea_fronts(pair, C, order):
    """the test that needs the op: before it the inpaint step of this list took its host route"""
    m, t = pair(C, "core", "start")
    names, got = m.get_grid_map_layers(pc.FILTER_PUBLISHER, order=order)
    assert names == pc.FILTER_PUBLISHER
    assert m.last_plugin_route == {"min_filter": "device", "smooth": "device", "inpaint": "device"}
    for k, n in enumerate(names):
        _check(got[k], _ref(t, n), order, n)
    msg = m.get_grid_map_message(pc.FILTER_PUBLISHER)
    assert msg.layers == pc.FILTER_PUBLISHER and m.last_plugin_route["inpaint"] == "device"
    for k, n in enumerate(msg.layers):
        _check(msg.data[k].data.reshape(C - 2, C - 2), _ref(t, n), "message", n)
    assert not gc.same_bits(_ref(t, "inpaint"), _ref(t, "elevation")).all()


def test_two_calls_around_a_frame_without_a_sync(tmp_path):
    C = 67
    m, t = ic.twins(C, ic.CORE_FRONTS, tmp_path / "p.yaml")
    try:
        lst = pc.FILTER_PUBLISHER
        before = {n: _ref(t, n) for n in lst}
        _, a = m.get_grid_map_layers(lst, order="message")
        _frame(m, C, 7); _frame(t, C, 7)
        _, b = m.get_grid_map_layers(lst, order="message")
        after = {n: _ref(t, n) for n in lst}
        assert m.last_plugin_route == {"min_filter": "device", "smooth": "device", "inpaint": "device"}
        for k, n in enumerate(lst):
            _check(a[k], before[n], "message", n + " before"); _check(b[k], after[n], "message", n + " after")
            assert not gc.same_bits(before[n], after[n]).all(), n
    finally:
        m.close(); t.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_planes_the_map_and_the_buffer_as_they_were(tmp_path):
    from elevation_mapping_cupy_amd import _lib
    C = 34
    m = ic.twins(C, ic.CORE_FRONTS, tmp_path / "p.yaml", "block")[0]
    try:
        lib, ctx = m._lib, m._ctx
        host_out = np.full((4, C - 2, C - 2), gc.POISON, np.uint32).view(np.float32)
        m.get_grid_map_layers(pc.FILTER_PUBLISHER, out=host_out.copy())      # four planes reserved, three of them written

        def planes():
            out = np.empty((4, C, C), np.float32)
            for k in range(4):
                assert lib.emap_plugin_plane_read(ctx, k, _lib.f32p(out[k])) == 0
            return out.tobytes()
        state = lambda: m.elevation_map.tobytes() + m.normal_map.tobytes() + planes() + host_out.tobytes()      # noqa: E731
        s0 = state()
        R = _lib.f32p(np.eye(3, dtype=np.float32).reshape(-1).copy())

        def chain(ops):
            table = (_lib.EmapPluginOp * len(ops))()
            for t_, o in zip(table, ops):
                t_.type, t_.dst_plane, t_.src_kind, t_.src_index, t_.i0, t_.i1, t_.flags, t_.f0 = o
            return lib.emap_plugin_chain(ctx, table, len(ops), R)

        good = (6, 2, 0, 0, 0, 0, 0, 0.0)
        chains = {
            "i0 17": [(6, 2, 0, 0, 17, 0, 0, 0.0)], "i0 -1": [(6, 2, 0, 0, -1, 0, 0, 0.0)], "i1 1": [(6, 2, 0, 0, 0, 1, 0, 0.0)], "flag 1": [(6, 2, 0, 0, 0, 0, 1, 0.0)],
            "flag 2": [(6, 2, 0, 0, 0, 0, 2, 0.0)], "dst beyond": [(6, 4, 0, 0, 0, 0, 0, 0.0)], "dst -1": [(6, -1, 0, 0, 0, 0, 0, 0.0)], "type 5": [(5, 2, 0, 0, 0, 0, 0, 0.0)],
            "type 7": [(7, 2, 0, 0, 0, 0, 0, 0.0)], "a bad op behind a good one": [good, (6, 3, 0, 0, 17, 0, 0, 0.0)],
        }
        for what, ops in chains.items():
            assert chain(ops) == -1, what
            assert b"emap_plugin_chain" in lib.emap_last_error(ctx), what
        assert state() == s0
        assert (host_out.view(np.uint32) == gc.POISON).all()
        assert chain([good, (6, 3, 1, 99, 16, 0, 0, 7.0)]) == 0        # src_* and f0 are ignored; the good call goes through afterwards
        after = np.frombuffer(planes(), np.float32).reshape(4, C, C)
        assert gc.same_bits(after[3], after[2]).all() and not gc.same_bits(after[2], after[1]).all()
    finally:
        m.close()


def test_a_strip_context_is_refused():
    from elevation_mapping_cupy_amd import _lib
    m = gc.start(34, strip=(0, 17, 0))
    try:
        ops = (_lib.EmapPluginOp * 1)()
        ops[0].type = 6
        assert m._lib.emap_plugin_chain(m._ctx, ops, 1, None) == -1 and b"single-strip" in m._lib.emap_last_error(m._ctx)
    finally:
        m.close()


# ---- 6. the switch --------------------------------------------------------------------------------------------------------------------------
def test_the_switch_forces_the_host_route_with_the_same_bits(tmp_path):
    C = 34
    m = ic.twins(C, ic.CORE_FRONTS, tmp_path / "p.yaml")[0]
    try:
        _, got = m.get_grid_map_layers(pc.FILTER_PUBLISHER, order="message")
        assert sorted(m.last_plugin_route.values()) == ["device", "device", "device"]
    finally:
        m.close()
    if vc.HALT.message is not None:
        pytest.fail("not started: an earlier child ended badly -- %s" % vc.HALT.message, pytrace=False)
    env = dict(EMAP_PLUGIN_RESIDENT="0", PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    try:
        z, _ = vc.run_child(os.path.join(ROOT, "tests", "_inpaint_chain_child.py"), "EMAP_PLUGIN_RESIDENT=0", env, (), str(tmp_path), 120, tracer=None)
    except vc.BadExit as e:
        vc.HALT.message = str(e)
        raise
    assert [str(r) for r in z["route"]] == ["host", "host", "host"] and [str(n) for n in z["names"]] == pc.FILTER_PUBLISHER
    assert gc.same_bits(z["layers"], got).all()
