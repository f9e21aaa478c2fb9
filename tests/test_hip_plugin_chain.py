"""GPU: publish-time plugins on resident planes (emap_plugin_chain, emap_plugin_planes, emap_publish_grid_map_ex; csrc/emap_plugchain.hip,
csrc/emap_api_plugchain.hip, kind 3 of k_grid_map).  No tolerance anywhere: every comparison is on uint32 views with NaN equal to NaN.
The yardstick is the plugins' host route -- one get_map_with_name_ref per layer -- taken from a TWIN map in the same state, because that
call changes PluginManager state (tests/_plug_cases.py).  Maps of cell_n 10, 34, 67, 100: less than one 32-wide grid tile, one tile, one
past two tiles, several 16 x 64 sweep / smooth tiles with a ragged edge; circular origin off zero, a shift pending, both orders."""
import ctypes as ct
import os
import subprocess
import sys

import numpy as np
import pytest

import _fixtures as fx
import _grid_cases as gc
import _plug_cases as pc
from conftest import ROOT

pytestmark = pytest.mark.gpu
_pairs, _refs = {}, {}
CONFIGS = {"ops": pc.ops_config, "erosion": lambda C: pc.erosion_config(), "core": lambda C: pc.CORE, "anymal": lambda C: pc.ANYMAL}


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """pair(C, config) -> (map, twin): built once per module, for the tests that do not change the map"""
    def get(C, cfg):
        if (C, cfg) not in _pairs:
            m, t = pc.twins(C, CONFIGS[cfg](C), tmp_path_factory.mktemp("plug") / ("%s_%d.yaml" % (cfg, C)))
            if cfg == "erosion":
                # the start state's traversability is close to binary: give the quantiser every value of 0 .. 1, and ero_const a flat layer
                # (time = 0, which a shift pads with 0 as well); writing a layer applies the pending shift, so move once more
                trav = pc.erosion_traversability(C)
                for x in (m, t):
                    x.set_layer_raw("traversability", trav)
                    x.set_layer_raw("time", np.zeros((C, C), np.float32))
                    x.move_to(gc.MOVE + np.array([0.04, -0.04, 0.02], np.float32), np.eye(3, dtype=np.float32))      # one more row and column
                    x.base_rotation = pc.TILT.copy()
            _pairs[(C, cfg)] = (m, t)
        return _pairs[(C, cfg)]
    yield get
    for m, t in _pairs.values():
        m.close(); t.close()
    _pairs.clear(); _refs.clear()


def _ref(m, name):
    out = np.zeros((m.cell_n - 2, m.cell_n - 2), np.float32)
    m.get_map_with_name_ref(name, out)
    return out


def _yardstick(pair, C, cfg):
    """the twin's host route for every plugin layer of the configuration, in configuration order (inputs before their readers), once"""
    if (C, cfg) not in _refs:
        twin = pair(C, cfg)[1]
        _refs[(C, cfg)] = {n: _ref(twin, n) for n in ["elevation", "traversability"] + twin.plugin_manager.layer_names}
        for r in _refs[(C, cfg)].values():
            r.setflags(write=False)
    return _refs[(C, cfg)]


def _check(got, ref, order, what):
    want = ref if order == "rows" else gc.message_plane(ref)
    assert got.shape == want.shape and got.dtype == np.float32, what
    ok = gc.same_bits(got, want)
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s (%s): %d of %d values differ bitwise, first at %s: %r vs %r" % (what, order, int((~ok).sum()), ok.size, i, got[i], want[i]))


def _differs(a, b):
    return not gc.same_bits(a, b).all()


# ---- 0. the twins are twins -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["ops", "erosion"])
@pytest.mark.parametrize("C", pc.SIZES)
def test_the_twins_hold_the_same_map(pair, C, cfg):
    m, t = pair(C, cfg)
    assert m.center[2] != 0 and (m.base_rotation == pc.TILT).all() and (t.base_rotation == pc.TILT).all()
    for n in gc.BUILTINS + tuple(m.semantic_map.layer_names):
        assert gc.same_bits(_ref(m, n), _ref(t, n)).all(), n
    assert m.plugin_manager.layer_names == t.plugin_manager.layer_names == pc.names_of(CONFIGS[cfg](C))


# ---- 1. each op alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["ops", "erosion"])
@pytest.mark.parametrize("C", pc.SIZES)
def test_each_op_alone_against_the_twin(pair, C, cfg):
    m = pair(C, cfg)[0]
    refs = _yardstick(pair, C, cfg)
    for order in pc.ORDERS:
        for n in m.plugin_manager.layer_names:
            names, got = m.get_grid_map_layers([n], order=order)
            assert names == [n] and m.last_plugin_route == {n: "device"}, n
            _check(got[0], refs[n], order, "%s at %d" % (n, C))
    assert m.plugin_manager.plugins[0].sweeps_run is None if cfg == "ops" else True      # the device route does not wait for the sweeps


@pytest.mark.parametrize("C", pc.SIZES)
def test_the_yardstick_can_tell_a_missing_step(pair, C):
    """preconditions on the twin's own output: a chain that skipped a sweep, a pass, the erosion, a flip or the transpose cannot pass"""
    r = _yardstick(pair, C, "ops")
    fin = lambda a: int(np.isfinite(a).sum())      # noqa: E731
    assert fin(r["min_filter"]) > fin(r["elevation"]) and fin(r["min5"]) > fin(r["elevation"])
    assert fin(r["min_filter"]) == r["min_filter"].size              # 30 sweeps close every hole of these maps: the NaN preconditions are on min_few
    assert 0 < fin(r["min_few"]) < r["min_few"].size and fin(r["min_few"]) > fin(r["elevation"])             # NaN and finite cells
    both = np.isfinite(r["smooth_few"]) & np.isfinite(r["min_few"])
    assert both.any() and (r["smooth_few"][both] != r["min_few"][both]).any() and fin(r["smooth_few"]) < fin(r["min_few"])      # NaN spreads
    assert _differs(r["max_filter"], r["min_filter"]) and _differs(r["smooth"], r["min_filter"]) and _differs(r["rce"], r["elevation"])
    assert _differs(r["rce_thr"], r["rce"]) and _differs(r["pub_00"], r["pub_01"]) and _differs(r["pub_00"], r["pub_10"]) and _differs(r["pub_10"], r["pub_11"])
    e = _yardstick(pair, C, "erosion")
    for rev in (False, True):
        base = e[pc.erosion_name(rev, 3, 0)]
        assert _differs(e[pc.erosion_name(rev, 3, 1)], base) and _differs(e[pc.erosion_name(rev, 4, 1)], e[pc.erosion_name(rev, 3, 1)])
        assert _differs(e[pc.erosion_name(rev, 3, 3)], e[pc.erosion_name(rev, 3, 1)])
    assert np.unique(e["ero_const"]).size == 1
    for d in (r, e):
        for n, a in d.items():
            # (ero_const is flat by construction; three 4 x 4 erosions reach 9 cells, across the 8 x 8 layer of cell_n 10: the minimum everywhere)
            # (the two built-ins are the helpers of the comparisons above: tests/test_hip_grid_map.py holds their own preconditions)
            if n not in ("ero_const", "elevation", "traversability") and not (C == 10 and n.endswith("k4_i3") and np.unique(a).size == 1):
                assert _differs(a, a.T) and _differs(a, a[::-1]) and _differs(a, a[:, ::-1]), n


# ---- 2. lists -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", pc.ORDERS)
@pytest.mark.parametrize("C", pc.SIZES)
def test_the_shipped_filter_publisher(pair, C, order):
    m, t = pair(C, "core")
    names, got = m.get_grid_map_layers(pc.FILTER_PUBLISHER, order=order)
    assert names == pc.FILTER_PUBLISHER
    assert m.last_plugin_route == {"min_filter": "device", "smooth": "device", "inpaint": "host"}      # elevation: a built-in, no plugin route
    for k, n in enumerate(names):
        _check(got[k], _ref(t, n), order, n)
    msg = m.get_grid_map_message(pc.FILTER_PUBLISHER + ["erosion"])
    assert msg.layers == pc.FILTER_PUBLISHER + ["erosion"] and m.last_plugin_route["erosion"] == "device"
    for k, n in enumerate(msg.layers):
        _check(msg.data[k].data.reshape(C - 2, C - 2), _ref(t, n), "message", n)


@pytest.mark.parametrize("order", pc.ORDERS)
@pytest.mark.parametrize("C", pc.SIZES)
def test_the_anymal_list_with_both_filters(pair, C, order):
    m, t = pair(C, "anymal")
    names, got = m.get_grid_map_layers(pc.ANYMAL_LIST, order=order)
    assert m.last_plugin_route == {"min_filter": "device", "max_filter": "device", "smooth": "device", "inpaint": "host"}
    for k, n in enumerate(names):
        _check(got[k], _ref(t, n), order, n)
    assert _differs(got[0], got[1])


def _frame(m, C, seed):
    R, t = fx.POSES["identity"]
    m.input_pointcloud(gc.semantic_frame(C, 3000, seed), gc.CHANNELS, R, t.copy() + m.center, 0.0, 0.0)


@pytest.mark.parametrize("order", pc.ORDERS)
def test_smooth_listed_first_reads_the_tick_before(order, tmp_path):
    C = 67
    m, t = pc.twins(C, pc.CORE, tmp_path / "p.yaml")
    try:
        lst = ["smooth", "min_filter"]
        _, a1 = m.get_grid_map_layers(lst, order=order)
        r1 = [_ref(t, n) for n in lst]
        _frame(m, C, 7); _frame(t, C, 7)
        _, a2 = m.get_grid_map_layers(lst, order=order)
        r2 = [_ref(t, n) for n in lst]
        for k, n in enumerate(lst):
            _check(a1[k], r1[k], order, n + " tick 1"); _check(a2[k], r2[k], order, n + " tick 2")
        assert m.last_plugin_route == {"smooth": "device", "min_filter": "device"}
        assert _differs(r2[0], _ref(t, "smooth")) and _differs(r1[1], r2[1])      # tick 2's smooth is NOT the smooth of tick 2's min_filter
    finally:
        m.close(); t.close()


@pytest.mark.parametrize("order", pc.ORDERS)
@pytest.mark.parametrize("C", pc.SIZES)
def test_permuted_slots_with_a_gap(pair, C, order):
    from elevation_mapping_cupy_amd import _lib
    m = pair(C, "ops")[0]
    r = _yardstick(pair, C, "ops")
    names = m.plugin_manager.layer_names
    lst = ["min_few", "pub_11", "rce", "pub_10"]
    m.get_grid_map_layers(lst)                                         # the chain leaves the planes; the table below reads them as they are
    flags = {"min_few": _lib.GRID_ADD_Z, "pub_11": _lib.GRID_FILL_NAN | _lib.GRID_ADD_Z, "rce": 0, "pub_10": _lib.GRID_FILL_NAN}
    slots = {"pub_10": 0, "min_few": 5, "elevation": 3, "rce": 2, "pub_11": 6}
    entries = [(_lib.GRID_PLUGIN, names.index(n), slots[n], flags[n]) for n in lst] + [(_lib.GRID_BUILTIN, 0, slots["elevation"])]
    out = np.full((7, C - 2, C - 2), gc.POISON, np.uint32).view(np.float32)
    m.publish_grid_layers(entries, out, order)
    for n, s in slots.items():
        _check(out[s], r[n], order, n)
    assert (out[[1, 4]].view(np.uint32) == gc.POISON).all()


@pytest.mark.parametrize("order", pc.ORDERS)
@pytest.mark.parametrize("C", pc.SIZES)
def test_fill_nan_beside_layers_of_the_cold_half_only(pair, C, order):
    """time and upper_bound need the cold half alone, so the launch loads no hot half and FILL_NAN takes is_valid from cold.w, its mirror"""
    m, t = pair(C, "ops")
    r = _yardstick(pair, C, "ops")
    lst = ["time", "pub_10", "upper_bound", "pub_11"]
    names, got = m.get_grid_map_layers(lst, order=order)
    assert names == lst and m.last_plugin_route == {"pub_10": "device", "pub_11": "device"}
    for k, n in enumerate(lst):
        _check(got[k], r[n] if n in r else _ref(t, n), order, n)
    assert np.isnan(got[1]).any() and np.isfinite(got[1]).any()


def test_two_calls_around_a_frame_without_a_sync(tmp_path):
    C = 67
    m, t = pc.twins(C, pc.ANYMAL, tmp_path / "p.yaml")
    try:
        lst = ["min_filter", "elevation", "smooth", "max_filter", "rgb"]
        before = {n: _ref(t, n) for n in lst}
        _, a = m.get_grid_map_layers(lst, order="message")
        _frame(m, C, 7); _frame(t, C, 7)
        _, b = m.get_grid_map_layers(lst, order="message")
        after = {n: _ref(t, n) for n in lst}
        for k, n in enumerate(lst):
            _check(a[k], before[n], "message", n + " before"); _check(b[k], after[n], "message", n + " after")
            assert _differs(before[n], after[n]), n
    finally:
        m.close(); t.close()


# ---- 3. coherence ---------------------------------------------------------------------------------------------------------------------
def test_the_host_sees_what_the_device_left(tmp_path):
    C = 34
    m, t = pc.twins(C, pc.CORE, tmp_path / "p.yaml")
    try:
        m.get_grid_map_layers(["min_filter", "erosion"])
        for n in ("min_filter", "erosion"):
            _ref(t, n)
        pm, pt = m.plugin_manager, t.plugin_manager
        assert gc.same_bits(pm.get_map_with_name("min_filter"), pt.get_map_with_name("min_filter")).all()
        assert gc.same_bits(pm.layers[3], pt.layers[3]).all() and gc.same_bits(pm.layers, pt.layers).all()
        # the host route of smooth after a device min_filter: the plane comes back for it
        m.get_grid_map_layers(["min_filter"])
        assert m.last_plugin_route == {"min_filter": "device"}
        assert gc.same_bits(_ref(m, "smooth"), _ref(t, "smooth")).all()
        # and a device smooth after a host min_filter: the layer goes up for it
        _ref(m, "min_filter")
        _, got = m.get_grid_map_layers(["smooth"])
        _check(got[0], _ref(t, "smooth"), "rows", "smooth after a host min_filter")
    finally:
        m.close(); t.close()


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
import _grid_cases as gc
import _plug_cases as pc
from pathlib import Path
cfg = Path(%r)
cfg.write_text(pc.yaml_of(pc.CORE))
m = gc.start(34, plugin_file=cfg)
names, got = m.get_grid_map_layers(pc.FILTER_PUBLISHER + ["erosion"], order="message")
np.save(%r, got)
print("ROUTE", sorted(m.last_plugin_route.items()))
m.close()
"""


def test_the_switch_forces_the_host_route_with_the_same_bits(tmp_path):
    m = pc.twins(34, pc.CORE, tmp_path / "p.yaml")[0]
    try:
        _, got = m.get_grid_map_layers(pc.FILTER_PUBLISHER + ["erosion"], order="message")
        assert sorted(m.last_plugin_route.values()) == ["device", "device", "device", "host"]
    finally:
        m.close()
    env = dict(os.environ, EMAP_PLUGIN_RESIDENT="0", PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    code = _CHILD % (os.path.join(ROOT, "tests"), str(tmp_path / "child.yaml"), str(tmp_path / "child.npy"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    route = [ln for ln in out.stdout.splitlines() if ln.startswith("ROUTE")]
    assert route == ["ROUTE " + str([(n, "host") for n in sorted(["min_filter", "smooth", "inpaint", "erosion"])])]
    assert gc.same_bits(np.load(tmp_path / "child.npy"), got).all()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_buffer_the_planes_and_the_map_as_they_were(tmp_path):
    from elevation_mapping_cupy_amd import _lib
    C = 34
    m = pc.twins(C, pc.CORE, tmp_path / "p.yaml")[0]
    try:
        M, lib, ctx = C - 2, m._lib, m._ctx
        m.get_grid_map_layers(["min_filter", "smooth", "erosion"])     # four planes reserved, three of them written
        n_sem = len(m.semantic_map.layer_names)

        def planes():
            out = np.empty((4, C, C), np.float32)
            for k in range(4):
                assert lib.emap_plugin_plane_read(ctx, k, _lib.f32p(out[k])) == 0
            return out.tobytes()
        state = lambda: m.elevation_map.tobytes() + m.normal_map.tobytes() + m.semantic_map.semantic_map.tobytes() + planes()      # noqa: E731
        s0 = state()
        out = np.full((3, M, M), gc.POISON, np.uint32).view(np.float32)
        R = _lib.f32p(np.eye(3, dtype=np.float32).reshape(-1).copy())

        def chain(ops, n=None, null_ops=False, rot=R):
            table = (_lib.EmapPluginOp * max(1, len(ops)))()
            for t_, o in zip(table, ops):
                t_.type, t_.dst_plane, t_.src_kind, t_.src_index, t_.i0, t_.i1, t_.flags, t_.f0 = o
            return lib.emap_plugin_chain(ctx, None if null_ops else table, len(ops) if n is None else n, rot)

        good = (2, 1, 1, 0, 0, 0, 0, 0.0)                            # smooth of plane 0 into plane 1
        chains = {
            "null ops": dict(ops=[good], null_ops=True), "no op": dict(ops=[]), "33 ops": dict(ops=[good] * 33), "type 5": dict(ops=[(5, 1, 0, 0, 0, 0, 0, 0.0)]),
            "type -1": dict(ops=[(-1, 1, 0, 0, 0, 0, 0, 0.0)]), "dst beyond": dict(ops=[good, (2, 4, 0, 0, 0, 0, 0, 0.0)]), "dst -1": dict(ops=[(0, -1, 0, 0, 1, 1, 0, 0.0)]),
            "src kind 2": dict(ops=[(2, 1, 2, 0, 0, 0, 0, 0.0)]), "layer 7": dict(ops=[(3, 1, 0, 7, 3, 1, 0, 0.0)]), "src plane beyond": dict(ops=[(2, 1, 1, 4, 0, 0, 0, 0.0)]),
            "smooth in place": dict(ops=[(2, 1, 1, 1, 0, 0, 0, 0.0)]), "dilation 33": dict(ops=[(0, 0, 0, 0, 33, 1, 0, 0.0)]), "sweeps 4097": dict(ops=[(1, 0, 0, 0, 1, 4097, 0, 0.0)]),
            "kernel 0": dict(ops=[(3, 1, 0, 3, 0, 1, 0, 0.0)]), "kernel 64": dict(ops=[(3, 1, 0, 3, 64, 1, 0, 0.0)]), "iterations 257": dict(ops=[(3, 1, 0, 3, 3, 257, 0, 0.0)]),
            "reverse on smooth": dict(ops=[(2, 1, 1, 0, 0, 0, 1, 0.0)]), "flag 4": dict(ops=[(3, 1, 0, 3, 3, 1, 4, 0.0)]), "no rotation": dict(ops=[(4, 1, 0, 0, 0, 0, 0, 0.0)], rot=None),
            "a bad op behind a good one": dict(ops=[(0, 0, 0, 0, 1, 2, 0, 0.0), (2, 1, 1, 1, 0, 0, 0, 0.0)]),
        }
        for what, kw in chains.items():
            assert chain(**kw) == -1, what
            assert b"emap_plugin_chain" in lib.emap_last_error(ctx), what
        assert lib.emap_plugin_planes(ctx, 33) == -1 and lib.emap_plugin_planes(ctx, -1) == -1 and b"emap_plugin_planes" in lib.emap_last_error(ctx)
        buf = _lib.f32p(np.zeros((C, C), np.float32))
        assert lib.emap_plugin_plane_write(ctx, 4, buf) == -1 and lib.emap_plugin_plane_read(ctx, -1, buf) == -1 and lib.emap_plugin_plane_write(ctx, 0, None) == -1

        def grid(entries, order=0, n=None, host_slots=None, null_table=False, null_out=False):
            table = (_lib.EmapGridLayerEx * max(1, len(entries)))()
            for g, e in zip(table, entries):
                g.kind, g.index, g.slot, g.flags = e
            return lib.emap_publish_grid_map_ex(ctx, None if null_table else table, len(entries) if n is None else n, order, ct.c_float(0.5), 0,
                                                None if null_out else _lib.f32p(out), out.shape[0] if host_slots is None else host_slots)
        ok = [(0, 0, 0, 0), (3, 0, 1, 3)]
        grids = {
            "null table": dict(entries=ok, null_table=True), "null out": dict(entries=ok, null_out=True), "no layer": dict(entries=[]), "33 layers": dict(entries=[(3, 0, 0, 0)] * 33, host_slots=64),
            "kind 4": dict(entries=[(4, 0, 0, 0)]), "kind -1": dict(entries=[(-1, 0, 0, 0)]), "order 2": dict(entries=ok, order=2), "built-in 9": dict(entries=[(0, 9, 0, 0)]),
            "semantic beyond": dict(entries=[(1, n_sem, 0, 0)]), "plane beyond": dict(entries=[(3, 4, 0, 0)]), "plane -1": dict(entries=[(0, 0, 0, 0), (3, -1, 1, 0)]),
            "flag 4": dict(entries=[(3, 0, 0, 4)]), "flags on a built-in": dict(entries=[(0, 0, 0, 1)]), "slot beyond": dict(entries=[(3, 0, 3, 0)]), "slot -1": dict(entries=[(3, 0, -1, 0)]),
            "slot twice": dict(entries=[(3, 0, 1, 0), (0, 0, 0, 0), (3, 1, 1, 0)]),
        }
        for what, kw in grids.items():
            assert grid(**kw) == -1, what
            assert b"emap_publish_grid_map_ex" in lib.emap_last_error(ctx), what
            assert (out.view(np.uint32) == gc.POISON).all(), what
        assert state() == s0
        assert chain([good]) == 0 and grid(ok) == 0                   # and the good calls do go through afterwards
        assert (out[2].view(np.uint32) == gc.POISON).all() and not (out[:2].view(np.uint32) == gc.POISON).any()
        assert lib.emap_plugin_planes(ctx, 6) == 0                    # growing keeps the planes and adds zero ones
        more = np.empty((2, C, C), np.float32)
        assert lib.emap_plugin_plane_read(ctx, 0, _lib.f32p(more[0])) == 0 and lib.emap_plugin_plane_read(ctx, 5, _lib.f32p(more[1])) == 0
        assert more[0].tobytes() == s0[-4 * C * C * 4:][:C * C * 4] and not more[1].any()
    finally:
        m.close()


def test_a_strip_context_is_refused():
    from elevation_mapping_cupy_amd import _lib
    C = 34
    m = gc.start(C, strip=(0, 17, 0))
    try:
        out = np.full((1, C - 2, C - 2), gc.POISON, np.uint32).view(np.float32)
        table = (_lib.EmapGridLayerEx * 1)()
        ops = (_lib.EmapPluginOp * 1)()
        ops[0].type, ops[0].i0, ops[0].i1 = 0, 1, 1
        assert m._lib.emap_plugin_planes(m._ctx, 1) == -1 and b"single-strip" in m._lib.emap_last_error(m._ctx)
        assert m._lib.emap_plugin_chain(m._ctx, ops, 1, None) == -1 and b"single-strip" in m._lib.emap_last_error(m._ctx)
        assert m._lib.emap_publish_grid_map_ex(m._ctx, table, 1, 0, ct.c_float(0.0), 0, _lib.f32p(out), 1) == -1
        assert b"single-strip" in m._lib.emap_last_error(m._ctx) and (out.view(np.uint32) == gc.POISON).all()
    finally:
        m.close()
