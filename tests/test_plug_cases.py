"""CPU: the Python side of the publish-time plugins on resident planes -- the op table plugin_chain_plan builds for the shipped lists, the
coherence bookkeeping of PluginManager against a stub library that records its calls, and the NumPy restatement of the erosion's
arithmetic (tests/_plug_cases.py) against plugins/erosion.py's own."""
import ctypes as ct

import numpy as np
import pytest

import _plug_cases as pc

LAYERS = ["elevation", "variance", "is_valid", "traversability", "time", "upper_bound", "is_upper_bound"]
SEM = ["s0", "s1", "c0", "rgb"]
C = 12


class _Lib:
    """records (function, plane) of every call; emap_plugin_plane_read fills the host array with 100 + plane, emap_erode erodes on the host"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, fn):
        def call(ctx, *a):
            if fn == "emap_plugin_chain":
                self.calls.append((fn, [(a[0][k].type, a[0][k].dst_plane, a[0][k].src_kind, a[0][k].src_index) for k in range(a[1])]))
            elif fn == "emap_erode":
                src, k, it, dst = a
                n = C
                np.ctypeslib.as_array(dst, (n, n))[...] = pc.erode_loop(np.ctypeslib.as_array(src, (n, n)), k, it)
            else:
                self.calls.append((fn, a[0]))
                if fn == "emap_plugin_plane_read":
                    np.ctypeslib.as_array(a[1], (C, C))[...] = 100 + a[0]
            return 0
        return call


class _Emap:
    def __init__(self):
        self._lib, self._ctx, self.cell_n, self.resolution = _Lib(), None, C, 0.04

    def _chk(self, rc):
        assert rc == 0


def _plan(entries, names, resident=True, emap=None):
    from elevation_mapping_cupy_amd.plugins.plugin_manager import plugin_chain_plan
    pm = pc.manager(entries, C, emap or _Emap())
    return plugin_chain_plan(names, pm.plugins, pm.layer_names, LAYERS, SEM, resident=resident), pm


def _brief(steps):
    return [(s[0], s[1]) + ((s[2]["type"], s[2]["dst_plane"], s[2]["src_kind"], s[2]["src_index"], s[2]["i0"], s[2]["i1"], s[2]["flags"]) if s[0] == "device" else ())
            for s in steps]


# ---- plugin_chain_plan ----------------------------------------------------------------------------------------------------------------
def test_the_shipped_core_list():
    steps, _ = _plan(pc.CORE, pc.FILTER_PUBLISHER)
    assert _brief(steps) == [("device", "min_filter", 0, 0, 0, 0, 1, 30, 0), ("device", "smooth", 2, 1, 1, 0, 0, 0, 0), ("host", "inpaint")]
    steps, _ = _plan(pc.CORE, ["erosion"])
    assert _brief(steps) == [("device", "erosion", 3, 3, 0, 3, 3, 1, 1)]       # traversability = RAW layer 3, kernel 3, one iteration, reversed


def test_the_anymal_list_holds_both_filters():
    steps, _ = _plan(pc.ANYMAL, pc.ANYMAL_LIST)
    assert _brief(steps) == [("device", "min_filter", 0, 0, 0, 0, 1, 30, 0), ("device", "max_filter", 1, 1, 0, 0, 5, 10, 0),
                             ("device", "smooth", 2, 2, 1, 0, 0, 0, 0), ("host", "inpaint")]


def test_a_reversed_list_keeps_its_order():
    steps, _ = _plan(pc.CORE, ["elevation", "smooth", "min_filter"])
    assert [(s[0], s[1]) for s in steps] == [("device", "smooth"), ("device", "min_filter")]
    assert steps[0][2]["src_kind"] == 1 and steps[0][2]["src_index"] == 0      # the plane min_filter left on the tick before


def test_a_semantic_input_goes_to_the_host():
    pm = pc.manager(pc.SEMANTIC_EROSION, C, _Emap())
    assert pm.plugins[0].device_op(LAYERS, pm.layer_names, SEM) is None
    steps, _ = _plan(pc.SEMANTIC_EROSION, ["erosion_sem"])
    assert steps == [("host", "erosion_sem")]
    smooth_sem = [pc._entry("smooth_filter", "smooth_sem", input_layer_name="s1")]
    assert _plan(smooth_sem, ["smooth_sem"])[0] == [("host", "smooth_sem")]
    own = [pc._entry("smooth_filter", "again", input_layer_name="again")]      # an op cannot read the plane it writes
    assert _plan(own, ["again"])[0] == [("host", "again")]


def test_a_mixed_list_and_the_switch():
    steps, pm = _plan(pc.CORE, ["inpaint", "min_filter", "ghost", "erosion", "smooth"])
    assert [(s[0], s[1]) for s in steps] == [("host", "inpaint"), ("device", "min_filter"), ("device", "erosion"), ("device", "smooth")]
    assert pm.plugins[2].plugin_inputs(pm.layer_names) == () and pm.plugins[1].plugin_inputs(pm.layer_names) == ("min_filter",)
    steps, _ = _plan(pc.CORE, pc.FILTER_PUBLISHER, resident=False)
    assert steps == [("host", "min_filter"), ("host", "smooth"), ("host", "inpaint")]


def test_every_op_of_the_gpu_cases_is_a_device_op():
    e = _Emap()
    e.resolution = pc.resolution(C)
    for entries in (pc.ops_config(C), pc.erosion_config()):
        steps, _ = _plan(entries, pc.names_of(entries), emap=e)
        assert [s[0] for s in steps] == ["device"] * len(entries)
    other = [pc._entry("robot_centric_elevation", "rce", resolution=0.05)]       # not the map's resolution: the op would multiply by another float
    assert _plan(other, ["rce"], emap=e)[0] == [("host", "rce")]


# ---- coherence ------------------------------------------------------------------------------------------------------------------------
class _Body:
    """a host plugin's body: records the plugin layers it is handed, returns a constant plane; plugin_inputs is the real plugin's"""

    def __init__(self, real, value):
        self.real, self.value, self.seen = real, value, None

    def plugin_inputs(self, names):
        return self.real.plugin_inputs(names)

    def __call__(self, elevation_map, layer_names, plugin_layers, plugin_layer_names, *args):
        self.seen = np.array(plugin_layers)
        return np.full((C, C), self.value, np.float32)


def _host_plugin(pm, name, value):
    """the host route of one plugin (PluginManager.update_with_name) with the body above; returns the plugin layers it saw"""
    idx = pm.layer_names.index(name)
    real = pm.plugins[idx]
    pm.plugins[idx] = body = _Body(real, value)
    try:
        pm.update_with_name(name, np.zeros((7, C, C), np.float32), LAYERS, np.zeros((4, C, C), np.float32), SEM, np.eye(3, dtype=np.float32), {})
    finally:
        pm.plugins[idx] = real
    return body.seen


def test_a_host_plugin_fetches_exactly_the_planes_it_reads():
    entries = pc.CORE + [pc._entry("smooth_filter", "smooth2", input_layer_name="min_filter")]
    e = _Emap()
    steps, pm = _plan(entries, ["min_filter", "smooth"], emap=e)
    route = pm.run_plan(steps, lambda n: pytest.fail("no host plugin in this list"))
    assert route == {"min_filter": "device", "smooth": "device"}
    assert e._lib.calls == [("emap_plugin_planes", 5), ("emap_plugin_chain", [(0, 0, 0, 0), (2, 1, 1, 0)])]      # ONE chain, no upload: nothing is newer on the host
    assert pm.plugins[0].sweeps_run is None
    del e._lib.calls[:]
    _host_plugin(pm, "inpaint", 7.0)                                   # Inpainting reads no plugin layer
    assert e._lib.calls == []
    seen = _host_plugin(pm, "smooth2", 8.0)                            # a host plugin that names min_filter as its input
    assert e._lib.calls == [("emap_plugin_plane_read", 0)]
    assert (seen[0] == 100).all() and not seen[1].any()                # it saw the downloaded plane; smooth stayed on the device
    del e._lib.calls[:]
    assert (pm.layers[1] == 101).all() and (pm.layers[2] == 7).all() and (pm.layers[4] == 8).all()      # attribute access: the rest comes back
    assert e._lib.calls == [("emap_plugin_plane_read", 1)]
    assert (pm.get_map_with_name("min_filter") == 100).all() and e._lib.calls == [("emap_plugin_plane_read", 1)]


def test_a_device_op_after_a_host_plugin_uploads_its_input_once():
    e = _Emap()
    steps, pm = _plan(pc.CORE, ["smooth"], emap=e)
    _host_plugin(pm, "min_filter", 3.0)                                # the host route computed min_filter: newer on the host
    route = pm.run_plan(steps, None)
    assert route == {"smooth": "device"}
    assert e._lib.calls == [("emap_plugin_planes", 4), ("emap_plugin_plane_write", 0), ("emap_plugin_chain", [(2, 1, 1, 0)])]
    del e._lib.calls[:]
    pm.run_plan(steps, None)                                           # the plane is up to date now
    assert e._lib.calls == [("emap_plugin_chain", [(2, 1, 1, 0)])]
    del e._lib.calls[:]
    steps, _ = _plan(pc.CORE, ["min_filter", "smooth"], emap=e)
    _host_plugin(pm, "min_filter", 4.0)
    pm.run_plan(steps, None)                                           # min_filter is rewritten by the chain itself: nothing to upload
    assert e._lib.calls == [("emap_plugin_chain", [(0, 0, 0, 0), (2, 1, 1, 0)])]


def test_a_host_plugin_in_the_list_splits_the_chain_only_when_it_reads_it():
    e = _Emap()
    ran = []
    steps, pm = _plan(pc.CORE, pc.FILTER_PUBLISHER, emap=e)
    route = pm.run_plan(steps, ran.append)
    assert route == {"min_filter": "device", "smooth": "device", "inpaint": "host"} and ran == ["inpaint"]
    assert [c[0] for c in e._lib.calls] == ["emap_plugin_planes", "emap_plugin_chain"]
    entries = pc.CORE + [pc._entry("max_layer_filter", "unknown_inputs", layers=["min_filter"], thresholds={}, default_value=0.0)]
    e = _Emap()
    steps, pm = _plan(entries, ["min_filter", "unknown_inputs", "smooth"], emap=e)
    assert [s[0] for s in steps] == ["device", "host", "device"]
    order = []
    e._lib.calls = order
    pm.run_plan(steps, lambda n: order.append(("host", n)))
    assert [c[0] for c in order] == ["emap_plugin_planes", "emap_plugin_chain", "host", "emap_plugin_chain"]      # plugin_inputs unknown: the chain runs first


# ---- the erosion's arithmetic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("k,it", [(1, 1), (3, 1), (4, 1), (3, 0), (3, 3)])
def test_the_restated_erosion_is_the_plugins(reverse, k, it):
    from elevation_mapping_cupy_amd.plugins.erosion import Erosion
    flat = 0
    for what, layer in pc.case_layers(C).items():
        plugin = Erosion(input_layer_name="traversability", kernel_size=k, iterations=it, reverse=reverse, emap=_Emap())
        planes = np.zeros((7, C, C), np.float32); planes[3] = layer
        want = plugin(planes, LAYERS, np.zeros((0, C, C), np.float32), [], np.zeros((0, C, C), np.float32), [])
        q = pc.erosion_quantise(layer, reverse)
        if q is None:
            flat += 1
            got = (np.float32(1) - (np.float32(1) - layer)) if reverse else layer      # the plugin un-reverses what it reversed: not the same bits
        else:
            assert q[0].min() == 0 and q[0].max() == 255, what
            got = pc.erosion_dequantise(pc.erode_loop(q[0], k, it), q[1], q[2], reverse)
        assert want.dtype == np.float32 and pc.gc.same_bits(got, want).all(), what
    assert flat == 2                                                   # the constant layer and the one with a NaN


def test_the_window_minimum_of_the_restatement():
    img = np.arange(25, dtype=np.float32).reshape(5, 5)
    assert (pc.erode_loop(img, 1, 3) == img).all() and (pc.erode_loop(img, 3, 0) == img).all()
    e3 = pc.erode_loop(img, 3, 1)
    assert e3[0, 0] == 0 and e3[2, 2] == 6 and e3[4, 4] == 18
    e4 = pc.erode_loop(img, 4, 1)                                      # anchor 2: rows r - 2 .. r + 1
    assert e4[2, 2] == 0 and e4[4, 4] == 12 and e4[1, 1] == 0


# ---- the case table's preconditions, counted where the oracle supplies the planes ------------------------------------------------------
def _published(plane):
    return np.flip(np.asarray(plane, np.float32)[1:-1, 1:-1])          # border stripped, both axes flipped


def _asymmetric(a):
    same = pc.gc.same_bits
    return not same(a, a.T).all() and not same(a, a[::-1]).all() and not same(a, a[:, ::-1]).all()


@pytest.mark.parametrize("C", pc.SIZES)
def test_the_case_table_can_tell_a_missing_step(C):
    """the min / smooth layers of tests/_plug_cases.ops_config on the oracle's map in the GPU test's start state, and the erosion cases on
    the restatement above: a chain that skipped a sweep, a pass, the erosion, a flip or the transpose would not reproduce them"""
    from oracle import emap_oracle as eo
    e = pc.oracle_start(C).elevation_map
    fin = lambda a: int(np.isfinite(a).sum())      # noqa: E731
    known = int((e[2][1:-1, 1:-1] > 0.5).sum())                        # the finite cells of the published elevation
    mf30, mf5, few = (_published(eo.min_filter(C, d, n, e[0], e[2])[0]) for d, n in ((1, 30), (5, 10), (1, 1)))
    assert 0 < known < few.size
    assert fin(mf30) > known and fin(mf5) > known
    # the shipped 30 sweeps (and 10 of radius 5) close every hole of these maps: the NaN preconditions need a filter that stops early,
    # which is why the case table carries min_few (one sweep), smooth_few and the erosion of min_few next to the shipped filters
    assert fin(mf30) == mf30.size and fin(mf5) == mf5.size
    assert known < fin(few) < few.size                                 # NaN and finite cells, more finite ones than the elevation
    smooth_few = _published(pc.box3_twice(eo.min_filter(C, 1, 1, e[0], e[2])[0]))      # (scipy's running sum cannot smooth a plane with NaN: _plug_cases.box3_twice)
    both = np.isfinite(smooth_few) & np.isfinite(few)
    assert both.any() and (smooth_few[both] != few[both]).any() and fin(smooth_few) < fin(few)       # NaN spreads through both passes
    raw30 = eo.min_filter(C, 1, 30, e[0], e[2])[0]
    smooth30 = _published(pc.box3_twice(raw30))
    assert np.allclose(pc.box3_twice(raw30), eo.smooth_filter(raw30), rtol=1e-6, atol=1e-6) and (smooth30 != mf30).any()
    for a in (mf30, mf5, few, smooth_few, smooth30):
        assert _asymmetric(a)
    assert pc.erosion_quantise(eo.min_filter(C, 1, 1, e[0], e[2])[0], False) is None                  # the erosion of min_few takes the flat rule
    trav = pc.erosion_traversability(C)
    for rev in (False, True):
        q, lo, hi = pc.erosion_quantise(trav, rev)
        out = {(k, it): _published(pc.erosion_dequantise(pc.erode_loop(q, k, it), lo, hi, rev)) for k in (1, 3, 4) for it in (0, 1, 3)}
        assert len(np.unique(q)) > 200 or C == 10                      # the quantiser sees (nearly) every level
        assert (out[(3, 1)] != out[(3, 0)]).any() and (out[(4, 1)] != out[(3, 1)]).any() and (out[(3, 3)] != out[(3, 1)]).any()
        assert pc.gc.same_bits(out[(1, 3)], out[(1, 0)]).all()          # a 1 x 1 window erodes nothing
        for (k, it), a in out.items():
            assert _asymmetric(a) or (C == 10 and (k, it) == (4, 3)), (k, it)      # (three 4 x 4 erosions reach across the 8 x 8 layer)


def test_a_write_through_the_layers_array_reaches_the_next_device_op():
    """`layers` hands out the host array to write into, as the reference's does: what the caller leaves there is uploaded before a device
    op reads it"""
    e = _Emap()
    steps, pm = _plan(pc.CORE, ["smooth"], emap=e)
    pm.run_plan(steps, None)
    del e._lib.calls[:]
    pm.layers[0][...] = 5.0
    pm.run_plan(steps, None)
    assert e._lib.calls == [("emap_plugin_plane_read", 1), ("emap_plugin_plane_write", 0), ("emap_plugin_chain", [(2, 1, 1, 0)])]
