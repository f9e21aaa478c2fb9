"""GPU: the semantic plugins on resident planes (emap_plugin_chain_ex; csrc/emap_plugchain.hip: k_semantic_filter, k_semantic_trav,
k_max_layer; csrc/emap_pca.hip).  The pointwise ops are compared bit for bit -- uint32 views, NaN equal to NaN -- with the plugins' host
route on a TWIN map (tests/_semplug_cases.py); FEATURES_PCA under the PCA condition (levels differ by at most 1, in at most 0.1 % of the
cells).  Maps of cell_n 10, 34, 67, 100; circular origin off zero, a shift pending, both orders."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _fixtures as fx
import _grid_cases as gc
import _plug_cases as pc
import _semplug_cases as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu
_pairs, _refs = {}, {}
INPUTS = ["featp_smooth", "hostp", "robot_centric_elevation"]      # the plugin planes the ops of ops_config read: device, host, device


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """pair(C, config) -> (map, twin): built once per module, for the tests that do not change the map"""
    def get(C, cfg):
        if (C, cfg) not in _pairs:
            _pairs[(C, cfg)] = tuple(sc.twins(C, sc.CONFIGS[cfg](C), tmp_path_factory.mktemp("semplug") / ("%s_%d.yaml" % (cfg, C))))
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
        _refs[(C, cfg)] = {n: _ref(twin, n) for n in ["elevation"] + twin.plugin_manager.layer_names}
        for r in _refs[(C, cfg)].values():
            r.setflags(write=False)
    return _refs[(C, cfg)]


def _is_pca(m, name):
    pm = m.plugin_manager
    return name in pm.layer_names and pm.plugin_names[pm.layer_names.index(name)] == "features_pca"


def _check(m, name, got, ref, order, what):
    want = ref if order == "rows" else gc.message_plane(ref)
    assert got.shape == want.shape and got.dtype == np.float32, what
    if _is_pca(m, name):
        sc.pca_condition(got, want, what)
        return
    ok = gc.same_bits(got, want)
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s (%s): %d of %d values differ bitwise, first at %s: %r vs %r" % (what, order, int((~ok).sum()), ok.size, i, got[i], want[i]))


def _plane(m, k):
    out = np.empty((m.cell_n, m.cell_n), np.float32)
    from elevation_mapping_cupy_amd import _lib
    assert m._lib.emap_plugin_plane_read(m._ctx, k, _lib.f32p(out)) == 0
    return out


def _semantic_names(m):
    pm = m.plugin_manager
    return [n for n, p in zip(pm.layer_names, pm.plugin_names) if p in ("semantic_filter", "semantic_traversability", "max_layer_filter", "features_pca")]


# ---- 0. the entry point, the twins -----------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_entry_point():
    from elevation_mapping_cupy_amd import _lib
    assert hasattr(_lib.load(), "emap_plugin_chain_ex")


@pytest.mark.parametrize("C", sc.SIZES)
def test_the_twins_hold_the_same_map(pair, C):
    m, t = pair(C, "ops")
    assert (m.base_rotation == pc.TILT).all() and (t.base_rotation == pc.TILT).all()
    assert m.semantic_map.layer_names == t.semantic_map.layer_names == ["s0", "s1", "c0", "rgb"] + sc.SEM_NAMES + sc.FEAT_NAMES
    for n in gc.BUILTINS + tuple(m.semantic_map.layer_names):
        assert gc.same_bits(_ref(m, n), _ref(t, n)).all(), n
    assert np.isfinite(m.get_layer_raw("elevation")).all()                      # a NaN feature has no PCA on either route
    cls = np.stack([m.semantic_map.get_layer(n) for n in sc.SEM_NAMES])
    assert np.isnan(cls).all(axis=0).any() and (np.isnan(cls).sum(axis=0) == 1).any()          # the NaN cells survived the move


# ---- 1. every op alone and the whole list -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", sc.SIZES)
def test_each_op_alone_against_the_twin(pair, C):
    m = pair(C, "ops")[0]
    refs = _yardstick(pair, C, "ops")
    pm = m.plugin_manager
    m.get_grid_map_layers(INPUTS)
    assert m.last_plugin_route == {"featp_smooth": "device", "hostp": "host", "robot_centric_elevation": "device"}
    twin_pm = pair(C, "ops")[1].plugin_manager
    for order in sc.ORDERS:
        for n in _semantic_names(m):
            names, got = m.get_grid_map_layers([n], order=order)
            assert names == [n] and m.last_plugin_route == {n: "device"}, n
            _check(m, n, got[0], refs[n], order, "%s at %d" % (n, C))
            if order == "rows" and not _is_pca(m, n):                        # the RAW plane: border included, no flip, no NaN fill
                k = pm.layer_names.index(n)
                assert gc.same_bits(_plane(m, k), twin_pm.host_layer(n)).all(), n


@pytest.mark.parametrize("order", sc.ORDERS)
@pytest.mark.parametrize("C", sc.SIZES)
def test_the_whole_list_in_one_call(pair, C, order):
    m = pair(C, "ops")[0]
    refs = _yardstick(pair, C, "ops")
    lst = m.plugin_manager.layer_names + ["elevation"]
    names, got = m.get_grid_map_layers(lst, order=order)
    assert names == lst
    assert m.last_plugin_route == {n: ("host" if n == "hostp" else "device") for n in m.plugin_manager.layer_names}
    for k, n in enumerate(names):
        _check(m, n, got[k], refs[n], order, "%s in the list at %d" % (n, C))


@pytest.mark.parametrize("C", sc.SIZES)
def test_the_yardstick_can_tell_a_missing_step(pair, C):
    r = _yardstick(pair, C, "ops")
    differs = lambda a, b: not gc.same_bits(a, b).all()      # noqa: E731
    # one source: id 0 everywhere; two sources: ids 0 and 1, and entries 1 and 2 of the table share a colour
    assert r["cls_one"].tobytes() == r["cls_none"].tobytes() == r["cls_two"].tobytes()
    assert len({r[n].tobytes() for n in ("max_categories", "cls_none", "cls_mixed")}) == 3
    assert np.unique(r["max_categories"].view(np.uint32)).tolist() == [0x5171a2, 0xbc3f3b] and np.unique(r["cls_mixed"].view(np.uint32)).size >= 4
    assert np.unique(r["cls_none"].view(np.uint32)).tolist() == [0x5171a2]
    assert np.isin(r["trav_rce"], [np.float32(0.1), np.float32(1.0)]).all()
    if C > 10:                                                                  # (the 8 x 8 published cells of cell_n 10 may all get a vote)
        assert differs(r["trav_inexact"], r["trav_exact"]) and np.unique(r["trav_inexact"]).size == 2
    assert np.isnan(r["trav_inexact_le"]).any()                                  # fill_nan in the grid launch
    ml = [r["ml_%s_%s" % (v, mm)] for v in sc.ML_VARIANTS for mm in ("min", "max")]
    assert len({a.tobytes() for a in ml}) == 12 or C == 10                      # (64 cells may not tell every pair of variants apart)
    assert len({a.tobytes() for a in ml}) >= 6 and np.isnan(r["ml_none_max"]).any()
    for n in sc.PCA_PATTERNS:
        lv = sc.levels(r[n])                                # (a component's 0 and 255 may lie in the border row the publisher strips)
        assert all(np.unique(lv[..., ch]).size > 8 for ch in range(3)), n
        assert differs(r[n], r[n].T) and differs(r[n], r[n][::-1]) and differs(r[n], r[n][:, ::-1]), n
    assert differs(r["pca3"], r["pca5"]) and differs(r["pca16"], r["pca"])


# ---- 2. source counts: the table handed to the entry point directly ---------------------------------------------------------------------------------
def _direct(m, op_type, dst, srcs, flags=0):
    """one op through emap_plugin_chain_ex; srcs: (kind, index, flags, f0, f1, d0)"""
    from elevation_mapping_cupy_amd import _lib
    ops = (_lib.EmapPluginOp * 1)()
    ops[0].type, ops[0].dst_plane, ops[0].src_index, ops[0].i0, ops[0].flags = op_type, dst, 0, len(srcs), flags
    table = (_lib.EmapPluginSrc * max(1, len(srcs)))()
    for t, q in zip(table, srcs):
        t.kind, t.index, t.flags, t.reserved, t.f0, t.f1, t.d0 = q[0], q[1], q[2], 0, q[3], q[4], q[5]
    rc = m._lib.emap_plugin_chain_ex(m._ctx, ops, 1, None, table, len(srcs))
    assert rc == 0, m._lib.emap_last_error(m._ctx)
    return _plane(m, dst)


def _source_arrays(m, srcs):
    out = []
    for q in srcs:
        out.append(m.get_layer_raw(q[1]) if q[0] == 0 else _plane(m, q[1]) if q[0] == 1 else m.semantic_map.get_layer(q[1]))
    return out


@pytest.mark.parametrize("C", sc.SIZES)
def test_the_largest_and_the_smallest_source_counts(pair, C):
    m = pair(C, "ops")[0]
    pm = m.plugin_manager
    m.get_grid_map_layers(INPUTS)                                              # the planes the tables below read
    pm._upload(pm.layer_names.index("hostp"))
    dst = pm.layer_names.index("cls_none")
    k_sm, k_host = pm.layer_names.index("featp_smooth"), pm.layer_names.index("hostp")
    pool = [(0, 3), (1, k_sm), (2, 4), (2, 5), (2, 6), (0, 0), (1, k_host), (2, 1), (0, 4)]      # every kind; the class layers hold the NaN / zero cells
    rng = np.random.default_rng(C)
    pick = lambda n, of=pool: [of[i] for i in rng.integers(0, len(of), n)]      # noqa: E731
    for n in (0, 1, 2, 64):
        srcs = [(k, i, 0, 0.0, 0.0, 0.0) for k, i in pick(n)]
        got = _direct(m, 7, dst, srcs)
        assert gc.same_bits(got, sc.filter_restated(_source_arrays(m, srcs), (C, C))).all(), "filter of %d" % n
    for n in (1, 16):
        srcs = [(k, i, int(rng.integers(0, 2)), 0.0, 0.0, float(rng.choice([0.3, 0.5, 0.0, 1.0]))) for k, i in pick(n, [q for q in pool if q[0] != 2])]
        got = _direct(m, 8, dst, srcs)
        assert gc.same_bits(got, sc.trav_restated(_source_arrays(m, srcs), [q[5] for q in srcs], [q[2] & 1 for q in srcs])).all(), "votes of %d" % n
        for take_min in (0, 1):
            srcs = [(k, i, int(rng.integers(0, 16)) << 1, 0.25, float(rng.choice([0.7, -1.5])), float(rng.choice([0.3, 0.0]))) for k, i in pick(n)]
            got = _direct(m, 9, dst, srcs, flags=4 if take_min else 0)
            steps = [dict(default=q[3] if q[2] & 2 else None, reverse=bool(q[2] & 4), scale=q[4] if q[2] & 8 else None, threshold=q[5] if q[2] & 16 else None) for q in srcs]
            assert gc.same_bits(got, sc.max_layer_restated(_source_arrays(m, srcs), steps, bool(take_min))).all(), "layer %s of %d" % ("min" if take_min else "max", n)


# ---- 3. FEATURES_PCA ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", sc.SIZES)
def test_the_pca_is_repeatable_bit_for_bit(pair, C):
    m = pair(C, "ops")[0]
    m.get_grid_map_layers(INPUTS)
    lst = list(sc.PCA_PATTERNS)
    _, a = m.get_grid_map_layers(lst, order="message")
    planes_a = [_plane(m, m.plugin_manager.layer_names.index(n)) for n in lst]
    _, b = m.get_grid_map_layers(lst, order="message")
    planes_b = [_plane(m, m.plugin_manager.layer_names.index(n)) for n in lst]
    assert a.tobytes() == b.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(planes_a, planes_b))
    assert m.last_plugin_route == {n: "device" for n in lst}


def test_a_constant_feature_stack_gives_level_zero(tmp_path):
    C = 34
    m, t = sc.twins(C, sc.TURTLE, tmp_path / "p.yaml", constant_features=True)
    try:
        _, got = m.get_grid_map_layers(["pca"])
        assert m.last_plugin_route == {"pca": "device"}
        assert not got.view(np.uint32).any() and not _ref(t, "pca").view(np.uint32).any()
    finally:
        m.close(); t.close()


# ---- 4. routes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", sc.ORDERS)
@pytest.mark.parametrize("C", sc.SIZES)
def test_the_turtle_bot_list_runs_on_the_device(pair, C, order):
    m, t = pair(C, "turtle")
    m.get_grid_map_layers(sc.TURTLE_INPUTS)                                     # (the yardstick computed them on the twin: configuration order)
    names, got = m.get_grid_map_layers(sc.TURTLE_LIST, order=order)
    assert names == sc.TURTLE_LIST and m.last_plugin_route == {n: "device" for n in sc.TURTLE_SEMANTIC}
    refs = _yardstick(pair, C, "turtle")
    for k, n in enumerate(names):
        _check(m, n, got[k], refs[n], order, n)
    msg = m.get_grid_map_message(sc.TURTLE_FULL)                               # a host plugin (inpaint) between semantic ops
    assert msg.layers == sc.TURTLE_FULL and m.last_plugin_route["inpaint"] == "host"
    assert all(m.last_plugin_route[n] == "device" for n in sc.TURTLE_SEMANTIC + ["min_filter", "smooth"])
    for k, n in enumerate(msg.layers):
        _check(m, n, msg.data[k].data.reshape(C - 2, C - 2), refs[n] if n in refs else _ref(t, n), "message", n + " in the full list")


@pytest.mark.parametrize("C", sc.SIZES)
def test_the_declined_configurations_take_the_host_route_with_the_twins_values(pair, C):
    m, t = pair(C, "decline")
    for rounds in range(2):                                                   # (sem_self and ml_self read their own previous output)
        names, got = m.get_grid_map_layers(sc.DECLINED)
        assert names == sc.DECLINED and m.last_plugin_route == {n: "host" for n in sc.DECLINED}
        for k, n in enumerate(names):
            assert gc.same_bits(got[k], _ref(t, n)).all(), n
    assert not got[sc.DECLINED.index("trav_missing")].any()                    # the host route printed and left the layer as it was


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
import _semplug_cases as sc
from pathlib import Path
m = sc.twins(34, sc.TURTLE, Path(%r))[0]
m.get_grid_map_layers(sc.TURTLE_INPUTS)
names, got = m.get_grid_map_layers(sc.TURTLE_LIST, order="message")
np.save(%r, got)
print("ROUTE", sorted(m.last_plugin_route.items()))
m.close()
"""


def test_the_switch_sends_all_four_layers_to_the_host(pair, tmp_path):
    m = pair(34, "turtle")[0]
    m.get_grid_map_layers(sc.TURTLE_INPUTS)
    _, got = m.get_grid_map_layers(sc.TURTLE_LIST, order="message")
    assert m.last_plugin_route == {n: "device" for n in sc.TURTLE_SEMANTIC}
    env = dict(os.environ, EMAP_PLUGIN_RESIDENT="0", PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    code = _CHILD % (os.path.join(ROOT, "tests"), str(tmp_path / "child.yaml"), str(tmp_path / "child.npy"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    route = [ln for ln in out.stdout.splitlines() if ln.startswith("ROUTE")]
    assert route == ["ROUTE " + str([(n, "host") for n in sorted(sc.TURTLE_SEMANTIC)])]
    child = np.load(tmp_path / "child.npy")
    for k, n in enumerate(sc.TURTLE_LIST):
        _check(m, n, got[k], gc.message_plane(child[k]), "message", n + " against the host route of a fresh process")


# ---- 5. coherence ---------------------------------------------------------------------------------------------------------------------------------
def test_host_writes_and_host_reads_around_the_chain(tmp_path):
    C = 34
    m, t = sc.twins(C, sc.ops_config(C), tmp_path / "p.yaml")
    try:
        pm, pt = m.plugin_manager, t.plugin_manager
        k = pm.layer_names.index("featp_smooth")
        m.get_grid_map_layers(INPUTS + ["cls_mixed", "ml_host"])
        for n in INPUTS + ["cls_mixed", "ml_host"]:
            _ref(t, n)
        # a host write through pm.layers into a plane semantic ops read: it goes up before the op runs
        mark = np.random.default_rng(3).uniform(-1, 2, (C, C)).astype(np.float32)
        pm.layers[k][...] = mark
        pt.layers[k][...] = mark
        for n in ("cls_mixed", "pca3", "trav_inexact"):
            _, got = m.get_grid_map_layers([n])
            assert m.last_plugin_route == {n: "device"}
            _check(m, n, got[0], _ref(t, n), "rows", n + " after a host write into its source")
        assert gc.same_bits(_plane(m, k), mark).all()
        # the host reads what the device left: get_map_with_name, layers, and the host route of a reader
        assert gc.same_bits(pm.get_map_with_name("cls_mixed"), pt.get_map_with_name("cls_mixed")).all()
        m.get_grid_map_layers(["max_categories", "trav_inexact_le"])
        _ref(t, "max_categories"); _ref(t, "trav_inexact_le")
        for n in ("max_categories", "trav_inexact_le", "trav_inexact"):
            assert gc.same_bits(pm.layers[pm.layer_names.index(n)], pt.layers[pt.layer_names.index(n)]).all(), n
        # get_map_with_name_ref of a semantic-plugin layer after the chain: the host route runs again, on the same inputs
        m.get_grid_map_layers(["ml_all_max", "cls_two"])
        for n in ("ml_all_max", "cls_two"):
            assert gc.same_bits(_ref(m, n), _ref(t, n)).all(), n
    finally:
        m.close(); t.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_map_the_semantic_planes_and_the_resident_planes_as_they_were(tmp_path):
    from elevation_mapping_cupy_amd import _lib
    C = 34
    m, t = sc.twins(C, sc.TURTLE, tmp_path / "p.yaml")
    try:
        lib, ctx = m._lib, m._ctx
        m.get_grid_map_layers(sc.TURTLE_LIST)                                  # eight planes reserved
        n_sem, n_planes = len(m.semantic_map.layer_names), 8

        def state():
            planes = np.stack([_plane(m, k) for k in range(n_planes)])
            return m.elevation_map.tobytes() + m.normal_map.tobytes() + m.semantic_map.semantic_map.tobytes() + planes.tobytes()
        s0 = state()

        def chain(ops, srcs, n_srcs=None, null_srcs=False, plain=False):
            table = (_lib.EmapPluginOp * max(1, len(ops)))()
            for t_, o in zip(table, ops):
                t_.type, t_.dst_plane, t_.src_kind, t_.src_index, t_.i0, t_.i1, t_.flags, t_.f0 = o
            side = (_lib.EmapPluginSrc * max(1, len(srcs)))()
            for s_, q in zip(side, srcs):
                s_.kind, s_.index, s_.flags, s_.reserved = q[:4]
                s_.d0 = 0.5
            if plain:
                return lib.emap_plugin_chain(ctx, table, len(ops), None)
            return lib.emap_plugin_chain_ex(ctx, table, len(ops), None, None if null_srcs else side, len(srcs) if n_srcs is None else n_srcs)

        sem3 = [(2, 4, 0, 0), (2, 5, 0, 0), (2, 6, 0, 0)]
        op = lambda type_, n, first=0, dst=4, i1=0, flags=0: (type_, dst, 0, first, n, i1, flags, 0.0)      # noqa: E731
        cases = {
            "run beyond the table": dict(ops=[op(7, 4)], srcs=sem3), "run starts beyond": dict(ops=[op(7, 1, first=3)], srcs=sem3), "run starts at -1": dict(ops=[op(7, 1, first=-1)], srcs=sem3),
            "a second op's run beyond": dict(ops=[op(7, 3), op(9, 2, first=2, dst=7)], srcs=sem3),
            "filter of 65": dict(ops=[op(7, 65)], srcs=sem3 * 22), "votes of 0": dict(ops=[op(8, 0, dst=5)], srcs=sem3), "votes of 17": dict(ops=[op(8, 17, dst=5)], srcs=[(0, 3, 0, 0)] * 17),
            "layer max of 0": dict(ops=[op(9, 0, dst=7)], srcs=sem3), "layer max of 17": dict(ops=[op(9, 17, dst=7)], srcs=sem3 * 6),
            "pca of 2": dict(ops=[op(10, 2, dst=6)], srcs=sem3), "pca of 17": dict(ops=[op(10, 17, dst=6)], srcs=sem3 * 6), "count -1": dict(ops=[op(7, -1)], srcs=sem3),
            "semantic layer beyond": dict(ops=[op(7, 1)], srcs=[(2, n_sem, 0, 0)]), "semantic layer -1": dict(ops=[op(7, 1)], srcs=[(2, -1, 0, 0)]),
            "plane beyond": dict(ops=[op(7, 1)], srcs=[(1, n_planes, 0, 0)]), "plane -1": dict(ops=[op(9, 1, dst=7)], srcs=[(1, -1, 0, 0)]), "map layer 7": dict(ops=[op(7, 1)], srcs=[(0, 7, 0, 0)]),
            "its own plane": dict(ops=[op(7, 2)], srcs=[(2, 4, 0, 0), (1, 4, 0, 0)]), "kind 3": dict(ops=[op(7, 1)], srcs=[(3, 0, 0, 0)]), "kind -1": dict(ops=[op(9, 1, dst=7)], srcs=[(-1, 0, 0, 0)]),
            "a semantic layer votes": dict(ops=[op(8, 1, dst=5)], srcs=[(2, 4, 0, 0)]),
            "a flag on a filter source": dict(ops=[op(7, 1)], srcs=[(2, 4, 1, 0)]), "a layer-max flag on a vote": dict(ops=[op(8, 1, dst=5)], srcs=[(0, 3, 2, 0)]),
            "flag 32": dict(ops=[op(9, 1, dst=7)], srcs=[(0, 3, 32, 0)]), "AT_MOST on the layer max": dict(ops=[op(9, 1, dst=7)], srcs=[(0, 3, 1, 0)]), "a flag on a pca source": dict(ops=[op(10, 3, dst=6)], srcs=[(2, 7, 0, 0), (2, 8, 4, 0), (2, 9, 0, 0)]),
            "reserved": dict(ops=[op(7, 1)], srcs=[(2, 4, 0, 1)]), "i1": dict(ops=[op(7, 3, i1=1)], srcs=sem3), "MIN on the filter": dict(ops=[op(7, 3, flags=4)], srcs=sem3),
            "REVERSE on the layer max": dict(ops=[op(9, 3, dst=7, flags=1)], srcs=sem3), "null table": dict(ops=[op(7, 3)], srcs=sem3, null_srcs=True),
            "n_srcs 2049": dict(ops=[op(7, 3)], srcs=sem3, n_srcs=2049), "n_srcs -1": dict(ops=[op(7, 0)], srcs=sem3, n_srcs=-1), "dst beyond": dict(ops=[op(7, 3, dst=n_planes)], srcs=sem3),
            "type 5": dict(ops=[op(5, 0)], srcs=sem3), "type 11": dict(ops=[op(11, 3)], srcs=sem3), "a bad op behind a good one": dict(ops=[op(7, 3), op(10, 2, dst=6)], srcs=sem3),
        }
        for what, kw in cases.items():
            assert chain(**kw) == -1, what
            assert b"emap_plugin_chain" in lib.emap_last_error(ctx), what
        for type_ in (7, 8, 9, 10):                                            # the plain call names the one that takes the table
            assert chain([op(type_, 3)], sem3, plain=True) == -1 and b"emap_plugin_chain_ex" in lib.emap_last_error(ctx), type_
        assert state() == s0
        # and the context still works: the good calls go through and leave what the twin's host route leaves
        assert chain([op(7, 3), op(7, 0, dst=7)], sem3) == 0 and chain([op(7, 0, dst=7)], [], null_srcs=True) == 0
        _ref(t, "max_categories")
        assert gc.same_bits(_plane(m, 4), t.plugin_manager.host_layer("max_categories")).all()
        assert np.unique(_plane(m, 7).view(np.uint32)).tolist() == [0x5171a2]
        names, got = m.get_grid_map_layers(sc.TURTLE_LIST)
        for k, n in enumerate(names):
            _check(m, n, got[k], _ref(t, n), "rows", n + " after the refusals")
    finally:
        m.close(); t.close()


def test_a_strip_context_is_refused():
    from elevation_mapping_cupy_amd import _lib
    m = gc.start(34, strip=(0, 17, 0))
    try:
        ops, srcs = (_lib.EmapPluginOp * 1)(), (_lib.EmapPluginSrc * 1)()
        ops[0].type = 7
        assert m._lib.emap_plugin_chain_ex(m._ctx, ops, 1, None, srcs, 0) == -1 and b"single-strip" in m._lib.emap_last_error(m._ctx)
    finally:
        m.close()


# ---- 7. frames and shifts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", sc.ORDERS)
def test_the_ops_see_a_fresh_frame_and_a_move(order, tmp_path):
    C = 67
    m, t = sc.twins(C, sc.TURTLE, tmp_path / "p.yaml")
    try:
        R, tr = fx.POSES["identity"]
        seen = []
        for step in range(3):
            if step == 1:                                                      # a frame with semantic channels
                for x in (m, t):
                    x.input_pointcloud(gc.semantic_frame(C, 3000, 7), gc.CHANNELS, R, tr.copy() + x.center, 0.0, 0.0)
            if step == 2:                                                      # a move: the class and feature layers shift with the map
                for x in (m, t):
                    x.move_to(x.center + np.array([-0.12, 0.08, 0.0]), np.eye(3, dtype=np.float32))
                    x.base_rotation = pc.TILT.copy()
            names, got = m.get_grid_map_layers(sc.TURTLE_LIST, order=order)
            assert m.last_plugin_route == {n: "device" for n in sc.TURTLE_SEMANTIC}
            for k, n in enumerate(names):
                _check(m, n, got[k], _ref(t, n), order, "%s at step %d" % (n, step))
            seen.append(got.copy())
        for k, n in enumerate(sc.TURTLE_LIST):
            if n != "semantic_traversability":                                 # (its two votes may well cover the same cells before and after a frame)
                assert not gc.same_bits(seen[1][k], seen[2][k]).all(), n
        assert not gc.same_bits(seen[0][sc.TURTLE_LIST.index("elevation")], seen[1][sc.TURTLE_LIST.index("elevation")]).all()
    finally:
        m.close(); t.close()
