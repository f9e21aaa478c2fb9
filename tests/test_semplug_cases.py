"""CPU: the Python side of the semantic plugins on resident planes (SemanticFilter, SemanticTraversability, MaxLayerFilter, FeaturesPca as
ops of emap_plugin_chain_ex) -- the side table plugin_chain_plan lays out, every configuration a plugin declines, the upload rule of
PluginManager.run_plan against a stub library, the NumPy restatement of each op's arithmetic (tests/_semplug_cases.py) against the
plugin's own __call__ bit for bit, the PCA condition, and the C ABI as far as a machine without a device goes."""
import ctypes as ct
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _grid_cases as gc
import _plug_cases as pc
import _semplug_cases as sc
from conftest import ROOT

C = 34
SEM = ["s0", "s1", "c0", "rgb"] + sc.SEM_NAMES + sc.FEAT_NAMES
HEADER = os.path.join(ROOT, "include", "emap_hip.h")


class _Lib:
    """records every call; a chain as (function, [(type, dst_plane, src_index, i0)], [(kind, index, flags)])"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, fn):
        def call(ctx, *a):
            if fn == "emap_plugin_chain":
                self.calls.append((fn, [(a[0][k].type, a[0][k].dst_plane, a[0][k].src_index, a[0][k].i0) for k in range(a[1])], []))
            elif fn == "emap_plugin_chain_ex":
                self.calls.append((fn, [(a[0][k].type, a[0][k].dst_plane, a[0][k].src_index, a[0][k].i0) for k in range(a[1])],
                                   [(a[3][k].kind, a[3][k].index, a[3][k].flags) for k in range(a[4])]))
            else:
                self.calls.append((fn, a[0]))
            return 0
        return call


class _Emap:
    def __init__(self):
        self._lib, self._ctx, self.cell_n, self.resolution = _Lib(), None, C, 0.04

    def _chk(self, rc):
        assert rc == 0


def _plan(entries, names, resident=True, sem=SEM):
    from elevation_mapping_cupy_amd.plugins.plugin_manager import plugin_chain_plan
    pm = pc.manager(entries, C, _Emap())
    return plugin_chain_plan(names, pm.plugins, pm.layer_names, sc.LAYERS, sem, resident=resident), pm


def _srcs(op):
    return [(q["kind"], q["index"], q["flags"]) for q in op["srcs"]]


# ---- plans ------------------------------------------------------------------------------------------------------------------------------
def test_the_turtle_bot_list_is_one_chain_with_a_side_table():
    from elevation_mapping_cupy_amd import _lib
    from elevation_mapping_cupy_amd.plugins.plugin_manager import side_table
    steps, pm = _plan(sc.TURTLE, sc.TURTLE_LIST)
    assert [(s[0], s[1]) for s in steps] == [("device", n) for n in sc.TURTLE_SEMANTIC]
    ops = [s[2] for s in steps]
    assert [o["type"] for o in ops] == [7, 10, 8, 9] and [o["dst_plane"] for o in ops] == [4, 6, 5, 7]
    # the runs lie one behind the other in plan order: 3 class layers, 16 features, 2 vote layers, 3 layers of the maximum
    assert [(o["src_index"], o["i0"]) for o in ops] == [(0, 3), (3, 16), (19, 2), (21, 3)] and all(o["i1"] == 0 and o["f0"] == 0.0 for o in ops)
    table = side_table(steps)
    assert len(table) == 24 and table[3:19] == ops[1]["srcs"]
    S, P, L = _lib.PLUGIN_SRC_SEMANTIC, _lib.PLUGIN_SRC_PLANE, _lib.PLUGIN_SRC_LAYER
    assert _srcs(ops[0]) == [(S, 4, 0), (S, 5, 0), (S, 6, 0)]
    assert _srcs(ops[1]) == [(S, 7 + f, 0) for f in range(16)]
    assert _srcs(ops[2]) == [(L, 3, _lib.PLUGIN_SRC_AT_MOST), (P, 3, 0)] and [q["d0"] for q in ops[2]["srcs"]] == [0.3, 0.5]
    Z, R, X, T = _lib.PLUGIN_SRC_ZERO_DEFAULT, _lib.PLUGIN_SRC_REVERSE, _lib.PLUGIN_SRC_SCALE, _lib.PLUGIN_SRC_THRESHOLD
    assert _srcs(ops[3]) == [(L, 3, Z | R | X), (S, 4, Z | X | T), (P, 5, Z | X)] and ops[3]["flags"] == 0
    assert [(q["f0"], q["f1"], q["d0"]) for q in ops[3]["srcs"]] == [(0.0, 1.0, 0.0), (0.0, 1.0, 0.5), (0.0, 1.0, 0.0)]
    steps, _ = _plan(sc.TURTLE, sc.TURTLE_LIST, resident=False)
    assert steps == [("host", n) for n in sc.TURTLE_SEMANTIC]


def test_the_source_order_is_map_layers_plugin_layers_semantic_layers():
    from elevation_mapping_cupy_amd import _lib
    steps, pm = _plan(sc.ops_config(C), ["cls_mixed", "pca16", "cls_none"])
    k = pm.layer_names.index("featp_smooth")
    S, P, L = _lib.PLUGIN_SRC_SEMANTIC, _lib.PLUGIN_SRC_PLANE, _lib.PLUGIN_SRC_LAYER
    assert _srcs(steps[0][2]) == [(L, 3, 0), (P, k, 0), (S, 4, 0), (S, 5, 0), (S, 6, 0)]
    assert _srcs(steps[1][2]) == [(L, 0, 0), (P, k, 0)] + [(S, 7 + f, 0) for f in range(14)]
    assert steps[2][2]["i0"] == 0 and steps[2][2]["srcs"] == [] and steps[2][2]["src_index"] == 5 + 16
    mm = _plan(sc.ops_config(C), ["ml_all_min", "ml_all_max", "ml_host"])[0]
    assert mm[0][2]["flags"] == _lib.PLUGIN_MIN and mm[1][2]["flags"] == 0
    assert [q["flags"] for q in mm[0][2]["srcs"]] == [2 | 4 | 8 | 16, 2 | 4 | 8, 2 | 8 | 16]
    assert _srcs(mm[2][2]) == [(P, pm.layer_names.index("hostp"), 0), (S, 5, 0)]       # the missing layer is skipped, as on the host


def test_every_op_of_the_gpu_cases_is_a_device_op_and_every_decline_case_is_not():
    entries = sc.ops_config(C)
    steps, _ = _plan(entries, pc.names_of(entries))
    assert [s[0] for s in steps] == ["device", "host"] + ["device"] * (len(entries) - 2)
    entries = sc.decline_config(C)
    steps, pm = _plan(entries, pc.names_of(entries))
    assert steps == [("host", n) for n in sc.DECLINED] and pc.names_of(entries) == sc.DECLINED
    for p, n in zip(pm.plugins, sc.DECLINED):
        own = n in ("sem_self", "ml_self")              # (these two describe an op; the plan declines it: a source is the op's own plane)
        assert (p.device_op(sc.LAYERS, pm.layer_names, SEM) is None) != own, n


def test_more_sources_than_an_op_takes_and_a_plane_beyond_the_32():
    many = ["cls_%02d" % k for k in range(65)]
    e = [pc._entry("semantic_filter", "f64", classes=["^cls_([0-5][0-9]|6[0-3])$"]), pc._entry("semantic_filter", "f65", classes=["^cls_.*$"]),
         pc._entry("semantic_traversability", "v17", layers=["time"] * 17, thresholds=[1.0] * 17, type=["x"] * 17),
         pc._entry("semantic_traversability", "v16", layers=["time"] * 16, thresholds=[1.0] * 16, type=["x"] * 16),
         pc._entry("max_layer_filter", "m17", layers=["time"] * 17, reverse=[False] * 17, thresholds=[False] * 17, scales=[1], default_value=0)]
    steps, _ = _plan(e, pc.names_of(e), sem=many)
    assert [(s[0], s[1]) for s in steps] == [("device", "f64"), ("host", "f65"), ("host", "v17"), ("device", "v16"), ("host", "m17")]
    assert steps[0][2]["i0"] == 64 and steps[3][2]["src_index"] == 64 and steps[3][2]["i0"] == 16
    # plugin layer 32 and beyond has no plane: neither as a destination nor as a source
    e = [pc._entry("smooth_filter", "p%02d" % k, input_layer_name="elevation") for k in range(33)]
    e.insert(5, pc._entry("max_layer_filter", "reads_33", layers=["p31", "time"], reverse=[False] * 2, thresholds=[False] * 2, scales=[1], default_value=0))
    e.append(pc._entry("semantic_filter", "beyond", classes=["^time$"]))
    steps, pm = _plan(e, ["reads_33", "beyond"])
    assert pm.layer_names.index("p31") == 32 and steps == [("host", "reads_33"), ("host", "beyond")]


def test_plugin_inputs_name_the_plugin_layers_the_host_route_reads():
    e = sc.ops_config(C)
    pm = pc.manager(e, C, _Emap())
    inp = {n: p.plugin_inputs(pm.layer_names) for n, p in zip(pm.layer_names, pm.plugins)}
    assert inp["max_categories"] == [] and inp["cls_mixed"] == ["featp_smooth"] and inp["trav_rce"] == ["robot_centric_elevation"]
    assert inp["ml_host"] == ["hostp"] and inp["pca3"] == ["featp_smooth"] and inp["pca"] == []
    d = pc.manager(sc.decline_config(C), C, _Emap())
    assert d.plugins[3].plugin_inputs(d.layer_names) is None            # a layer-name default: whatever it names


def test_run_plan_uploads_every_host_newer_plane_a_semantic_op_reads():
    e = sc.ops_config(C)
    pm = pc.manager(e, C, _Emap())
    lib = pm.emap._lib
    names = pm.layer_names
    k_sm, k_host, k_rce = names.index("featp_smooth"), names.index("hostp"), names.index("robot_centric_elevation")
    from elevation_mapping_cupy_amd.plugins.plugin_manager import plugin_chain_plan
    ran = []

    def host_step(n):
        ran.append(n)
        pm._newer[names.index(n)] = "host"

    def run(lst):
        del lib.calls[:]
        steps = plugin_chain_plan(lst, pm.plugins, names, sc.LAYERS, SEM)
        return pm.run_plan(steps, host_step)
    # a fresh manager: nothing to upload; the smooth and the op that reads it share one chain, which is the _ex call
    assert run(["featp_smooth", "cls_mixed"]) == {"featp_smooth": "device", "cls_mixed": "device"}
    assert [c[0] for c in lib.calls] == ["emap_plugin_planes", "emap_plugin_chain_ex"]
    assert lib.calls[1][1] == [(2, k_sm, 0, 0), (7, names.index("cls_mixed"), 0, 5)] and len(lib.calls[1][2]) == 5
    # a chain without a semantic op stays the plain call
    run(["featp_smooth"])
    assert [c[0] for c in lib.calls] == ["emap_plugin_chain"]
    # host-newer planes named by ANY source go up (ml_host reads hostp as its first source, cls_mixed featp_smooth as its second), each once
    pm._newer[k_sm] = pm._newer[k_host] = "host"
    run(["ml_host", "cls_mixed", "pca3"])
    assert lib.calls[:3] == [("emap_plugin_plane_write", k_host), ("emap_plugin_chain_ex", [(9, names.index("ml_host"), 0, 2)], [(1, k_host, 0), (2, 5, 0)]),
                             ("emap_plugin_plane_write", k_sm)]
    assert lib.calls[3][0] == "emap_plugin_chain_ex" and [o[0] for o in lib.calls[3][1]] == [7, 10] and len(lib.calls) == 4
    assert [(o[2], o[3]) for o in lib.calls[3][1]] == [(0, 5), (5, 3)]          # the runs are re-based to the chain's own table
    # a plane a pending op writes is NOT uploaded over, although the host array is marked newer
    pm._newer[k_rce] = "host"
    run(["robot_centric_elevation", "trav_rce"])
    assert [c[0] for c in lib.calls] == ["emap_plugin_chain_ex"] and pm._newer[k_rce] == "device"
    # the host plugin in between reads no plane of the chain, so the chain waits; the upload of ITS plane for the op behind it enqueues the chain first
    run(["max_categories", "hostp", "ml_host"])
    assert ran == ["hostp"] and [c[0] for c in lib.calls] == ["emap_plugin_chain_ex", "emap_plugin_plane_write", "emap_plugin_chain_ex"] and lib.calls[1][1] == k_host
    assert [o[0] for o in lib.calls[0][1]] == [7] and [o[0] for o in lib.calls[2][1]] == [9]


# ---- the arithmetic: the restatement against the plugins' own __call__ --------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    """layers in the layout a plugin receives: (7, C, C) map layers, the plugin layers of ops_config, the semantic layers"""
    rng = np.random.default_rng(5)
    emap = rng.uniform(-0.4, 0.6, (7, C, C)).astype(np.float32)
    emap[2] = (rng.uniform(0, 1, (C, C)) > 0.3).astype(np.float32)
    emap[3] = sc.traversability_layer(C)
    emap[4] = rng.integers(0, 6, (C, C)).astype(np.float32)
    entries = sc.ops_config(C)
    pm = pc.manager(entries, C, _Emap())
    plug = np.zeros((len(pm.plugins), C, C), np.float32)
    plug[pm.layer_names.index("featp_smooth")] = pc.box3_twice(emap[0])
    plug[pm.layer_names.index("hostp")] = rng.uniform(-0.4, 0.6, (C, C)).astype(np.float32)
    plug[pm.layer_names.index("hostp")][3, 4:7] = (0.0, -0.0, np.nan)
    plug[pm.layer_names.index("robot_centric_elevation")] = rng.uniform(0, 1, (C, C)).astype(np.float32)
    sem = np.concatenate([rng.uniform(0, 1, (4, C, C)).astype(np.float32), sc.class_layers(C), sc.feature_layers(C)], axis=0)
    for a in (emap, plug, sem):
        a.setflags(write=False)
    return emap, plug, sem, pm


def _host(pm, name, emap, plug, sem):
    p = pm.plugins[pm.layer_names.index(name)]
    return np.asarray(p(emap, sc.LAYERS, plug, pm.layer_names, sem, SEM), np.float32)


def _restated(pm, name, emap, plug, sem):
    from elevation_mapping_cupy_amd import _lib
    op = pm.plugins[pm.layer_names.index(name)].device_op(sc.LAYERS, pm.layer_names, SEM)
    arrays = [(emap, plug, sem)[q["kind"]][q["index"]] for q in op["srcs"]]
    if op["type"] == "semantic_filter":
        return sc.filter_restated(arrays, (C, C))
    if op["type"] == "semantic_trav":
        return sc.trav_restated(arrays, [q["d0"] for q in op["srcs"]], [q["flags"] & _lib.PLUGIN_SRC_AT_MOST for q in op["srcs"]])
    if op["type"] == "max_layer":
        steps = [dict(default=q["f0"] if q["flags"] & _lib.PLUGIN_SRC_ZERO_DEFAULT else None, reverse=bool(q["flags"] & _lib.PLUGIN_SRC_REVERSE),
                      scale=q["f1"] if q["flags"] & _lib.PLUGIN_SRC_SCALE else None, threshold=q["d0"] if q["flags"] & _lib.PLUGIN_SRC_THRESHOLD else None)
                 for q in op["srcs"]]
        return sc.max_layer_restated(arrays, steps, bool(op["flags"] & _lib.PLUGIN_MIN))
    return sc.pca_restated(arrays)


def test_the_colour_dealing_is_the_plugins_table():
    from elevation_mapping_cupy_amd.plugins.semantic_filter import SemanticFilter
    enc = SemanticFilter().color_encoding.view(np.uint32)
    assert (sc.colour_of(np.arange(1, 256)) == enc).all()
    assert [hex(int(v)) for v in sc.colour_of(np.array([1, 2, 3]))] == ["0x5171a2", "0x5171a2", "0xbc3f3b"]


def test_the_pointwise_restatements_leave_the_plugins_bits(inputs):
    emap, plug, sem, pm = inputs
    names = [n for n, p in zip(pm.layer_names, pm.plugin_names) if p in ("semantic_filter", "semantic_traversability", "max_layer_filter")]
    assert len(names) == 5 + 4 + 13
    for n in names:
        host, mine = _host(pm, n, emap, plug, sem), _restated(pm, n, emap, plug, sem)
        ok = gc.same_bits(host, mine)
        assert ok.all(), "%s: %d cells differ, first at %s" % (n, int((~ok).sum()), tuple(np.argwhere(~ok)[0]))
    # the cases do what they are there for: ties, both zeros, NaN in every position; 0.3f is above 0.3; a NaN result; a zero's sign
    cls = sc.class_layers(C)
    r = C // 2
    ids = np.argmax(cls, axis=0)
    assert list(ids[r, 2:6]) == [0, 0, 0, 1] and list(ids[r + 1, 2:6]) == [0, 1, 2, 0]
    t = emap[3]
    le, ge = _host(pm, "trav_inexact_le", emap, plug, sem), sc.trav_restated([t], [0.3], [False])
    at = t == np.float32(0.3)
    assert at.any() and (le[at] == np.float32(0.1)).all() and (ge[at] == 1.0).all() and np.isnan(t).any() and (le[np.isnan(t)] == np.float32(0.1)).all()
    none_max, none_min = _host(pm, "ml_none_max", emap, plug, sem), _host(pm, "ml_none_min", emap, plug, sem)
    assert np.isnan(none_max).any() and (np.isnan(none_max) == np.isnan(none_min)).all() and not gc.same_bits(none_max, none_min).all()
    assert len({_host(pm, "ml_%s_%s" % (v, mm), emap, plug, sem).tobytes() for v in sc.ML_VARIANTS for mm in ("min", "max")}) == 12


def test_the_later_of_two_equal_zeros_is_kept():
    z = np.zeros((C, C), np.float32)
    for a, b in ((z, -z), (-z, z)):
        for take_min in (False, True):
            host = np.stack([a, b]).min(axis=0) if take_min else np.stack([a, b]).max(axis=0)
            mine = sc.max_layer_restated([a, b], [{}, {}], take_min)
            assert gc.same_bits(host, mine).all() and (np.signbit(mine) == np.signbit(b)).all()
    mixed = np.stack([np.where(z > 1, 1, 0), -z])          # int64 beside float32: float64, and -0 survives the way back to float32
    assert mixed.dtype == np.float64 and np.signbit(mixed.max(axis=0).astype(np.float32)).all()


@pytest.mark.parametrize("name", list(sc.PCA_PATTERNS))
def test_the_pca_restatement_meets_the_pca_condition_against_the_plugin(inputs, name):
    emap, plug, sem, pm = inputs
    host, mine = _host(pm, name, emap, plug, sem), _restated(pm, name, emap, plug, sem)
    sc.pca_condition(mine, host, name)
    lv = sc.levels(host)
    assert all(lv[..., ch].min() == 0 and lv[..., ch].max() == 255 for ch in range(3)), "every component spans its range"


@pytest.mark.parametrize("cell_n", sc.SIZES)
@pytest.mark.parametrize("F", [3, 5, 16])
def test_the_feature_layers_have_a_separated_spectrum(F, cell_n):
    """adjacent leading eigenvalues a factor of 1.65 apart: an eigenvector moves by about eps / (relative gap) under a perturbation of
    eps, so two correct solvers agree to 1e-15 and a level flips only where a score lies that close to a level's edge"""
    feat = sc.feature_layers(cell_n)
    assert np.abs(feat[0]).max() > 1.0                      # the first feature exceeds the clip
    assert min(sc.eigen_ratios(feat[:F])) >= 1.65, sc.eigen_ratios(feat[:F])


def test_pca3_agrees_with_scikit_learn_when_it_is_installed():
    decomposition = pytest.importorskip("sklearn.decomposition")
    from elevation_mapping_cupy_amd.plugins.features_pca import _pca3
    x = np.clip(sc.feature_layers(C).reshape(16, -1).T, -1, 1).astype(np.float64)
    for F in (3, 5, 16):
        want = decomposition.PCA(n_components=3).fit_transform(x[:, :F])
        assert np.abs(_pca3(x[:, :F]) - want).max() < 1e-12


def test_a_constant_stack_gives_level_zero():
    feat = np.broadcast_to((np.arange(16, dtype=np.float32) / np.float32(8) - np.float32(0.5))[:, None, None], (16, C, C))
    from elevation_mapping_cupy_amd.plugins.features_pca import FeaturesPca
    host = FeaturesPca(process_layer_names=["^feat_.*$"])(np.zeros((7, C, C), np.float32), sc.LAYERS, np.zeros((0, C, C), np.float32), [], feat, sc.FEAT_NAMES)
    assert not host.view(np.uint32).any() and not sc.pca_restated(feat).view(np.uint32).any()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_the_side_table_record_and_the_constants_have_the_headers_values():
    from elevation_mapping_cupy_amd import _lib
    h = open(HEADER).read()
    body = re.search(r"typedef struct emap_plugin_src \{(.*?)\} emap_plugin_src;", h, flags=re.S).group(1)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    cls = _lib.EmapPluginSrc
    names = [f[0] for f in cls._fields_]
    assert names == fields == ["kind", "index", "flags", "reserved", "f0", "f1", "d0"]
    consts = ["EMAP_PLUGIN_SEMANTIC_FILTER", "EMAP_PLUGIN_SEMANTIC_TRAV", "EMAP_PLUGIN_MAX_LAYER", "EMAP_PLUGIN_FEATURES_PCA", "EMAP_PLUGIN_SRC_LAYER",
              "EMAP_PLUGIN_SRC_PLANE", "EMAP_PLUGIN_SRC_SEMANTIC", "EMAP_PLUGIN_MIN", "EMAP_PLUGIN_SRC_AT_MOST", "EMAP_PLUGIN_SRC_ZERO_DEFAULT",
              "EMAP_PLUGIN_SRC_REVERSE", "EMAP_PLUGIN_SRC_SCALE", "EMAP_PLUGIN_SRC_THRESHOLD", "EMAP_PLUGIN_MAX_SRCS", "EMAP_PLUGIN_INPAINT_FRONTS", "EMAP_ABI_VERSION"]
    lines = ['printf("%zu %zu", sizeof(emap_plugin_src), sizeof(emap_plugin_op));'] + ['printf(" %%zu", offsetof(emap_plugin_src, %s));' % n for n in names]
    lines += ['printf("\\n");', 'printf("%s\\n", %s);' % (" ".join(["%d"] * len(consts)), ", ".join(consts))]
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write('#include "emap_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert [int(x) for x in out[0].split()] == [ct.sizeof(cls), ct.sizeof(_lib.EmapPluginOp)] + [getattr(cls, n).offset for n in names] == [32, 32, 0, 4, 8, 12, 16, 20, 24]
    P = dict(_lib.PLUGIN_OPS, **_lib.PLUGIN_OPS_EX)
    assert [int(x) for x in out[1].split()] == [P["semantic_filter"], P["semantic_trav"], P["max_layer"], P["features_pca"], _lib.PLUGIN_SRC_LAYER, _lib.PLUGIN_SRC_PLANE,
                                                _lib.PLUGIN_SRC_SEMANTIC, _lib.PLUGIN_MIN, _lib.PLUGIN_SRC_AT_MOST, _lib.PLUGIN_SRC_ZERO_DEFAULT, _lib.PLUGIN_SRC_REVERSE,
                                                _lib.PLUGIN_SRC_SCALE, _lib.PLUGIN_SRC_THRESHOLD, _lib.PLUGIN_MAX_SRCS, P["inpaint_fronts"], _lib.ABI_VERSION] \
        == [7, 8, 9, 10, 0, 1, 2, 4, 1, 2, 4, 8, 16, 2048, 6, 3]
    assert 5 not in P.values() and sorted(_lib.PLUGIN_SRC_LIMITS.items()) == [(7, (0, 64)), (8, (1, 16)), (9, (1, 16)), (10, (3, 16))]


def test_the_entry_point_is_declared_exported_bound_and_refuses_a_null_context():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "emap_plugin_chain_ex" in _lib.SYMBOLS and hasattr(lib, "emap_plugin_chain_ex") and len(lib.emap_plugin_chain_ex.argtypes) == 6
    assert re.search(r"\bint emap_plugin_chain_ex\(emap_ctx\* ctx, const emap_plugin_op\* ops, int32_t n_ops, const float\* rotation9, "
                     r"const emap_plugin_src\* srcs, int32_t n_srcs\);", h)
    ops, srcs = (_lib.EmapPluginOp * 1)(), (_lib.EmapPluginSrc * 1)()
    ops[0].type = 7
    assert lib.emap_plugin_chain_ex(None, ops, 1, None, srcs, 1) == -1 and lib.emap_plugin_chain_ex(None, None, 0, None, None, 0) == -1
    assert lib.emap_abi_version() == 3 and "#define EMAP_ABI_VERSION 3" in h
