"""CPU: the inpainting op of the plugin chain (EMAP_PLUGIN_INPAINT_FRONTS) as far as a machine without a device goes -- the plan
plugin_chain_plan builds for the filter publisher with method "telea_fronts", PluginManager's coherence bookkeeping against a stub
library that records its calls, the constant in the header (compiled as C) and in the binding, the NumPy restatement of the plugin's
arithmetic around the fill (tests/_inpaint_chain_cases.py) against plugins/inpainting.py's own, and the preconditions of the GPU case
table counted on its states."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _inpaint_chain_cases as ic
import _plug_cases as pc
import _telea_fronts as tf
from conftest import ROOT

LAYERS = ["elevation", "variance", "is_valid", "traversability", "time", "upper_bound", "is_upper_bound"]
SEM = ["s0", "s1", "c0", "rgb"]
C = 12


class _Lib:
    """records (function, plane or op table) of every call; emap_plugin_plane_read fills the host array with 100 + plane"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, fn):
        def call(ctx, *a):
            if fn == "emap_plugin_chain":
                self.calls.append((fn, [(a[0][k].type, a[0][k].dst_plane, a[0][k].i0, a[0][k].i1, a[0][k].flags) for k in range(a[1])]))
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


# ---- plan -------------------------------------------------------------------------------------------------------------------------------
def test_the_filter_publisher_with_telea_fronts_is_three_device_steps():
    steps, pm = _plan(ic.CORE_FRONTS, pc.FILTER_PUBLISHER)
    assert _brief(steps) == [("device", "min_filter", 0, 0, 0, 0, 1, 30, 0), ("device", "smooth", 2, 1, 1, 0, 0, 0, 0), ("device", "inpaint", 6, 2, 0, 0, 0, 0, 0)]
    assert steps[2][2]["f0"] == 0.0 and pm.plugins[2].plugin_inputs(pm.layer_names) == ()
    steps, _ = _plan(ic.ops_config(), ["inp_s4", "inp_11", "inp_s16"])
    assert [(s[2]["type"], s[2]["dst_plane"], s[2]["i0"]) for s in steps] == [(6, 5, 4), (6, 3, 0), (6, 6, 16)]


def test_the_default_method_keeps_the_plan_of_today():
    steps, _ = _plan(pc.CORE, pc.FILTER_PUBLISHER)
    assert _brief(steps) == [("device", "min_filter", 0, 0, 0, 0, 1, 30, 0), ("device", "smooth", 2, 1, 1, 0, 0, 0, 0), ("host", "inpaint")]
    from elevation_mapping_cupy_amd.plugins.inpainting import Inpainting
    assert Inpainting().method == "telea"
    for method in ("telea", "ns", "front", "no such name"):
        assert Inpainting(method=method).device_op(LAYERS, [], SEM) is None, method
    assert Inpainting(method="telea_fronts").device_op(LAYERS, [], SEM) == dict(type="inpaint_fronts", src=None, i0=0)
    assert Inpainting(method="telea_fronts", steps=4).device_op(LAYERS, [], SEM) == dict(type="inpaint_fronts", src=None, i0=4)


def test_the_switch_sends_everything_to_the_host():
    steps, _ = _plan(ic.CORE_FRONTS, pc.FILTER_PUBLISHER, resident=False)
    assert steps == [("host", "min_filter"), ("host", "smooth"), ("host", "inpaint")]


# ---- coherence --------------------------------------------------------------------------------------------------------------------------
def test_the_device_inpaint_moves_no_plane_until_the_host_asks():
    e = _Emap()
    steps, pm = _plan(ic.CORE_FRONTS, pc.FILTER_PUBLISHER, emap=e)
    pm.plugins[2].fronts_run = 7
    route = pm.run_plan(steps, lambda n: pytest.fail("no host plugin in this list"))
    assert route == {"min_filter": "device", "smooth": "device", "inpaint": "device"}
    assert e._lib.calls == [("emap_plugin_planes", 4), ("emap_plugin_chain", [(0, 0, 1, 30, 0), (2, 1, 0, 0, 0), (6, 2, 0, 0, 0)])]      # ONE chain, no upload, no download
    assert pm._newer[2] == "device" and pm.plugins[2].fronts_run is None       # nothing waited for the largest front
    del e._lib.calls[:]
    assert (pm.host_layer("inpaint") == 102).all()
    assert e._lib.calls == [("emap_plugin_plane_read", 2)] and pm._newer[2] is None      # exactly one download, of that plane
    pm.host_layer("inpaint")
    assert e._lib.calls == [("emap_plugin_plane_read", 2)]
    del e._lib.calls[:]
    pm.run_plan([s for s in steps if s[1] == "inpaint"], None)      # the op alone: it reads the map, never a plane
    assert e._lib.calls == [("emap_plugin_chain", [(6, 2, 0, 0, 0)])] and pm._newer[2] == "device"


# ---- header and binding -----------------------------------------------------------------------------------------------------------------
def test_the_constant_is_6_in_the_header_and_in_the_binding():
    from elevation_mapping_cupy_amd import _lib
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write('#include "emap_hip.h"\n#include <stdio.h>\nint main(void) { printf("%d %d %d\\n", EMAP_PLUGIN_INPAINT_FRONTS, EMAP_PLUGIN_ROBOT_CENTRIC, '
                             'EMAP_ABI_VERSION); return 0; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert [int(x) for x in out] == [6, 4, 3]
    assert _lib.PLUGIN_OPS["inpaint_fronts"] == 6 and 5 not in _lib.PLUGIN_OPS.values() and _lib.ABI_VERSION == 3
    assert sorted(_lib.PLUGIN_OPS.values()) == [0, 1, 2, 3, 4, 6]


# ---- the arithmetic around the fill --------------------------------------------------------------------------------------------------------
class _IdentityFill:
    """libemap_hip.so as far as Inpainting(method="telea") uses it, the fill replaced by the identity"""

    @staticmethod
    def emap_inpaint_telea_u8(img, mask, rows, cols, radius, out):
        assert radius == 1
        np.ctypeslib.as_array(out, (rows, cols))[...] = np.ctypeslib.as_array(img, (rows, cols))
        return 0


def test_the_restated_arithmetic_is_the_plugins(monkeypatch):
    from elevation_mapping_cupy_amd import _lib
    from elevation_mapping_cupy_amd.plugins.inpainting import Inpainting
    monkeypatch.setattr(_lib, "load", lambda: _IdentityFill)
    flat = 0
    for what, (h, valid) in ic.range_layers(C).items():
        planes = np.zeros((7, C, C), np.float32); planes[0], planes[2] = h, valid
        want = Inpainting(cell_n=C, method="telea")(planes, LAYERS, np.zeros((0, C, C), np.float32), [])
        got = ic.inpaint_plane(h, valid, fill=lambda q8, mask: q8)
        flat += ic.inpaint_range(h, valid) is None
        assert got.dtype == np.float32 and (np.asarray(want, np.float32) == want).all(), what      # float64 holding float32 values
        assert pc.gc.same_bits(got, np.asarray(want, np.float32)).all(), what
    assert flat == 2                                                   # no known cell, every cell known
    L = ic.range_layers(C)
    assert ic.inpaint_range(*L["constant"])[1] == 1.0 and ic.inpaint_range(*L["zeros only"])[1] == 1.0      # the span rule
    lo, span = ic.inpaint_range(*L["negative"])
    assert lo < 0 and ic.inpaint_quantise(L["negative"][0], lo, span)[ic.known_of(L["negative"][1])].max() == 255
    q = ic.inpaint_quantise(L["clip"][0], *ic.inpaint_range(*L["clip"]))
    assert q[0, 1] == 255 and q[5, 5] == 0                             # unknown cells beyond the known range are clipped, not wrapped
    k = ic.known_of(L["half"][1])
    assert k[2, 2] and not k[3, 3]                                     # >= 0.5


# ---- preconditions of the GPU case table ---------------------------------------------------------------------------------------------------
def _asymmetric(a):
    same = pc.gc.same_bits
    return not same(a, a.T).all() and not same(a, a[::-1]).all() and not same(a, a[:, ::-1]).all()


def _state(size, case):
    if case == "start":
        e = pc.oracle_start(size).elevation_map
        return np.asarray(e[0], np.float32), np.asarray(e[2], np.float32)
    return ic.case_planes(size, case)


@pytest.mark.parametrize("size", ic.SIZES)
def test_the_case_table_can_tell_a_missing_step(size):
    deep = 0
    for case in ic.HOLED:
        h, valid = _state(size, case)
        k = ic.known_of(valid)
        assert 0 < int(k.sum()) < k.size, case                         # unknown cells and known cells
        d = tf.distance(~k)
        deep += int(d.max()) > 16                                      # more than one launch does work at the default S
        lo, span = ic.inpaint_range(h, valid)
        q8 = ic.inpaint_quantise(h, lo, span)
        out8 = tf.inpaint_fronts(q8, (~k).astype(np.uint8))
        assert (out8 != q8).any() and (out8[k] == q8[k]).all(), case   # filled != input, and only in the hole
        plane = ic.inpaint_plane(h, valid)
        assert _asymmetric(plane) and _asymmetric(plane[1:-1, 1:-1]), case
        assert not pc.gc.same_bits(plane, h).all(), case               # de-quantised: not the elevation either
    assert deep >= 1 or size < 34
    hole = ~ic.known_of(ic.case_planes(size, "block")[1])
    assert hole[0].any() and hole[-1].any() and hole[:, -1].any()      # the hole touches the border
    assert (ic.case_planes(size, "block")[1] == 0.5).sum() == 1        # one cell that is known here and invalid for fill_nan
    for case in ic.DEGENERATE[1:]:
        h, valid = ic.case_planes(size, case)
        if case == "all_valid":
            assert ic.inpaint_range(h, valid) is None
        else:
            k = ic.known_of(valid)
            assert 0 < int(k.sum()) < k.size and ic.inpaint_range(h, valid)[1] == 1.0 and np.unique(ic.inpaint_plane(h, valid)).size == 1


def test_the_corner_case_reaches_the_geometric_bound():
    """one known cell in a corner: max d = rows + cols - 2, so the last front belongs to the last launch of ceil((2 C - 2) / S); a chain
    with one launch less leaves the input value in the far corner, which is not the filled one"""
    size = 34
    h, valid = ic.case_planes(size, "corner")
    k = ic.known_of(valid)
    d = tf.distance(~k)
    assert int(k.sum()) == 1 and int(d.max()) == 2 * size - 2 == 66 and d[0, size - 1] == 66
    assert -(-66 // 16) == 5 and 4 * 16 < 65                           # fronts 65 and 66 are the fifth launch's alone
    lo, span = ic.inpaint_range(h, valid)
    q8 = ic.inpaint_quantise(h, lo, span)
    out8 = tf.inpaint_fronts(q8, (~k).astype(np.uint8))
    assert span == 1.0 and out8[0, size - 1] != q8[0, size - 1] and out8[1, size - 1] != q8[1, size - 1]
