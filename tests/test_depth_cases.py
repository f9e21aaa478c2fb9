"""CPU: the depth-image input's case table, scene and bindings (tests/_depth_cases.py; the GPU side is tests/test_hip_depth.py).

The table must reach every k_depth_cloud instantiation, every uniform branch of its channel record and every alignment class; the
scene must hold every invalid kind and still feed the frame: these are conditions on the INPUTS of the GPU tests, checked where no GPU
is needed.  The bindings are checked as far as a machine without a device allows."""
import ctypes as ct
from collections import Counter

import numpy as np
import pytest

import _depth_cases as dc
from oracle import emap_oracle as eo

BIG = [c for c in dc.CASES if dc.n_rows(c) >= 64]


def test_the_table_reaches_every_instantiation_branch_and_alignment_class():
    inst = Counter(dc.instantiation(c) for c in dc.CASES)
    assert set(inst) == {(dt, cf, q) for dt in (0, 1) for cf in (False, True) for q in (False, True)}, inst
    assert all(v >= 2 for v in inst.values()), inst
    quad = [c for c in dc.CASES if c["step"] == 1]
    n4 = Counter(dc.n_rows(c) % 4 for c in quad)
    assert set(n4) == {0, 1, 2, 3}, n4                      # the scalar tail of the four-row lanes: absent, 1, 2, 3 rows
    assert any(dc.n_rows(c) < 4 for c in quad) and any(dc.n_rows(c) > 4 * 256 for c in quad)      # the tail alone; more than one workgroup
    assert any(c["W"] % 4 for c in quad if dc.n_rows(c) >= 8)      # a group of four spans a row end
    k4 = Counter(dc.kc(c) % 4 for c in dc.CASES)
    assert set(k4) == {0, 1, 2, 3}, k4
    assert {dc.kc(c) for c in dc.CASES} >= {0, 1, 3, 4, 5, 16}
    # the record's branches: none, colour alone, features alone, both; 16-byte stores with and without colour, in both lane shapes
    assert {(c["rgb"], c["K"] > 0) for c in dc.CASES} == {(False, False), (True, False), (False, True), (True, True)}
    assert {(c["step"] == 1, c["rgb"]) for c in dc.CASES if dc.kc(c) and dc.kc(c) % 4 == 0} == {(True, True), (False, True), (False, False)}
    assert {c["step"] for c in dc.CASES} == {1, 2, 3, 7} and any(c["step"] > max(c["H"], c["W"]) for c in dc.CASES)
    assert {(c["H"], c["W"]) for c in dc.CASES} >= {(1, 1), (1, 7), (5, 1), (3, 5), (4, 4), (17, 31), (64, 64), (60, 80), (480, 640)}
    assert len({dc.case_key(c) for c in dc.CASES}) == len(dc.CASES)


def test_the_restatement_on_a_hand_computed_image():
    f32 = np.float32
    depth = np.array([[1.0, 0.0, 2.0], [np.nan, 8.0, 0.5]], f32)
    desc = dict(fx=2.0, fy=4.0, cx=0.5, cy=0.25, step=1)
    xyz, chan = dc.backproject(desc, depth, rgb=np.array([[[1, 2, 3]] * 3] * 2, np.uint8))
    assert xyz.shape == (6, 3) and chan.shape == (6, 1)
    assert np.array_equal(xyz[0], f32([-0.25, -0.0625, 1.0])) and np.array_equal(xyz[2], f32([1.5, -0.125, 2.0])) and np.array_equal(xyz[5], f32([0.375, 0.09375, 0.5]))
    for i in (1, 3, 4):                                      # 0, NaN, == max_depth
        assert (xyz[i].view(np.uint32) == 0x7FC00000).all()
    assert (chan.view(np.uint32) == 0x010203).all()
    raw = np.array([[1000, 0, 9000]], np.uint16)
    xyz, _ = dc.backproject(dict(desc, depth_scale=0.001), raw)
    assert xyz[0, 2] == f32(1000) * f32(0.001) and np.isnan(xyz[1:]).all()
    xyz, _ = dc.backproject(dict(desc, step=2), depth)       # rows 0; columns 0, 2
    assert xyz.shape == (2, 3) and xyz[1, 2] == 2.0
    xyz, _ = dc.backproject(dict(desc, confidence_threshold=0.5), depth, confidence=np.array([[0.5, 1, np.nan], [1, 1, 0.4]], f32))
    assert np.isnan(xyz[:, 2]).tolist() == [False, True, True, True, True, True]


@pytest.mark.parametrize("c", BIG, ids=dc.case_key)
def test_the_scene_holds_every_invalid_kind_and_still_feeds_the_frame(c):
    s = dc.scene(c)
    step = c["step"]
    xyz, chan = dc.restated(s)
    n = dc.n_rows(c)
    assert xyz.shape == (n, 3) and chan.shape == (n, dc.kc(c))
    kind = s["kind"][::step, ::step].reshape(-1)
    ok = ~np.isnan(xyz[:, 2])
    for k in dc.kinds_of(c):
        hit = kind == dc.KINDS.index(k) + 1
        assert hit.any() and not ok[hit].any(), k           # the kind occurs among the SAMPLED pixels, and the contract rejects it
    assert ok[kind == 0].all()
    assert ok.sum() * 2 >= n, (ok.sum(), n)
    # every row of a pixel is NaN in all three columns or in none, with the contract's bit pattern
    bits = xyz.view(np.uint32)
    assert ((bits == 0x7FC00000).all(axis=1) == ~ok).all() and np.isfinite(xyz[ok]).all()
    # the oracle's frame on the restated cloud fuses at least half the pixels (every valid point lies within 1 m of the map centre)
    t = dc.CAM_T.copy()
    p_map = xyz[ok] @ dc.CAM_R.T + t
    assert np.abs(p_map[:, :2]).max() < 1.0
    C = 66 if max(c["H"], c["W"]) <= 64 or (c["H"], c["W"]) == (60, 80) else 258
    om = eo.OracleMap(eo.make_params(eo.YAML, cell_n=C))
    cloud = np.ascontiguousarray(np.concatenate([xyz, chan], axis=1))
    om.update_map_with_kernel(cloud, dc.CAM_R, t, 0.0, 0.0)
    fused = int(om.last["cnt"].sum())
    assert fused * 2 >= n, (fused, n)
    if c["K"]:                                               # cases with feature channels: the fusion set of semantic_yaml66
        names = dc.channel_names(c)
        col = {nm: 3 + i for i, nm in enumerate(names)}
        avg = [nm for nm in names if dc.CHANNEL_FUSIONS.get(nm, dc.CHANNEL_FUSIONS["default"]) == "average"]
        cls = [nm for nm in names if dc.CHANNEL_FUSIONS.get(nm) == "class_average"]
        rgb = [nm for nm in names if dc.CHANNEL_FUSIONS.get(nm) == "color"]
        layers = {nm: i for i, nm in enumerate(avg + cls + rgb)}
        om.semantic_update(cloud, dc.CAM_R, t, average=[(col[a], layers[a]) for a in avg], class_average=[(col[a], layers[a]) for a in cls],
                           color=[(col[a], layers[a]) for a in rgb], n_layers=len(layers), alpha=0.5)
        touched = om.last["cnt"] > 0
        assert touched.sum() > 16
        for a in avg + rgb:
            assert (om.semantic_map[layers[a]][touched].view(np.uint32) != 0).mean() > 0.9, a


def test_the_60x80_image_is_mapped_on_the_small_map():
    """(the rule above in words: images up to 64 x 64 and the robot-scale 60 x 80 one go to the 66^2 map, 480 x 640 to 258^2)"""
    assert {(c["H"], c["W"]) for c in BIG} == {(17, 31), (64, 64), (60, 80), (480, 640)}


# ---- bindings, as far as a machine without a device goes ----------------------------------------------------------------------------
def test_both_entry_points_are_bound_and_exported():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    for s in ("emap_bind_depth_image", "emap_get_bound_points"):
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    assert ct.sizeof(_lib.EmapDepthDesc) == 56
    assert [f[0] for f in _lib.EmapDepthDesc._fields_] == ["height", "width", "depth_dtype", "step", "has_rgb", "n_features", "fx", "fy", "cx", "cy",
                                                            "depth_scale", "min_depth", "max_depth", "confidence_threshold"]


def test_a_null_context_is_refused_without_a_device():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    d = _lib.EmapDepthDesc(4, 4, 0, 1, 0, 0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 8.0, 0.0)
    img = np.ones((4, 4), np.float32)
    n = ct.c_int64(-7)
    assert lib.emap_bind_depth_image(None, ct.byref(d), ct.c_void_p(img.ctypes.data), None, None, None, ct.byref(n)) == -1 and n.value == -7
    out = np.zeros((16, 3), np.float32)
    assert lib.emap_get_bound_points(None, ct.c_void_p(out.ctypes.data), None) == -1 and not out.any()


def test_the_compat_package_offers_the_same_class():
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        from elevation_mapping_cupy.elevation_mapping import ElevationMap as Compat
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))
    for m in ("bind_depth_image", "input_depth_image", "bound_points"):
        assert callable(getattr(Compat, m))
