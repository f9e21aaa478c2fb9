"""GPU: the planar regions on the device (emap_planar_regions / csrc/emap_regions.hip; ElevationMap.get_planar_regions, trace_mask).
The yardstick is the host model (elevation_mapping_cupy_amd/planar_regions.py, checked on the CPU by
tests/test_planar_region_cases.py): the counts, every ring record and every vertex compared bit for bit, the poison behind each output
buffer intact.  The scenes and sizes are those of tests/_planar_region_cases.py; end to end the scenes of tests/_planar_terrain_cases.py
on a map in the start state of tests/_grid_cases.py.  No test provokes a fault: every refusal happens before a launch.  Reference:
ContourExtraction.cpp:28-128, Upsampling.cpp:12-68, PlanarRegion.cpp:5-50."""
import ctypes as ct

import numpy as np
import pytest

import _grid_cases as gc
import _plane_seg_cases as pc
import _planar_region_cases as rc
import _planar_terrain_cases as tc
from elevation_mapping_cupy_amd import planar_regions as pr

pytestmark = pytest.mark.gpu
POISON = 0x5A5A5A5A
_maps = {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_shared_maps():
    yield
    for m in _maps.values():
        m.close()
    _maps.clear()


def _shared(C=34):
    if C not in _maps:
        _maps[C] = gc.start(C)
    return _maps[C]


def _raw(m, labels, n_labels=1, mode=0, margin_size=1, cap_r=None, cap_v=None, null=(), side=None):
    """the C call on buffers of exactly the capacities, poison behind them: (rc, rings, vertices, n_rings, n_vertices, untouched)"""
    from elevation_mapping_cupy_amd import _lib
    P = _lib.EmapRegionParams(mode, margin_size)
    if labels is not None:
        labels = np.ascontiguousarray(labels, np.int32)
    side = (0 if labels is None else labels.shape[0]) if side is None else side
    cap_r = 4096 if cap_r is None else cap_r
    cap_v = 32768 if cap_v is None else cap_v
    rings, verts = np.full((max(cap_r, 0) + 2) * 8, POISON, np.uint32), np.full((max(cap_v, 0) + 2) * 2, POISON, np.uint32)
    n_r, n_v = ct.c_int64(-7), ct.c_int64(-7)
    rc_ = m._lib.emap_planar_regions(m._ctx, None if labels is None else labels.ctypes.data_as(ct.POINTER(ct.c_int32)), side, n_labels, None if "params" in null else ct.byref(P),
                                     None if "rings" in null else rings.ctypes.data_as(ct.POINTER(_lib.EmapRegionRing)), cap_r,
                                     None if "vertices" in null else verts.ctypes.data_as(ct.POINTER(ct.c_int32)), cap_v,
                                     None if "n_rings" in null else ct.byref(n_r), None if "n_vertices" in null else ct.byref(n_v))
    untouched = bool((rings == POISON).all() and (verts == POISON).all() and n_r.value == -7 and n_v.value == -7)
    return rc_, rings, verts, n_r.value, n_v.value, untouched


def _check(m, labels, n_labels, mode, margin, what):
    want = pr.trace_labels(labels, n_labels, margin, mode)
    nr, nv = len(want.rings), len(want.vertices)
    rc_, rings, verts, n_r, n_v, _ = _raw(m, labels, n_labels, mode, margin, cap_r=nr, cap_v=nv)      # exactly what the answer needs
    assert rc_ == 0, (what, m._lib.emap_last_error(m._ctx))
    assert (n_r, n_v) == (nr, nv), (what, n_r, n_v, nr, nv)
    assert (rings[8 * nr:] == POISON).all() and (verts[2 * nv:] == POISON).all(), what      # the poison behind each buffer
    got_r, got_v = rings[:8 * nr].view(pr.RING_DTYPE), verts[:2 * nv].view(np.int32).reshape(nv, 2)
    for f in pr.RING_DTYPE.names:
        assert (got_r[f] == want.rings[f]).all(), "%s: ring field %s, first at %s" % (what, f, np.flatnonzero(got_r[f] != want.rings[f])[:3].tolist())
    assert (got_v == want.vertices).all(), "%s: %d vertices differ, first at %s" % (what, int((got_v != want.vertices).any(axis=1).sum()),
                                                                                  np.flatnonzero((got_v != want.vertices).any(axis=1))[:3].tolist())
    return want


@pytest.mark.parametrize("M", rc.LABEL_SIZES)
def test_every_label_scene_and_margin(M):
    """U = 22, 34, 97, 193, 364: one tile, a tile border, ragged tiles, the crack mask and the pixel masks past one scan trip"""
    m = _shared()
    for name, (L, n) in rc.label_scenes(M).items():
        for margin in (rc.MARGINS if M <= 65 else (1,)):
            want = _check(m, L, n, 0, margin, "%s at %d, margin %d" % (name, M, margin))
            if name == "lines" and margin == 1:
                assert [g["label"] for g in pr.assemble(want.rings, want.vertices)] == [2]      # one cell wide: no region; two: by the fallback
            if name == "empty":
                assert len(want.rings) == 0


@pytest.mark.parametrize("M", rc.RAW_SIZES)
def test_every_mask_of_the_raw_mode(M):
    m = _shared()
    for name, X in rc.raw_scenes(M).items():
        want = _check(m, X, 1, 1, 0, "%s at %d" % (name, M))
        if name == "spiral":
            assert int((want.rings["image"] == 0).sum()) == 1 and want.rings["n_vertices"][0] > M      # ONE border, every doubling round
        if name == "checkerboard":
            assert int((want.rings["image"] == 0).sum()) > (M - 2) * (M - 2) // 2      # one component, a hole ring per inner background pixel
    got = m.trace_mask(rc.raw_scenes(33)["staircases"])
    want = pr.trace_labels(rc.raw_scenes(33)["staircases"], 1, 0, 1)
    assert m.last_planar_regions_route == "device" and rc.same_answer(got, want) and len(got.polygons) == len(pr.assemble(want.rings, want.vertices))


def _write(m, h):
    C = m.cell_n
    valid = ~np.isnan(h)
    m.set_layer_raw("elevation", pc.logical_plane(np.where(valid, h, np.float32(0.0)), C))
    m.set_layer_raw("is_valid", pc.logical_plane(valid, C))


@pytest.mark.parametrize("C", (34, 67))
def test_end_to_end_on_the_terrain_scenes(C, monkeypatch):
    """get_planar_regions = the model on get_planar_terrain's labels; the resident labels = the same labels uploaded; the plane
    coordinates = the host route's words"""
    m = _shared(C)
    for name in ("pieces", "hills"):
        h, over = tc.scenes(C - 2)[name]
        _write(m, h)
        P = pc.params(**over)
        for margin in (1, 0):
            t = m.get_planar_terrain(preprocess={}, **P)
            got = m.get_planar_regions(preprocess={}, margin_size=margin, **P)
            assert m.last_planar_regions_route == "device" and m.last_planar_terrain_route == "device", name
            assert got.labels.tobytes() == t.labels.tobytes() and got.planes.tobytes() == t.planes.tobytes() and tc.same_words(got.smooth_planar, t.smooth_planar)
            want = pr.trace_labels(t.labels, t.n_labels, margin, 0)
            assert rc.same_answer(got, want), (name, margin, len(got.rings), len(want.rings))
            rc_, rings, verts, n_r, n_v, _ = _raw(m, None, 0, 0, margin)                       # the labels the call above left on the context
            up = _raw(m, t.labels, t.n_labels, 0, margin)
            assert rc_ == 0 and up[0] == 0 and (n_r, n_v) == (len(want.rings), len(want.vertices)) and (rings == up[1]).all() and (verts == up[2]).all()
            monkeypatch.setenv("EMAP_REGIONS_RESIDENT", "0")
            host = m.get_planar_regions(preprocess={}, margin_size=margin, **P)
            monkeypatch.delenv("EMAP_REGIONS_RESIDENT")
            assert m.last_planar_regions_route == "host" and rc.same_answer(host, got) and len(host.regions) == len(got.regions)
            labels_seen = [g.label for g in got.regions]
            assert labels_seen == sorted(labels_seen) and set(labels_seen) <= set(int(x) for x in t.planes["label"])
            for a, b in zip(got.regions, host.regions):
                assert a.label == b.label and a.bbox2d == b.bbox2d and tc.same_words(a.transform_plane_to_world, b.transform_plane_to_world)
                assert tc.same_words(a.boundary["outer_plane"], b.boundary["outer_plane"]) and len(a.insets) == len(b.insets) >= 1
                for x, y in zip(a.insets, b.insets):
                    assert tc.same_words(x["outer_plane"], y["outer_plane"]) and (x["outer"] == y["outer"]).all()
        if name == "pieces":
            assert len(got.regions) >= 2


def test_refusals_leave_the_outputs_untouched():
    from elevation_mapping_cupy_amd._lib import EmapError
    m = gc.start(34)
    try:
        L = rc.label_scenes(12)["ring with an island"][0]
        rc_, _, _, _, _, untouched = _raw(m, None)
        assert rc_ == -1 and untouched and b"no valid resident labels" in m._lib.emap_last_error(m._ctx)      # no segmentation yet
        _write(m, tc.scenes(32)["terraces"][0])
        m.get_planar_terrain()
        assert _raw(m, None)[0] == 0
        assert _raw(m, None, side=32)[0] == 0 and _raw(m, None, side=12)[0] == -1
        m.clear()
        rc_, _, _, _, _, untouched = _raw(m, None)
        assert rc_ == -1 and untouched and b"no valid resident labels" in m._lib.emap_last_error(m._ctx)      # ... and none after clear()
        cases = {"null params": dict(null=("params",)), "null n_rings": dict(null=("n_rings",)), "null n_vertices": dict(null=("n_vertices",)),
                 "null rings with a capacity": dict(null=("rings",)), "null vertices with a capacity": dict(null=("vertices",)),
                 "mode 2": dict(mode=2), "mode -1": dict(mode=-1), "margin 15": dict(margin_size=15), "margin -1": dict(margin_size=-1),
                 "negative ring capacity": dict(cap_r=-1), "negative vertex capacity": dict(cap_v=-1), "a label beyond n_labels": dict(n_labels=1),
                 "negative n_labels": dict(n_labels=-1), "a mask with a 2": dict(mode=1), "side 1": dict(side=1), "side 0 with labels": dict(side=0),
                 "a side beyond the cap": dict(side=7725)}
        for what, kw in cases.items():
            rc_, _, _, _, _, untouched = _raw(m, L, **dict(dict(n_labels=2), **kw))
            assert rc_ == -1 and untouched, what
            assert b"emap_planar_regions" in m._lib.emap_last_error(m._ctx), what
        rc_, rings, verts, n_r, n_v, _ = _raw(m, L, 2, cap_r=1)      # a capacity too small: the counts are reported, nothing else is written
        want = pr.trace_labels(L, 2, 1)
        assert rc_ == -1 and (n_r, n_v) == (len(want.rings), len(want.vertices)) and n_r > 1 and (rings == POISON).all() and (verts == POISON).all()
        rc_, rings, verts, n_r, n_v, _ = _raw(m, L, 2, cap_v=3)
        assert rc_ == -1 and (n_r, n_v) == (len(want.rings), len(want.vertices)) and (rings == POISON).all() and (verts == POISON).all()
        assert _raw(m, L, 2)[0] == 0
        for bad in (dict(margin_size=15), dict(margin_size=-1), dict(kernel_size=4)):
            with pytest.raises(ValueError):
                m.get_planar_regions(**bad)
        for bad in (np.full((4, 4), 2), np.zeros((1, 1)), np.zeros((3, 4))):
            with pytest.raises(ValueError):
                m.trace_mask(bad)
    finally:
        m.close()
    m = gc.start(34, strip=(0, 17, 0))
    try:
        rc_, _, _, _, _, untouched = _raw(m, rc.label_scenes(12)["full"][0])
        assert rc_ == -1 and untouched and b"single-strip" in m._lib.emap_last_error(m._ctx)
        with pytest.raises(EmapError):
            m.get_planar_regions()
        with pytest.raises(EmapError):
            m.trace_mask(np.ones((4, 4), np.int32))
    finally:
        m.close()
