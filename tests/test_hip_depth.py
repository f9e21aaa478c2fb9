"""GPU: depth-image input (emap_bind_depth_image / k_depth_cloud, csrc/emap_depth.hip).  The cloud the device back-projects from a
depth camera's images equals the NumPy restatement of the contract (tests/_depth_cases.py) BIT FOR BIT, for every case of the table --
every kernel instantiation, lane shape, tail and record width -- and a frame fed through input_depth_image leaves the map a frame fed
the restated cloud through input_pointcloud leaves, on every frame path (reference: the sensor package's host back-projection,
pointcloud_node.py:205-250, 261-269, in front of input_pointcloud, EM/elevation_mapping.py:434-466)."""
import ctypes as ct

import numpy as np
import pytest

import _depth_cases as dc
from _util import assert_planes_equal, make_parameter
from oracle import emap_oracle as eo

pytestmark = pytest.mark.gpu
NO_RAYS = dict(eo.YAML, enable_visibility_cleanup=False)
NORMALS = ["nx", "ny", "nz"]
_cache = {}


def _scene(c):
    """scene and restated cloud of a case: computed once, shared, never written to"""
    k = dc.case_key(c)
    if k not in _cache:
        s = dc.scene(c)
        xyz, chan = dc.restated(s)
        for a in (xyz, chan, s["depth"]):
            a.setflags(write=False)
        _cache[k] = (s, xyz, chan)
    return _cache[k]


def _map(C, cfg=NO_RAYS):
    from elevation_mapping_cupy_amd.elevation_mapping import ElevationMap
    m = ElevationMap(make_parameter(cfg, C))
    m.param.pointcloud_channel_fusions = dict(dc.CHANNEL_FUSIONS)
    return m


@pytest.fixture(scope="module")
def small_map():
    m = _map(66)
    yield m
    m.close()


def _case(H, W, step=1, **kw):
    got = [c for c in dc.CASES if (c["H"], c["W"], c["step"]) == (H, W, step) and all(c[k] == v for k, v in kw.items())]
    assert len(got) == 1, (H, W, step, kw)
    return got[0]


def _same_bytes(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (what, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        bad = np.argwhere(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32))
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d values differ bitwise, first at %s: %r vs %r" % (what, len(bad), a.size, i, a[i], b[i]))


# ---- 1. cloud bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", dc.CASES, ids=dc.case_key)
def test_the_bound_cloud_is_the_restated_cloud_bit_for_bit(c, small_map):
    s, xyz, chan = _scene(c)
    n = small_map.bind_depth_image(s["depth"], s["K"], **dc.keywords(s))
    assert n == dc.n_rows(c) == xyz.shape[0]
    got_xyz, got_chan = small_map.bound_points()
    _same_bytes(got_xyz, xyz, "xyz")
    _same_bytes(got_chan, chan, "channels")


# ---- 2. frame equality ---------------------------------------------------------------------------------------------------------------
def _frames(c, k):
    """frame k of a three-frame walk: the scene seen from a camera that has moved with the map, the surface a little closer each time"""
    s, _, _ = _scene(c)
    s = dict(s)
    depth = s["depth"].copy()
    depth[s["kind"] == 0] -= np.uint16(15 * k) if c["u16"] else np.float32(0.015 * k)      # (the seeded invalid patches stay what they are)
    s["depth"] = depth
    xyz, chan = dc.restated(s)
    pos = np.array([0.08 * k, -0.12 * k, 0.0], np.float32)
    return s, np.ascontiguousarray(np.concatenate([xyz, chan], axis=1)), pos


def _equal_maps(a, b, what):
    assert_planes_equal(a.elevation_map, b.elevation_map, what=what)
    assert_planes_equal(a.normal_map, b.normal_map, names=NORMALS, what=what + " normals")
    assert a.traversability_input.tobytes() == b.traversability_input.tobytes(), what + " traversability_input"
    if a.semantic_map.layer_names:
        assert a.semantic_map.layer_names == b.semantic_map.layer_names
        assert_planes_equal(a.semantic_map.semantic_map, b.semantic_map.semantic_map, names=a.semantic_map.layer_names, what=what + " semantic")


def _walk(c, C, cfg, scatter, path, semantics=None):
    a, b = _map(C, cfg), _map(C, cfg)
    names = dc.channel_names(c)
    try:
        for m in (a, b):
            m.set_scatter_mode(scatter)
        for k in range(3):
            s, cloud, pos = _frames(c, k)
            noise = 0.0 if k == 0 else 1.0
            for m in (a, b):
                m.move_to(pos, np.eye(3, dtype=np.float32))
            t = dc.CAM_T + pos
            a.input_depth_image(s["depth"], s["K"], names, dc.CAM_R, t.copy(), noise, noise, **dc.keywords(s))
            b.input_pointcloud(cloud, ["x", "y", "z"] + names, dc.CAM_R, t.copy(), noise, noise)
            assert a.last_update_path() == b.last_update_path() == path, (k, a.last_update_path(), b.last_update_path())
            if semantics:
                assert a.last_frame_semantics() == b.last_frame_semantics() and a.last_frame_semantics() in semantics, (k, a.last_frame_semantics(), b.last_frame_semantics())
            for m in (a, b):
                m.update_time()
            _equal_maps(a, b, "frame %d" % k)
        assert int((a.elevation_map[2] > 0.5).sum()) > 200      # the frames did fuse
        if names:
            assert int((a.semantic_map.semantic_map != 0).sum()) > 200
    finally:
        a.close(); b.close()


def test_robot_scale_frames_take_the_one_launch_path():
    _walk(_case(60, 80, 1), 66, NO_RAYS, "auto", "small_frame")


@pytest.mark.parametrize("rays", [False, True])
@pytest.mark.parametrize("scatter", ["auto", "binned"])
def test_vga_frames_on_the_tile_path(scatter, rays):
    """307200 rows are beyond the atomic path's share of scatter mode auto: both settings sort by tile"""
    _walk(_case(480, 640, 1, K=0), 258, eo.YAML if rays else NO_RAYS, scatter, "binned")


def test_vga_frames_carry_colour_and_three_features_through_the_frame():
    _walk(_case(480, 640, 1, K=3), 258, NO_RAYS, "binned", "binned", semantics=("in_tile_pass", "carried"))      # (32-byte records either way; which: by the frame's heavy tiles)


def test_small_frames_with_channels_run_the_stand_alone_semantic_kernels():
    _walk(_case(64, 64, 1), 66, NO_RAYS, "auto", "atomic", semantics=("separate",))


# ---- 3. uint16 against float32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [_case(17, 31, 2), _case(480, 640, 1, K=3)], ids=dc.case_key)
def test_uint16_depth_equals_the_float_image_of_one_multiply(c, small_map):
    s, _, _ = _scene(c)
    assert s["depth"].dtype == np.uint16
    kw = dc.keywords(s)
    small_map.bind_depth_image(s["depth"], s["K"], **kw)
    want = small_map.bound_points()
    as_float = s["depth"].astype(np.float32) * np.float32(dc.DEPTH_SCALE)
    small_map.bind_depth_image(as_float, s["K"], **dict(kw, depth_scale=None))
    got = small_map.bound_points()
    _same_bytes(got[0], want[0], "xyz")
    _same_bytes(got[1], want[1], "channels")


# ---- 4. interleaving with small frames -----------------------------------------------------------------------------------------------
def test_depth_frames_and_host_clouds_pipeline_as_small_frames():
    """eight robot-scale frames, no sync between them: the small frames in flight keep raw pointers to the clouds they read, so a bind
    that overwrites the owned buffer settles them first"""
    c = _case(60, 80, 1)
    a, b = _map(66), _map(66)
    try:
        for k in range(8):
            s, xyz, pos = _frames(c, k % 3)                           # (no channels: the cloud is xyz)
            t = dc.CAM_T + pos
            if k % 2 == 0:
                a.input_depth_image(s["depth"], s["K"], [], dc.CAM_R, t.copy(), 1.0, 1.0, **dc.keywords(s))
            else:
                a.input_pointcloud(xyz, ["x", "y", "z"], dc.CAM_R, t.copy(), 1.0, 1.0)
            b.input_pointcloud(xyz, ["x", "y", "z"], dc.CAM_R, t.copy(), 1.0, 1.0)
            assert a.last_update_path() == b.last_update_path() == "small_frame", k
        _equal_maps(a, b, "after eight frames")
        assert a.small_frame_aborts() == 0 and b.small_frame_aborts() == 0
        assert int((a.elevation_map[2] > 0.5).sum()) > 200
    finally:
        a.close(); b.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_leave_the_binding_alone(small_map):
    from elevation_mapping_cupy_amd._lib import EmapDepthDesc
    m = small_map
    c = _case(17, 31, 1)
    s, xyz, chan = _scene(c)
    m.bind_depth_image(s["depth"], s["K"], **dc.keywords(s))
    before = m.bound_points()
    depth = np.ones((4, 6), np.float32); raw = np.ones((4, 6), np.uint16)
    rgb = np.zeros((4, 6, 3), np.uint8); feats = np.zeros((16, 4, 6), np.float32); conf = np.ones((4, 6), np.float32)
    good = dict(height=4, width=6, depth_dtype=0, step=1, has_rgb=0, n_features=0, fx=5.0, fy=5.0, cx=2.5, cy=1.5, depth_scale=1.0,
                min_depth=0.0, max_depth=8.0, confidence_threshold=0.0)
    nan, inf = float("nan"), float("inf")

    def call(change, depth_ptr=depth, rgb_ptr=None, feat_ptr=None, desc=True):
        d = EmapDepthDesc(**dict(good, **change))
        n = ct.c_int64(-7)
        p = lambda a: None if a is None else ct.c_void_p(a.ctypes.data)
        rc = m._lib.emap_bind_depth_image(m._ctx, ct.byref(d) if desc else None, p(depth_ptr), p(rgb_ptr), p(feat_ptr), p(conf), ct.byref(n))
        return rc, n.value

    bad = [dict(height=0), dict(height=8193), dict(width=0), dict(width=8193), dict(height=-1), dict(step=0), dict(step=65), dict(step=-3),
           dict(fx=0.0), dict(fy=0.0), dict(fx=nan), dict(fy=inf), dict(fx=-inf), dict(cx=nan), dict(cy=inf), dict(min_depth=nan), dict(max_depth=inf),
           dict(max_depth=0.0), dict(min_depth=2.0, max_depth=2.0), dict(min_depth=3.0, max_depth=2.0), dict(min_depth=-0.5),
           dict(depth_dtype=2), dict(depth_dtype=-1)]
    for change in bad:
        assert call(change) == (-1, -7), change
    for scale in (0.0, -0.001, nan, inf):
        assert call(dict(depth_dtype=1, depth_scale=scale), depth_ptr=raw) == (-1, -7), scale
    assert call(dict(has_rgb=1, n_features=16), rgb_ptr=rgb, feat_ptr=feats) == (-1, -7)        # Kc = 17
    assert call(dict(n_features=17), feat_ptr=feats) == (-1, -7)
    assert call(dict(n_features=-1), feat_ptr=feats) == (-1, -7)
    assert call({}, depth_ptr=None) == (-1, -7)                      # null required pointers
    assert call({}, desc=False) == (-1, -7)
    assert call(dict(has_rgb=1)) == (-1, -7)
    assert call(dict(n_features=2)) == (-1, -7)
    assert b"emap_bind_depth_image" in m._lib.emap_last_error(m._ctx)
    after = m.bound_points()
    _same_bytes(after[0], before[0], "xyz after the refusals")
    _same_bytes(after[1], before[1], "channels after the refusals")
    _same_bytes(after[0], xyz, "xyz")
    assert call({}) == (0, 24) and call(dict(depth_dtype=1, depth_scale=0.001), depth_ptr=raw) == (0, 24)      # the base description itself is accepted
    assert call(dict(has_rgb=1, n_features=15), rgb_ptr=rgb, feat_ptr=feats) == (0, 24)


def test_nothing_bound_is_reported_and_any_bound_cloud_reads_back():
    m = _map(66)
    try:
        out = np.zeros((4, 3), np.float32)
        assert m._lib.emap_get_bound_points(m._ctx, ct.c_void_p(out.ctypes.data), None) == -3      # EMAP_ERR_NO_POINTS
        rng = np.random.default_rng(3)
        p = rng.random((1001, 7)).astype(np.float32)
        p[5, :3] = np.nan
        m.bind_points(p)                                             # an uploaded cloud: de-interleaved on the way
        xyz, chan = m.bound_points()
        _same_bytes(xyz, np.ascontiguousarray(p[:, :3]), "uploaded xyz")
        _same_bytes(chan, np.ascontiguousarray(p[:, 3:]), "uploaded channels")
    finally:
        m.close()


# ---- 6. buffer history ---------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_the_buffers_held():
    m = _map(66)
    try:
        big, tiny = _case(480, 640, 1, K=3), _case(3, 5, 1)
        sb, xyz_b, chan_b = _scene(big)
        st, xyz_t, chan_t = _scene(tiny)
        m.bind_depth_image(sb["depth"], sb["K"], **dc.keywords(sb))
        first = m.bound_points()
        m.bind_depth_image(st["depth"], st["K"], **dc.keywords(st))
        mid = m.bound_points()
        m.bind_depth_image(sb["depth"], sb["K"], **dc.keywords(sb))
        third = m.bound_points()
        _same_bytes(first[0], third[0], "xyz 1 vs 3"); _same_bytes(first[1], third[1], "channels 1 vs 3")
        _same_bytes(first[0], xyz_b, "xyz"); _same_bytes(mid[0], xyz_t, "xyz of the small image"); _same_bytes(mid[1], chan_t, "channels of the small image")
    finally:
        m.close()
