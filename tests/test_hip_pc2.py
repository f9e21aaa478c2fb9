"""GPU: PointCloud2 input (emap_bind_cloud_message / k_cloud_unpack, csrc/emap_cloudmsg.hip).  The cloud the device unpacks from a
message's bytes equals the NumPy restatement of the contract (tests/_pc2_cases.py) BIT FOR BIT, for every case of the table -- both
kernel instantiations, every datatype, tile size, row alignment and record width -- and a frame fed through input_pointcloud2 leaves
the map a frame fed the restated cloud through input_pointcloud leaves, on every frame path (reference: the node's host gather,
elevation_mapping_ros.cpp:319-338, in front of input_pointcloud, EM/elevation_mapping.py:434-466)."""
import ctypes as ct

import numpy as np
import pytest

import _depth_cases as dc
import _pc2_cases as pc
from _util import assert_planes_equal, make_parameter
from oracle import emap_oracle as eo

pytestmark = pytest.mark.gpu
NO_RAYS = dict(eo.YAML, enable_visibility_cleanup=False)
NORMALS = ["nx", "ny", "nz"]
_cache = {}


def _message(c):
    """message, keywords and restated cloud of a case: computed once, shared, never written to"""
    k = pc.case_key(c)
    if k not in _cache:
        data, kw, _ = pc.message(c)
        d, names = pc.descriptor(c)
        xyz, chan = pc.unpack(data, d)
        for a in (xyz, chan):
            a.setflags(write=False)
        _cache[k] = (data, kw, d, xyz, chan)
    return _cache[k]


def _scene(H, W, colour, k, layout):
    key = (H, W, colour, k, layout)
    if key not in _cache:
        xyz, chan, names = pc.scene_cloud(H, W, colour, k)
        data, kw = pc.scene_message(xyz, chan, names, layout)
        cloud = np.ascontiguousarray(np.concatenate([xyz, chan], axis=1))
        cloud.setflags(write=False)
        _cache[key] = (data, kw, cloud, names)
    return _cache[key]


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


def _find(layout, **kw):
    got = [c for c in pc.CASES if c["layout"] == layout and all(c[k] == v for k, v in kw.items())]
    assert len(got) == 1, (layout, kw)
    return got[0]


def _same_bytes(a, b, what, nan_cols=()):
    """bit for bit; in the columns of nan_cols (converted from float64): both NaN or the same bits"""
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (what, a.shape, b.shape)
    ua, ub = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    diff = ua != ub
    for c in nan_cols:
        diff[:, c] &= ~(np.isnan(a[:, c]) & np.isnan(b[:, c]))
    if diff.any():
        bad = np.argwhere(diff)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d values differ bitwise, first at %s: %r (%#x) vs %r (%#x)" % (what, len(bad), a.size, i, a[i], ua[i], b[i], ub[i]))


def _bind_and_compare(m, c):
    data, kw, d, xyz, chan = _message(c)
    n = m.bind_pointcloud2(data, **kw)
    assert n == c["height"] * c["width"] == xyz.shape[0]
    got_xyz, got_chan = m.bound_points()
    _same_bytes(got_xyz, xyz, "xyz")
    _same_bytes(got_chan, chan, "channels", nan_cols=[k - 3 for k in range(3, d.n_cols) if d.conv[k] == 8])
    return got_xyz, got_chan


# ---- 1. cloud bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.CASES, ids=pc.case_key)
def test_the_bound_cloud_is_the_restated_cloud_bit_for_bit(c, small_map):
    _bind_and_compare(small_map, c)


class _Msg:
    pass


def test_a_message_object_binds_like_its_bytes(small_map):
    """duck-typed: anything with the attributes of sensor_msgs.msg.PointCloud2, its fields objects with name / offset / datatype / count"""
    c = _find("22", height=3, width=37, row_pad=6, typed=True)
    data, kw, d, xyz, chan = _message(c)
    msg = _Msg()
    msg.data, msg.width, msg.height, msg.point_step, msg.row_step, msg.is_bigendian = bytearray(data), kw["width"], kw["height"], kw["point_step"], kw["row_step"], False
    msg.fields = []
    for f in kw["fields"]:
        o = _Msg(); o.name, o.offset, o.datatype, o.count = f
        msg.fields.append(o)
    assert small_map.bind_pointcloud2(msg, typed=True) == 111
    got = small_map.bound_points()
    _same_bytes(got[0], xyz, "xyz"); _same_bytes(got[1], chan, "channels")
    assert small_map.bound_channels == ["intensity", "ring", "time"]


def test_a_message_of_several_upload_chunks_arrives_whole(small_map):
    """9.8 MB: the host copies it into the pinned slot chunk by chunk on the worker threads, a DMA behind each chunk"""
    data, kw, cloud, names = _scene(480, 640, True, 0, "rgbf32")
    assert len(data) > 4 * (2 << 20) and len(data) % (2 << 20) != 0
    assert small_map.bind_pointcloud2(data, **kw) == 480 * 640
    xyz, chan = small_map.bound_points()
    _same_bytes(xyz, np.ascontiguousarray(cloud[:, :3]), "xyz"); _same_bytes(chan, np.ascontiguousarray(cloud[:, 3:]), "channels")


# ---- 2. frame equality ---------------------------------------------------------------------------------------------------------------
def _equal_maps(a, b, what):
    assert_planes_equal(a.elevation_map, b.elevation_map, what=what)
    assert_planes_equal(a.normal_map, b.normal_map, names=NORMALS, what=what + " normals")
    assert a.traversability_input.tobytes() == b.traversability_input.tobytes(), what + " traversability_input"
    if a.semantic_map.layer_names:
        assert a.semantic_map.layer_names == b.semantic_map.layer_names
        assert_planes_equal(a.semantic_map.semantic_map, b.semantic_map.semantic_map, names=a.semantic_map.layer_names, what=what + " semantic")


def _walk(H, W, colour, layout, C, cfg, scatter, path, semantics=None):
    a, b = _map(C, cfg), _map(C, cfg)
    try:
        for m in (a, b):
            m.set_scatter_mode(scatter)
        for k in range(3):
            data, kw, cloud, names = _scene(H, W, colour, k, layout)
            pos = np.array([0.08 * k, -0.12 * k, 0.0], np.float32)
            noise = 0.0 if k == 0 else 1.0
            for m in (a, b):
                m.move_to(pos, np.eye(3, dtype=np.float32))
            t = dc.CAM_T + pos
            a.input_pointcloud2(data, dc.CAM_R, t.copy(), noise, noise, **kw)
            b.input_pointcloud(cloud, ["x", "y", "z"] + names, dc.CAM_R, t.copy(), noise, noise)
            assert a.bound_channels == names
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
    _walk(60, 80, False, "xyz22u", 66, NO_RAYS, "auto", "small_frame")


@pytest.mark.parametrize("rays", [False, True])
@pytest.mark.parametrize("scatter", ["auto", "binned"])
def test_vga_frames_on_the_tile_path(scatter, rays):
    """the 480 x 640 scene as a message of 32-byte points: 307200 rows sort by tile under both settings"""
    _walk(480, 640, False, "xyz32", 258, eo.YAML if rays else NO_RAYS, scatter, "binned")


def test_vga_frames_carry_colour_and_three_features_through_the_frame():
    _walk(480, 640, True, "rgbf32", 258, NO_RAYS, "binned", "binned", semantics=("in_tile_pass", "carried"))


# ---- 3. the three doors, pipelined ---------------------------------------------------------------------------------------------------
def test_the_three_doors_pipeline_as_small_frames():
    """eight robot-scale frames of different sizes, no sync between them, alternately a message, a host cloud and a depth image: the
    message and the depth image share the pinned slots and the owned cloud, and the small frames in flight keep raw pointers to the
    clouds they read"""
    shapes = [(60, 80), (48, 64), (30, 40)]
    a, b = _map(66), _map(66)
    try:
        for k in range(8):
            H, W = shapes[(k // 3 + k) % 3]
            data, kw, cloud, _ = _scene(H, W, False, k % 3, "xyz22u")
            pos = np.array([0.08 * (k % 3), -0.12 * (k % 3), 0.0], np.float32)
            t = dc.CAM_T + pos
            if k % 3 == 0:
                a.input_pointcloud2(data, dc.CAM_R, t.copy(), 1.0, 1.0, **kw)
            elif k % 3 == 1:
                a.input_pointcloud(cloud, ["x", "y", "z"], dc.CAM_R, t.copy(), 1.0, 1.0)
            else:
                s = dc.scene(dc._c(H, W, 1, 0, 0, 0, 0))
                depth = s["depth"].copy()
                depth[s["kind"] == 0] -= np.float32(0.015 * (k % 3))
                a.input_depth_image(depth, s["K"], [], dc.CAM_R, t.copy(), 1.0, 1.0, **dict(dc.keywords(s)))
            b.input_pointcloud(cloud, ["x", "y", "z"], dc.CAM_R, t.copy(), 1.0, 1.0)
            assert a.last_update_path() == b.last_update_path() == "small_frame", (k, a.last_update_path(), b.last_update_path())
        _equal_maps(a, b, "after eight frames")
        assert a.small_frame_aborts() == 0 and b.small_frame_aborts() == 0
        assert int((a.elevation_map[2] > 0.5).sum()) > 200
    finally:
        a.close(); b.close()


# ---- 4. buffer history ---------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_the_buffers_held():
    m = _map(66)
    try:
        mid, big, tiny = _find("typed47", width=257, typed=True), _find("22", width=4097, typed=True), _find("256", width=1, typed=False)
        first = _bind_and_compare(m, mid)
        _bind_and_compare(m, big)
        second = _bind_and_compare(m, mid)
        _bind_and_compare(m, tiny)
        third = _bind_and_compare(m, mid)
        for other in (second, third):
            assert first[0].tobytes() == other[0].tobytes() and first[1].tobytes() == other[1].tobytes()      # (the float64 NaN's bits as well: same code, same input)
    finally:
        m.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_leave_the_binding_alone(small_map):
    from elevation_mapping_cupy_amd._lib import EmapCloudMsgDesc
    m = small_map
    before = _bind_and_compare(m, _find("22", height=3, width=37, row_pad=6, typed=True))
    data = np.zeros(4096, np.uint8)
    good = dict(height=2, width=5, point_step=24, row_step=128, is_bigendian=0, n_cols=5)
    good_off, good_conv = [0, 4, 8, 12, 16], [0, 0, 0, 4, 8]

    def call(change=None, off=None, conv=None, desc=True, ptr=True):
        d = EmapCloudMsgDesc(**dict(good, **(change or {})))
        for k, (o, c) in enumerate(zip(off or good_off, conv or good_conv)):
            d.offset[k], d.conv[k] = o, c
        n = ct.c_int64(-7)
        rc = m._lib.emap_bind_cloud_message(m._ctx, ct.byref(d) if desc else None, ct.c_void_p(data.ctypes.data) if ptr else None, ct.byref(n))
        return rc, n.value

    bad = [dict(is_bigendian=1), dict(height=0), dict(width=0), dict(height=-1), dict(width=-5),
           dict(height=1 << 13, width=(1 << 13) + 1, point_step=1, row_step=(1 << 13) + 1),      # n > 2^26
           dict(point_step=0), dict(point_step=257, row_step=2048), dict(point_step=-4),
           dict(row_step=119), dict(row_step=0), dict(row_step=-128),
           dict(height=1 << 16, row_step=1 << 15),                                               # height * row_step = 2^31
           dict(n_cols=2), dict(n_cols=20), dict(n_cols=-1)]
    for change in bad:
        assert call(change) == (-1, -7), change
    assert call(conv=[0, 0, 0, 9, 0]) == (-1, -7) and call(conv=[0, -1, 0, 0, 0]) == (-1, -7)     # unknown conv
    assert call(off=[0, 4, -1, 12, 16]) == (-1, -7)                                              # negative offset
    for off, conv in (([0, 4, 8, 12, 21], [0, 0, 0, 0, 0]), ([0, 4, 8, 12, 21], [0, 0, 0, 0, 7]), ([0, 4, 8, 12, 17], [0, 0, 0, 0, 8]),
                      ([0, 4, 8, 23, 16], [0, 0, 0, 3, 0]), ([0, 4, 8, 24, 16], [0, 0, 0, 2, 0]), ([22, 4, 8, 12, 16], good_conv)):
        assert call(off=off, conv=conv) == (-1, -7), (off, conv)                                 # a column that leaves the point
    assert call(desc=False) == (-1, -7) and call(ptr=False) == (-1, -7)                          # null pointers
    assert b"emap_bind_cloud_message" in m._lib.emap_last_error(m._ctx)
    after = m.bound_points()
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    # the base description is accepted, and so are the last values inside every limit
    assert call() == (0, 10)
    assert call(off=[0, 4, 8, 22, 16], conv=[0, 0, 0, 4, 8]) == (0, 10) and call(off=[20, 4, 8, 23, 16], conv=[7, 0, 0, 1, 8]) == (0, 10)
    assert call(dict(point_step=256, row_step=1280, n_cols=3)) == (0, 10) and call(dict(row_step=120)) == (0, 10)
    # ... and the Python door refuses what the C contract would read beyond: a message shorter than it says
    c = _find("22", height=3, width=37, row_pad=6, typed=True)
    msg, kw = _message(c)[:2]
    with pytest.raises(ValueError):
        m.bind_pointcloud2(msg[:-1], **kw)
