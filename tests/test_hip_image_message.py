"""GPU: image message input (emap_input_image_message / k_image_frame, csrc/emap_image_msg.hip).  A camera frame fed as the BYTES of a
sensor_msgs/Image leaves the correspondence and every semantic layer that ElevationMap.input_image leaves when it is fed the planes the
node would have made of that message (tests/_img_cases.py: the contract restated in NumPy) -- bit for bit, for every case of the table:
every element type, channel count, named encoding, byte order, row step and kernel variant -- and what the oracle computes from those
planes.  Reference: the node's host conversion (elevation_mapping_ros.cpp:375-446) in front of input_image (EM/elevation_mapping.py:
468-562, EM/semantic_map.py:261-309)."""
import ctypes as ct

import numpy as np
import pytest

import _cam_cases as cam
import _fixtures as fx
import _img_cases as ic
from _util import assert_planes_equal, make_parameter
from oracle import emap_oracle as eo

pytestmark = pytest.mark.gpu
_cache = {}


def _msg(c):
    """message bytes and restated planes of a case: computed once, shared, never written to"""
    k = ic.case_key(c)
    if k not in _cache:
        data = ic.message(c)
        pl = ic.planes(c, data)
        pl.setflags(write=False)
        _cache[k] = (data, pl)
    return _cache[k]


def _map(C, weights=None, strip=None):
    from elevation_mapping_cupy_amd.elevation_mapping import ElevationMap
    m = ElevationMap(make_parameter(ic.config(), C, weights=weights), strip=strip)
    m.param.image_channel_fusions = dict(ic.CHANNEL_FUSIONS)
    return m


def _start(C, weights=None):
    """the state every case starts from: the terrain frame, then a move that leaves the circular origin off zero and a shift pending"""
    m = _map(C, weights)
    m.input_pointcloud(ic.terrain(C), ["x", "y", "z"], ic.R0, ic.T0.copy(), 0.0, 0.0)
    m.move_to(ic.MOVE, np.eye(3, dtype=np.float32))
    return m


def _find(enc, **kw):
    got = [c for c in ic.CASES if c["enc"] == enc and all(c[k] == v for k, v in kw.items())]
    assert got, (enc, kw)
    return got[0]


def _feed_message(m, c, data=None):
    K, D, R, t = ic.camera(c["C"], c["H"], c["W"])
    m.input_image_message(_msg(c)[0] if data is None else data, c["channels"], R, t, K, D, **ic.keywords(c))


def _feed_planes(m, c, pl=None):
    K, D, R, t = ic.camera(c["C"], c["H"], c["W"])
    pl = _msg(c)[1] if pl is None else pl
    m.input_image([p for p in pl], c["channels"], R, t, K, D, "radtan", c["H"], c["W"])


def _bits_equal(a, b, what):
    """bit for bit; a NaN sample: both NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    if diff.any():
        i = tuple(np.argwhere(diff)[0])
        raise AssertionError("%s: %d of %d values differ bitwise, first at %s: %r vs %r" % (what, int(diff.sum()), a.size, i, a[i], b[i]))


def _same_frame(a, b, what):
    ua, va = a.get_image_correspondence()
    ub, vb = b.get_image_correspondence()
    assert np.array_equal(va, vb), what + ": valid"
    assert ua.view(np.uint32).tobytes() == ub.view(np.uint32).tobytes(), what + ": uv"
    assert a.semantic_map.layer_names == b.semantic_map.layer_names, what
    _bits_equal(a.semantic_map.semantic_map, b.semantic_map.semantic_map, what + ": layers")
    return ua, va


def _layers(m):
    return dict(zip(m.semantic_map.layer_names, m.semantic_map.semantic_map))


# ---- 0. the state the CPU coverage proof was made on ---------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [66, 98])
def test_the_starting_state_is_the_oracles(C):
    """tests/test_img_cases.py proves the coverage of the table on the ORACLE's map: the heights and the validity the correspondence
    reads are the same here, and so is the correspondence itself"""
    m = _start(C)
    try:
        _, want, center = ic.oracle_state(C)
        assert np.array_equal(m.center, center)
        got = m.elevation_map
        assert_planes_equal(got[[0, 2]], want[[0, 2]], names=["elevation", "is_valid"], what="start")
    finally:
        m.close()


# ---- 1. table equivalence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ic.CASES, ids=ic.case_key)
def test_a_message_leaves_what_its_planes_leave_bit_for_bit(c):
    a, b = _start(c["C"]), _start(c["C"])
    try:
        _feed_message(a, c)
        _feed_planes(b, c)
        uv, va = _same_frame(a, b, ic.case_key(c))
        ouv, ova = ic.correspondence(c["C"], c["H"], c["W"])
        assert np.array_equal(va, ova.astype(bool)) and np.array_equal(uv, ouv)       # the cells whose coverage the CPU test proved
        assert va.sum() >= 100
        sem = a.semantic_map.semantic_map
        assert sem.shape[0] == len(set(c["channels"])) and all((layer[va] != 0).any() for layer in sem)
    finally:
        a.close(); b.close()


# ---- 2. against the oracle -----------------------------------------------------------------------------------------------------------
def _against_oracle(c, frames=1):
    m = _start(c["C"])
    try:
        data, pl = _msg(c)
        sem = None
        for k in range(frames):
            if k == 0:
                d, p = data, pl
            else:                                   # a second, different message of the same layout: the rows in reverse order
                d = np.ascontiguousarray(np.asarray(data).reshape(c["H"], c["step"])[::-1]).reshape(-1)
                p = ic.planes(c, d)
                assert not np.array_equal(p, pl)
            _feed_message(m, c, d)
            sem = ic.oracle_fuse(c, p, sem)
        got = _layers(m)
        assert list(got) == list(sem)
        for name in sem:
            _bits_equal(got[name], sem[name], "%s layer %s" % (ic.case_key(c), name))
            assert (sem[name] != 0).sum() >= 100
    finally:
        m.close()


def test_exponential_twice_blends_like_the_oracle():
    _against_oracle(_find("mono16", big=False), frames=2)
    _against_oracle(_find("32SC1", step_mode="odd"), frames=2)


def test_colour_from_bgr8_and_rgba8_like_the_oracle():
    _against_oracle(_find("bgr8", H=48))
    c = _find("rgba8", C=66)
    assert c["channels"] == ["rgb", "a"]
    _against_oracle(c)


def test_one_layer_named_twice_is_fused_in_table_order():
    c = _find("32FC2", channels=["f0", "f0"])
    _against_oracle(c)


def _camera_args(m, c):
    from elevation_mapping_cupy_amd.elevation_mapping import camera_cell
    K, D, R, t = ic.camera(c["C"], c["H"], c["W"])
    P = (K @ np.concatenate([R, t[:, None]], 1)).astype(np.float32)
    x1, y1, z1 = camera_cell(m.center, m.cell_n, cam.RES, R, t)
    arrs = [np.ascontiguousarray(P.reshape(-1)), np.ascontiguousarray(K.reshape(-1)), np.ascontiguousarray(D), np.ascontiguousarray(m.center, np.float32)]
    return float(x1), float(y1), float(z1), arrs


def _raw_call(m, c, data, specs, change=None, null=None, cell=None, n_specs=None):
    """emap_input_image_message itself; change: descriptor fields to override, null: the name of the pointer to pass as NULL"""
    from elevation_mapping_cupy_amd._lib import EmapImageMsgDesc, EmapImageSpec, f32p
    d = EmapImageMsgDesc(height=c["H"], width=c["W"], step=c["step"], elem=c["elem"], n_chan=c["n_chan"], is_bigendian=int(c["big"]), swap_rb=int(c["swap"]))
    for k, v in (change or {}).items():
        setattr(d, k, v)
    x1, y1, z1, arrs = _camera_args(m, c)
    if cell is not None:
        x1, y1 = cell
    sp = (EmapImageSpec * max(len(specs), 1))()
    for s, (kind, layer, plane, alpha) in zip(sp, specs):
        s.kind, s.layer, s.plane, s.alpha = kind, layer, plane, alpha
    ptr = dict(desc=ct.byref(d), data=ct.c_void_p(data.ctypes.data), P=f32p(arrs[0]), K=f32p(arrs[1]), D=f32p(arrs[2]), center=f32p(arrs[3]), specs=sp)
    if null:
        ptr[null] = None
    return m._lib.emap_input_image_message(m._ctx, ptr["desc"], ptr["data"], x1, y1, z1, ptr["P"], ptr["K"], ptr["D"], ptr["center"], ptr["specs"],
                                           len(specs) if n_specs is None else n_specs)


def test_the_average_kind_through_the_table():
    """kind 2 (average_correspondences_to_map_kernel: the sample replaces the value) has no image plugin; the table reaches it"""
    c = _find("16SC3", H=48)
    m = _start(c["C"])
    try:
        data, pl = _msg(c)
        m.semantic_map.add_layer("avg"); m.semantic_map.add_layer("exp")
        m.semantic_map.set_layer("avg", np.full((c["C"], c["C"]), 7.0, np.float32))
        assert _raw_call(m, c, data, [(2, 0, 2, 0.0), (0, 1, 1, 0.25), (2, 1, 0, 0.0), (0, 1, 2, 0.5)]) == 0
        P, _, _ = ic.oracle_state(c["C"])
        uv, va = ic.correspondence(c["C"], c["H"], c["W"])
        avg, ex = np.full((c["C"], c["C"]), 7.0, np.float32), np.zeros((c["C"], c["C"]), np.float32)
        eo.image_fuse(P, "average", avg, pl[2], uv, va, c["H"], c["W"])
        eo.image_fuse(P, "exponential", ex, pl[1], uv, va, c["H"], c["W"], 0.25)
        eo.image_fuse(P, "average", ex, pl[0], uv, va, c["H"], c["W"])
        eo.image_fuse(P, "exponential", ex, pl[2], uv, va, c["H"], c["W"], 0.5)
        got = _layers(m)
        _bits_equal(got["avg"], avg, "average"); _bits_equal(got["exp"], ex, "exponential over average")
        assert (avg != 7.0).sum() >= 100 and (avg == 7.0).sum() >= 100
    finally:
        m.close()


# ---- 3. slot reuse -------------------------------------------------------------------------------------------------------------------
def test_three_messages_back_to_back_equal_the_serial_result():
    """no sync between the calls: both pinned slots are used, the first is used again, and each grows on the way"""
    seq = [_find("8SC2", H=48), _find("64FC1", step_mode="odd", big=False, H=48), _find("16UC3", H=48)]
    assert len({len(_msg(c)[0]) for c in seq}) == 3
    a, b = _start(66), _start(66)
    try:
        for c in seq:
            _feed_message(a, c)
        for c in seq:
            _feed_message(b, c)
            b.sync()
        _same_frame(a, b, "pipelined vs serial")
        sem = None
        for c in seq:
            sem = ic.oracle_fuse(c, _msg(c)[1], sem)
        got = _layers(a)
        assert list(got) == list(sem)
        for name in sem:
            _bits_equal(got[name], sem[name], "layer " + name)
    finally:
        a.close(); b.close()


# ---- 4. borrowed bytes ---------------------------------------------------------------------------------------------------------------
def test_the_callers_bytes_are_only_borrowed():
    c = _find("rgb16", big=False)
    a, b = _start(66), _start(66)
    try:
        mine = np.array(_msg(c)[0])
        _feed_message(a, c, mine)
        mine[:] = 0xFF                       # right after the call returns, before anything waited for the device
        a.sync()
        _feed_message(b, c)
        _same_frame(a, b, "overwritten after the call")
    finally:
        a.close(); b.close()


# ---- 5. the bound cloud --------------------------------------------------------------------------------------------------------------
def test_the_bound_cloud_stays_bound_around_a_camera_frame(weights):
    C = 66
    c = _find("bgra8", C=66)
    m = _start(C, weights)
    orc = eo.OracleMap(eo.make_params(ic.config(), cell_n=C, mode="reference_fp16", weights=weights))
    try:
        orc.update_map_with_kernel(ic.terrain(C), ic.R0, ic.T0)
        orc.move_to(ic.MOVE)
        p2 = fx.cloud(C, 15000, 3)
        p2[:, 2] = (0.02 * np.cos(p2[:, 0] * 2.5) - 1.0).astype(np.float32)
        t2 = (ic.T0 + ic.MOVE).astype(np.float32)
        t2_rel = t2 - m.center
        m.input_pointcloud(p2, ["x", "y", "z"], ic.R0, t2.copy(), 0.0, 0.0)              # a robot-scale frame, not waited for
        assert m.last_update_path() == "small_frame"
        _feed_message(m, c)
        xyz, chan = m.bound_points()
        assert xyz.tobytes() == p2.tobytes() and chan.shape == (15000, 0)
        orc.update_map_with_kernel(p2, ic.R0, t2_rel)
        K, D, R, t = ic.camera(C, c["H"], c["W"])
        Pm, x1, y1, z1 = fx.camera_inputs(m.center, C, cam.RES, K, R, t)
        uv, va = eo.image_correspondence(orc.P, orc.elevation_map, x1, y1, z1, Pm.ravel(), K.ravel(), D, c["H"], c["W"], m.center)
        huv, hva = m.get_image_correspondence()
        assert va.sum() >= 100 and np.array_equal(hva, va.astype(bool)) and np.array_equal(huv, uv)
        pl = _msg(c)[1]
        sem = {n: np.zeros((C, C), np.float32) for n in ("rgb", "a")}
        eo.image_fuse(orc.P, "color", sem["rgb"], pl, uv, va, c["H"], c["W"])
        eo.image_fuse(orc.P, "exponential", sem["a"], pl[1], uv, va, c["H"], c["W"], 0.7)
        got = _layers(m)
        for name in sem:
            _bits_equal(got[name], sem[name], "layer " + name)
        assert_planes_equal(m.elevation_map, orc.elevation_map, what="after the camera frame")
        # a point-cloud frame AFTER the image, on the cloud that is still bound
        m.update_map_with_kernel(None, [], ic.R0, t2.copy(), 0.0, 0.0, want_stats=False)
        orc.update_map_with_kernel(p2, ic.R0, t2_rel)
        assert_planes_equal(m.elevation_map, orc.elevation_map, what="frame on the still-bound cloud")
    finally:
        m.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_correspondence_and_layers_alone():
    c = _find("rgba8", C=66)
    m = _start(66)
    try:
        _feed_message(m, c)
        data = np.array(_msg(c)[0])
        assert m.semantic_map.layer_names == ["rgb", "a"]
        good = [(1, 0, 0, 0.0), (0, 1, 1, 0.7)]

        def state():
            uv, va = m.get_image_correspondence()
            return uv.tobytes(), va.tobytes(), m.semantic_map.semantic_map.tobytes()

        before = state()
        tight1 = dict(n_chan=1, step=c["W"])                                   # a one-channel view of the same bytes
        plain = [(0, 0, 0, 0.7)]
        refusals = [dict(null=n) for n in ("desc", "data", "P", "K", "D", "center", "specs")]
        refusals += [dict(cell=(1.5, 3.0)), dict(cell=(float("nan"), 3.0)), dict(cell=(3.0, float("inf"))), dict(cell=(3.0, 70000.0))]      # what emap_image_correspondence refuses
        refusals += [dict(change=dict(height=0)), dict(change=dict(height=8193)), dict(change=dict(width=0)), dict(change=dict(width=8193, step=8193 * 4)),
                     dict(change=dict(height=-1)), dict(change=dict(width=-4))]
        refusals += [dict(change=dict(step=c["W"] * 4 - 1)), dict(change=dict(step=0)), dict(change=dict(step=-c["step"]))]
        refusals += [dict(change=dict(height=8192, step=1 << 18))]             # height * step = 2^31
        refusals += [dict(change=dict(elem=-1)), dict(change=dict(elem=7)), dict(change=dict(n_chan=0)), dict(change=dict(n_chan=5, step=c["W"] * 5))]
        refusals += [dict(n_specs=0), dict(n_specs=5), dict(n_specs=-1)]
        refusals += [dict(specs=[(-1, 0, 0, 0.7)]), dict(specs=[(3, 0, 0, 0.7)]), dict(specs=[(0, -1, 0, 0.7)]), dict(specs=[(0, 2, 0, 0.7)]),
                     dict(specs=[(0, 0, 4, 0.7)]), dict(specs=[(0, 0, -1, 0.7)]), dict(specs=good + [(2, 1, 4, 0.0)])]
        refusals += [dict(specs=[(1, 0, 0, 0.0)], change=dict(n_chan=2, step=c["W"] * 2)), dict(specs=plain, change=dict(n_chan=2, swap_rb=1))]
        refusals += [dict(specs=[(1, 0, 0, 0.0)], change=dict(height=2400, width=2400, n_chan=3, step=7200)),      # 3 H W > 2^24 with colour
                     dict(specs=plain, change=dict(height=4097, width=4096, **dict(tight1, step=4096)))]          # H W > 2^24
        for r in refusals:
            r = dict(r)
            specs = r.pop("specs", good)
            assert _raw_call(m, c, data, specs, **r) == -1, r
            assert b"emap_input_image_message" in m._lib.emap_last_error(m._ctx), r
            assert state() == before, r
        # the last values inside the limits are accepted: 3 H W = 2^24 exactly is too large a message to build here, so the small ones
        assert _raw_call(m, c, data, plain, change=tight1) == 0
        assert _raw_call(m, c, data, good) == 0
        strip = _map(66, strip=(0, 33, 0))
        try:
            strip.semantic_map.add_layer("rgb"); strip.semantic_map.add_layer("a")
            assert _raw_call(strip, c, data, good) == -1
            assert b"single-strip" in strip._lib.emap_last_error(strip._ctx)
        finally:
            strip.close()
    finally:
        m.close()


def test_the_python_door_refuses_what_it_can_see():
    c = _find("rgb8")
    m = _start(66)
    try:
        K, D, R, t = ic.camera(66, c["H"], c["W"])
        data = _msg(c)[0]
        kw = ic.keywords(c)
        with pytest.raises(ValueError):
            m.input_image_message(data, ["rgb", "extra"], R, t, K, D, **kw)                  # 4 planes asked of a 3-plane image (the node drops the frame)
        with pytest.raises(ValueError):
            m.input_image_message(data, ["f0"], R, t, K, D, **kw)
        with pytest.raises(ValueError):
            m.input_image_message(data[:-1], ["rgb"], R, t, K, D, **kw)                      # shorter than it says
        with pytest.raises(ValueError):
            m.input_image_message(data, ["rgb"], R, t, K, D, **dict(kw, encoding="bayer_rggb8"))
        with pytest.raises(ValueError):
            m.input_image_message(data, ["rgb"], R, t, **kw)                                 # no K, no camera_info
        assert m.semantic_map.layer_names == []

        class Obj:
            pass
        msg, info = Obj(), Obj()
        msg.data, msg.height, msg.width, msg.encoding, msg.is_bigendian, msg.step = bytes(data), c["H"], c["W"], c["enc"], 0, c["step"]
        info.K, info.D, info.distortion_model = [float(x) for x in K.reshape(-1)], [], "plumb_bob"
        m.input_image_message(msg, ["rgb"], R, t, camera_info=info)                          # a message object and a CameraInfo, duck typed
        b = _start(66)
        try:
            _feed_planes(b, c)
            _same_frame(m, b, "message object")
        finally:
            b.close()
    finally:
        m.close()
