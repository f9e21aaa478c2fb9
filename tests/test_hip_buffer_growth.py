"""GPU: a context buffer that GROWS while the work of the call before is still enqueued (csrc/emap_host.h: grow, Stage).  The rest of
the suite grows most buffers from empty; here every buffer family is first sized by a small call and then, with no emap_sync in
between, outgrown by a larger one.  Every result must equal, bit for bit, that of a second context that ran the same calls with
emap_sync after each of them.  Public C ABI only, on a 32 x 32 map; each case is a few milliseconds of GPU work."""
import ctypes as ct

import numpy as np
import pytest

from elevation_mapping_cupy_amd import _lib
from elevation_mapping_cupy_amd.parameter import Parameter

pytestmark = pytest.mark.gpu

C = 32
RES = 0.04
EYE = np.eye(3, dtype=np.float32).reshape(-1).copy()
DOWN = np.diag([1.0, -1.0, -1.0]).astype(np.float32)      # a sensor that looks down: its +z is the map's -z


def _vp(a):
    return ct.c_void_p(a.ctypes.data)


class Ctx:
    """one context; `sync` = emap_sync after every call"""

    def __init__(self, sync):
        self.lib, self.sync, self.ctx = _lib.load(), sync, ct.c_void_p()
        p = Parameter(resolution=RES, enable_visibility_cleanup=False, enable_overlap_clearance=False)
        P = _lib.fill_params(p, C, "fp32")
        assert self.lib.emap_create(ct.byref(P), None, 0, ct.c_void_p(0), ct.byref(self.ctx)) == 0

    def call(self, name, *args):
        rc = getattr(self.lib, name)(self.ctx, *args)
        assert rc == 0, (name, rc, self.lib.emap_last_error(self.ctx))
        if self.sync:
            assert self.lib.emap_sync(self.ctx) == 0

    def close(self):
        self.lib.emap_destroy(self.ctx)

    # ---- the calls the cases are made of ----
    def upload(self, pts):
        self.call("emap_upload_points", _vp(pts), ct.c_int64(pts.shape[0]), ct.c_int64(pts.shape[1]), 0)

    def update(self, R=EYE, t=(0.0, 0.0, 1.0)):
        t = np.asarray(t, np.float32)
        self.call("emap_update", _lib.f32p(R), _lib.f32p(t), ct.c_double(0.0), ct.c_double(0.0), None)

    def layers(self):
        out = np.empty((7, C, C), np.float32)
        for k in range(7):
            self.call("emap_get_layer", k, _lib.f32p(out[k]))
        return out

    def seed(self):
        """a frame that leaves most cells valid"""
        self.upload(cloud(3000, 7))
        self.update()


def cloud(n, seed):
    """n points under a sensor one metre above the map centre, spread over the whole map with a gentle relief"""
    rng = np.random.default_rng(seed)
    p = np.empty((n, 3), np.float32)
    p[:, :2] = rng.uniform(-0.6, 0.6, (n, 2))
    p[:, 2] = -1.0 + 0.05 * np.sin(7.0 * p[:, 0]) + 0.03 * np.cos(5.0 * p[:, 1])
    return p


def both(sequence):
    """the results of `sequence(ctx)` without and with emap_sync after every call"""
    out = []
    for sync in (False, True):
        c = Ctx(sync)
        try:
            out.append(sequence(c))
        finally:
            c.close()
    return out


def assert_same_bits(got, want):
    assert got.keys() == want.keys()
    for k in got:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert a.tobytes() == b.tobytes(), "%s: %d of %d bytes differ" % (k, int((a.view(np.uint8) != b.view(np.uint8)).sum()), a.nbytes)


def test_point_index_buffers_grow_behind_a_smaller_call():
    def sequence(c):
        res = {}
        for n in (64, 4096):
            c.upload(cloud(n, n))
            idx, valid, inside = np.empty(n, np.int32), np.empty(n, np.uint8), np.empty(n, np.uint8)
            c.call("emap_point_index", _lib.f32p(EYE), _lib.f32p(np.array([0, 0, 1], np.float32)), _vp(idx), _vp(valid), _vp(inside))
            res.update({"idx%d" % n: idx, "valid%d" % n: valid, "inside%d" % n: inside})
        return res
    got, want = both(sequence)
    assert_same_bits(got, want)
    assert got["valid4096"].sum() > 4000 and got["inside4096"].sum() > 4000 and len(np.unique(got["idx4096"])) > 500


def test_grid_map_buffer_grows_from_one_layer_to_five():
    M = C - 2

    def sequence(c):
        c.seed()
        res = {}
        for n in (1, 5):
            table = (_lib.EmapGridLayer * n)()
            for k in range(n):
                table[k].kind, table[k].index, table[k].slot = _lib.GRID_BUILTIN, k, k
            out = np.full((n, M, M), np.nan, np.float32)
            c.call("emap_publish_grid_map", table, n, _lib.GRID_ORDERS["rows"], ct.c_float(0.0), 1, _lib.f32p(out), n)
            res["grid%d" % n] = out
        return res
    got, want = both(sequence)
    assert_same_bits(got, want)
    assert np.isfinite(got["grid5"][0]).sum() > 300 and got["grid1"].tobytes() == got["grid5"][:1].tobytes()


def test_plugin_chain_scratch_and_counters_grow_behind_a_smaller_chain():
    def chain(c, ops):
        table = (_lib.EmapPluginOp * len(ops))()
        for t_, o in zip(table, ops):
            t_.type, t_.dst_plane, t_.src_kind, t_.src_index, t_.i0, t_.i1, t_.flags, t_.f0 = o
        c.call("emap_plugin_chain", table, len(ops), _lib.f32p(EYE))

    def sequence(c):
        c.seed()
        c.call("emap_plugin_planes", 3)
        ops = _lib.PLUGIN_OPS
        chain(c, [(ops["smooth"], 0, _lib.PLUGIN_SRC_LAYER, 0, 0, 0, 0, 0.0)])                     # one scratch plane, no counter
        chain(c, [(ops["erosion"], 1, _lib.PLUGIN_SRC_LAYER, 0, 3, 1, 0, 0.0),                      # three planes + five, three counters
                  (ops["min_filter"], 2, _lib.PLUGIN_SRC_LAYER, 0, 1, 2, 0, 0.0)])
        planes = np.empty((3, C, C), np.float32)
        for k in range(3):
            c.call("emap_plugin_plane_read", k, _lib.f32p(planes[k]))
        return {"planes": planes}
    got, want = both(sequence)
    assert_same_bits(got, want)
    for p in got["planes"]:
        assert (p[np.isfinite(p)] != 0).sum() > 100


def test_image_buffer_grows_from_8x8_to_48x64():
    cam = np.array([0.0, 0.0, 1.6])
    t = (-DOWN.astype(np.float64) @ cam).astype(np.float32)

    def sequence(c):
        c.seed()
        c.call("emap_semantic_configure", 1)
        for (H, W), seed in (((8, 8), 1), ((48, 64), 2)):
            K = np.array([[W, 0, W / 2], [0, W, H / 2], [0, 0, 1]], np.float32)
            Pm = np.ascontiguousarray((K @ np.concatenate([DOWN, t[:, None]], 1)).astype(np.float32).reshape(-1))
            c.call("emap_image_correspondence", ct.c_float(C / 2), ct.c_float(C / 2), ct.c_float(1.6), _lib.f32p(Pm),
                   _lib.f32p(np.ascontiguousarray(K.reshape(-1))), _lib.f32p(np.zeros(5, np.float32)), ct.c_float(H), ct.c_float(W), _lib.f32p(np.zeros(3, np.float32)))
            img = np.random.default_rng(seed).uniform(0.5, 1.5, (H, W)).astype(np.float32)
            c.call("emap_image_fuse", 0, 0, _lib.f32p(img), 1, H, W, ct.c_double(0.7))
        layer = np.empty((C, C), np.float32)
        c.call("emap_semantic_get_layer", 0, _lib.f32p(layer))
        return {"layer": layer}
    got, want = both(sequence)
    assert_same_bits(got, want)
    assert (got["layer"] != 0).sum() > 100


def test_binned_frame_buffers_grow_from_300_points_to_5000():
    def sequence(c):
        c.call("emap_set_scatter_mode", 2)
        path = ct.c_int32(-1)
        for n in (300, 5000):
            c.upload(cloud(n, n))
            c.update()
            c.call("emap_last_update_path", ct.byref(path))
            assert path.value & 3 == 1      # binned
        return {"map": c.layers()}
    got, want = both(sequence)
    assert_same_bits(got, want)
    assert (got["map"][2] == 1).sum() > 500


def test_owned_cloud_grows_while_it_is_the_bound_one():
    def sequence(c):
        res = {}
        for (H, W), colour in (((8, 8), False), ((24, 32), True)):
            depth = (1.0 + 0.05 * np.random.default_rng(H).uniform(0, 1, (H, W))).astype(np.float32)
            rgb = np.random.default_rng(W).integers(0, 256, (H, W, 3)).astype(np.uint8)
            d = _lib.EmapDepthDesc(H, W, 0, 1, int(colour), 0, W, W, W / 2, H / 2, 1.0, 0.1, 8.0, 0.0)
            n = ct.c_int64(0)
            c.call("emap_bind_depth_image", ct.byref(d), _vp(depth), _vp(rgb) if colour else None, None, None, ct.byref(n))
            assert n.value == H * W
            c.update(DOWN.reshape(-1).copy(), (0.0, 0.0, 1.2))
            if colour:      # (the read-back waits for the stream: only behind the last frame)
                xyz, chan = np.empty((H * W, 3), np.float32), np.empty((H * W, 1), np.float32)
                c.call("emap_get_bound_points", _vp(xyz), _vp(chan))
                res.update(xyz=xyz, chan=chan)
        res["map"] = c.layers()
        return res
    got, want = both(sequence)
    assert_same_bits(got, want)
    assert (got["map"][2] == 1).sum() > 100 and np.isfinite(got["xyz"]).all()
