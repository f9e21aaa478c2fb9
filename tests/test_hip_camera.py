"""GPU: the camera path on the case table of tests/_cam_cases.py (tests/test_cam_cases.py proves on the CPU that the table reaches
every branch and that every walk ends) against the oracle, which equals the reference kernels
(tests/test_oracle_vs_reference_source.py::test_image_correspondence_and_fusions): correspondences with array_equal, fused layers
bit for bit, the image buffer's regrow path, and the C ABI's guard on the camera cell."""
import ctypes as ct

import numpy as np
import pytest

import _cam_cases as cc
from _util import make_pair
from oracle import emap_oracle as eo

pytestmark = pytest.mark.gpu

CFG = dict(eo.YAML, enable_visibility_cleanup=False)
EMAP_ERR_INVALID = -1


def _f32p(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_float))


def _setup(c):
    """(hip, oracle params, injected map) of a case: move_to first, so that the known map lies on a shifted circular origin"""
    hip, orc = make_pair(CFG, c["C"], c["mode"])
    if c["shift"]:
        s = c["shift"]
        hip.move_to(np.array([s[0] * cc.RES, s[1] * cc.RES, s[2]]), np.eye(3))
    assert np.array_equal(hip.center, cc.center_of(c))
    m = cc.camera_map(c["C"])
    hip.elevation_map = m
    if c["tol"] is not None:
        hip._chk(hip._lib.emap_image_set_tolerance(hip._ctx, ct.c_double(c["tol"])))
    return hip, orc.P, m


def _correspond(hip, inputs, H, W):
    """emap_image_correspondence through the C ABI; returns its status"""
    Pm, x1, y1, z1, K, D, center = inputs
    keep = [np.ascontiguousarray(a, np.float32).ravel() for a in (Pm, K, D, center)]
    return hip._lib.emap_image_correspondence(hip._ctx, ct.c_float(x1), ct.c_float(y1), ct.c_float(z1), _f32p(keep[0]), _f32p(keep[1]),
                                              _f32p(keep[2]), ct.c_float(float(H)), ct.c_float(float(W)), _f32p(keep[3]))


@pytest.mark.parametrize("name", [c["name"] for c in cc.cases()])
def test_input_image_matches_oracle_on_every_case(name):
    c = cc.by_name(name)
    hip, P, m = _setup(c)
    K, D, R, t, H, W = cc.camera_of(c)
    uv, va, _ = cc.oracle_run(eo, P, c, m)
    feat = np.random.default_rng(3).uniform(0, 1, (H, W)).astype(np.float32)
    want = np.zeros((c["C"], c["C"]), np.float32)
    for frame in range(2):                                                # the second frame blends with the first
        hip.input_image([feat * (1 + frame)], ["feat"], R, t, K, D, "radtan", H, W)
        huv, hva = hip.get_image_correspondence()
        assert np.array_equal(hva, va.astype(bool)) and np.array_equal(huv, uv), name
        eo.image_fuse(P, "exponential", want, feat * (1 + frame), uv, va, H, W, 0.7)
        assert np.array_equal(hip.semantic_map.get_layer("feat").view(np.uint32), want.view(np.uint32)), name
    assert va.sum() > 100 or name.startswith("negative_x") and va.sum() > 5


def _sized(c, H, W):
    """the case's camera with another image size and the same field of view"""
    return dict(c, H=H, W=W, f=c["f"] * W / c["W"])


@pytest.mark.parametrize("name", ["down_seam_radtan", "low_wall_seam"])
def test_fusions_on_a_shifted_map_and_the_image_buffer_regrow_path(name):
    """three frames of 16 x 16, then 48 x 64, then 8 x 8 pixels in ONE context (emap_image_fuse's buffer grows once and is then larger
    than needed): exponential with alpha 0.7 / 0.25 / 0.7 into layer index 2, colour into 3, kind 2 (the sample replaces the value)
    into 1, all on a map whose circular origin is shifted in both axes; layer 0 must stay untouched.  The same correspondences
    through emap_image_fuse_arrays give the same planes."""
    base = cc.by_name(name)
    C = base["C"]
    hip, P, m = _setup(base)
    for layer in ("l0", "l1", "l2", "l3"):
        hip.semantic_map.add_layer(layer)
    rng = np.random.default_rng(8)
    start = rng.uniform(0, 1, (4, C, C)).astype(np.float32)
    for k in range(4):
        hip.semantic_map.set_layer(k, start[k])
    want = start.copy()
    for (H, W), alpha in zip(((16, 16), (48, 64), (8, 8)), (0.7, 0.25, 0.7)):
        c = _sized(base, H, W)
        uv, va, inputs = cc.oracle_run(eo, P, c, m)
        assert va.sum() > 100
        assert _correspond(hip, inputs, H, W) == 0
        huv, hva = hip.get_image_correspondence()
        assert np.array_equal(hva, va.astype(bool)) and np.array_equal(huv, uv), (name, H, W)
        img = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
        rgb = rng.integers(0, 256, (3, H, W)).astype(np.float32)
        before = want.copy()
        for kind, code, layer, image, n_planes in (("exponential", 0, 2, img[1], 1), ("color", 1, 3, rgb, 3), ("average", 2, 1, img[2], 1)):
            image = np.ascontiguousarray(image)
            hip._chk(hip._lib.emap_image_fuse(hip._ctx, code, layer, _f32p(image), n_planes, H, W, ct.c_double(alpha)))
            eo.image_fuse(P, kind, want[layer], image, uv, va, H, W, alpha)
            # the same kernel on caller arrays (what the kernel factories of the compat package bind): logical planes, no origin
            out = np.zeros((C, C), np.float32)
            src = np.ascontiguousarray(before[layer]); v8 = np.ascontiguousarray(va, np.uint8)
            hip._chk(hip._lib.emap_image_fuse_arrays(hip._ctx, code, _f32p(src), _f32p(image), n_planes, H, W, _f32p(uv),
                                                     v8.ctypes.data_as(ct.POINTER(ct.c_uint8)), ct.c_double(alpha), _f32p(out)))
            assert np.array_equal(out.view(np.uint32), want[layer].view(np.uint32)), (name, H, W, kind, "arrays")
        got = hip.semantic_map.semantic_map
        for k in range(4):
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (name, H, W, "layer %d" % k)
        assert (want[1] != before[1]).sum() > 100 and np.array_equal(want[0], start[0])


def test_the_c_abi_refuses_a_camera_cell_the_walk_cannot_reach():
    """emap_image_correspondence returns the argument error BEFORE any launch for a camera cell that is not finite, not integer valued
    or beyond the cap -- the walk would not end there -- and leaves the previous correspondence as it was.  (Safe only because the guard
    returns before the launch: never run these calls against a library without it.)"""
    c = cc.by_name("down")
    hip, P, m = _setup(c)
    _, _, _, _, H, W = cc.camera_of(c)
    uv, va, inputs = cc.oracle_run(eo, P, c, m)
    assert _correspond(hip, inputs, H, W) == 0
    Pm, x1, y1, z1, K, D, center = inputs
    for bad in (3.5, np.nan, np.inf, -np.inf, 4294967296.0, -1e9, 65537.0):
        for bx, by in ((bad, y1), (x1, bad)):
            assert _correspond(hip, (Pm, bx, by, z1, K, D, center), H, W) == EMAP_ERR_INVALID, bad
            assert b"camera cell" in hip._lib.emap_last_error(hip._ctx)
            huv, hva = hip.get_image_correspondence()
            assert np.array_equal(hva, va.astype(bool)) and np.array_equal(huv, uv), bad
    with pytest.raises(ValueError):                    # and the public entry point refuses the pose itself
        far = np.array([-70000 * cc.RES, 0, 1.6])
        R = cc.camera_of(c)[2]
        hip.input_image([np.zeros((H, W), np.float32)], ["feat"], R, (-R.astype(np.float64) @ far).astype(np.float32), K, D, "radtan", H, W)
    huv, hva = hip.get_image_correspondence()
    assert np.array_equal(hva, va.astype(bool)) and np.array_equal(huv, uv)
