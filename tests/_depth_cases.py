"""Depth-image input (emap_bind_depth_image): the contract restated in NumPy, the scene the tests look at, and the case table.

The restatement is the contract of include/emap_hip.h, statement for statement, in float32 (reference: the sensor package's
create_pcl_from_image / process_image, pointcloud_node.py:205-250, 261-269): NumPy's float32 subtract, multiply and divide round to
nearest like the device's (the kernel keeps subnormals and its division is correctly rounded: csrc/emap_depth.hip), so the tests
compare BITS."""
import zlib

import numpy as np

QNAN = np.uint32(0x7FC00000)
KINDS = ("zero", "negative", "nan", "inf", "far", "low_conf", "nan_conf")
CHANNEL_FUSIONS = {"rgb": "color", "c0": "class_average", "default": "average"}      # the fusion set of golden/semantic_yaml66.npz


def backproject(desc, depth, rgb=None, features=None, confidence=None):
    """(xyz (n, 3), chan (n, Kc)) float32 of the sampled grid.  desc: dict with fx, fy, cx, cy, step and optionally depth_scale,
    min_depth, max_depth, confidence_threshold."""
    f32 = np.float32
    step = int(desc.get("step", 1))
    H, W = depth.shape
    vs, us = np.arange(0, H, step), np.arange(0, W, step)
    d = depth[np.ix_(vs, us)]
    with np.errstate(all="ignore"):
        z = d.astype(f32) * f32(desc["depth_scale"]) if depth.dtype == np.uint16 else d.astype(f32)      # uint16: ONE float32 multiply
        valid = np.isfinite(z) & (z > f32(desc.get("min_depth", 0.0))) & (z < f32(desc.get("max_depth", 8.0)))
        if confidence is not None:
            valid &= confidence[np.ix_(vs, us)].astype(f32) >= f32(desc.get("confidence_threshold", 0.0))      # (NaN >= thr is False)
        u = np.broadcast_to(us.astype(f32)[None, :], z.shape)
        v = np.broadcast_to(vs.astype(f32)[:, None], z.shape)
        x = ((u - f32(desc["cx"])) * z) / f32(desc["fx"])
        y = ((v - f32(desc["cy"])) * z) / f32(desc["fy"])
    assert x.dtype == y.dtype == z.dtype == np.float32
    xyz = np.stack([x, y, z], axis=-1).reshape(-1, 3).copy()
    xyz.view(np.uint32)[~valid.reshape(-1)] = QNAN
    cols = []
    if rgb is not None:
        c = rgb[np.ix_(vs, us)].astype(np.uint32)
        cols.append(((c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]).reshape(-1).view(np.float32))
    if features is not None:
        for k in range(features.shape[0]):
            cols.append(features[k][np.ix_(vs, us)].astype(f32).reshape(-1))
    chan = np.stack(cols, axis=1).astype(f32) if cols else np.zeros((xyz.shape[0], 0), f32)
    if cols:      # (astype keeps float32 bits; the colour column is a subnormal bit pattern and must not pass through arithmetic)
        assert chan.dtype == np.float32
    return xyz, np.ascontiguousarray(chan)


# ---- the scene -----------------------------------------------------------------------------------------------------------------------
CAM_T = np.array([0.1, -0.05, 1.2], np.float32)
CAM_R = np.diag([1.0, -1.0, -1.0]).astype(np.float32)      # looks straight down
DEPTH_SCALE = 0.001
CONF_THR = 0.5


def case_key(c):
    return "%dx%d_s%d_%s_%s_%s%d" % (c["H"], c["W"], c["step"], "u16" if c["u16"] else "f32", "conf" if c["conf"] else "noconf", "rgb" if c["rgb"] else "k", c["K"])


def intrinsics(H, W):
    return np.array([[0.8 * W, 0.0, (W - 1) / 2 + 0.25], [0.0, 0.8 * W, (H - 1) / 2 - 0.5], [0.0, 0.0, 1.0]])


def kinds_of(c):
    """the invalid kinds a case can hold: a uint16 image has no negative, NaN or infinite pixel; the confidence kinds need the image"""
    k = ["zero", "far"] + ([] if c["u16"] else ["negative", "nan", "inf"]) + (["low_conf", "nan_conf"] if c["conf"] else [])
    return [x for x in KINDS if x in k]


def scene(c):
    """dict(depth, K, desc, rgb, features, confidence, kind): `kind` (H, W) int8 = index into KINDS + 1 of the pixel's seeded invalid
    patch, 0 where the pixel is left valid"""
    H, W, step = c["H"], c["W"], c["step"]
    rng = np.random.default_rng(zlib.crc32(case_key(c).encode()))
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = (1.2 - 0.15 * np.sin(6 * np.pi * u / W) * np.cos(2 * np.pi * v / H)).astype(np.float32)
    conf = (0.6 + 0.4 * rng.random((H, W))).astype(np.float32)
    kind = np.zeros((H, W), np.int8)
    Hs, Ws = -(-H // step), -(-W // step)
    kinds = kinds_of(c)
    per = max(1, (Hs * Ws) // 160)                    # patches per kind: 2 x 2 pixels anchored ON the sampled grid, at most 2.5 % each
    for k in kinds:
        for _ in range(per):
            r, q = int(rng.integers(Hs)) * step, int(rng.integers(Ws)) * step
            kind[r:r + 2, q:q + 2] = KINDS.index(k) + 1
    raw = None
    if c["u16"]:
        raw = np.rint(depth.astype(np.float64) / DEPTH_SCALE).astype(np.uint16)
        raw[kind == 1] = 0
        raw[kind == 5] = rng.choice(np.array([8000, 9000, 65535], np.uint16), size=int((kind == 5).sum()))
    else:
        depth[kind == 1] = 0.0
        depth[kind == 2] = -1.2
        depth[kind == 3] = np.nan
        depth[kind == 4] = np.inf
        depth[kind == 5] = rng.choice(np.array([8.0, 8.5, 1e30], np.float32), size=int((kind == 5).sum()))
    conf[kind == 6] = 0.25
    conf[kind == 7] = np.nan
    Km = intrinsics(H, W)
    desc = dict(fx=Km[0, 0], fy=Km[1, 1], cx=Km[0, 2], cy=Km[1, 2], step=step, depth_scale=DEPTH_SCALE if c["u16"] else None,
                min_depth=0.0, max_depth=8.0, confidence_threshold=CONF_THR if c["conf"] else 0.0)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8) if c["rgb"] else None
    feats = None
    if c["K"]:
        feats = rng.random((c["K"], H, W)).astype(np.float32)
        if c["K"] >= 3:
            feats[2] = np.floor(3 * feats[2])          # a class-like channel for class_average
    return dict(depth=raw if c["u16"] else depth, K=Km, desc=desc, rgb=rgb, features=feats, confidence=conf if c["conf"] else None, kind=kind)


def keywords(s):
    """the keyword arguments of ElevationMap.bind_depth_image / input_depth_image for a scene"""
    d = s["desc"]
    return dict(depth_scale=d["depth_scale"], rgb=s["rgb"], features=s["features"], confidence=s["confidence"],
                confidence_threshold=d["confidence_threshold"], min_depth=d["min_depth"], max_depth=d["max_depth"], step=d["step"])


def restated(s):
    return backproject(s["desc"], s["depth"], s["rgb"], s["features"], s["confidence"])


def channel_names(c):
    """colour, then features: two averaged channels, a class channel, further averaged ones"""
    return (["rgb"] if c["rgb"] else []) + [("c0" if k == 2 else "s%d" % k) for k in range(c["K"])]


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def _c(H, W, step, u16, conf, rgb, K):
    return dict(H=H, W=W, step=step, u16=bool(u16), conf=bool(conf), rgb=bool(rgb), K=K)


# (H, W) x step x dtype x confidence x Kc, crossed sparsely.  Beyond the issue's lists: 2 x 3 (the only way to n % 4 == 2 with step 1)
# and Kc = 2 (the class Kc % 4 == 2).
CASES = [
    _c(1, 1, 1, 0, 0, 0, 0),          # n = 1: the tail alone
    _c(1, 7, 1, 1, 1, 1, 0),          # n = 7
    _c(5, 1, 1, 0, 1, 0, 3),          # n = 5, one column
    _c(2, 3, 1, 1, 0, 1, 1),          # n = 6: n % 4 == 2, Kc = 2
    _c(3, 5, 1, 1, 0, 1, 3),          # n = 15: tail + groups that span row ends, Kc = 4
    _c(3, 5, 2, 0, 1, 1, 0),
    _c(4, 4, 1, 0, 0, 1, 4),          # n = 16: no tail, Kc = 5
    _c(4, 4, 7, 1, 0, 0, 0),          # a step larger than the image: one row
    _c(17, 31, 1, 0, 1, 1, 15),       # odd on both axes, Kc = 16 with colour
    _c(17, 31, 2, 1, 0, 1, 0),
    _c(17, 31, 3, 0, 0, 0, 3),
    _c(64, 64, 1, 1, 1, 1, 3),
    _c(64, 64, 7, 0, 1, 1, 3),
    _c(60, 80, 1, 0, 0, 0, 0),
    _c(60, 80, 2, 1, 1, 1, 1),
    _c(60, 80, 3, 1, 1, 0, 16),       # Kc = 16 without colour
    _c(480, 640, 1, 1, 0, 1, 3),
    _c(480, 640, 1, 0, 1, 0, 0),
    _c(480, 640, 2, 0, 0, 0, 3),
]


def instantiation(c):
    """which k_depth_cloud<DT, CONF, QUAD> a case launches"""
    return (int(c["u16"]), c["conf"], c["step"] == 1)


def n_rows(c):
    return -(-c["H"] // c["step"]) * -(-c["W"] // c["step"])


def kc(c):
    return int(c["rgb"]) + c["K"]
