"""PointCloud2 input (emap_bind_cloud_message): the contract restated in NumPy, message building, the scene and the case table.

`unpack` is the contract of include/emap_hip.h, statement for statement (reference: the node's gather loop,
elevation_mapping_cupy/src/elevation_mapping_ros.cpp:319-338): a conv 0 column IS the four message bytes, a typed column is the
little-endian value converted by ONE astype(np.float32), which rounds to nearest even, keeps subnormals and turns a float64 beyond
float32 into +-inf exactly as the device's single conversion does -- so the GPU tests compare BITS (a float64 NaN: NaN-ness only)."""
import zlib

import numpy as np

import _depth_cases as dc

INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 = range(1, 9)      # sensor_msgs/PointField datatypes
DTYPE = {INT8: "<i1", UINT8: "<u1", INT16: "<i2", UINT16: "<u2", INT32: "<i4", UINT32: "<u4", FLOAT32: "<f4", FLOAT64: "<f8"}
SIZE = {0: 4, INT8: 1, UINT8: 1, INT16: 2, UINT16: 2, INT32: 4, UINT32: 4, FLOAT32: 4, FLOAT64: 8}


# ---- the contract ----------------------------------------------------------------------------------------------------------------------
def unpack(data, desc):
    """(xyz (n, 3), chan (n, n_cols - 3)) float32 of a message; desc: struct emap_cloud_msg_desc (or anything with its attributes)"""
    H, W, ps, rs, nc = int(desc.height), int(desc.width), int(desc.point_step), int(desc.row_step), int(desc.n_cols)
    raw = np.frombuffer(data, np.uint8, H * rs).reshape(H, rs)
    pts = raw[:, :W * ps].reshape(H * W, ps)                 # row i = r W + c: the point at byte r row_step + c point_step
    cols = []
    for c in range(nc):
        off, conv = int(desc.offset[c]), int(desc.conv[c])
        assert 0 <= off and off + SIZE[conv] <= ps, "column %d does not lie inside the point (refused by the contract)" % c
        b = np.ascontiguousarray(pts[:, off:off + SIZE[conv]])
        if conv == 0:
            cols.append(b.view("<u4").reshape(-1).view(np.float32))      # the bytes are the float: no arithmetic touches them
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                cols.append(b.view(DTYPE[conv]).reshape(-1).astype(np.float32))
    m = np.stack(cols, axis=1)
    assert m.dtype == np.float32
    return np.ascontiguousarray(m[:, :3]), np.ascontiguousarray(m[:, 3:])


def pack(columns, layout, height=1, width=None, row_pad=0, seed=0):
    """the bytes of a message: columns {field name: (n,) array}, written at the layout's offsets in the field's datatype (a uint32
    array under a FLOAT32 field gives the float's BITS); every byte no field covers, row padding included, is seeded junk"""
    n = len(next(iter(columns.values())))
    width = n // height if width is None else width
    assert height * width == n
    ps = layout["point_step"]
    rs = width * ps + row_pad
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, (height, rs), dtype=np.uint8)
    pts = np.empty((n, ps), np.uint8)
    pts[:] = buf[:, :width * ps].reshape(n, ps)
    for name, off, dt, count in layout["fields"]:
        if name not in columns:
            continue
        a = np.asarray(columns[name])
        a = a.view("<f4") if (dt == FLOAT32 and a.dtype == np.uint32) else a.astype(DTYPE[dt])
        pts[:, off:off + SIZE[dt]] = np.ascontiguousarray(a).view(np.uint8).reshape(n, SIZE[dt])
    buf[:, :width * ps] = pts.reshape(height, width * ps)
    return buf.tobytes(), rs


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------
def _layout(ps, *fields):
    return dict(point_step=ps, fields=[(nm, off, dt, 1) for nm, off, dt in fields])


_XYZ = (("x", 0, FLOAT32), ("y", 4, FLOAT32), ("z", 8, FLOAT32))
LAYOUTS = {
    "12": _layout(12, *_XYZ),
    "13": _layout(13, *_XYZ, ("tag", 12, UINT8)),
    "16": _layout(16, *_XYZ, ("intensity", 12, FLOAT32)),
    "20": _layout(20, *_XYZ, ("rgb", 16, FLOAT32)),
    "22": _layout(22, *_XYZ, ("intensity", 12, FLOAT32), ("ring", 16, UINT16), ("time", 18, FLOAT32)),      # Velodyne
    "32": _layout(32, *_XYZ, ("rgb", 16, FLOAT32)),                                                         # PCL PointXYZRGB
    "48": _layout(48, *_XYZ, ("f0", 16, FLOAT32), ("f1", 20, FLOAT32), ("f2", 24, FLOAT32), ("f3", 28, FLOAT32)),
    "256": _layout(256, *_XYZ, *[("c%d" % k, 16 + 12 * k, FLOAT32) for k in range(16)]),
    # Ouster-like: mixed types, everything 4-byte sized is 4-aligned
    "ouster48": _layout(48, *_XYZ, ("intensity", 16, FLOAT32), ("t", 20, UINT32), ("reflectivity", 24, UINT16), ("ring", 26, UINT16),
                        ("ambient", 28, UINT16), ("range", 32, UINT32)),
    # all eight datatypes, an odd point_step, a FLOAT64 at an offset that is 4- but not 8-aligned
    "typed47": _layout(47, *_XYZ, ("i8", 12, INT8), ("u8", 13, UINT8), ("i16", 14, INT16), ("u16", 16, UINT16), ("i32", 18, INT32),
                       ("u32", 23, UINT32), ("f32", 27, FLOAT32), ("f64", 36, FLOAT64)),
    # the scene's clouds: xyz alone at unaligned offsets of a 22-byte point; colour and three features in a 32-byte point
    "xyz22u": _layout(22, ("x", 2, FLOAT32), ("y", 10, FLOAT32), ("z", 18, FLOAT32)),
    "xyz32": _layout(32, *_XYZ),
    "rgbf32": _layout(32, *_XYZ, ("rgb", 16, FLOAT32), ("s0", 20, FLOAT32), ("s1", 24, FLOAT32), ("c0", 28, FLOAT32)),
}

_F64_EDGES = np.array([1e39, -1e39, 3.4028235677973366e38,                 # overflow: +inf, -inf; FLT_MAX + half an ulp: the tie goes to +inf
                       1e-40, -1e-45, 2.0 ** -150, 1.5 * 2.0 ** -149, 2.0 ** -150 * (1 + 2.0 ** -40),      # float32 subnormals; ties at the bottom: 0, 2^-148; just above the tie: 2^-149
                       1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50,      # half-ulp ties (to even: down, up), just above a tie
                       np.nan, -0.0, np.inf, 3.4028234663852886e38, 0.1], np.float64)
_U32_EDGES = np.array([2 ** 24 + 1, 2 ** 24 + 3, 2 ** 24 + 2, 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 25 + 3, 2 ** 32 - 1, 2 ** 32 - 128, 2 ** 32 - 129, 2 ** 31 + 128, 0, 1], np.uint32)
_I32_EDGES = np.array([-2 ** 31, 2 ** 31 - 1, -2 ** 24 - 1, 2 ** 24 + 1, -2 ** 24 - 3, 2 ** 31 - 65, 2 ** 31 - 64, -1, 0], np.int32)
_F32_BITS = np.array([0x7FA12345, 0xFFC00001, 0x00000001, 0x807FFFFF, 0x80000000, 0x7F800000, 0x00ABCDEF], np.uint32)      # NaN payloads, subnormals, -0, inf, a colour


def columns(layout, n, seed):
    """random columns of a layout, the edges of every datatype in their first rows (as many as n holds)"""
    rng = np.random.default_rng(seed)
    out = {}
    for name, _, dt, _ in layout["fields"]:
        if name in ("rgb", "rgba"):
            a = rng.integers(0, 1 << 24, n, dtype=np.uint32)              # the packed colour: a subnormal bit pattern
        elif dt == FLOAT32:
            a = rng.standard_normal(n).astype(np.float32).view(np.uint32).copy()
            if name not in ("x", "y", "z"):
                k = min(n, len(_F32_BITS)); a[:k] = _F32_BITS[:k]
            elif n > 8:
                a[7] = 0x7FC00000 if name == "y" else a[7]                # a NaN row
        elif dt == FLOAT64:
            a = (rng.standard_normal(n) * 10.0 ** rng.integers(-44, 40, n).astype(np.float64)).astype(np.float64)
            k = min(n, len(_F64_EDGES)); a[:k] = _F64_EDGES[:k]
        else:
            info = np.iinfo(np.dtype(DTYPE[dt]))
            a = rng.integers(info.min, int(info.max) + 1, n, dtype=np.int64).astype(DTYPE[dt])
            edges = {UINT32: _U32_EDGES, INT32: _I32_EDGES}.get(dt, np.array([info.min, info.max, 0], DTYPE[dt]))
            k = min(n, len(edges)); a[:k] = edges[:k]
        out[name] = a
    return out


# ---- the case table --------------------------------------------------------------------------------------------------------------------
def _case(layout, n=None, typed=False, channels=None, height=1, width=None, row_pad=0):
    width = n if width is None else width
    return dict(layout=layout, height=height, width=width, row_pad=row_pad, typed=bool(typed), channels=channels)


def case_key(c):
    return "%s_%dx%d%s_%s%s" % (c["layout"], c["height"], c["width"], "+%d" % c["row_pad"] if c["row_pad"] else "", "typed" if c["typed"] else "move",
                                "" if c["channels"] is None else "_" + "-".join(c["channels"]))


# sizes straddle every tile T = 1024 (point_step <= 16), 512 (<= 32), 256 (<= 64), 64 (256) and the groups of four of the stores
_SIZES = {
    "12": [1, 4, 1023, 1025, 4097],
    "13": [2, 3, 1025, 4097],
    "16": [5, 64, 1023, 1025],
    "20": [63, 257, 513, 1025],
    "22": [1, 3, 65, 127, 129, 511, 1023, 1025, 4097],
    "32": [2, 255, 256, 1025],
    "48": [5, 255, 257, 1023],
    "256": [1, 63, 64, 65, 129],
    "ouster48": [127, 256, 4097],
    "typed47": [1, 3, 129, 257, 1025],
}
CASES = []
for _name, _ns in _SIZES.items():
    _mixed = any(dt != FLOAT32 for _, _, dt, _ in LAYOUTS[_name]["fields"])
    for _k, _n in enumerate(_ns):
        for _typed in ((False, True) if _mixed or _k == 0 else (False,)):
            # (the 13-byte point: the node's 4-byte memcpy of the UINT8 at offset 12 would leave the point, which the contract refuses --
            # moved, the message gives its xyz alone)
            CASES.append(_case(_name, _n, _typed, channels=[] if _name == "13" and not _typed else None))
CASES += [
    _case("22", typed=False, height=3, width=37, row_pad=6),      # organised, row starts not 16-byte aligned
    _case("22", typed=True, height=3, width=37, row_pad=6),
    _case("22", typed=True, height=3, width=37),                  # the same cloud with tight rows
    _case("22", typed=False, height=3, width=37),
    _case("16", typed=False, height=5, width=129, row_pad=8),     # padded rows that stay dword aligned: the ALIGNED4 kernel by rows
    _case("22", typed=True, height=8, width=70, row_pad=3),       # rows that start on odd bytes: every class 7 r mod 16
    _case("22", typed=True, height=2, width=1030, row_pad=1),     # ... and rows of several tiles each
    _case("256", typed=False, height=4, width=130, row_pad=4),    # several tiles a row on the dword path; row starts 0, 4, 8, 12 mod 16
    _case("22", 257, True, channels=["ring", "time"]),            # Kc = 2
    _case("22", 66, False, channels=["time", "intensity"]),
    _case("ouster48", 1023, True, channels=["range", "ring", "intensity", "t", "ambient"]),      # Kc = 5
    _case("ouster48", 130, False, channels=["range", "ring", "intensity", "t", "ambient"]),
    _case("ouster48", 258, True, channels=["t", "range", "intensity"]),      # UINT32 columns on the dword path
    _case("256", 67, False, channels=["c3", "c0", "c15"]),        # Kc = 3 out of a wide point
    _case("48", 1026, False, channels=[]),                        # Kc = 0 with fields left out
]


def message(c):
    """(data, keywords, columns) of a case: keywords for ElevationMap.bind_pointcloud2 / pointcloud2_descriptor"""
    lay = LAYOUTS[c["layout"]]
    n = c["height"] * c["width"]
    seed = zlib.crc32(case_key(c).encode())
    cols = columns(lay, n, seed)
    data, rs = pack(cols, lay, c["height"], c["width"], c["row_pad"], seed + 1)
    kw = dict(fields=lay["fields"], width=c["width"], height=c["height"], point_step=lay["point_step"], row_step=rs, channels=c["channels"], typed=c["typed"])
    return data, kw, cols


def descriptor(c):
    from elevation_mapping_cupy_amd.elevation_mapping import pointcloud2_descriptor
    lay = LAYOUTS[c["layout"]]
    return pointcloud2_descriptor(lay["fields"], c["width"], c["height"], lay["point_step"], c["width"] * lay["point_step"] + c["row_pad"],
                                  False, c["channels"], c["typed"])


def tile(point_step):
    """points per workgroup (csrc/emap_launch.h: cloud_unpack_tile), restated"""
    t = 1024
    while t > 64 and t * point_step > 16384:
        t //= 2
    return t


def aligned4(d):
    """which k_cloud_unpack<ALIGNED4> a descriptor launches (csrc/emap_api_cloudmsg.hip), restated"""
    tight = d.row_step == d.width * d.point_step
    return (d.point_step % 4 == 0 and (tight or d.row_step % 4 == 0) and
            all(d.offset[c] % 4 == 0 and SIZE[d.conv[c]] == 4 for c in range(d.n_cols)))


# ---- the scene: the depth cases' back-projected floor, carried as a message -----------------------------------------------------------
def scene_cloud(H, W, rgb_and_features, k=0):
    """(xyz (n, 3), chan (n, Kc), names): frame k of a walk over the wavy floor of tests/_depth_cases.py (NaN rows where the depth
    image has its seeded invalid patches), with colour, two averaged features and a class channel or with none"""
    c = dc._c(H, W, 1, 0, 0, int(rgb_and_features), 3 if rgb_and_features else 0)
    s = dc.scene(c)
    s["depth"] = s["depth"].copy()
    s["depth"][s["kind"] == 0] -= np.float32(0.015 * k)
    xyz, chan = dc.restated(s)
    return xyz, chan, dc.channel_names(c)


def scene_message(xyz, chan, names, layout_name, seed=5):
    lay = LAYOUTS[layout_name]
    cols = {"x": xyz[:, 0].view(np.uint32), "y": xyz[:, 1].view(np.uint32), "z": xyz[:, 2].view(np.uint32)}
    for i, nm in enumerate(names):
        cols[nm] = np.ascontiguousarray(chan[:, i]).view(np.uint32)
    data, rs = pack({k: np.ascontiguousarray(v) for k, v in cols.items()}, lay, 1, xyz.shape[0], 0, seed)
    return data, dict(fields=lay["fields"], width=xyz.shape[0], height=1, point_step=lay["point_step"], row_step=rs)
