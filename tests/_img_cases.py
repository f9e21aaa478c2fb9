"""Image message input (emap_input_image_message / k_image_frame): the message -> planes contract restated in NumPy, message
building, the map state and camera poses of the GPU test, and the case table.  tests/test_img_cases.py proves on the CPU that the
restatement equals an independent per-pixel struct.unpack loop, that the oracle's correspondence of every case samples the image's
four borders and its last pixel, and that the table reaches every kernel variant; tests/test_hip_image_message.py runs the table on
the GPU against ElevationMap.input_image fed the restated planes.

A case is a dict: enc (the sensor_msgs/Image encoding string), elem / n_chan / swap (what it must parse to), big (is_bigendian), H, W,
step_mode ("tight" | "odd" | "pad64") and step, C (map side), channels (the channel list handed to the door), variant (the k_image_frame
instantiation the launcher selects: 0, 1, 2, 3 for elements of 1, 2, 4, 8 bytes)."""
import struct

import numpy as np

import _cam_cases as cam
import _fixtures as fx

ELEMS = ("8U", "8S", "16U", "16S", "32S", "32F", "64F")            # the OpenCV depth codes 0 .. 6
SIZES = (1, 1, 2, 2, 4, 4, 8)
NP_CODE = ("u1", "i1", "u2", "i2", "i4", "f4", "f8")
STRUCT_CODE = ("B", "b", "H", "h", "i", "f", "d")
NAMED = {"mono8": ("8U", 1, False), "mono16": ("16U", 1, False), "rgb8": ("8U", 3, False), "rgba8": ("8U", 4, False),
         "bgr8": ("8U", 3, True), "bgra8": ("8U", 4, True), "rgb16": ("16U", 3, False), "rgba16": ("16U", 4, False),
         "bgr16": ("16U", 3, False), "bgra16": ("16U", 4, False)}
REFUSED_ENCODINGS = ("bayer_rggb8", "bayer_bggr16", "yuv422", "yuv422_yuy2", "nv21", "", "rgb", "8U", "8UC5", "8UC0", "12UC1", "32UC1", "64FC41", "64F",
                     "RGB8", "mono32", "bgr32", " rgb8")
POISON = 0xA5
STEP_MODES = ("tight", "odd", "pad64")
CHANNEL_FUSIONS = {"rgb": "color", "default": "exponential"}
VARIANT_OF_SIZE = {1: 0, 2: 1, 4: 2, 8: 3}
N_VARIANTS = 4
F32_SPECIALS = (np.nan, np.inf, -np.inf, 1e-40, -0.0, 3.4e38)                                  # 1e-40: a float32 subnormal
F64_SPECIALS = (np.nan, 1e300, -1e300, 1e-40, 1.0 + 2.0 ** -30, 3.5e38, 1e-50, -(2.0 ** 24 + 1.0))  # beyond float32, subnormal there, ties and roundings


def step_of(mode, tight):
    if mode == "tight":
        return tight
    if mode == "odd":                       # one more byte; two where that would be even: every other row starts at an odd address
        return tight + 1 if tight % 2 == 0 else tight + 2
    return (tight // 64 + 1) * 64           # the next multiple of 64 that leaves padding


def _case(enc, H=48, W=64, mode="tight", big=False, C=66, channels=None):
    if enc in NAMED:
        e, n, swap = NAMED[enc]
    else:
        e, n, swap = enc[:-2], int(enc[-1]), False
    elem = ELEMS.index(e)
    colour_ok = e in ("8U", "16U")                      # colour cases use values >= 0 only
    if channels is None:
        channels = {1: ["f0"], 2: ["f0", "f1"], 3: ["rgb"] if colour_ok else ["f0", "f1", "f2"],
                    4: ["rgb", "a"] if colour_ok else ["f0", "f1", "f2", "f3"]}[n]
    tight = W * n * SIZES[elem]
    return dict(enc=enc, elem=elem, n_chan=n, swap=swap, big=bool(big and SIZES[elem] > 1), H=H, W=W, step_mode=mode, step=step_of(mode, tight), C=C,
                channels=list(channels), variant=VARIANT_OF_SIZE[SIZES[elem]])


def _table():
    out = []
    # every element type x 1 .. 4 channels; step mode and byte order rotate so that every element type meets all three step modes and
    # (where it has more than one byte) both byte orders
    for ei, e in enumerate(ELEMS):
        for n in (1, 2, 3, 4):
            out.append(_case("%sC%d" % (e, n), mode=STEP_MODES[(ei + n) % 3], big=n % 2 == 0))
    # the other byte order of every multi-byte element, on the misaligned step
    for e in ELEMS[2:]:
        out.append(_case(e + "C1", mode="odd", big=True))
        out.append(_case(e + "C2", mode="odd", big=False))
    # every named encoding
    for k, enc in enumerate(NAMED):
        out.append(_case(enc, mode=STEP_MODES[k % 3], big=False))
    for k, enc in enumerate(("mono16", "rgb16", "rgba16", "bgr16", "bgra16")):
        out.append(_case(enc, mode=STEP_MODES[(k + 1) % 3], big=True))
    # colour next to plain planes on the same message; one layer named twice (the in-thread order)
    out.append(_case("8UC4", mode="odd", channels=["f0", "f1", "f2", "f3"]))
    out.append(_case("32FC2", mode="tight", channels=["f0", "f0"]))
    # the small images
    out.append(_case("8UC1", H=1, W=1))
    out.append(_case("64FC4", H=1, W=1, mode="odd", big=True))
    out.append(_case("16UC3", H=1, W=1, mode="pad64"))
    out.append(_case("bgr8", H=5, W=3, mode="odd"))
    out.append(_case("16SC3", H=5, W=3, mode="odd", big=True))
    out.append(_case("32FC2", H=5, W=3, mode="pad64"))
    out.append(_case("64FC1", H=5, W=3, mode="odd"))
    out.append(_case("32SC4", H=5, W=3, mode="tight", big=True))
    # the larger map: more than one workgroup row of the seam, the distorted camera
    out.append(_case("rgba8", C=98, mode="odd"))
    return out


def case_key(c):
    return "%s-%dx%d-%s-%s-C%d-%s" % (c["enc"], c["H"], c["W"], c["step_mode"], "be" if c["big"] else "le", c["C"], "+".join(c["channels"]))


CASES = _table()


# ---- values and message -------------------------------------------------------------------------------------------------------------
def values(c):
    """(H, W, n_chan) array of the element's native dtype.  The value of a sample follows from its serial number (v W + u) n_chan + c,
    so a wrong channel, row or column shows; multi-byte values differ in every byte, so a wrong byte order shows; wherever the type
    can hold them all the samples are unique."""
    H, W, n, e = c["H"], c["W"], c["n_chan"], ELEMS[c["elem"]]
    s = np.arange(H * W * n, dtype=np.int64).reshape(H, W, n)
    if e in ("8U", "8S"):
        v = ((s * 167 + (s >> 8) * 59 + 7) & 0xFF).astype(np.uint8)
        return v if e == "8U" else v.view(np.int8)
    if e == "16U":
        return (s * 5 + 1).astype(np.uint16)                               # < 65536 for 48 x 64 x 4
    if e == "16S":
        return (s * 5 - 30000).astype(np.int16)
    if e == "32S":                                                         # a bijection of the serial: almost all beyond 2^24 (rounded by the conversion)
        return (((s + 1) * 2654435761) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    specials = F32_SPECIALS if e == "32F" else F64_SPECIALS
    v = (s * 0.37 - 1000.0 + (0.0 if e == "32F" else 1e-9) * s).astype(NP_CODE[c["elem"]])
    flat, sf = v.reshape(-1), s.reshape(-1)
    pix, ch = sf // n, sf % n
    pick = (pix + ch) % 5 == 2                                             # every fifth sample of every channel is a special value, in rotation
    flat[pick] = np.array(specials, v.dtype)[(pix[pick] // 5 + pix[pick] // W + ch[pick]) % len(specials)]
    return v


def message(c):
    """the message's bytes (height * step, padding = POISON) as a read-only uint8 array"""
    es = SIZES[c["elem"]]
    tight = c["W"] * c["n_chan"] * es
    rows = np.full((c["H"], c["step"]), POISON, np.uint8)
    wire = values(c).astype((">" if c["big"] else "<") + NP_CODE[c["elem"]])
    rows[:, :tight] = wire.view(np.uint8).reshape(c["H"], tight)
    data = rows.reshape(-1)
    data.setflags(write=False)
    return data


def keywords(c):
    return dict(height=c["H"], width=c["W"], encoding=c["enc"], is_bigendian=c["big"], step=c["step"])


# ---- the contract, twice ------------------------------------------------------------------------------------------------------------
def planes(c, data):
    """(n_chan, H, W) float32: what the node hands input_image for this message (cvtColor for bgr8 / bgra8, split, cv2eigen)"""
    es, n = SIZES[c["elem"]], c["n_chan"]
    tight = c["W"] * n * es
    rows = np.asarray(data, np.uint8)[:c["H"] * c["step"]].reshape(c["H"], c["step"])[:, :tight]
    px = np.ascontiguousarray(rows).view((">" if c["big"] else "<") + NP_CODE[c["elem"]]).reshape(c["H"], c["W"], n)
    order = [2 - p if c["swap"] and p in (0, 2) else p for p in range(n)]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(px[:, :, order].transpose(2, 0, 1).astype(np.float32))


def planes_loop(c, data):
    """the same by an independent route: one struct.unpack per sample at its byte address"""
    es, n = SIZES[c["elem"]], c["n_chan"]
    fmt = (">" if c["big"] else "<") + STRUCT_CODE[c["elem"]]
    raw = bytes(np.asarray(data, np.uint8))
    out = np.empty((n, c["H"], c["W"]), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in range(n):
            ch = 2 - p if c["swap"] and p in (0, 2) else p
            for v in range(c["H"]):
                for u in range(c["W"]):
                    out[p, v, u] = np.float32(struct.unpack_from(fmt, raw, v * c["step"] + (u * n + ch) * es)[0])
    return out


# ---- map state and cameras ----------------------------------------------------------------------------------------------------------
R0, T0 = fx.POSES["identity"]
MOVE = np.array([0.12, -0.2, 0.05], np.float32)        # 3 rows, -5 columns, 5 cm: a circular origin off zero and a pending shift
# camera position relative to the map centre after the move (cells, cells, metres above it), focal length in pixels and yaw per (C, H, W):
# chosen so that the oracle's correspondence alone meets the coverage condition (tests/test_img_cases.py asserts it)
POSES = {
    (66, 48, 64): dict(pos=(-3.0, 2.0, 1.5), f=40.0, yaw=0.0, dist=False),
    (66, 5, 3): dict(pos=(-1.5, 2.5, 1.6), f=4.0, yaw=0.1, dist=False),
    (66, 1, 1): dict(pos=(-1.5, 2.5, 1.6), f=2.0, yaw=0.3, dist=False),
    (98, 48, 64): dict(pos=(-3.0, 1.0, 2.3), f=40.0, yaw=0.0, dist=True),
}
_cache = {}


def terrain(C):
    """the cloud of the first frame: fx.cloud's footprint over a gentle relief (nothing occludes a camera that looks down)"""
    p = fx.cloud(C, 20000, 0)
    p[:, 2] = (0.03 * np.sin(p[:, 0] * 3.0) + 0.02 * np.cos(p[:, 1] * 2.0) - 1.0).astype(np.float32)
    return p


def config():
    from oracle import emap_oracle as eo
    return dict(eo.YAML, enable_visibility_cleanup=False)


def oracle_state(C):
    """(oracle parameters, elevation map (7, C, C), centre) of the state every GPU case starts from: the terrain frame, then MOVE"""
    if ("state", C) not in _cache:
        from oracle import emap_oracle as eo
        orc = eo.OracleMap(eo.make_params(config(), cell_n=C, mode="reference_fp16"))
        orc.update_map_with_kernel(terrain(C), R0, T0)
        orc.move_to(MOVE)
        m = orc.elevation_map.copy(); m.setflags(write=False)
        _cache[("state", C)] = (orc.P, m, orc.center.astype(np.float32).copy())
    return _cache[("state", C)]


def camera(C, H, W):
    """K, D, R (world -> camera), t of the (C, H, W) pose"""
    p = POSES[(C, H, W)]
    _, _, center = oracle_state(C)
    K = np.array([[p["f"], 0, W / 2], [0, p["f"], H / 2], [0, 0, 1]], np.float32)
    D = cam.DIST.copy() if p["dist"] else np.zeros(5, np.float32)
    R = cam._rot_down(p["yaw"])
    pos = center.astype(np.float64) + np.array([p["pos"][0] * cam.RES, p["pos"][1] * cam.RES, p["pos"][2]])
    t = (-R.astype(np.float64) @ pos).astype(np.float32)
    return K, D, R, t


def correspondence(C, H, W):
    """the oracle's (uv, valid) of the (C, H, W) pose on oracle_state(C); computed once"""
    if ("corr", C, H, W) not in _cache:
        from elevation_mapping_cupy_amd.elevation_mapping import camera_cell
        from oracle import emap_oracle as eo
        P, m, center = oracle_state(C)
        K, D, R, t = camera(C, H, W)
        x1, y1, z1 = camera_cell(center, C, cam.RES, R, t)
        Pm = (K @ np.concatenate([R, t[:, None]], 1)).astype(np.float32)
        uv, va = eo.image_correspondence(P, m, x1, y1, z1, Pm.ravel(), K.ravel(), D, H, W, center)
        uv.setflags(write=False); va.setflags(write=False)
        _cache[("corr", C, H, W)] = (uv, va)
    return _cache[("corr", C, H, W)]


def sampled_pixels(C, H, W):
    """(v, u) integer arrays of the pixels the visible cells sample"""
    uv, va = correspondence(C, H, W)
    ok = va != 0
    return uv[1][ok].astype(np.int32), uv[0][ok].astype(np.int32)


def entries(c):
    """the entry table of a case as update_layers_image would make its calls with CHANNEL_FUSIONS: (kind name, layer name, plane)"""
    out = []
    for j, ch in enumerate(c["channels"]):
        out.append(("color", ch, 0) if ch == "rgb" else ("exponential", ch, j))
    return out


def oracle_fuse(c, pl, sem=None):
    """the semantic layers (dict name -> (C, C) float32) after the case's frame on the oracle, from planes `pl`; `sem` = layers before"""
    from oracle import emap_oracle as eo
    P, _, _ = oracle_state(c["C"])
    uv, va = correspondence(c["C"], c["H"], c["W"])
    sem = {} if sem is None else sem
    for kind, name, plane in entries(c):
        layer = sem.setdefault(name, np.zeros((c["C"], c["C"]), np.float32))
        eo.image_fuse(P, kind, layer, pl if kind == "color" else pl[plane], uv, va, c["H"], c["W"], 0.7)
    return sem
