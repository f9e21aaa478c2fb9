"""What the tests of the semantic plugins on resident planes share (tests/test_semplug_cases.py on the CPU, tests/test_hip_semantic_chain.py
on the GPU): the extra semantic layers, the plugin configurations, the twin start state and the NumPy restatement of the arithmetic of
the four ops of emap_plugin_chain_ex (include/emap_hip.h).

As in tests/_plug_cases.py the yardstick of every value is the host route of the plugins, taken from a TWIN map.  The maps of
_grid_cases.start carry the semantic layers s0 s1 c0 rgb; here sem_0 .. sem_2 (class scores) and feat_0 .. feat_15 (features) are added
with semantic_map.set_layer, and the raw traversability is replaced by a layer that holds exact tenths, both zeros and NaN."""
import numpy as np

import _grid_cases as gc
import _plug_cases as pc

SIZES = pc.SIZES
ORDERS = pc.ORDERS
LAYERS = ["elevation", "variance", "is_valid", "traversability", "time", "upper_bound", "is_upper_bound"]
SEM_NAMES = ["sem_0", "sem_1", "sem_2"]
FEAT_NAMES = ["feat_%d" % f for f in range(16)]
_entry = pc._entry


# ---- the extra layers -------------------------------------------------------------------------------------------------------------------
def class_layers(C, seed=21):
    """(3, C, C) class scores in quarters, so that ties are common; around the centre: an exact three-way tie, a -0.0 / 0.0 pair in both
    orders above a smaller third, a NaN in the first, the middle and the last source, and an all-NaN cell"""
    rng = np.random.default_rng(seed)
    a = (rng.integers(-2, 6, (3, C, C)) * 0.25).astype(np.float32)
    r = C // 2
    a[:, r, 2] = 0.75
    a[:, r, 3] = (-0.0, 0.0, -1.0)
    a[:, r, 4] = (0.0, -0.0, -1.0)
    a[:, r, 5] = (-1.0, -0.0, 0.0)
    a[:, r + 1, 2] = (np.nan, 5.0, 1.0)
    a[:, r + 1, 3] = (5.0, np.nan, 7.0)
    a[:, r + 1, 4] = (1.0, 5.0, np.nan)
    a[:, r + 1, 5] = np.nan
    return a


def feature_layers(C, seed=22):
    """(16, C, C): scale_f * (sin-cos pattern + 0.3 noise) with scale_f = 1.6 / (1 + f): the first feature exceeds the clip at +-1, the
    variances fall like 1 / (1 + f)^2, so the spectrum of the covariance is well separated"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(C, dtype=np.float64), np.arange(C, dtype=np.float64), indexing="ij")
    out = np.empty((16, C, C), np.float32)
    for f in range(16):
        pattern = np.sin((0.37 + 0.11 * f) * x + 0.5 * f) * np.cos((0.23 + 0.07 * f) * y - 0.3 * f)
        out[f] = (1.6 / (1 + f) * (pattern + 0.3 * rng.standard_normal((C, C)))).astype(np.float32)
    return out


def traversability_layer(C, seed=23):
    """the raw traversability the votes and the layer maximum run on: exact tenths as float32 (0.3f is above the double 0.3), +0, -0, 1 and NaN"""
    rng = np.random.default_rng(seed)
    t = (rng.integers(0, 11, (C, C)) / 10.0).astype(np.float32)
    r = C // 2
    t[r - 1, 2:6] = (0.3, -0.0, 0.0, np.nan)
    t[r - 2, 2:4] = (np.nan, 1.0)
    return t


def eigen_ratios(features):
    """ratios of adjacent leading eigenvalues (1/2, 2/3, 3/4) of the covariance of the clipped features (F, C, C)"""
    x = np.clip(features.reshape(len(features), -1).T.astype(np.float64), -1, 1)
    w = np.sort(np.linalg.eigvalsh(np.cov(x.T)))[::-1]
    return [w[k] / w[k + 1] for k in range(min(3, len(w) - 1))]


# ---- configurations -----------------------------------------------------------------------------------------------------------------------
ML_SRC = ["traversability", "featp_smooth", "sem_0"]          # a map layer, a plugin plane, a semantic layer
ML_VARIANTS = {                                                # every per-source step of MAX_LAYER alone, none, and all together
    "none": dict(default_value=0, reverse=[False] * 3, scales=[1, 1, 1], thresholds=[False] * 3),
    "default": dict(default_value=0.25, reverse=[False] * 3, scales=[1, 1, 1], thresholds=[False] * 3),
    "reverse": dict(default_value=0, reverse=[True, False, True], scales=[1, 1, 1], thresholds=[False] * 3),
    "scale": dict(default_value=0, reverse=[False] * 3, scales=[0.7, -1.3, 1], thresholds=[False] * 3),
    "threshold": dict(default_value=0, reverse=[False] * 3, scales=[1, 1, 1], thresholds=[0.3, 0.05, 0.5]),
    "all": dict(default_value=0.1, reverse=[True, True, False], scales=[0.7, 1.9, -0.5], thresholds=[0.3, False, -0.2]),      # a mixed stack: int64 beside float32
}
PCA_PATTERNS = {
    "pca3": ["^elevation$", "^featp_smooth$", "^feat_0$"],
    "pca5": ["^elevation$", "^featp_smooth$", "^feat_[0-2]$"],
    "pca16": ["^elevation$", "^featp_smooth$", "^feat_([0-9]|1[0-3])$"],
    "pca": ["^feat_.*$"],
}


def ops_config(C):
    """every op of emap_plugin_chain_ex, one layer each, behind the three plugins whose planes they read: a device op (featp_smooth,
    robot_centric_elevation) and a host plugin (hostp: Inpainting with OpenCV-free telea on the host)"""
    e = [
        _entry("smooth_filter", "featp_smooth", input_layer_name="elevation"),
        _entry("inpainting", "hostp", height=True, method="telea"),
        _entry("robot_centric_elevation", "robot_centric_elevation", height=True, resolution=pc.resolution(C), use_threshold=False),
        _entry("semantic_filter", "max_categories", classes=["^sem_.*$"]),
        _entry("semantic_filter", "cls_none", classes=["^nothing$"]),
        _entry("semantic_filter", "cls_one", classes=["^sem_1$"]),
        _entry("semantic_filter", "cls_two", classes=["^sem_[01]$"]),
        _entry("semantic_filter", "cls_mixed", classes=["^traversability$", "^featp_smooth$", "^sem_.*$"]),
        _entry("semantic_traversability", "trav_rce", layers=["traversability", "robot_centric_elevation"], thresholds=[0.3, 0.5], type=["traversability", "elevation"]),
        _entry("semantic_traversability", "trav_exact", layers=["time", "traversability", "traversability"], thresholds=[3.0, 1.0, 0.0], type=["traversability", "x", "traversability"]),
        _entry("semantic_traversability", "trav_inexact", layers=["traversability", "featp_smooth"], thresholds=[0.3, 0.3], type=["x", "traversability"]),
        _entry("semantic_traversability", "trav_inexact_le", fill_nan=True, layers=["traversability"], thresholds=[0.3], type=["traversability"]),
    ]
    for v, kw in ML_VARIANTS.items():
        for mm in ("min", "max"):
            e.append(_entry("max_layer_filter", "ml_%s_%s" % (v, mm), layers=ML_SRC, min_or_max=mm, **kw))
    e.append(_entry("max_layer_filter", "ml_host", layers=["hostp", "ghost", "sem_1"], reverse=[False] * 3, thresholds=[False] * 3, scales=[1], default_value=0))
    for n, pat in PCA_PATTERNS.items():
        e.append(_entry("features_pca", n, process_layer_names=pat))
    return e


def decline_config(C):
    """the configurations a semantic plugin declines: its own layer among its sources, a PCA of 2 and of 17 layers, a layer-name default,
    no layer found, a missing vote layer -- all on the host route, with the host route's values"""
    return [
        _entry("semantic_filter", "sem_self", classes=["^sem_.*$"]),
        _entry("features_pca", "pca_two", process_layer_names=["^feat_[01]$"]),
        _entry("features_pca", "pca_17", process_layer_names=["^feat_.*$", "^elevation$"]),
        _entry("max_layer_filter", "ml_layer_default", layers=["traversability", "sem_0"], reverse=[False, False], thresholds=[False, False], scales=[1], default_value="time"),
        _entry("max_layer_filter", "ml_nothing", layers=["ghost"], reverse=[False], thresholds=[False], scales=[1], default_value=0.5),
        _entry("semantic_traversability", "trav_missing", layers=["traversability", "sem_0"], thresholds=[0.5, 0.5], type=["traversability", "x"]),
        _entry("max_layer_filter", "ml_self", layers=["ml_self", "sem_0"], reverse=[False, False], thresholds=[False, False], scales=[1], default_value=0),
    ]


DECLINED = ["sem_self", "pca_two", "pca_17", "ml_layer_default", "ml_nothing", "trav_missing", "ml_self"]

# the reference's config/setups/turtle_bot/plugin_config.yaml with its two disabled entries switched on, and a layer maximum beside them
TURTLE = [
    _entry("min_filter", "min_filter", height=True, dilation_size=1, iteration_n=30),
    _entry("smooth_filter", "smooth", height=True, input_layer_name="min_filter"),
    _entry("inpainting", "inpaint", height=True, method="telea"),
    _entry("robot_centric_elevation", "robot_centric_elevation", height=True, resolution=0.04, threshold=1.1, use_threshold=True),
    _entry("semantic_filter", "max_categories", classes=["^sem_.*$"]),
    _entry("semantic_traversability", "semantic_traversability", layers=["traversability", "robot_centric_elevation"], thresholds=[0.3, 0.5],
           type=["traversability", "elevation"]),
    _entry("features_pca", "pca", process_layer_names=["^feat_.*$"]),
    _entry("max_layer_filter", "max_layer", layers=["traversability", "sem_0", "semantic_traversability"], reverse=[True, False, False],
           thresholds=[False, 0.5, False], scales=[1.0, 1.0, 1.0], default_value=0.0),
]
TURTLE_INPUTS = ["min_filter", "smooth", "inpaint", "robot_centric_elevation"]      # the plugin planes in front of the semantic plugins
TURTLE_SEMANTIC = ["max_categories", "pca", "semantic_traversability", "max_layer"]
TURTLE_LIST = ["max_categories", "pca", "semantic_traversability", "max_layer", "elevation"]      # a semantic publisher's list
TURTLE_FULL = ["min_filter", "smooth", "inpaint", "elevation", "rgb", "max_categories", "semantic_traversability", "pca", "max_layer"]      # a host plugin between semantic ops

CONFIGS = {"ops": ops_config, "decline": decline_config, "turtle": lambda C: TURTLE}
EXTRA_MOVE = np.array([0.04, -0.04, 0.02], np.float32)      # one more row and column: a shift is pending again after the layers were written


def dress(m, C, constant_features=False):
    """the extra semantic layers and the traversability on one map, then a move: the circular origin is off zero and a shift is pending"""
    cls, feat = class_layers(C), feature_layers(C)
    if constant_features:
        # eighths from -0.5 to 1.375: every sum of them is exact in double, so the means are the values and every centred value is 0
        feat = np.broadcast_to((np.arange(16, dtype=np.float32) / np.float32(8) - np.float32(0.5))[:, None, None], feat.shape)
    for n in SEM_NAMES + FEAT_NAMES:
        m.semantic_map.add_layer(n)
    for k, n in enumerate(SEM_NAMES):
        m.semantic_map.set_layer(n, cls[k])
    if not constant_features:
        for k, n in enumerate(FEAT_NAMES):
            m.semantic_map.set_layer(n, feat[k])
    m.set_layer_raw("traversability", traversability_layer(C))
    m.move_to(gc.MOVE + EXTRA_MOVE, np.eye(3, dtype=np.float32))
    m.base_rotation = pc.TILT.copy()
    if constant_features:                  # (behind the move: the band a move clears in the semantic layers would not be constant)
        for k, n in enumerate(FEAT_NAMES):
            m.semantic_map.set_layer(n, feat[k])
    return m


def twins(C, entries, path, **kw):
    return [dress(m, C, **kw) for m in pc.twins(C, entries, path)]


# ---- the arithmetic of the four ops, restated on NumPy arrays ---------------------------------------------------------------------------------
def colour_of(index):
    """entry `index` (1-based) of the colour table by integer dealing: bit 3 j + ch of the index -> bit 7 - j of channel ch; 1, 2, 3 overridden"""
    index = np.asarray(index, np.uint32)
    rgb = [np.zeros(index.shape, np.uint32) for _ in range(3)]
    for j in range(8):
        for ch in range(3):
            rgb[ch] |= ((index >> np.uint32(3 * j + ch)) & np.uint32(1)) << np.uint32(7 - j)
    for idx, col in ((1, (81, 113, 162)), (2, (81, 113, 162)), (3, (188, 63, 59))):
        for ch in range(3):
            rgb[ch] = np.where(index == idx, np.uint32(col[ch]), rgb[ch])
    return (rgb[0] << np.uint32(16)) | (rgb[1] << np.uint32(8)) | rgb[2]


def filter_restated(sources, shape):
    """SEMANTIC_FILTER: the first NaN wins, otherwise the first maximum (a later value wins only when it is greater)"""
    best = np.zeros(shape, np.int64)
    if len(sources):
        bv = np.array(sources[0], np.float32)
        nan = np.isnan(bv)
        for k in range(1, len(sources)):
            v = np.asarray(sources[k], np.float32)
            take_nan = ~nan & np.isnan(v)
            with np.errstate(invalid="ignore"):
                take = ~nan & ~take_nan & (v > bv)
            best = np.where(take_nan | take, k, best)
            bv = np.where(take, v, bv)
            nan |= take_nan
    return colour_of(best + 1).astype(np.uint32).view(np.float32)


def trav_restated(sources, thresholds, at_most):
    """SEMANTIC_TRAV: the comparison in double, a NaN never votes, 1.0f where somebody voted and 0.1f elsewhere"""
    any_ = np.zeros(np.asarray(sources[0]).shape, bool)
    for s, t, le in zip(sources, thresholds, at_most):
        x = np.asarray(s, np.float32).astype(np.float64)
        with np.errstate(invalid="ignore"):
            any_ |= (x <= np.float64(t)) if le else (x >= np.float64(t))
    return np.where(any_, np.float32(1.0), np.float32(0.1)).astype(np.float32)


def max_layer_restated(sources, steps, take_min):
    """MAX_LAYER: per source dict(default=float | None, reverse=bool, scale=float | None, threshold=float | None), everything in float32;
    then acc = acc > x ? acc : x (acc < x for the minimum) in order, NaN if any source is NaN"""
    acc, nan = None, None
    for s, st in zip(sources, steps):
        x = np.array(s, np.float32)
        if st.get("default") is not None:
            x = np.where(x == np.float32(0), np.float32(st["default"]), x)
        if st.get("reverse"):
            x = np.float32(1.0) - x
        if st.get("scale") is not None:
            x = x * np.float32(st["scale"])
        if st.get("threshold") is not None:
            with np.errstate(invalid="ignore"):
                x = np.where(x > np.float32(st["threshold"]), np.float32(1), np.float32(0))
        x = x.astype(np.float32)
        if acc is None:
            acc, nan = x, np.isnan(x)
        else:
            with np.errstate(invalid="ignore"):
                acc = np.where((acc < x) if take_min else (acc > x), acc, x)
            nan = nan | np.isnan(x)
    return np.where(nan, np.float32(np.nan), acc).astype(np.float32)


def pca_restated(sources):
    """FEATURES_PCA as the device computes it: clip, double; means; the centred moments in a second pass; eigh; eigenvalues descending;
    the sign rule; scores; lo / hi / span; truncated levels packed 0x00RRGGBB.  sources: (F, C, C)"""
    src = np.asarray(sources, np.float32)
    shape = src.shape[1:]
    x = np.clip(src, np.float32(-1), np.float32(1)).reshape(len(src), -1).T.astype(np.float64)
    d = x - x.mean(axis=0)
    w, v = np.linalg.eigh(d.T @ d)
    order = np.argsort(-w, kind="stable")[:3]
    vecs = v[:, order].T
    big = np.argmax(np.abs(vecs), axis=1)
    sign = np.where(vecs[np.arange(3), big] < 0, -1.0, 1.0)
    scores = d @ (vecs * sign[:, None]).T
    lo, hi = scores.min(axis=0), scores.max(axis=0)
    span = np.where(hi > lo, hi - lo, 1.0)
    lev = ((scores - lo) / span * 255).astype(np.uint8).astype(np.uint32).reshape(shape + (3,))
    return ((lev[..., 0] << np.uint32(16)) | (lev[..., 1] << np.uint32(8)) | lev[..., 2]).view(np.float32)


def levels(packed):
    """(..., 3) int16 levels r, g, b of a packed colour plane"""
    u = np.ascontiguousarray(packed, np.float32).view(np.uint32)
    return np.stack([(u >> np.uint32(16)) & np.uint32(255), (u >> np.uint32(8)) & np.uint32(255), u & np.uint32(255)], axis=-1).astype(np.int16)


PCA_MAX_LEVEL = 1            # the PCA condition: levels differ by at most 1 per channel,
PCA_MAX_CELLS = 0.001        # and in at most 0.1 % of the cells


def pca_disagreement(got, ref):
    """(cells that differ, largest level difference, top byte clean) of two packed PCA planes"""
    d = np.abs(levels(got) - levels(ref))
    clean = not ((np.ascontiguousarray(got, np.float32).view(np.uint32) >> np.uint32(24)).any())
    return int((d.max(axis=-1) > 0).sum()), int(d.max()), clean


def pca_condition(got, ref, what=""):
    cells, lev, clean = pca_disagreement(got, ref)
    print("PCA %s: %d of %d cells differ, by at most %d levels" % (what, cells, np.asarray(ref).size, lev))
    assert clean, what
    assert lev <= PCA_MAX_LEVEL and cells <= PCA_MAX_CELLS * np.asarray(ref).size, "%s: %d cells differ, by up to %d levels" % (what, cells, lev)
