"""What the tests of the inpainting op of the plugin chain share (EMAP_PLUGIN_INPAINT_FRONTS; tests/test_inpaint_chain_cases.py on the CPU,
tests/test_hip_inpaint_chain.py and its child tests/_inpaint_chain_child.py on the GPU): the plugin configurations, the map states the
op runs on, and the NumPy restatement of what plugins/inpainting.py does around the fill, every rounding to float32 written out.

The yardstick of every value on the GPU is the plugin's HOST route of method "telea_fronts" on a twin map (tests/_plug_cases.py)."""
import numpy as np

import _grid_cases as gc
import _plug_cases as pc
import _telea_fronts as tf

F32 = np.float32
SIZES = gc.SIZES                     # 10: one partial fronts tile; 34, 67, 100: 2, 3, 4 tiles of 30 per axis at S = 16
STEPS = (0, 1, 4, 16)
HOLED = ("start", "block")           # states with known and unknown cells and a spread of heights
DEGENERATE = ("none", "all_valid", "constant")


def _inpaint(layer, fill_nan=False, height=False, **extra):
    return pc._entry("inpainting", layer, fill_nan=fill_nan, height=height, method="telea_fronts", **extra)


# the shipped core configuration with the device method named
CORE_FRONTS = [e if e[0] != "inpaint" else _inpaint("inpaint", height=True) for e in pc.CORE]
PUBLISHED = ["inp_00", "inp_01", "inp_10", "inp_11"]                   # fill_nan x is_height_layer
STEP_LAYERS = ["inp_01"] + ["inp_s%d" % s for s in STEPS[1:]]          # i0 = 0, 1, 4, 16


def ops_config():
    return [_inpaint("inp_%d%d" % (f, h), fill_nan=f, height=h) for f in (0, 1) for h in (0, 1)] + \
           [_inpaint("inp_s%d" % s, height=True, steps=s) for s in STEPS[1:]]


# ---- the states ---------------------------------------------------------------------------------------------------------------------------
def elevation_plane(C, seed=21):
    """heights on both sides of zero, no symmetry"""
    r, c = np.meshgrid(np.arange(C, dtype=np.float64), np.arange(C, dtype=np.float64), indexing="ij")
    noise = np.random.default_rng(seed).uniform(-0.05, 0.05, (C, C))
    return (0.4 * np.sin(0.31 * r) + 0.3 * np.cos(0.23 * c + 0.4) - 0.35 + 0.002 * r + noise).astype(F32)


def case_planes(C, case):
    """(elevation, is_valid) that ``apply_case`` writes, or None for the cases that write no layer ("start", "none")"""
    h = elevation_plane(C)
    v = np.zeros((C, C), F32)
    if case == "block":              # an L of known cells in one corner: the hole touches three borders, max d is far beyond 16 from 34 on
        v[:3, :max(3, C // 3)] = 1.0
        v[:max(2, C // 4), :2] = 1.0
        v[1, 1] = 0.5                # known for THIS plugin (>= 0.5), not valid for fill_nan (> 0.5)
        v[C // 2, C // 2] = 0.49     # unknown
    elif case == "corner":           # ONE known cell in a corner: max d = 2 C - 2, the geometric bound itself
        v[C - 1, 0] = 1.0
    elif case == "constant":         # no spread: span = 1
        h = np.full((C, C), 0.25, F32)
        v = (np.random.default_rng(5).uniform(0.0, 1.0, (C, C)) < 0.6).astype(F32)
    elif case == "all_valid":
        v[...] = 1.0
    else:
        return None
    return h, v


def apply_case(m, C, case):
    """bring a map of _grid_cases.start into the state `case`.  "start" keeps the start state (holes between the frames' points, a shift
    pending); writing a layer writes the pending shift out, so the written states have their circular origin off zero and no shift pending"""
    if case == "none":
        m.clear()
    elif case != "start":
        h, v = case_planes(C, case)
        m.set_layer_raw("elevation", h)
        m.set_layer_raw("is_valid", v)


def twins(C, entries, path, case="start"):
    pair = pc.twins(C, entries, path)
    for m in pair:
        apply_case(m, C, case)
    return pair


# ---- plugins/inpainting.py around the fill, restated with explicit float32 roundings -------------------------------------------------------
def known_of(valid):
    return np.asarray(valid, F32) >= F32(0.5)


def inpaint_range(h, valid):
    """(h_min, span) as float32, or None where the plugin returns the elevation as it is (no known cell, or every cell known)"""
    k = known_of(valid)
    if not k.any() or k.all():
        return None
    x = np.asarray(h, F32)[k]
    lo, hi = x.min(), x.max()
    span = F32(np.float64(hi) - np.float64(lo)) if hi > lo else F32(1.0)
    return lo, span


def inpaint_quantise(h, lo, span):
    v = (np.asarray(h, F32) - lo) * F32(255) / span                    # three float32 operations
    assert v.dtype == F32
    return np.trunc(np.minimum(np.maximum(v, F32(0)), F32(255))).astype(np.uint8)


def inpaint_dequantise(out8, lo, span):
    v = np.asarray(out8).astype(F32) * span / F32(255) + lo            # three float32 operations
    assert v.dtype == F32
    return v


def inpaint_plane(h, valid, fill=tf.inpaint_fronts):
    """the plane the op leaves: float32, (C, C), border included"""
    r = inpaint_range(h, valid)
    if r is None:
        return np.asarray(h, F32)
    q8 = inpaint_quantise(h, *r)
    return inpaint_dequantise(fill(q8, (~known_of(valid)).astype(np.uint8)), *r)


def range_layers(C=12, seed=3):
    """(elevation, is_valid) pairs the restatement is checked on: negative heights, both zeros, a constant, a range whose double
    difference is no float32, a known cell at is_valid == 0.5, unknown cells beyond the known range on both sides (the clip)"""
    rng = np.random.default_rng(seed)
    mask = (rng.uniform(0.0, 1.0, (C, C)) < 0.7).astype(F32)
    mask[0, 0], mask[0, 1] = 1.0, 0.0
    neg = rng.uniform(-3.0, -1.0, (C, C)).astype(F32)
    zeros = np.zeros((C, C), F32); zeros[::2] = -0.0; zeros[0, 0] = 0.5
    zeros_only = np.zeros((C, C), F32); zeros_only[::2] = -0.0
    odd = rng.uniform(0.0, 1.0, (C, C)).astype(F32); odd[0, 0] = F32(1.0); odd[1, 1] = F32(-2.0 ** -30)
    odd_mask = mask.copy(); odd_mask[1, 1] = 1.0
    assert F32(np.float64(odd.max()) - np.float64(odd.min())) != np.float64(odd.max()) - np.float64(odd.min())
    half = mask.copy(); half[2, 2] = 0.5; half[3, 3] = np.nextafter(F32(0.5), F32(0))
    clip = rng.uniform(0.0, 1.0, (C, C)).astype(F32); clip[0, 1] = 7.0; clip[5, 5] = -7.0
    clip_mask = mask.copy(); clip_mask[5, 5] = 0.0
    return {"negative": (neg, mask), "zeros": (zeros, mask), "zeros only": (zeros_only, mask), "constant": (np.full((C, C), 0.25, F32), mask),
            "odd span": (odd, odd_mask), "half": (rng.uniform(-1.0, 1.0, (C, C)).astype(F32), half), "clip": (clip, clip_mask),
            "none known": (neg, np.zeros((C, C), F32)), "all known": (neg, np.ones((C, C), F32))}
