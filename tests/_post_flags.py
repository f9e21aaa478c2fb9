"""Scene and sequence table of tests/test_hip_post_flags.py and -- run as a program -- the child process that plays a PLAN on the GPU five
ways with whatever stencil tile height and split capacity the hooks of its environment select (read once per process):

    EMAP_TEST_FLAGS_PLAN=<plan.json> python tests/_post_flags.py <out.npz>

Without a visibility pass the stencil pass a frame takes along (tests/_post_lean.py) has one reader, the drift gate's test
traversability > traversability_inlier in k_tile_count.  POST_OUT_TRAV writes that predicate as a byte per cell into a flag plane and no
word into the hot half; the 3-cell border, which the stencils do not decide, gets "use the word you hold" (emap_api.hip: count_impl).
The five ways:
    "flags"  the default, nothing is read before the sequence is over
    "word"   EMAP_POST_FLAGS=0: the pass taken along stores the traversability word, as it did before there was a flag plane
    "full"   EMAP_POST_LEAN=0: the pass taken along writes everything
    "off"    EMAP_POST_DEFER=0: every frame launches its own pass
    "each"   the default, and the traversability plane is read after every step (a read launches what is owed)

The scenes of the other stencil tests (uniform noise) give the gate next to nothing to decide: a few inliers per frame, it never fires.
Here the cloud samples a smooth surface whose roughness grows across the map, so thousands of points per frame pass the other three
inlier conditions and the traversability of their cells spreads over 0.4 .. 1; the PARENT plays every sequence on the oracle first, takes
traversability_inlier from the oracle's traversability plane (a quantile over the cells that receive such points) and hands the values
to the child in the plan -- the child never sees the oracle."""
import ctypes as ct
import json
import os
import sys

import numpy as np

import _post_deferred as pd

MAPS = pd.MAPS
WAYS = ("flags", "word", "full", "off", "each")
RES = 0.04
CH = ["x", "y", "z", "s0", "s1", "c0", "rgb"]                                   # as tests/test_hip_frame_semantics.py
FUSIONS = {"rgb": "color", "c0": "class_average", "default": "average"}
PATCH = ((51.2, 56.8), (71.2, 76.8))      # cell-index ranges of the heavy patch: inside ONE 16 x 64 tile whichever axis is the row and whichever way it runs
HEAVY_EXTRA = 6000                        # points of the patch: more than the 4096 records a tile workgroup takes before it is split

# name -> (maps, steps).  A step: ("frame", seed, n points[, want stats]) | ("heavy", seed, n[, stats]) = a frame whose cloud piles
# HEAVY_EXTRA points into PATCH | ("sem", seed, n) = a frame that declares a semantic fusion (32-byte records) | ("shift", rows, cols) |
# ("thr", q) = emap_set_params with traversability_inlier at quantile q of the traversability of the next frame's candidate cells |
# ("border",) = emap_set_layer(traversability) with the 3-cell border set to a checkerboard of 0.99 / 0.01.
SEQUENCES = {
    "run5": ("abcd", [("frame", 1, 30000), ("frame", 2, 30000), ("frame", 3, 4097), ("frame", 4, 30000), ("frame", 5, 30000, True)]),
    "stats": ("ab", [("frame", 6, 30000), ("frame", 7, 30000, True), ("frame", 8, 30000), ("frame", 9, 4097, True)]),
    "shifted": ("cd", [("shift", 5, 37), ("frame", 10, 30000), ("frame", 11, 30000), ("frame", 12, 30000), ("frame", 13, 30000, True)]),
    "heavy": ("ab", [("frame", 14, 30000), ("heavy", 15, 30000), ("heavy", 16, 30000), ("heavy", 17, 30000, True)]),
    "rs2": ("ad", [("frame", 18, 30000), ("sem", 19, 30000), ("sem", 20, 30000), ("frame", 21, 30000, True)]),
    "thr_change": ("bc", [("frame", 22, 30000), ("frame", 23, 30000), ("frame", 24, 30000, True), ("thr", 0.3), ("frame", 25, 30000), ("frame", 26, 30000), ("frame", 27, 30000, True)]),
    "border": ("abcd", [("frame", 28, 30000), ("frame", 29, 30000), ("border",), ("frame", 30, 30000), ("frame", 31, 30000), ("frame", 32, 30000, True)]),
}
FRAME_STEPS = ("frame", "heavy", "sem")
# Bits 16 | 32 of emap_last_update_path per FRAME for the ways "flags" and "word", from the rules of tests/_post_lean.py: a frame takes
# the pass along (lean: 16, the gate is open in every frame here) when the frame before it was a binned whole-map frame and nothing
# entered the library in between -- emap_shift, emap_set_params, emap_set_layer and emap_get_stats behind a frame with a stats pointer
# all launch the owed pass in full.  The other three ways: 0 for every frame.
LEAN_BITS = {
    "run5": [0, 16, 16, 16, 16],
    "stats": [0, 16, 0, 16],
    "shifted": [0, 16, 16, 16],
    "heavy": [0, 16, 16, 16],
    "rs2": [0, 0, 16, 16],                # (the first frame that declares a fusion adds the layers: emap_sem_ensure launches the owed pass)
    "thr_change": [0, 16, 16, 0, 16, 16],
    "border": [0, 16, 0, 16, 16],
}


def cloud(C, seed, n, kind="frame"):
    """n points (sensor frame, pose pd.pose()) of a surface fixed in the map frame: a smooth wave + a per-cell offset whose amplitude
    grows with x from 0 to 5 cm + 2 mm of noise + a drift of 0 .. 8 mm that changes with the seed (so the error sums are not zero);
    NaN rows as the other stencil tests have them.  "heavy": HEAVY_EXTRA more points inside PATCH; "sem": four channel columns."""
    rng = np.random.default_rng(seed)
    R, t = pd.pose()
    L = C * RES / 2 * 0.995      # (into the 3-cell border, which the stencils do not decide)
    x, y = rng.uniform(-L, L, n), rng.uniform(-L, L, n)
    if kind == "heavy":
        (a0, a1), (b0, b1) = PATCH
        x = np.concatenate([x, rng.uniform((a0 - C / 2) * RES, (a1 - C / 2) * RES, HEAVY_EXTRA)])
        y = np.concatenate([y, rng.uniform((b0 - C / 2) * RES, (b1 - C / 2) * RES, HEAVY_EXTRA)])
    ix, iy = np.floor(x / RES), np.floor(y / RES)
    h = np.sin(ix * 12.9898 + iy * 78.233) * 43758.5453
    z = 0.12 * np.sin(2.0 * x) * np.cos(1.5 * y) + 0.05 * (x + L) / (2 * L) * (h - np.floor(h) - 0.5) + 0.002 * (seed % 5) + rng.normal(0, 0.002, x.size)
    pm = np.stack([x, y, z], 1)
    p = ((pm - t.astype(np.float64)) @ R.astype(np.float64)).astype(np.float32)
    if kind == "sem":
        ch = rng.uniform(0, 1, (p.shape[0], 4)).astype(np.float32)
        ch[:, 3] = rng.integers(0, 1 << 24, p.shape[0], dtype=np.uint32).view(np.float32)
        p = np.concatenate([p, ch], axis=1)
    p[seed % 7::97, :3] = np.nan
    return np.ascontiguousarray(p)


def border_plane(trav):
    """the plane of the ("border",) step: `trav` with its 3-cell border set to a checkerboard of 0.99 / 0.01 (float32)"""
    a = np.array(trav, np.float32)
    C = a.shape[0]
    i, j = np.meshgrid(np.arange(C), np.arange(C), indexing="ij")
    ring = (i < 3) | (i >= C - 3) | (j < 3) | (j >= C - 3)
    a[ring] = np.where((i + j) % 2 == 0, np.float32(0.99), np.float32(0.01))[ring]
    return a


def key_of(name, m, way):
    return "%s_%s_%s" % (name, m, way)


class Player:
    """plays steps on a HIP map; thr: the resolved thresholds of the ("thr", q) steps, in order"""

    def __init__(self, rt, hip, C, way, thr):
        self.rt, self.hip, self.C, self.way, self.thr, self.dev = rt, hip, C, way, list(thr), []
        self.bits, self.paths, self.stats = [], [], []

    def step(self, s):
        h = self.hip
        R, t = pd.pose()
        if s[0] in FRAME_STEPS:
            p = cloud(self.C, s[1], s[2], s[0])
            want = len(s) > 3 and bool(s[3])
            d = self.rt.malloc(p.nbytes); self.rt.h2d(d, p); self.dev.append(d)      # (a device-resident cloud: an upload would launch the owed pass)
            h.bind_points_device(d.value, p.shape[0], p.shape[1])
            st = h.update_map_with_kernel(None, CH[3:] if s[0] == "sem" else [], R, t.copy(), 1.0, 1.0, want_stats=want)
            v = ct.c_int32(-1)
            h._chk(h._lib.emap_last_update_path(h._ctx, ct.byref(v)))
            self.bits.append(int(v.value)); self.paths.append(h.last_update_path())
            self.stats.append([float(st.err_sum), float(st.err_cnt), float(st.gate_fired)] if want else [np.nan, -1.0, -1.0])
        elif s[0] == "shift":
            h.shift_map_xy(np.array([s[1], s[2]]))
        elif s[0] == "thr":
            h.param.traversability_inlier = float(self.thr.pop(0))
            h.reload_params()
        elif s[0] == "border":
            h.set_layer_raw("traversability", border_plane(np.array(h.elevation_map)[3]))
        if self.way == "each":
            np.array(h.elevation_map)

    def finish(self, out, key):
        h = self.hip
        out[key + "_map"] = np.array(h.elevation_map, np.float32)
        out[key + "_normal"] = np.array(h.normal_map, np.float32)
        out[key + "_trav_in"] = np.array(h.traversability_input, np.float32)
        out[key + "_add"] = np.array([h.get_additive_mean_error()], np.float64)
        v = ct.c_uint32(0)
        h._chk(h._lib.emap_post_fused_launches(h._ctx, ct.byref(v)))
        out[key + "_fused"] = np.array([int(v.value)], np.int64)
        out[key + "_bits"] = np.array(self.bits, np.int64)
        out[key + "_paths"] = np.array(",".join(self.paths))
        out[key + "_stats"] = np.array(self.stats, np.float64).reshape(-1, 3)
        h.sync()
        h.close()
        for d in self.dev:
            self.rt.free(d)


def make(weights, C, mode, thr0, sem):
    from _util import make_pair
    hip, _ = make_pair(dict(pd.config({}), traversability_inlier=float(thr0)), C, mode, weights)
    hip.set_scatter_mode("binned")
    if sem:
        hip.param.pointcloud_channel_fusions = dict(FUSIONS)
    return hip


def main(path):
    from _variant_children import child_setup
    weights = child_setup()
    import bench
    with open(os.environ["EMAP_TEST_FLAGS_PLAN"]) as f:
        plan = json.load(f)                 # [{"name", "map", "thr0", "thr": [...]}]
    rt = bench.Hip()
    out = {}
    for way in WAYS:
        os.environ["EMAP_POST_DEFER"] = "0" if way == "off" else "1"
        os.environ["EMAP_POST_LEAN"] = "0" if way == "full" else "1"
        os.environ["EMAP_POST_FLAGS"] = "0" if way == "word" else "1"
        for case in plan:
            name, m = case["name"], case["map"]
            C, mode = MAPS[m]
            steps = SEQUENCES[name][1]
            pl = Player(rt, make(weights, C, mode, case["thr0"], any(s[0] == "sem" for s in steps)), C, way, case["thr"])
            for s in steps:
                pl.step(s)
            pl.finish(out, key_of(name, m, way))
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
