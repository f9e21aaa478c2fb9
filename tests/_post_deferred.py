"""Sequence table of tests/test_hip_post_deferred.py and -- run as a program -- the child process that plays every sequence on the GPU
three ways with whatever stencil tile height the EMAP_POST_* hooks of its environment select (read once per process):

    python tests/_post_deferred.py <out.npz>

A whole-map frame on the binned path leaves its stencil pass pending; the next such frame runs it in one launch with its own histogram
(k_post_hist), every other call launches it first (emap_api.hip: frame_impl, post_settle).  The three ways:
    "end"   deferral on, the planes are read only when the sequence is over
    "each"  deferral on, the planes are read after every step (every read launches a pending pass: today's launches)
    "off"   EMAP_POST_DEFER=0
The parent compares the three bit for bit, with the oracle, and checks the counter of fused launches each way."""
import ctypes as ct
import os
import sys

import numpy as np

# (cell_n, index mode) of a sequence: 202 = interior tiles for both tile heights, 130 = a last tile of 2 rows by 2 columns
MAPS = {"a": (202, "reference_fp16"), "b": (130, "fp32"), "c": (130, "reference_fp16"), "d": (202, "fp32")}
BIG = 131072 + 64                 # a cloud that takes the binned path in auto mode (BIN_MIN_POINTS of emap_api.hip)
WAYS = ("end", "each", "off")

# name -> (maps, configuration, steps).  A step: ("frame", seed, n points) | ("shift", rows, cols) | ("vartime",) | ("clear",) |
# ("staged",) = emap_dilate + emap_post_part(0) | ("max_wg", n) = EMAP_POST_FUSE_MAX_WG from here on | ("timing", on).
# Clouds of 1, 4097 and 20000 points: fewer than 8 chunks, a chunk count that is no multiple of 8 with a last chunk of one point, and
# a last partial chunk; every cloud of more than 16 points carries NaN rows.
SEQUENCES = {
    "four_frames": ("abcd", {}, [("frame", 1, 20000), ("frame", 2, 1), ("frame", 3, 4097), ("frame", 4, 20000)]),
    "shift": ("ab", {}, [("frame", 5, 4097), ("shift", 3, -2), ("frame", 6, 20000)]),
    "vartime": ("cd", {}, [("frame", 7, 20000), ("vartime",), ("frame", 8, 4097)]),
    "small_between": ("a", {"auto": True}, [("frame", 9, BIG), ("frame", 10, 3000), ("frame", 11, BIG), ("frame", 12, BIG)]),
    "rays": ("ab", {"rays": True}, [("frame", 13, 20000), ("vartime",), ("frame", 14, 20000), ("frame", 15, 20000), ("frame", 25, 4097)]),
    "staged": ("ac", {}, [("frame", 16, 20000), ("staged",), ("frame", 17, 4097)]),
    "clear": ("bd", {}, [("frame", 18, 20000), ("clear",), ("frame", 19, 20000)]),
    "max_wg": ("a", {}, [("max_wg", 8), ("frame", 20, 20000), ("frame", 21, 4097), ("frame", 22, 20000)]),
    "timing": ("b", {}, [("timing", 1), ("frame", 23, 20000), ("frame", 24, 20000)]),
}
# binned frames that can take the pass of the frame before them along ("end"): consecutive binned frames with nothing between them
FUSED_END = {"four_frames": 3, "shift": 0, "vartime": 0, "small_between": 1, "rays": 2, "staged": 0, "clear": 0, "max_wg": 0, "timing": 0}
TWO_CONTEXTS = [("frame", 31, 20000), ("frame", 32, 4097), ("frame", 33, 20000)]      # per context, alternating; fused: 2 each
CLOSE_PENDING = [("frame", 41, 20000), ("frame", 42, 20000)]                          # then close with the pass pending


def config(opts):
    from oracle import emap_oracle as eo
    if opts.get("rays"):
        return dict(eo.YAML)                                                         # visibility pass + overlap clearance on
    return dict(eo.YAML, enable_visibility_cleanup=False, enable_overlap_clearance=False)


def cloud(C, seed, n):
    import _fixtures as fx
    p = fx.cloud(C, n, seed, dz=-0.01 * (seed % 5))
    if n > 16:
        p[seed % 7::97] = np.nan
    return p


def pose():
    import _fixtures as fx
    return fx.POSES["rotated"]


def play_oracle(orc, steps):
    R, t = pose()
    for s in steps:
        if s[0] == "frame":
            orc.update_map_with_kernel(cloud(orc.C, s[1], s[2]), R, t, 1.0, 1.0)
        elif s[0] == "shift":
            orc.shift_map_xy(np.array([s[1], s[2]]))
        elif s[0] == "vartime":
            orc.update_variance(); orc.update_time()
        elif s[0] == "clear":
            orc.elevation_map[...] = 0; orc.elevation_map[1] = np.float32(orc.P.initial_variance)
            orc.mean_error = 0.0; orc.additive_mean_error = np.float32(0.0)
        elif s[0] == "staged":
            orc.dilate(); orc.traversability(); orc.normals()


class Player:
    """plays steps on a HIP map from device-resident clouds"""

    def __init__(self, rt, hip, C, way):
        self.rt, self.hip, self.C, self.way, self.dev, self.paths = rt, hip, C, way, [], []

    def fused(self):
        v = ct.c_uint32(0)
        self.hip._chk(self.hip._lib.emap_post_fused_launches(self.hip._ctx, ct.byref(v)))
        return int(v.value)

    def planes(self):
        h = self.hip
        return np.array(h.elevation_map), np.array(h.normal_map), np.array(h.traversability_input)

    def step(self, s):
        h = self.hip
        R, t = pose()
        if s[0] == "frame":
            p = cloud(self.C, s[1], s[2])
            d = self.rt.malloc(p.nbytes); self.rt.h2d(d, p); self.dev.append(d)
            h.bind_points_device(d.value, p.shape[0], 3)
            h.update_map_with_kernel(None, [], R, t.copy(), 1.0, 1.0, want_stats=False)
            self.paths.append(h.last_update_path())
        elif s[0] == "shift":
            h.shift_map_xy(np.array([s[1], s[2]]))
        elif s[0] == "vartime":
            h.update_variance(); h.update_time()
        elif s[0] == "clear":
            h.clear()
        elif s[0] == "staged":
            h.stage("dilate"); h._chk(h._lib.emap_post_part(h._ctx, 0))
        elif s[0] == "max_wg":
            os.environ["EMAP_POST_FUSE_MAX_WG"] = str(s[1])
        elif s[0] == "timing":
            h._chk(h._lib.emap_enable_stage_timing(h._ctx, int(s[1])))
        if self.way == "each":
            self.planes()

    def finish(self, out, key):
        m, n, ti = self.planes()
        out[key + "_map"], out[key + "_normal"], out[key + "_trav_in"] = m, n, ti
        out[key + "_fused"] = np.array([self.fused()], np.int64)
        self.hip.sync()
        self.hip.close()
        for d in self.dev:
            self.rt.free(d)


def make(weights, C, mode, opts):
    from _util import make_pair
    hip, _ = make_pair(config(opts), C, mode, weights)
    hip.set_scatter_mode("auto" if opts.get("auto") else "binned")
    return hip


def key_of(name, m, way):
    return "%s_%s_%s" % (name, m, way)


def main(path):
    from _variant_children import child_setup
    weights = child_setup()
    import bench
    rt = bench.Hip()
    out = {}
    for way in WAYS:
        os.environ["EMAP_POST_DEFER"] = "0" if way == "off" else "1"
        for name, (maps, opts, steps) in SEQUENCES.items():
            for m in maps:
                os.environ.pop("EMAP_POST_FUSE_MAX_WG", None)
                C, mode = MAPS[m]
                pl = Player(rt, make(weights, C, mode, opts), C, way)
                for s in steps:
                    pl.step(s)
                out[key_of(name, m, way) + "_paths"] = np.array(",".join(pl.paths))
                if name == "timing":
                    ms = (ct.c_float * 10)()
                    pl.hip._chk(pl.hip._lib.emap_get_stage_times(pl.hip._ctx, ms))
                    out[key_of(name, m, way) + "_stage_ms"] = np.array(list(ms), np.float32)
                pl.finish(out, key_of(name, m, way))
        os.environ.pop("EMAP_POST_FUSE_MAX_WG", None)
        # two contexts alternating: each keeps its own pending pass
        C, mode = MAPS["a"]
        two = [Player(rt, make(weights, C, mode, {}), C, way) for _ in range(2)]
        for i, s in enumerate(TWO_CONTEXTS):
            for k, pl in enumerate(two):
                pl.step((s[0], s[1] + 100 * k, s[2]))
        for k, pl in enumerate(two):
            pl.finish(out, key_of("two_contexts%d" % k, "a", way))
        # close with the pass pending: nothing may fault, and a context created afterwards works
        pl = Player(rt, make(weights, C, mode, {}), C, way)
        for s in CLOSE_PENDING:
            pl.step(s)
        pl.hip.close()                            # (the counter is not read: reading it would launch the pass)
        for d in pl.dev:
            rt.free(d)
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
