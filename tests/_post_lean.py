"""Sequence table of tests/test_hip_post_lean.py and -- run as a program -- the child process that plays every sequence on the GPU four
ways with whatever stencil tile height the EMAP_POST_* hooks of its environment select (read once per process):

    python tests/_post_lean.py <out.npz>

A frame that takes the pending stencil pass of the frame before along in its histogram launch (tests/_post_deferred.py) lets it write
only what the frame itself reads -- traversability for the drift statistics, the normals too in front of a visibility pass -- and a
frame that reads nothing of it (drift gate ruled out, no visibility pass) launches no stencil workgroup at all; either way the pass
stays owed until a full pass has run (emap_api.hip: count_impl, post_settle).  The four ways:
    "lean"  the default, the planes are read only when the sequence is over
    "full"  EMAP_POST_LEAN=0: the pass taken along writes everything
    "off"   EMAP_POST_DEFER=0: every frame launches its own pass
    "each"  the default, and traversability_input and the normals are read after every step (a read launches what is owed)
The parent compares the four bit for bit, with the oracle, and checks bits 16 (taken along lean) and 32 (left owed without a launch) of
emap_last_update_path for every frame of every way."""
import ctypes as ct
import os
import sys

import numpy as np

import _post_deferred as pd

MAPS, BIG = pd.MAPS, pd.BIG
WAYS = ("lean", "full", "off", "each")
OPEN, SHUT = 1.0, 0.0             # position / orientation noise of a frame: above the thresholds (the drift gate may fire) or not

# name -> (maps, options, steps).  A step: ("frame", seed, n points, noise[, want stats]) | ("rays", on) = emap_set_params with the
# visibility pass switched | ("shift", rows, cols) | ("vartime",)
SEQUENCES = {
    "open4": ("abcd", {}, [("frame", 1, 20000, OPEN), ("frame", 2, 1, OPEN), ("frame", 3, 4097, OPEN), ("frame", 4, 20000, OPEN)]),
    "shut4": ("ab", {}, [("frame", 5, 20000, SHUT), ("frame", 6, 4097, SHUT), ("frame", 7, 20000, SHUT), ("frame", 8, 20000, SHUT)]),
    "alternate": ("cd", {}, [("frame", 9, 20000, OPEN), ("frame", 10, 20000, SHUT), ("frame", 11, 4097, OPEN), ("frame", 12, 20000, SHUT), ("frame", 13, 20000, OPEN)]),
    "rays_between": ("ab", {}, [("frame", 14, 20000, OPEN), ("frame", 15, 20000, OPEN), ("rays", 1), ("frame", 16, 20000, OPEN), ("frame", 17, 20000, SHUT),
                                ("frame", 18, 4097, OPEN), ("rays", 0), ("frame", 19, 20000, SHUT), ("frame", 20, 20000, OPEN)]),
    "shift": ("cd", {}, [("frame", 21, 20000, OPEN), ("frame", 22, 4097, OPEN), ("shift", 3, -2), ("frame", 23, 20000, OPEN), ("frame", 24, 20000, OPEN)]),
    "vartime": ("ab", {}, [("frame", 25, 20000, OPEN), ("frame", 26, 20000, SHUT), ("vartime",), ("frame", 27, 4097, OPEN), ("frame", 28, 20000, OPEN)]),
    "small_between": ("a", {"auto": True}, [("frame", 29, BIG, OPEN), ("frame", 30, BIG, OPEN), ("frame", 31, 3000, OPEN), ("frame", 32, BIG, OPEN), ("frame", 33, BIG, SHUT)]),
    "stats": ("cd", {}, [("frame", 34, 20000, OPEN, True), ("frame", 35, 20000, OPEN), ("frame", 36, 4097, OPEN, True), ("frame", 37, 20000, OPEN), ("frame", 38, 20000, OPEN)]),
}
# Bits 16 | 32 of emap_last_update_path per FRAME, way "lean", worked out from the rules: a frame takes a pass along when the frame
# before it was a binned whole-map frame and nothing entered the library in between (emap_set_params, emap_shift, emap_update_variance /
# _time and emap_get_stats behind a frame with a stats pointer all launch the owed pass in full); it runs lean (16) when it reads
# something -- gate open, or a visibility pass, which never goes beyond dropping traversability_input -- and is skipped (32) with the gate shut
# and no visibility pass.  The other three ways: 0 for every frame.
LEAN_BITS = {
    "open4": [0, 16, 16, 16],
    "shut4": [0, 32, 32, 32],
    "alternate": [0, 32, 16, 32, 16],
    "rays_between": [0, 16, 0, 16, 16, 0, 16],
    "shift": [0, 16, 0, 16],
    "vartime": [0, 32, 0, 16],
    "small_between": [0, 16, 0, 0, 32],
    "stats": [0, 0, 16, 0, 16],
}
RAY_FRAMES = {"rays_between": [2, 3, 4]}      # frames that run a visibility pass: bit 32 never, whatever the gate


def play_oracle(orc, steps):
    R, t = pd.pose()
    for s in steps:
        if s[0] == "frame":
            orc.update_map_with_kernel(pd.cloud(orc.C, s[1], s[2]), R, t, s[3], s[3])
        elif s[0] == "rays":
            orc.P.enable_visibility_cleanup = int(s[1])
        else:
            pd.play_oracle(orc, [s])


class Player(pd.Player):
    """pd.Player with a noise per frame, the raw path word per frame and the parameter switch"""

    def __init__(self, rt, hip, C, way):
        pd.Player.__init__(self, rt, hip, C, way)
        self.bits = []

    def step(self, s):
        h = self.hip
        if s[0] == "frame":
            R, t = pd.pose()
            p = pd.cloud(self.C, s[1], s[2])
            d = self.rt.malloc(p.nbytes); self.rt.h2d(d, p); self.dev.append(d)
            h.bind_points_device(d.value, p.shape[0], 3)
            h.update_map_with_kernel(None, [], R, t.copy(), s[3], s[3], want_stats=len(s) > 4 and bool(s[4]))
            v = ct.c_int32(-1)
            h._chk(h._lib.emap_last_update_path(h._ctx, ct.byref(v)))
            self.paths.append(h.last_update_path()); self.bits.append(int(v.value))
        elif s[0] == "rays":
            h.param.enable_visibility_cleanup = bool(s[1])
            h.reload_params()
        else:
            pd.Player.step(self, s)
            return
        if self.way == "each":
            np.array(h.normal_map), np.array(h.traversability_input)


def main(path):
    from _variant_children import child_setup
    weights = child_setup()
    import bench
    rt = bench.Hip()
    out = {}
    for way in WAYS:
        os.environ["EMAP_POST_DEFER"] = "0" if way == "off" else "1"
        os.environ["EMAP_POST_LEAN"] = "0" if way == "full" else "1"
        for name, (maps, opts, steps) in SEQUENCES.items():
            for m in maps:
                C, mode = MAPS[m]
                pl = Player(rt, pd.make(weights, C, mode, opts), C, "each" if way == "each" else "end")
                for s in steps:
                    pl.step(s)
                key = pd.key_of(name, m, way)
                out[key + "_paths"] = np.array(",".join(pl.paths))
                out[key + "_bits"] = np.array(pl.bits, np.int64)
                pl.finish(out, key)
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
