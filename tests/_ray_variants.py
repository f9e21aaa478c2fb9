"""Case table of tests/test_hip_ray_variants.py and test_ray_variant_cases.py, and -- run as a program -- the child process that executes
every case on the GPU with whatever k_rays variant the EMAP_RAY_* hooks of its environment select (emap_kernels.hip: launch_rays_i reads
EMAP_RAY_LMAP and EMAP_RAY_WINDOW once per process; emap_api.hip: build_ray_tables reads EMAP_RAY_IDX; so one process is one variant):

    python tests/_ray_variants.py <out.npz>

Every case is two whole frames with rays and overlap clearance on a fresh context.  The parent runs the same calls on the oracle
(run_case) and compares the recorded arrays."""
import sys

import numpy as np

RES = 0.04
FRAME_DZ = (0.0, -0.2)
TIME_TICKS = 10                   # update_time() calls after each frame: the second frame then meets cells of every age class

# `t`: sensor position in metres relative to the map centre.  `move`: cells the map is moved by between the two frames (the circular
# origin is then off zero when the second frame's bitmap is read).  `window`: (r0, nr, w0, wpr) -- first row, rows, first 32-bit word
# column, word columns of the part of the inert bitmap a windowed LDS launch stages, None where no window applies.  Derived BY HAND from
# the rule "per axis: rows / columns within max_ray_length * 1.004 + (|t_axis| + max_ray_length) * (1/512 in reference_fp16, 1e-5 in fp32)
# + 2 cells of the sensor's coordinate on that axis, floored, widened by 2 cells, clamped to the map; columns widened to whole pieces of
# 128; refused when the map's row of ceil(C / 64) 64-bit words is no whole number of pieces, or when nothing is saved" and kept as
# literals on purpose.  (`outside`: the sensor stands 0.62 m beyond row 0 -- at 0.9 m no ray reaches 44 columns sideways inside the
# map, which tests/test_ray_variant_cases.py asks of every side; rows: D = 2.008 + 10.3/512 + 0.08 = 2.108 m, last row
# floor(192 - 207.5 + 52.7) + 2 = 39.)  E.g. centre384:
# D = 2.008 + 2/512 + 0.08 = 2.0919 m = 52.3 cells; rows floor(192 - 52.3) - 2 = 137 ... floor(192 + 52.3) + 2 = 246: 110 rows; columns
# 137 ... 246 lie in piece 1 (columns 128 ... 255): w0 = 4, wpr = 4.  piece_lo: t_y = -0.36 m = -9 cells, first column 137 - 9 = 128;
# one cell lower (piece_lo-1) it is 127 and piece 0 joins.
CASES = [
    dict(key="centre384", C=384, mode="reference_fp16", mrl=2.0, t=(0.0, 0.0, 1.0), pose="identity", N=140000, move=None, window=(137, 110, 4, 4)),
    dict(key="rot384", C=384, mode="reference_fp16", mrl=2.0, t=(0.3, -0.2, 1.1), pose="rotated", N=140000, move=(3, 2), window=(145, 109, 4, 4)),
    dict(key="piece_lo", C=384, mode="reference_fp16", mrl=2.0, t=(0.0, -0.36, 1.0), pose="rotated", N=140000, move=None, window=(137, 110, 4, 4)),
    dict(key="piece_lo-1", C=384, mode="reference_fp16", mrl=2.0, t=(0.0, -0.40, 1.0), pose="rotated", N=140000, move=None, window=(137, 110, 0, 8)),
    dict(key="two_pieces", C=384, mode="reference_fp16", mrl=2.0, t=(0.0, 2.8, 1.0), pose="identity", N=140000, move=None, window=(137, 110, 4, 8)),
    dict(key="corner_a", C=384, mode="reference_fp16", mrl=2.0, t=(-7.0, 6.9, 1.0), pose="rotated", N=140000, move=None, window=(0, 72, 8, 4)),
    dict(key="corner_b", C=384, mode="reference_fp16", mrl=2.0, t=(7.5, -7.5, 1.0), pose="rotated", N=140000, move=(-5, 7), window=(324, 60, 0, 4)),
    dict(key="outside", C=384, mode="reference_fp16", mrl=2.0, t=(-8.3, 0.1, 1.0), pose="rotated", N=140000, move=None, window=(0, 40, 4, 4)),
    dict(key="narrow200", C=200, mode="reference_fp16", mrl=2.0, t=(3.0, -2.8, 1.1), pose="rotated", N=140000, move=None, window=(120, 80, 0, 4)),
    dict(key="rows_only200", C=200, mode="reference_fp16", mrl=2.0, t=(0.0, 0.0, 1.0), pose="identity", N=140000, move=None, window=(45, 110, 0, 8)),
    dict(key="refused300", C=300, mode="reference_fp16", mrl=2.0, t=(0.3, -0.2, 1.1), pose="rotated", N=140000, move=None, window=None),
    dict(key="whole128", C=128, mode="reference_fp16", mrl=10.0, t=(0.0, 0.0, 1.0), pose="rotated", N=140000, move=None, window=None),
    dict(key="fp32_corner", C=384, mode="fp32", mrl=2.0, t=(-7.0, 6.9, 1.0), pose="rotated", N=140000, move=None, window=(0, 72, 8, 4)),
    dict(key="fp32_centre", C=384, mode="fp32", mrl=2.0, t=(0.3, -0.2, 1.1), pose="rotated", N=140000, move=(3, 2), window=(145, 109, 4, 4)),
    dict(key="n131072", C=200, mode="reference_fp16", mrl=2.0, t=(0.3, -0.2, 1.1), pose="rotated", N=131072, move=None, window=(53, 109, 0, 8)),
    dict(key="n131071", C=200, mode="reference_fp16", mrl=2.0, t=(0.3, -0.2, 1.1), pose="rotated", N=131071, move=None, window=None),
    dict(key="stats384", C=384, mode="reference_fp16", mrl=2.0, t=(-7.0, 6.9, 1.0), pose="rotated", N=140000, move=None, window=(0, 72, 8, 4), stats=True),
]
KEYS = [c["key"] for c in CASES]
SMALL_CLOUD_KEY = "n131071"       # the one case below the launcher's 131 072-point threshold: 256 threads, four lanes per ray, bitmap in global memory


def case_of(key):
    return CASES[KEYS.index(key)]


def case_seed(case):
    return 100 * (KEYS.index(case["key"]) + 1)


def case_config(case, yaml):
    """the frame configuration: the repository's YAML (rays and overlap clearance on) with the case's ray length"""
    cfg = dict(yaml, max_ray_length=case["mrl"])
    assert cfg["enable_visibility_cleanup"] and cfg["enable_overlap_clearance"]
    return cfg


def case_inputs(case):
    """(R, t0, [cloud of frame 0, cloud of frame 1]): numpy only, the same in the child and in the parent"""
    import _fixtures as fx
    R = fx.POSES[case["pose"]][0]
    seed = case_seed(case)
    return R, np.array(case["t"], np.float32), [fx.cloud(case["C"], case["N"], seed + f, dz=FRAME_DZ[f]) for f in range(2)]


def run_case(m, is_hip, case):
    """the case's two frames on a HIP map or on the oracle (same calls as tests/_post_variants.py: run_frames); returns the ray pass's
    visit count per frame: the oracle's always, the HIP map's where its context counts them (0 otherwise)"""
    R, t0, clouds = case_inputs(case)
    if not is_hip:
        m.center = np.zeros(3, np.float32)
    visits = []
    for f, p in enumerate(clouds):
        if f and case["move"]:
            m.move(np.array([case["move"][0] * RES, case["move"][1] * RES, 0.0], np.float64))
        t = (t0 + m.center).astype(np.float32)
        if is_hip:
            m.update_map_with_kernel(p, [], R, t, 1.0, 1.0)
            visits.append(int(m.stats().ray_visits))
        else:
            m.update_map_with_kernel(p, R, (t - m.center).astype(np.float32), 1.0, 1.0)
            visits.append(int(m.last.get("ray_visits", 0)))             # (0: the oracle ran without its ray pass)
        for _ in range(TIME_TICKS):
            m.update_time()
    return visits


def oracle_run(case, weights, cleanup=True):
    """the case on the oracle: (elevation_map, normal_map, traversability_input, visits per frame), read-only arrays"""
    from oracle import emap_oracle as eo
    cfg = case_config(case, eo.YAML)
    if not cleanup:
        cfg["enable_visibility_cleanup"] = False
    orc = eo.OracleMap(eo.make_params(cfg, cell_n=case["C"], mode=case["mode"], weights=weights))
    visits = run_case(orc, False, case)
    out = tuple(np.array(a, np.float32) for a in (orc.elevation_map, orc.normal_map, orc.traversability_input))
    for a in out:
        a.setflags(write=False)
    return out + (visits,)


def main(path):
    from _variant_children import child_setup
    weights = child_setup()
    from _util import make_pair
    from oracle import emap_oracle as eo
    out = {}
    for case in CASES:
        hip, _ = make_pair(case_config(case, eo.YAML), case["C"], case["mode"], weights)
        if case.get("stats"):
            hip._chk(hip._lib.emap_enable_stage_timing(hip._ctx, 2))      # the STATS = true instantiation of k_rays
        visits = run_case(hip, True, case)
        key = case["key"]
        out[key + "_map"] = hip.elevation_map
        out[key + "_normal"] = hip.normal_map
        out[key + "_trav_in"] = hip.traversability_input
        if case.get("stats"):
            out[key + "_ray_visits"] = np.array(visits, np.uint64)
        hip.close()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
