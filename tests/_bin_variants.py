"""Case table of tests/test_hip_bin_variants.py and tests/test_bin_variant_cases.py, and -- run as a program -- the child process that
executes every case on the GPU with whatever variants of the tile-binned scatter the hooks of its environment select (emap_api.hip:
EMAP_SPLIT, EMAP_SPLIT_CAP, EMAP_BIN_STRIP, EMAP_BIN_CHUNK, EMAP_SEM_CARRY; emap_binned.hip: EMAP_HIST_BLOCK, EMAP_SCATTER_BLOCK; all
read once per process, so one process is one variant):

    python tests/_bin_variants.py <out.npz>

Every case is two or three frames on a fresh context with the binned scatter forced, TIME_TICKS update_time() calls after each frame.
The child runs no oracle code (it takes the configuration dictionaries from the oracle's module, nothing else) and reads no reference
file; its inputs are numpy only and the same in the child and in the parent, which runs the same frames on the oracle (oracle_run) and
compares the recorded arrays.

`kind`: "whole" = emap_update frames, "staged" = the staged entry points (count, gate, fuse, commit, average, ...), "sem" = whole
frames that declare an RGB / semantic fusion, "strip" = two row strips as threads (run_strips: emap_update_sharded over the in-process RCCL stand-in).  `cloud`: ("uniform",) |
("squeeze", share, scale, (dx, dy)): that share of fx.cloud scaled about the sensor and moved by (dx, dy) metres in the sensor frame --
OFF the sensor, so that the squeezed points stay beyond min_valid_distance -- | ("tile",): all points in one 16 x 64 tile (tile_cloud) |
("semantic",): fx.semantic_cloud.  `heavy_from`: the first frame in which a sort bin holds more than 4096 records (None: never) --
tests/test_bin_variant_cases.py checks the column against the oracle's point_index."""
import sys

import numpy as np

RES = 0.04
TIME_TICKS = 3
CH = ["x", "y", "z", "s0", "s1", "c0", "rgb"]                                   # as tests/test_hip_frame_semantics.py
FUSIONS = {"rgb": "color", "c0": "class_average", "default": "average"}
SPLIT_CAP = 4096                  # records per part (emap_device.h), as a literal
BLOCK_NS = (262144, 262145, 300000, 524289)

CASES = [
    dict(key="uniform202", kind="whole", C=202, N=27000, mode="reference_fp16", rays=False, pose="rotated", stack=0, noise=1.0, frames=2, cloud=("uniform",), heavy_from=None),
    dict(key="uniform202_rays", kind="whole", C=202, N=27000, mode="reference_fp16", rays=True, pose="rotated", stack=0, noise=1.0, frames=2, cloud=("uniform",), heavy_from=None),
    dict(key="fp32_202", kind="whole", C=202, N=27000, mode="fp32", rays=True, pose="rotated", stack=0, noise=1.0, frames=2, cloud=("uniform",), heavy_from=None),
] + [
    dict(key="blocks%d" % n, kind="whole", C=128, N=n, mode="reference_fp16", rays=False, pose="rotated", stack=0, noise=1.0, frames=2, cloud=("uniform",), heavy_from=0)
    for n in BLOCK_NS
] + [
    dict(key="heavy202", kind="whole", C=202, N=150000, mode="reference_fp16", rays=False, pose="rotated", stack=0, noise=1.0, frames=3, cloud=("squeeze", 0.6, 0.1, (1.2, 0.8)), heavy_from=0),
    dict(key="heavy202_rays", kind="whole", C=202, N=150000, mode="reference_fp16", rays=True, pose="rotated", stack=0, noise=1.0, frames=3, cloud=("squeeze", 0.6, 0.1, (1.2, 0.8)), heavy_from=0),
    dict(key="heavy400_stack2", kind="whole", C=400, N=200000, mode="reference_fp16", rays=False, pose="rotated", stack=2, noise=1.0, frames=3, cloud=("squeeze", 0.6, 0.05, (1.5, -1.0)), heavy_from=0),
    dict(key="gate_shut", kind="whole", C=202, N=150000, mode="reference_fp16", rays=False, pose="rotated", stack=0, noise=0.0, frames=3, cloud=("squeeze", 0.6, 0.1, (1.2, 0.8)), heavy_from=0),
    dict(key="slots1100", kind="whole", C=1100, N=100000, mode="reference_fp16", rays=False, pose="identity", stack=64, noise=1.0, frames=2, cloud=("uniform",), heavy_from=0),
    dict(key="parts_clamp", kind="whole", C=66, N=900000, mode="reference_fp16", rays=False, pose="identity", stack=0, noise=1.0, frames=2, cloud=("tile",), heavy_from=0),
    dict(key="staged_heavy", kind="staged", C=202, N=150000, mode="reference_fp16", rays=False, pose="rotated", stack=0, noise=1.0, frames=3, cloud=("squeeze", 0.6, 0.1, (1.2, 0.8)), heavy_from=0),
    dict(key="sem_stack4", kind="sem", C=200, N=60000, mode="reference_fp16", rays=False, pose="rotated", stack=4, noise=1.0, frames=3, cloud=("semantic",), heavy_from=0),
    dict(key="sem_stack4_rays", kind="sem", C=200, N=60000, mode="reference_fp16", rays=True, pose="rotated", stack=4, noise=1.0, frames=2, cloud=("semantic",), heavy_from=0),
    dict(key="sem_slots1100", kind="sem", C=1100, N=99999, mode="reference_fp16", rays=False, pose="identity", stack=64, noise=1.0, frames=2, cloud=("semantic",), heavy_from=0),
    dict(key="strip130_27000", kind="strip", C=130, N=27000, mode="reference_fp16", rays=False, pose="rotated", stack=0, noise=1.0, frames=2, cloud=("uniform",), heavy_from=None),
    dict(key="strip130_50000", kind="strip", C=130, N=50000, mode="reference_fp16", rays=False, pose="rotated", stack=0, noise=1.0, frames=2, cloud=("uniform",), heavy_from=None),
    dict(key="strip130_27000_fp32", kind="strip", C=130, N=27000, mode="fp32", rays=False, pose="rotated", stack=0, noise=1.0, frames=2, cloud=("uniform",), heavy_from=None),
]
KEYS = [c["key"] for c in CASES]
WORLD = 2                          # ranks of a strip case
# the cases that run the same clouds as heavy202 (other settings, other entry points)
HEAVY202_KEYS = ("heavy202", "heavy202_rays", "gate_shut", "staged_heavy")


def case_of(key):
    return CASES[KEYS.index(key)]


def case_seed(case):
    if case["key"] in HEAVY202_KEYS:
        return 100 * (KEYS.index("heavy202") + 1)
    if case["key"] in ("sem_stack4", "sem_stack4_rays"):
        return 0                   # fx.semantic_cloud(200, 60000, f): the clouds of tests/test_hip_frame_semantics.py
    return 100 * (KEYS.index(case["key"]) + 1)


def case_config(case, yaml):
    """the frame configuration: the repository's YAML with the visibility pass on or off (overlap clearance stays on)"""
    cfg = dict(yaml, enable_visibility_cleanup=bool(case["rays"]))
    assert cfg["enable_overlap_clearance"] and cfg["enable_drift_compensation"]
    return cfg


# parts_clamp: the 16 x 64 tile of rows 0 ... 15, columns 0 ... 63 of the 66-cell map (cell = floor(coordinate / RES + 33), identity
# pose): x in [-1.32, -0.68) m, y in [-1.32, 1.24) m.  The cloud keeps clear of the border cells (row 0, column 0: never inside) and of
# the tile's far edges: rows 2 ... 14, columns 2 ... 61.  The sensor stands over the map's centre, 0.7 m and more from every point.
TILE_X = (-1.24, -0.74)
TILE_Y = (-1.24, 1.14)


def tile_cloud(C, N, seed, dz):
    import _fixtures as fx
    assert C == 66
    p = fx.cloud(C, N, seed, dz=dz)
    L = np.float32(C * RES / 2)
    for a, (lo, hi) in ((0, TILE_X), (1, TILE_Y)):
        p[:, a] = (p[:, a] + L) / (2 * L) * np.float32(hi - lo) + np.float32(lo)
    return p


def case_inputs(case):
    """(R, t, [cloud per frame]): numpy only, the same in the child and in the parent; t is relative to the map's centre (which never moves)"""
    import _fixtures as fx
    R, t = fx.POSES[case["pose"]]
    C, N, seed, kind = case["C"], case["N"], case_seed(case), case["cloud"][0]
    clouds = []
    for f in range(case["frames"]):
        dz = -0.03 * f
        if kind == "semantic":
            p = fx.semantic_cloud(C, N, seed + f)
        elif kind == "tile":
            p = tile_cloud(C, N, seed + f, dz)
        else:
            p = fx.cloud(C, N, seed + f, dz=dz)
            if kind == "squeeze":
                _, share, scale, (dx, dy) = case["cloud"]
                k = int(N * share)
                p[:k, :2] *= np.float32(scale)
                p[:k, 0] += np.float32(dx); p[:k, 1] += np.float32(dy)
        clouds.append(p)
    return R, t.copy(), clouds


def oracle_params(case, weights):
    from oracle import emap_oracle as eo
    return eo.make_params(case_config(case, eo.YAML), cell_n=case["C"], mode=case["mode"], weights=weights)


def oracle_run(case, weights):
    """the case on the oracle, whole map: dict of read-only arrays (map, normal, trav_in, add; sem for the semantic cases)"""
    from oracle import emap_oracle as eo
    orc = eo.OracleMap(oracle_params(case, weights))
    R, t, clouds = case_inputs(case)
    for p in clouds:
        orc.update_map_with_kernel(p, R, t, case["noise"], case["noise"])       # (the staged entry points run the same sequence)
        if case["kind"] == "sem":
            orc.semantic_update(p, R, t, average=[(3, 0), (4, 1)], class_average=[(5, 2)], color=[(6, 3)], alpha=0.5)
        for _ in range(TIME_TICKS):
            orc.update_time()
    out = dict(map=np.array(orc.elevation_map, np.float32), normal=np.array(orc.normal_map, np.float32),
               trav_in=np.array(orc.traversability_input, np.float32), add=np.array([float(orc.additive_mean_error)], np.float64))
    if case["kind"] == "sem":
        out["sem"] = np.array(orc.semantic_map[:4], np.float32)
    for a in out.values():
        a.setflags(write=False)
    return out


def records_per_bin(case, weights=None):
    """per frame: records (valid points inside the map) per sort bin as bin_of() (emap_binned.hip) defines it on a whole-map context whose
    origin has not moved: bin = (row // (16 * sub)) * ceil(C / 64) + column // 64, sub = the case's stack (1 without).  From the
    oracle's point_index."""
    from oracle import emap_oracle as eo
    orc = eo.OracleMap(oracle_params(case, weights))
    R, t, clouds = case_inputs(case)
    C, sub = case["C"], max(1, case["stack"])
    tx, ty = (C + 63) // 64, (C + 16 * sub - 1) // (16 * sub)
    out = []
    for p in clouds:
        idx, valid, inside = orc.point_index(p, R, t)
        idx = idx[(valid != 0) & (inside != 0)].astype(np.int64)
        out.append(np.bincount((idx // C) // (16 * sub) * tx + (idx % C) // 64, minlength=tx * ty))
    return out


def wanted_parts(n):
    """extra parts the bins of `n` records each WANT (split_parts() - 1 of emap_device.h, by its definition: parts of at most 4096 records, at most 128 parts)"""
    n = np.asarray(n, np.int64)
    return np.where(n > SPLIT_CAP, np.minimum((n + SPLIT_CAP - 1) // SPLIT_CAP, 128) - 1, 0)


def run_strips(cfg, C, mode, weights, clouds, R, t, noise):
    """every cloud as one frame of the library's own sharded frame (emap_update_sharded) on WORLD strip contexts -- threads of this
    process on one GPU, the in-process stand-in for RCCL of tests/fake_rccl/ -- with the binned scatter forced and TIME_TICKS
    update_time() calls after each frame, as _strips_vs_single of tests/test_hip_comm.py runs them; no torch in this process.  Returns one
    tuple per rank: (row_begin, rows, elevation_map, normal_map, additive_mean_error)."""
    import ctypes as ct
    import threading
    from _util import rccl_stand_in
    from elevation_mapping_cupy_amd import _lib
    from elevation_mapping_cupy_amd.configs import parameter_from
    from elevation_mapping_cupy_amd.sharded import HipStripEngine, NativeComm, ShardedElevationMap
    lib_path = rccl_stand_in("blocking")
    uid = (ct.c_uint8 * 128)()                        # one id for all ranks (what the bootstrap channel distributes in a real launch)
    assert _lib.load().emap_comm_unique_id(lib_path.encode(), uid) == 0
    out, errs = [None] * WORLD, []

    def run(rank):
        try:
            eng = HipStripEngine(parameter_from(cfg, C, mode, weights), rank, WORLD, 0)
            eng.map.set_scatter_mode("binned")
            comm = NativeComm(eng, rank=rank, world=WORLD, bootstrap=False, uid=bytes(uid), rccl_path=lib_path)
            sm = ShardedElevationMap(eng, comm, False, cfg["enable_overlap_clearance"])
            for p in clouds:
                eng.bind_points(p)
                sm.update(R, t, noise, noise)
                for _ in range(TIME_TICKS):
                    eng.update_time()
            eng.sync()
            out[rank] = (eng.map.row_begin, eng.map.rows, eng.map.elevation_map, eng.map.normal_map, eng.map.get_additive_mean_error())
            eng.lib.emap_comm_destroy(eng.ctx)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(WORLD)]
    [x.start() for x in th]
    [x.join(timeout=120) for x in th]
    assert not any(x.is_alive() for x in th), "a rank is stuck in the exchange"
    assert not errs, errs
    return out


def _run_hip(case, weights, out):
    from _util import make_parameter
    from elevation_mapping_cupy_amd.elevation_mapping import ElevationMap
    from oracle.emap_oracle import YAML                   # the configuration dictionary only
    key, cfg = case["key"], case_config(case, YAML)
    R, t, clouds = case_inputs(case)
    if case["kind"] == "strip":
        from oracle.emap_oracle import DEFAULTS
        full = dict(DEFAULTS); full.update(cfg)
        res = run_strips(full, case["C"], case["mode"], weights, clouds, R, t, case["noise"])
        out[key + "_rows"] = np.array([[r0, rows] for r0, rows, _, _, _ in res], np.int64)
        out[key + "_add"] = np.array([add for _, _, _, _, add in res], np.float64)
        for r, (_, _, m, nm, _) in enumerate(res):
            out["%s_r%d_map" % (key, r)] = np.array(m, np.float32)
            out["%s_r%d_normal" % (key, r)] = np.array(nm, np.float32)
        return
    hip = ElevationMap(make_parameter(cfg, case["C"], case["mode"], weights))
    hip.set_scatter_mode("binned", case["stack"])
    if case["kind"] == "sem":
        hip.param.pointcloud_channel_fusions = dict(FUSIONS)
    paths, sems = [], []
    for p in clouds:
        if case["kind"] == "staged":
            hip.bind_points(p)
            hip.stage("count", R, t)
            hip.stage("gate", position_noise=case["noise"], orientation_noise=case["noise"])
            hip.stage("fuse", R, t)
            hip.stage("commit")
            hip.stage("average")
            hip.stage("overlap", t=float(np.float32(t[2])))
            hip.stage("dilate")
            hip.stage("traversability_normals")
        elif case["kind"] == "sem":
            hip.input_pointcloud(p, CH, R, t.copy(), case["noise"], case["noise"])
        else:
            hip.update_map_with_kernel(p, [], R, t.copy(), case["noise"], case["noise"])
        if case["kind"] != "staged":
            paths.append(hip.last_update_path()); sems.append(hip.last_frame_semantics())
        for _ in range(TIME_TICKS):
            hip.update_time()
    out[key + "_map"] = np.array(hip.elevation_map, np.float32)
    out[key + "_normal"] = np.array(hip.normal_map, np.float32)
    out[key + "_trav_in"] = np.array(hip.traversability_input, np.float32)
    out[key + "_add"] = np.array([hip.get_additive_mean_error()], np.float64)
    out[key + "_path"] = np.array(paths, dtype="U16")
    out[key + "_sempath"] = np.array(sems, dtype="U16")
    if case["kind"] == "sem":
        assert list(hip.semantic_map.layer_names) == CH[3:], hip.semantic_map.layer_names
        out[key + "_sem"] = np.array(hip.semantic_map.semantic_map, np.float32)
    hip.close()


def main(path):
    from _variant_children import child_setup
    weights = child_setup()
    out = {}
    for case in CASES:
        _run_hip(case, weights, out)
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
