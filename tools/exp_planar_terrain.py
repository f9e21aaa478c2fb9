#!/usr/bin/env python
"""Single-question experiment: what does the planar-terrain door (ElevationMap.get_planar_terrain) save?

On a 202^2 (robot scale) and a 1024^2 map, the terrain scene and the NaN checkerboard of tools/exp_plane_segmentation.py, with the
reference's defaults (preprocessing 3 x 1; kd = 11, kb = 7, kg = 3 cells at 4 cm; offset 1; 2 cm).  Two routes, on ONE box, a FRESH
PROCESS per run, ALTERNATING run by run and alternating who goes first:
  A  the only route that exists without the door: get_grid_map_layers of the source layer (M^2 floats over PCIe) and the host model of
     the same contract (planar_terrain.py, plane_segmentation.py) with scipy.ndimage.label for the components
  B  get_planar_terrain: one chain of launches, the segmentation's two waits, then the four planes, the labels and the plane records
There is no earlier device route and the reference's C++ (Eigen, OpenCV, grid_map, CGAL) cannot be built here: this is a statement of
what the door saves over downloading the map and running the same contract in NumPy -- NOT a speed-up over the reference.  Host wall
time per call inside each child after its warm-up calls; p50 [p10, p90] over all runs of a route.  The planes, labels and records of
both routes are compared by digest.  No threshold is set.  The first lines carry the source stamp and the kernel-source hash."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PLANES = ("elevation", "smooth_planar", "plane_classification", "elevation_before_postprocess")


def kernel_source_hash():
    h = hashlib.sha256()
    for f in ("emap_terrain.hip", "emap_api_terrain.hip", "emap_planeseg.hip", "emap_api_planeseg.hip", "emap_launch.h"):
        h.update(open(os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def scipy_roots(nan):
    from scipy import ndimage
    lab, _ = ndimage.label(nan)
    return lab.astype(np.int64) - 1


def route_a(m):
    from scipy import ndimage
    from elevation_mapping_cupy_amd import plane_segmentation as ps
    from elevation_mapping_cupy_amd import planar_terrain as pt
    from elevation_mapping_cupy_amd.elevation_mapping import grid_cell_positions
    pt.nan_roots = scipy_roots
    _, planes = m.get_grid_map_layers(["elevation"])
    h = planes[0]
    M = h.shape[0]
    res = float(np.float32(m.resolution))
    xs, ys = grid_cell_positions((float(m.center[0]), float(m.center[1])), res, M)
    e = pt.median(pt.inpaint_min(h), 3, 1)
    cos_plane, cos_local, cos_angle = ps.cosines(30.0, 35.0, 25.0)
    win = ps.window_pass(e, 3, res, 0.02 * 0.02, cos_local)
    lab, n = ndimage.label(win.planar)
    first = ndimage.minimum(np.arange(M * M).reshape(M, M), lab, np.arange(1, n + 1)).astype(np.int64) if n else np.zeros(0, np.int64)
    root = np.where(lab > 0, first[np.maximum(lab, 1) - 1] if n else 0, -1)
    labels, recs, _ = ps.label_planes(e, win.normals, root, lab.astype(np.int32), res, (float(xs[0]), float(ys[0])), 4, cos_plane, 0.025, cos_angle)
    r = pt.postprocess(e, labels, res, None)
    return r, labels, n, recs


def child(a):
    from tools.exp_grid_map import prepared_map
    from tools.exp_plane_segmentation import logical_plane, scene
    m = prepared_map(a.cell_n)
    M = a.cell_n - 2
    h = scene(M, a.scene)
    valid = ~np.isnan(h)
    m.set_layer_raw("elevation", logical_plane(np.where(valid, h, np.float32(0.0)), a.cell_n))
    m.set_layer_raw("is_valid", logical_plane(valid, a.cell_n))
    times = []
    for k in range(a.warmup + a.ticks):
        t0 = time.perf_counter()
        if a.route == "a":
            r, labels, n, recs = route_a(m)
        else:
            r = m.get_planar_terrain(preprocess={})
            labels, n, recs = r.labels, r.n_labels, r.planes
        t1 = time.perf_counter()
        if k >= a.warmup:
            times.append(1e3 * (t1 - t0))
    d = hashlib.sha256(np.ascontiguousarray(labels).tobytes() + recs.tobytes() + b"".join(np.ascontiguousarray(getattr(r, p)).tobytes() for p in PLANES)).hexdigest()[:16]
    print(json.dumps({"ms": times, "n_labels": int(n), "n_planes": int(len(recs)), "digest": d}))
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=4, help="fresh processes per route")
    ap.add_argument("--ticks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cells", type=int, nargs="*", default=[202, 1024])
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--route")
    ap.add_argument("--scene")
    ap.add_argument("--cell-n", dest="cell_n", type=int)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import bench
    print("# tools/exp_planar_terrain.py: whole-map download + host model with scipy.ndimage.label (A) against get_planar_terrain (B), the reference's defaults; a fresh process per run, alternating on one box; host wall ms per call, p50 [p10, p90]")
    print("# what the door saves over the only route that exists without it -- not a speed-up over the reference's C++, which cannot be built here")
    print("# source_stamp: %s  kernel_source_hash: %s" % (bench.source_stamp(), kernel_source_hash()), flush=True)
    bad = False
    for cell_n in a.cells:
        for name in ("terrain", "checkerboard"):
            ms, seen = {"a": [], "b": []}, {}
            for k in range(a.runs):
                for route in (("a", "b") if k % 2 == 0 else ("b", "a")):
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--route", route, "--scene", name, "--cell-n", str(cell_n), "--ticks", str(a.ticks), "--warmup", str(a.warmup)]
                    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                    if res.returncode != 0:
                        print(res.stderr[-2000:], file=sys.stderr)
                        sys.exit(2)                                          # a child that failed: nothing more is started
                    rec = json.loads(res.stdout.strip().splitlines()[-1])
                    ms[route] += rec["ms"]
                    seen.setdefault(route, set()).add((rec["n_labels"], rec["n_planes"], rec["digest"]))
            same = len(seen["a"]) == 1 and seen["a"] == seen["b"]
            n_labels, n_planes, _ = next(iter(seen["b"]))
            M = cell_n - 2
            row = {"cell_n": cell_n, "scene": name, "n_labels": n_labels, "n_planes": n_planes, "runs": a.runs, "ticks": a.ticks, "same_answer": bool(same),
                   "bytes_d2h_a": 4 * M * M, "bytes_d2h_b": 8 + 5 * 4 * M * M + 160 * n_planes,
                   "a_ms_p50_p10_p90": [round(float(np.percentile(ms["a"], q)), 3) for q in (50, 10, 90)],
                   "b_ms_p50_p10_p90": [round(float(np.percentile(ms["b"], q)), 3) for q in (50, 10, 90)],
                   "a_over_b": round(float(np.percentile(ms["a"], 50) / np.percentile(ms["b"], 50)), 1)}
            print(json.dumps(row), flush=True)
            bad = bad or not same
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
