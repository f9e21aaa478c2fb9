#!/usr/bin/env python
"""Single-question experiment: what does the planar-regions door (ElevationMap.get_planar_regions) save?

On a 202^2 (robot scale) and a 1024^2 map, the terrain scene and the NaN checkerboard of tools/exp_plane_segmentation.py, with the
reference's defaults (preprocessing 3 x 1, the default postprocessing, marginSize 1).  Two routes, on ONE box, a FRESH PROCESS per run,
ALTERNATING run by run and alternating who goes first:
  A  the only route that exists without the door: get_planar_terrain (its labels come back anyway) and the host model of the contour
     stage on them (planar_regions.py, scipy.ndimage.label for the components)
  B  get_planar_regions: the terrain chain, then the regions chain on the labels where they lie; a few kilobytes of rings and vertices
     come back
There is no earlier device route and the reference's C++ (OpenCV, CGAL) cannot be built here: this is a statement of what the door
saves over running the same contract in NumPy on the downloaded labels -- NOT a speed-up over the reference.  Host wall time per call
inside each child after its warm-up calls; p50 [p10, p90] over all runs of a route.  The rings and vertices of both routes are compared
by digest.  No threshold is set.  The first lines carry the source stamp and the kernel-source hash.  --stages: one more child per case
that times the device stage alone (emap_planar_regions on the resident labels) call by call."""
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


def kernel_source_hash():
    h = hashlib.sha256()
    for f in ("emap_regions.hip", "emap_api_regions.hip", "emap_planeseg.hip", "emap_api_planeseg.hip", "emap_cloudout.hip", "emap_launch.h"):
        h.update(open(os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def scipy_roots8(X, merge=True):
    """planar_regions.components8 with scipy: the root of a component is its smallest idx"""
    from scipy import ndimage
    lab, n = ndimage.label(X != 0, structure=np.ones((3, 3), bool))
    if not n:
        return np.full(X.shape, -1, np.int32)
    first = ndimage.minimum(np.arange(X.size).reshape(X.shape), lab, np.arange(1, n + 1)).astype(np.int64)
    return np.where(lab > 0, first[np.maximum(lab, 1) - 1], -1).astype(np.int32)


def child(a):
    from elevation_mapping_cupy_amd import planar_regions as pr
    from tools.exp_grid_map import prepared_map
    from tools.exp_plane_segmentation import logical_plane, scene
    pr.components8 = scipy_roots8
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
            r = m.get_planar_terrain(preprocess={})
            t = pr.trace_labels(r.labels, r.n_labels, 1, 0)
            rings, vertices = t.rings, t.vertices
            regions = pr.build_regions(rings, vertices, r.planes, r.resolution, r.origin_xy)
        elif a.route == "b":
            r = m.get_planar_regions(preprocess={})
            rings, vertices, regions = r.rings, r.vertices, r.regions
        else:                                                  # the device stage alone, on the labels the terrain call left
            if k == 0:
                r = m.get_planar_terrain(preprocess={})
                t0 = time.perf_counter()
            rings, vertices = m._planar_regions_call(None, 0, 0, 0, 1)
            regions = []
        t1 = time.perf_counter()
        if k >= a.warmup:
            times.append(1e3 * (t1 - t0))
    d = hashlib.sha256(rings.tobytes() + vertices.tobytes()).hexdigest()[:16]
    print(json.dumps({"ms": times, "n_labels": int(r.n_labels), "n_rings": int(len(rings)), "n_vertices": int(len(vertices)), "n_regions": len(regions), "digest": d}))
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=4, help="fresh processes per route")
    ap.add_argument("--ticks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cells", type=int, nargs="*", default=[202, 1024])
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--route")
    ap.add_argument("--scene")
    ap.add_argument("--cell-n", dest="cell_n", type=int)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import bench
    print("# tools/exp_planar_regions.py: get_planar_terrain + the host model of the contour stage with scipy.ndimage.label (A) against get_planar_regions (B), the reference's defaults, marginSize 1; a fresh process per run, alternating on one box; host wall ms per call, p50 [p10, p90]")
    print("# what the door saves over the only route that exists without it -- not a speed-up over the reference's C++, which cannot be built here")
    print("# source_stamp: %s  kernel_source_hash: %s" % (bench.source_stamp(), kernel_source_hash()), flush=True)
    bad = False

    def run(route, name, cell_n):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--route", route, "--scene", name, "--cell-n", str(cell_n), "--ticks", str(a.ticks), "--warmup", str(a.warmup)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            print(res.stderr[-2000:], file=sys.stderr)
            sys.exit(2)                                          # a child that failed: nothing more is started
        return json.loads(res.stdout.strip().splitlines()[-1])
    for cell_n in a.cells:
        for name in ("terrain", "checkerboard"):
            ms, seen = {"a": [], "b": []}, {}
            for k in range(a.runs):
                for route in (("a", "b") if k % 2 == 0 else ("b", "a")):
                    rec = run(route, name, cell_n)
                    ms[route] += rec["ms"]
                    seen.setdefault(route, set()).add((rec["n_labels"], rec["n_rings"], rec["n_vertices"], rec["n_regions"], rec["digest"]))
            same = len(seen["a"]) == 1 and seen["a"] == seen["b"]
            n_labels, n_rings, n_vertices, n_regions, _ = next(iter(seen["b"]))
            row = {"cell_n": cell_n, "scene": name, "n_labels": n_labels, "n_rings": n_rings, "n_vertices": n_vertices, "n_regions": n_regions, "runs": a.runs, "ticks": a.ticks,
                   "same_answer": bool(same), "bytes_d2h_regions": 24 + 32 * n_rings + 8 * n_vertices,
                   "a_ms_p50_p10_p90": [round(float(np.percentile(ms["a"], q)), 3) for q in (50, 10, 90)],
                   "b_ms_p50_p10_p90": [round(float(np.percentile(ms["b"], q)), 3) for q in (50, 10, 90)],
                   "a_over_b": round(float(np.percentile(ms["a"], 50) / np.percentile(ms["b"], 50)), 1)}
            if a.stages:
                st = run("stage", name, cell_n)["ms"]
                row["regions_stage_ms_p50_p10_p90"] = [round(float(np.percentile(st, q)), 3) for q in (50, 10, 90)]
            print(json.dumps(row), flush=True)
            bad = bad or not same
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
