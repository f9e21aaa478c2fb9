#!/usr/bin/env python
"""Single-question experiment: what does the plane-segmentation door (ElevationMap.get_plane_segmentation) save?

On a 202^2 (robot scale) and a 1024^2 map, a terrain scene (terraces and a 20 degree ramp on a floor) and the NaN checkerboard (M^2 / 2
one-cell labels, no plane).  Two routes, on ONE box, a FRESH PROCESS per run, ALTERNATING run by run and alternating who goes first:
  A  the only route that exists without the door: get_grid_map_layers of the source layer (M^2 floats over PCIe) and the host model of
     the same contract (plane_segmentation.py: window planes in NumPy) with scipy.ndimage.label for the components
  B  get_plane_segmentation: the chain of launches, 8 bytes of counts, then the label plane and the plane records
There is no earlier device route and the reference's C++ (Eigen, OpenCV, grid_map, CGAL) cannot be built here: this is a statement of
what the door saves over downloading the map and segmenting it in NumPy -- NOT a speed-up over the reference.  Host wall time per call
inside each child after its warm-up calls; p50 [p10, p90] over all runs of a route.  The labels and plane records of both routes are
compared (B's bytes against A's: same labels, same records).  No threshold is set.  The first lines carry the source stamp."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(M, name):
    i, j = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    if name == "checkerboard":
        return np.where((i + j) % 2 == 0, np.float32(0.5), np.float32(np.nan)).astype(np.float32)
    h = np.zeros((M, M), np.float32)
    h[:, M // 3:] += np.float32(0.2)                                        # terraces
    h[:, 2 * M // 3:] += np.float32(0.2)
    ramp = (i >= M // 2) & (j < M // 3 - 4)
    h[ramp] = (np.tan(np.deg2rad(20.0)) * 0.04 * (i - M // 2))[ramp].astype(np.float32)
    return h


def route_a(m):
    from scipy import ndimage
    from elevation_mapping_cupy_amd import plane_segmentation as ps
    from elevation_mapping_cupy_amd.elevation_mapping import grid_cell_positions
    _, planes = m.get_grid_map_layers(["elevation"])
    h = planes[0]
    res = float(np.float32(m.resolution))
    xs, ys = grid_cell_positions((float(m.center[0]), float(m.center[1])), res, h.shape[0])
    cos_plane, cos_local, cos_angle = ps.cosines(30.0, 35.0, 25.0)
    win = ps.window_pass(h, 3, res, 0.02 * 0.02, cos_local)
    lab, n = ndimage.label(win.planar)
    M = h.shape[0]
    first = ndimage.minimum(np.arange(M * M).reshape(M, M), lab, np.arange(1, n + 1)).astype(np.int64) if n else np.zeros(0, np.int64)
    root = np.where(lab > 0, first[np.maximum(lab, 1) - 1] if n else 0, -1)      # every cell's first cell: what label_planes groups by
    labels, recs, _ = ps.label_planes(h, win.normals, root, lab.astype(np.int32), res, (float(xs[0]), float(ys[0])), 4, cos_plane, 0.025, cos_angle)
    return labels, n, recs


def logical_plane(pub, C):
    """the (C, C) logical plane whose published view (border stripped, both axes flipped) is ``pub``"""
    out = np.zeros((C, C), np.float32)
    out[1:C - 1, 1:C - 1] = np.asarray(pub, np.float32)[::-1, ::-1]
    return out


def child(a):
    from tools.exp_grid_map import prepared_map
    m = prepared_map(a.cell_n)
    M = a.cell_n - 2
    h = scene(M, a.scene)
    valid = ~np.isnan(h)
    m.set_layer_raw("elevation", logical_plane(np.where(valid, h, np.float32(0.0)), a.cell_n))
    m.set_layer_raw("is_valid", logical_plane(valid, a.cell_n))
    out = np.zeros((M, M), np.int32)
    times = []
    for k in range(a.warmup + a.ticks):
        t0 = time.perf_counter()
        if a.route == "a":
            labels, n, recs = route_a(m)
        else:
            r = m.get_plane_segmentation(out=out)
            labels, n, recs = r.labels, r.n_labels, r.planes
        t1 = time.perf_counter()
        if k >= a.warmup:
            times.append(1e3 * (t1 - t0))
    import hashlib
    print(json.dumps({"ms": times, "n_labels": int(n), "n_planes": int(len(recs)), "digest": hashlib.sha256(np.ascontiguousarray(labels).tobytes() + recs.tobytes()).hexdigest()[:16]}))
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5, help="fresh processes per route")
    ap.add_argument("--ticks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, nargs="*", default=[202, 1024])
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--route")
    ap.add_argument("--scene")
    ap.add_argument("--cell-n", dest="cell_n", type=int)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import bench
    print("# tools/exp_plane_segmentation.py: whole-map download + host model with scipy.ndimage.label (A) against get_plane_segmentation (B); a fresh process per run, alternating on one box; host wall ms per call, p50 [p10, p90]")
    print("# what the door saves over the only route that exists without it -- not a speed-up over the reference's C++, which cannot be built here")
    print("# source_stamp: %s" % bench.source_stamp(), flush=True)
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
                   "bytes_d2h_a": 4 * M * M, "bytes_d2h_b": 8 + 4 * M * M + 160 * n_planes,
                   "a_ms_p50_p10_p90": [round(float(np.percentile(ms["a"], q)), 3) for q in (50, 10, 90)],
                   "b_ms_p50_p10_p90": [round(float(np.percentile(ms["b"], q)), 3) for q in (50, 10, 90)],
                   "a_over_b": round(float(np.percentile(ms["a"], 50) / np.percentile(ms["b"], 50)), 1)}
            print(json.dumps(row), flush=True)
            bad = bad or not same
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
