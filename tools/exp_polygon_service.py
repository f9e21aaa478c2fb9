#!/usr/bin/env python
"""Single-question experiment: what does the safety-polygon service cost, by route?

A 202^2 (robot scale) and a 1024^2 map whose cells are known.  Three questions per map: ONE polygon (get_polygon_traversability), and
batches of 16 and 256 footprints of about 0.5 m x 0.3 m (get_polygons_traversability; a tree without the batch door -- the parent
commit, handed in with --parent -- answers a batch with that many single calls).  Routes: `device` (this tree), `host` (this tree with
EMAP_POLYGON_RESIDENT=0) and, with --parent PATH, `parent` (that checkout's package and library).  Every run is a FRESH process, the
routes ALTERNATE run by run on one box (--rounds times each), and the runs of a route are pooled: host wall time per call, p50 and
p10 / p90.  The conditions are relative: the device route's median for one polygon below the parent's (or, without --parent, the
host route's) on both maps, and a batch of 256 cheaper than 256 single calls of the parent.  One JSON line per (map, question)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (16, 256)


def footprints(n, half_map, rng):
    """n rectangles of 0.5 m x 0.3 m, turned and placed anywhere inside the map"""
    out = []
    for _ in range(n):
        c, a = rng.uniform(-half_map + 0.5, half_map - 0.5, 2), rng.uniform(0, np.pi)
        R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        out.append(c + np.array([[-0.25, -0.15], [0.25, -0.15], [0.25, 0.15], [-0.25, 0.15]]) @ R.T)
    return out


def child(a):
    sys.path.insert(0, a.root)
    from elevation_mapping_cupy_amd import ElevationMap
    from elevation_mapping_cupy_amd.configs import CORE_PARAM_YAML, parameter_from
    cell_n = a.cells[0]
    m = ElevationMap(parameter_from(dict(CORE_PARAM_YAML, enable_visibility_cleanup=False), cell_n))
    rng = np.random.default_rng(7)
    L = cell_n * m.resolution / 2
    n = min(4 * cell_n * cell_n, 1 << 22)
    p = np.empty((n, 3), np.float32)
    p[:, 0] = rng.uniform(-L, L, n); p[:, 1] = rng.uniform(-L, L, n); p[:, 2] = -1.0 + 0.05 * np.sin(3.0 * p[:, 0]) * np.cos(2.0 * p[:, 1])
    m.input_pointcloud(p, ["x", "y", "z"], np.eye(3, dtype=np.float32), np.array([0, 0, 1.0], np.float32), 0.0, 0.0)
    m.move_to(np.array([0.12, -0.2, 0.05], np.float32), np.eye(3, dtype=np.float32))
    m.sync()
    half = (cell_n - 2) * m.resolution / 2
    one = footprints(1, half, rng)[0] * 2.0 + m.center[:2]                     # the node's check: a 1 m x 0.6 m footprint
    many = {b: [f + m.center[:2] for f in footprints(b, half, rng)] for b in BATCHES}
    result = np.zeros(3)
    batch_door = hasattr(m, "get_polygons_traversability")

    def batch(polys):
        if batch_door:
            m.get_polygons_traversability(polys)
        else:
            for q in polys:
                m.get_polygon_traversability(q, result)

    rec = {}
    for key, fn, ticks in [("one", lambda: m.get_polygon_traversability(one, result), a.ticks)] + \
                          [("batch%d" % b, (lambda b=b: batch(many[b])), max(3, a.ticks * 4 // (b * (1 if batch_door and a.route == "device" else 8)))) for b in BATCHES]:
        warm = a.warmup if key == "one" else 1
        for k in range(warm + ticks):
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if k >= warm:
                rec.setdefault(key, []).append(1e3 * (t1 - t0))
    took = getattr(m, "last_polygon_route", None)
    m.close()
    print(json.dumps({"cell_n": cell_n, "route": a.route, "took": took, "result": [float(x) for x in result], "ms": rec}), flush=True)


def pct(x):
    return [round(float(np.percentile(x, q)), 4) for q in (50, 10, 90)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--cells", type=int, nargs="*", default=[202, 1024])
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--route", default="device")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    routes = [("device", ROOT, "1"), ("host", ROOT, "0")] + ([("parent", os.path.abspath(a.parent), "1")] if a.parent else [])
    for cell_n in a.cells:
        pooled = {}
        for r in range(a.rounds):
            for route, root, resident in (routes if r % 2 == 0 else routes[::-1]):      # alternate, and alternate who goes first
                env = dict(os.environ, EMAP_POLYGON_RESIDENT=resident)
                env.pop("EMAP_HIP_LIB", None)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--route", route, "--root", root, "--cells", str(cell_n),
                                      "--ticks", str(a.ticks), "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    sys.stderr.write(out.stderr[-2000:])
                    return 1                                                    # nothing more is started behind a run that ended badly
                got = json.loads(out.stdout.strip().splitlines()[-1])
                assert got["took"] in (None, "device" if route == "device" else "host"), got["took"]
                for key, v in got["ms"].items():
                    pooled.setdefault(key, {}).setdefault(route, []).extend(v)
        base = "parent" if a.parent else "host"
        for key, by in pooled.items():
            line = {"cell_n": cell_n, "question": key, "rounds": a.rounds, "baseline": base}
            for route, v in by.items():
                line[route + "_ms_p50_p10_p90"] = pct(v); line[route + "_n"] = len(v)
            p50 = {route: float(np.percentile(v, 50)) for route, v in by.items()}
            line["device_over_" + base] = round(p50["device"] / p50[base], 4)
            if key == "one":
                line["device_below_" + base] = bool(p50["device"] < p50[base])
            else:
                single = float(np.percentile(pooled["one"][base], 50))
                line["device_batch_over_n_single_" + base] = round(p50["device"] / (int(key[5:]) * single), 5)
                line["device_batch_below_n_single_" + base] = bool(p50["device"] < int(key[5:]) * single)
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
