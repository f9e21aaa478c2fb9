#!/usr/bin/env python
"""Single-question experiment: what does a semantic publisher's tick cost with the semantic plugins as ops of the plugin chain?

The tick: get_grid_map_message(['max_categories', 'pca', 'semantic_traversability', 'elevation']) into a kept buffer on a 202^2 (robot
scale) and a 1024^2 map -- max_categories = semantic_filter over 3 class layers, pca = features_pca over 8 feature layers,
semantic_traversability = votes of traversability and robot_centric_elevation (the reference's turtle-bot configuration with its
disabled entries switched on).  The map holds one frame and a pending shift; the class and feature layers are written with
semantic_map.set_layer.

The yardstick is ANOTHER TREE of this repository -- the parent commit checked out and built beside this one -- where the four plugins
take their host route (every matching layer down over PCIe, NumPy, the SVD of a cell_n^2 x 8 matrix, the plane into the host array).
This file runs unchanged on either tree: it uses nothing the parent lacks.

    python tools/exp_semantic_plugins.py --parent /path/to/parent/tree --runs 5 --out profiles/<stamp>_semantic_plugins.json

alternates the two trees on one box, a FRESH PROCESS per run (python tools/exp_semantic_plugins.py --tree <tree> --cell-n <n>), and
reports per size the median of the runs' p50 tick and their spread (min .. max) for both trees.  No time is fixed in advance; `faster`
says whether this tree's median is below the parent's.  A run's own line: host wall time per tick, p50 and p10 / p90 of --ticks ticks
after --warmup (the ticks end early once --seconds are spent, never before 3), and the route each plugin layer took."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST = ["max_categories", "pca", "semantic_traversability", "elevation"]
PLUGINS = """
robot_centric_elevation: {enable: True, fill_nan: False, is_height_layer: True, layer_name: robot_centric_elevation, extra_params: {resolution: %r, threshold: 1.1, use_threshold: True}}
semantic_filter: {type: semantic_filter, enable: True, fill_nan: False, is_height_layer: False, layer_name: max_categories, extra_params: {classes: ['^sem_.*$']}}
semantic_traversability: {type: semantic_traversability, enable: True, fill_nan: False, is_height_layer: False, layer_name: semantic_traversability,
  extra_params: {layers: [traversability, robot_centric_elevation], thresholds: [0.3, 0.5], type: [traversability, elevation]}}
features_pca: {type: features_pca, enable: True, fill_nan: False, is_height_layer: False, layer_name: pca, extra_params: {process_layer_names: ['^feat_.*$']}}
"""


def prepared_map(tree, cell_n, plugin_file):
    sys.path.insert(0, tree)
    from elevation_mapping_cupy_amd import ElevationMap
    from elevation_mapping_cupy_amd.configs import CORE_PARAM_YAML, parameter_from
    p = parameter_from(dict(CORE_PARAM_YAML, enable_visibility_cleanup=False), cell_n)
    with open(plugin_file, "w") as f:
        f.write(PLUGINS % float(p.resolution))
    p.plugin_config_file = plugin_file
    m = ElevationMap(p)
    rng = np.random.default_rng(7)
    L = cell_n * m.resolution / 2
    n = min(cell_n * cell_n // 2, 1 << 22)
    pts = np.empty((n, 3), np.float32)
    pts[:, 0] = rng.uniform(-L, L, n); pts[:, 1] = rng.uniform(-L, L, n); pts[:, 2] = -1.0 + 0.02 * np.sin(3.0 * pts[:, 0])
    m.input_pointcloud(pts, ["x", "y", "z"], np.eye(3, dtype=np.float32), np.array([0, 0, 1.0], np.float32), 0.0, 0.0)
    y, x = np.meshgrid(np.arange(cell_n, dtype=np.float32), np.arange(cell_n, dtype=np.float32), indexing="ij")
    for k in range(3):
        m.semantic_map.add_layer("sem_%d" % k)
        m.semantic_map.set_layer("sem_%d" % k, (np.sin(0.05 * (k + 1) * x) * np.cos(0.03 * (k + 2) * y) + 0.2 * rng.standard_normal((cell_n, cell_n))).astype(np.float32))
    for f in range(8):
        m.semantic_map.add_layer("feat_%d" % f)
        pattern = np.sin((0.037 + 0.011 * f) * x + 0.5 * f) * np.cos((0.023 + 0.007 * f) * y - 0.3 * f)
        m.semantic_map.set_layer("feat_%d" % f, (1.6 / (1 + f) * (pattern + 0.3 * rng.standard_normal((cell_n, cell_n)))).astype(np.float32))
    m.move_to(np.array([0.12, -0.2, 0.05], np.float32), np.eye(3, dtype=np.float32))
    m.sync()
    return m


def one_run(args):
    tree = os.path.abspath(args.tree)
    with tempfile.TemporaryDirectory() as td:
        m = prepared_map(tree, args.cell_n, os.path.join(td, "plugins.yaml"))
        M = args.cell_n - 2
        buf = np.empty((len(LIST), M, M), np.float32)
        times = []
        t_end = time.perf_counter() + args.seconds
        for k in range(args.warmup + args.ticks):
            t0 = time.perf_counter()
            msg = m.get_grid_map_message(LIST, out=buf)
            dt = time.perf_counter() - t0
            if k >= args.warmup:
                times.append(dt * 1e3)
            if len(times) >= 3 and time.perf_counter() > t_end:
                break
        route = dict(getattr(m, "last_plugin_route", {}))
        pca = msg.data[LIST.index("pca")].data.view(np.uint32)
        line = dict(what="semantic publisher tick", tree=tree, cell_n=args.cell_n, layers=LIST, ticks=len(times), p50_ms=float(np.percentile(times, 50)),
                    p10_ms=float(np.percentile(times, 10)), p90_ms=float(np.percentile(times, 90)), route=route,
                    pca_levels_used=int(np.unique(pca).size), classes_seen=int(np.unique(msg.data[0].data.view(np.uint32)).size))
        m.close()
    print(json.dumps(line))
    return line


def alternate(args):
    trees = (("parent", os.path.abspath(args.parent)), ("this", os.path.abspath(args.tree)))
    out = []
    for cell_n in args.sizes:
        runs = {"parent": [], "this": []}
        for r in range(args.runs):
            for name, tree in trees:                       # alternating, one process with the GPU open at a time
                cmd = [sys.executable, os.path.join(tree, "tools", "exp_semantic_plugins.py") if os.path.exists(os.path.join(tree, "tools", "exp_semantic_plugins.py"))
                       else os.path.abspath(__file__), "--tree", tree, "--cell-n", str(cell_n), "--ticks", str(args.ticks), "--warmup", str(args.warmup),
                       "--seconds", str(args.seconds)]
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
                if res.returncode != 0:
                    sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
                    raise SystemExit("run of the %s tree failed (exit %d): no further runs" % (name, res.returncode))
                runs[name].append(json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]))
        rec = dict(what="semantic publisher tick, trees alternated, a fresh process per run", cell_n=cell_n, runs=args.runs, layers=LIST)
        for name in runs:
            p50 = [x["p50_ms"] for x in runs[name]]
            rec[name] = dict(median_p50_ms=float(np.median(p50)), min_p50_ms=float(min(p50)), max_p50_ms=float(max(p50)), p50_ms=p50,
                             ticks=[x["ticks"] for x in runs[name]], route=runs[name][-1]["route"])
        rec["faster"] = rec["this"]["median_p50_ms"] < rec["parent"]["median_p50_ms"]
        rec["speedup"] = rec["parent"]["median_p50_ms"] / rec["this"]["median_p50_ms"]
        print(json.dumps(rec))
        out.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/exp_semantic_plugins.py", stamp=time.strftime("%Y-%m-%dT%H:%M:%S"), records=out), f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=HERE, help="the tree whose package is measured (default: this one)")
    ap.add_argument("--parent", help="another tree to alternate with: the yardstick")
    ap.add_argument("--cell-n", type=int, default=202)
    ap.add_argument("--sizes", type=int, nargs="+", default=[202, 1024])
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=20.0, help="end a run's ticks once this long was spent (never before 3 ticks)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=300.0)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.parent:
        alternate(args)
    else:
        one_run(args)


if __name__ == "__main__":
    main()
