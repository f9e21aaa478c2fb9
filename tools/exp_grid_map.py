#!/usr/bin/env python
"""Single-question experiment: what does a GridMap message cost at the map's output door?

A publisher's tick on a 202^2 (robot scale) and a 1024^2 map whose cells are known and whose `rgb` layer is fused, for two layer lists:
the shipped publisher ['elevation', 'traversability', 'variance', 'rgb'] and the nine built-in layers.  Two routes, in ONE process on
one box, ALTERNATING tick by tick on the same map (both only read it):
  A  the node's route: per layer get_map_with_name_ref into a row-major buffer (the wrapper's RowMatrixXf), a transposing copy into
     a column-major buffer (gridMap.add) and a plain copy (GridMapRosConverter::toMessage)  -- elevation_mapping_wrapper.cpp:213-252
  B  get_grid_map_message: one launch writes every layer in the message's layout, one copy, one wait
`a_device` is route A WITHOUT its two host copies per layer: the device calls alone.  The nine built-ins reach route B the way the node
reaches the normals -- the six cell layers with normal_color=True -- so B also carries the `color` layer there (ten layers against
A's nine).  Host wall time per tick: p50 and p10 / p90 of --ticks ticks after --warmup.  The one condition: for two or more layers B
must not be slower than a_device (it moves the same bytes with fewer launches and waits); `b_not_slower_than_a_device` reports it.
One JSON line per (map, list)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elevation_mapping_cupy_amd import ElevationMap  # noqa: E402
from elevation_mapping_cupy_amd.configs import CORE_PARAM_YAML, parameter_from  # noqa: E402

SHIPPED = ["elevation", "traversability", "variance", "rgb"]
CELL_LAYERS = ["elevation", "variance", "traversability", "time", "upper_bound", "is_upper_bound"]
NORMALS = ["normal_x", "normal_y", "normal_z"]


def prepared_map(cell_n):
    cfg = dict(CORE_PARAM_YAML, enable_visibility_cleanup=False)
    m = ElevationMap(parameter_from(cfg, cell_n))
    m.param.pointcloud_channel_fusions = {"rgb": "color", "default": "average"}
    rng = np.random.default_rng(7)
    L = cell_n * m.resolution / 2
    n = min(4 * cell_n * cell_n, 1 << 22)
    p = np.empty((n, 4), np.float32)
    p[:, 0] = rng.uniform(-L, L, n); p[:, 1] = rng.uniform(-L, L, n); p[:, 2] = -1.0 + 0.02 * np.sin(3.0 * p[:, 0])
    p[:, 3] = rng.integers(0, 1 << 24, n, dtype=np.uint32).view(np.float32)
    m.input_pointcloud(p, ["x", "y", "z", "rgb"], np.eye(3, dtype=np.float32), np.array([0, 0, 1.0], np.float32), 0.0, 0.0)
    m.move_to(np.array([0.12, -0.2, 0.05], np.float32), np.eye(3, dtype=np.float32))
    m.sync()
    return m


def pct(x):
    return [round(float(np.percentile(x, q)), 4) for q in (50, 10, 90)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cells", type=int, nargs="*", default=[202, 1024])
    a = ap.parse_args()
    for cell_n in a.cells:
        m = prepared_map(cell_n)
        M = cell_n - 2
        for what, a_layers, b_layers, b_color in (("shipped", SHIPPED, SHIPPED, False), ("nine_builtins", CELL_LAYERS + NORMALS, CELL_LAYERS, True)):
            rows = np.zeros((len(a_layers), M, M), np.float32)
            col = np.zeros((len(a_layers), M, M), np.float32)                 # grid_map's column-major MatrixXf: element (i, j) at j * M + i
            wire = np.zeros((len(a_layers), M * M), np.float32)
            rec = {"a": [], "a_device": [], "b": []}
            msg = m.get_grid_map_message(b_layers, normal_color=b_color)
            buf = np.zeros((len(msg.layers), M, M), np.float32)               # the publisher keeps its buffer between ticks, as route A keeps its three
            for k in range(a.warmup + a.ticks):
                for route in (("a", "b") if k % 2 == 0 else ("b", "a")):      # alternate, and alternate who goes first
                    t0 = time.perf_counter()
                    if route == "a":
                        dev = 0.0
                        for j, name in enumerate(a_layers):
                            t1 = time.perf_counter()
                            m.get_map_with_name_ref(name, rows[j])
                            dev += time.perf_counter() - t1
                            np.copyto(col[j], rows[j].T)                      # gridMap.add(name, RowMatrixXf)
                            np.copyto(wire[j], col[j].reshape(-1))            # toMessage
                    else:
                        msg = m.get_grid_map_message(b_layers, normal_color=b_color, out=buf)
                    t2 = time.perf_counter()
                    if k >= a.warmup:
                        rec[route].append(1e3 * (t2 - t0))
                        if route == "a":
                            rec["a_device"].append(1e3 * dev)
            same = all(np.array_equal(wire[a_layers.index(n)].view(np.uint32), d.data.view(np.uint32)) or
                       bool((np.isnan(wire[a_layers.index(n)]) == np.isnan(d.data)).all() and
                            np.array_equal(wire[a_layers.index(n)][~np.isnan(d.data)].view(np.uint32), d.data[~np.isnan(d.data)].view(np.uint32)))
                       for n, d in zip(msg.layers, msg.data) if n in a_layers)
            p50 = {k: float(np.percentile(v, 50)) for k, v in rec.items()}
            out = {"cell_n": cell_n, "list": what, "layers_a": len(a_layers), "layers_b": len(msg.layers), "ticks": a.ticks,
                   "layers_equal_bitwise": bool(same), "b_over_a": round(p50["b"] / p50["a"], 4), "b_over_a_device": round(p50["b"] / p50["a_device"], 4),
                   "b_not_slower_than_a_device": bool(p50["b"] <= p50["a_device"])}
            for key, v in rec.items():
                out[key + "_ms_p50_p10_p90"] = pct(v)
            print(json.dumps(out), flush=True)
        m.close()


if __name__ == "__main__":
    main()
