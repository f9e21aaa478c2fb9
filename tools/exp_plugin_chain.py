#!/usr/bin/env python
"""Single-question experiment: what do the plugin layers of a GridMap publisher cost on resident planes?

A publisher's tick on a 202^2 (robot scale) and a 1024^2 map with the shipped plugin configuration (min_filter: 1 x 30 sweeps, smooth of
min_filter, inpaint: telea on the host), for two layer lists: ['min_filter', 'smooth', 'elevation'] and the shipped filter publisher
['min_filter', 'smooth', 'inpaint', 'elevation'].  Two routes, in ONE process on one box, ALTERNATING tick by tick on the same map (both
only read the map; each recomputes the plugin layers it publishes):
  A  the node's route: per layer get_map_with_name_ref (plugin layers: host route, every plane over PCIe twice) into a row-major buffer,
     a transposing copy into a column-major buffer (gridMap.add) and a plain copy (GridMapRosConverter::toMessage)
  B  get_grid_map_message into a kept buffer: device-capable plugins in one chain of launches without a wait, one grid launch that reads
     their resident planes next to the cells, one copy, one wait; the host inpainting as in A
With --inpaint-method telea_fronts the inpaint layer names the device method: route A runs the plugin's host route
of it (two byte images up, a 4-byte read-back, the result down), route B the op of the chain, and only the filter publisher's list is
run.  --points-per-cell sets the frame the map holds (0.5: half the cells stay unknown; 4: a nearly full map, where max d is small and
almost every k_fr_advance launch of the chain's fixed count is empty); the line then carries max d of the map, the launches the chain
enqueues and the launches that find a front.
`a_device` is route A WITHOUT its two host copies per layer.  `a_inpaint` is the inpaint layer's share of a_device (the same host code
runs inside B).  Host wall time per tick: p50 and p10 / p90 of --ticks ticks after --warmup.  The one condition: B must not be slower
than a_device; `b_not_slower_than_a_device` reports it.  The bits of both routes are compared after each series.  One JSON line per
(map, list)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elevation_mapping_cupy_amd import ElevationMap  # noqa: E402
from elevation_mapping_cupy_amd.configs import CORE_PARAM_YAML, parameter_from  # noqa: E402

PLUGINS = """
min_filter: {enable: True, fill_nan: False, is_height_layer: True, layer_name: min_filter, extra_params: {dilation_size: 1, iteration_n: 30}}
smooth_filter: {enable: True, fill_nan: False, is_height_layer: True, layer_name: smooth, extra_params: {input_layer_name: min_filter}}
inpainting: {enable: True, fill_nan: False, is_height_layer: True, layer_name: inpaint, extra_params: {method: %s}}
"""
LISTS = (("filters", ["min_filter", "smooth", "elevation"]), ("filter_publisher", ["min_filter", "smooth", "inpaint", "elevation"]))


def prepared_map(cell_n, plugin_file, points_per_cell=0.5):
    cfg = dict(CORE_PARAM_YAML, enable_visibility_cleanup=False)
    p = parameter_from(cfg, cell_n)
    p.plugin_config_file = plugin_file
    m = ElevationMap(p)
    rng = np.random.default_rng(7)
    L = cell_n * m.resolution / 2
    n = min(int(cell_n * cell_n * points_per_cell), 1 << 22)    # 0.5: half the cells stay unknown, the filters have work to do
    pts = np.empty((n, 3), np.float32)
    pts[:, 0] = rng.uniform(-L, L, n); pts[:, 1] = rng.uniform(-L, L, n); pts[:, 2] = -1.0 + 0.02 * np.sin(3.0 * pts[:, 0])
    m.input_pointcloud(pts, ["x", "y", "z"], np.eye(3, dtype=np.float32), np.array([0, 0, 1.0], np.float32), 0.0, 0.0)
    m.move_to(np.array([0.12, -0.2, 0.05], np.float32), np.eye(3, dtype=np.float32))
    m.sync()
    return m


def max_l1_distance(known):
    """max over the cells of the L1 distance to the nearest known cell (the d of csrc/emap_inpaint_fronts.hip); 0 without a known cell"""
    if not known.any():
        return 0
    big = known.size
    g = np.where(known, 0, big).astype(np.int64)
    for axis in (0, 1):
        g = np.moveaxis(g, axis, 0)
        for i in range(1, g.shape[0]):
            np.minimum(g[i], g[i - 1] + 1, out=g[i])
        for i in range(g.shape[0] - 2, -1, -1):
            np.minimum(g[i], g[i + 1] + 1, out=g[i])
        g = np.moveaxis(g, 0, axis)
    return int(g.max())


def pct(x):
    return [round(float(np.percentile(x, q)), 4) for q in (50, 10, 90)]


def same_bits(a, b):
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cells", type=int, nargs="*", default=[202, 1024])
    ap.add_argument("--inpaint-method", default="telea", choices=["telea", "telea_fronts"])
    ap.add_argument("--points-per-cell", type=float, default=0.5)
    ap.add_argument("--routes", default="ab", choices=["ab", "b"], help="b: route B alone (a kernel trace of the chain's launches only)")
    a = ap.parse_args()
    fronts = a.inpaint_method == "telea_fronts"
    with tempfile.NamedTemporaryFile("w", suffix=".yaml", delete=False) as f:
        f.write(PLUGINS % a.inpaint_method)
    try:
        for cell_n in a.cells:
            m = prepared_map(cell_n, f.name, a.points_per_cell)
            M = cell_n - 2
            for what, layers in (LISTS[1:] if fronts else LISTS):
                rows = np.zeros((len(layers), M, M), np.float32)
                col = np.zeros((len(layers), M, M), np.float32)               # grid_map's column-major MatrixXf: element (i, j) at j * M + i
                wire = np.zeros((len(layers), M * M), np.float32)
                buf = np.zeros((len(layers), M, M), np.float32)               # the publisher keeps its buffer between ticks, as route A keeps its three
                rec = {"a": [], "a_device": [], "a_inpaint": [], "b": []}
                for k in range(a.warmup + a.ticks):
                    for route in (("b",) if a.routes == "b" else ("a", "b") if k % 2 == 0 else ("b", "a")):  # alternate, and alternate who goes first
                        t0 = time.perf_counter()
                        if route == "a":
                            dev = inp = 0.0
                            for j, name in enumerate(layers):
                                t1 = time.perf_counter()
                                m.get_map_with_name_ref(name, rows[j])
                                dt = time.perf_counter() - t1
                                dev += dt
                                inp += dt if name == "inpaint" else 0.0
                                np.copyto(col[j], rows[j].T)                  # gridMap.add(name, RowMatrixXf)
                                np.copyto(wire[j], col[j].reshape(-1))        # toMessage
                        else:
                            msg = m.get_grid_map_message(layers, out=buf)
                        t2 = time.perf_counter()
                        if k >= a.warmup:
                            rec[route].append(1e3 * (t2 - t0))
                            if route == "a":
                                rec["a_device"].append(1e3 * dev); rec["a_inpaint"].append(1e3 * inp)
                if a.routes == "b":
                    print(json.dumps({"cell_n": cell_n, "list": what, "layers": layers, "ticks": a.ticks, "route_b": m.last_plugin_route,
                                      "b_ms_p50_p10_p90": pct(rec["b"])}), flush=True)
                    continue
                same = msg.layers == layers and all(same_bits(wire[j], msg.data[j].data) for j in range(len(layers)))
                p50 = {k: float(np.percentile(v, 50)) for k, v in rec.items()}
                out = {"cell_n": cell_n, "list": what, "layers": layers, "ticks": a.ticks, "route_b": m.last_plugin_route, "layers_equal_bitwise": bool(same),
                       "b_over_a": round(p50["b"] / p50["a"], 4), "b_over_a_device": round(p50["b"] / p50["a_device"], 4),
                       "b_not_slower_than_a_device": bool(p50["b"] <= p50["a_device"])}
                if fronts:
                    dmax = max_l1_distance(m.get_layer_raw(2) >= 0.5)
                    out.update(inpaint_method=a.inpaint_method, points_per_cell=a.points_per_cell, max_d=dmax,
                               advance_launches_enqueued=-(-(2 * cell_n - 2) // 16), advance_launches_with_a_front=-(-dmax // 16))
                for key, v in rec.items():
                    out[key + "_ms_p50_p10_p90"] = pct(v)
                print(json.dumps(out), flush=True)
            m.close()
    finally:
        os.unlink(f.name)


if __name__ == "__main__":
    main()
