#!/usr/bin/env python
"""Single-question experiment: what does the map's point-cloud output (the node's elevation_map_points publisher) cost?

A publisher's tick on a 202^2 (robot scale) and a 1024^2 map, the layer lists [elevation] and the shipped publisher's four layers, with
0 %, about 50 % and 100 % of the cells valid.  Two routes, in ONE process on one box, ALTERNATING tick by tick on the same map (both
only read it) and alternating who goes first:
  A  the only way without the door: get_grid_map_message of the WHOLE map into a kept buffer (M^2 floats per layer over PCIe), then
     the NumPy compaction on the host -- isfinite, nonzero, two gathers for x and y, one gather per layer, the interleave into a kept
     record buffer
  B  get_point_cloud_message into a kept buffer: one upload of the position tables, three launches, the 4-byte count, then exactly
     n * point_step bytes
Host wall time per tick: p50 and p10 / p90 of --ticks ticks after --warmup.  After each series the bytes of B are compared with those
of A.  No ratio is fixed in advance: at 100 % fill with [elevation] alone B moves three floats per cell where A moves one, and may
lose that row; whatever comes is reported.  The exit status is 1 only if the bytes differ.  The first lines carry the source stamp
(bench.py: source_stamp); then one JSON line per (map, list, fill)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elevation_mapping_cupy_amd.elevation_mapping import grid_cell_positions  # noqa: E402
from tools.exp_grid_map import SHIPPED, pct, prepared_map  # noqa: E402

LISTS = {"elevation": ["elevation"], "shipped": SHIPPED}
FILLS = (0.0, 0.5, 1.0)


def compact(msg, xs, ys, rec):
    """route A's host walk: the valid cells of the whole-map message as records x, y, z, then the other layers, in iterator order"""
    planes = [d.data for d in msg.data]                                     # flat, column-major: iteration order
    lin = np.flatnonzero(np.isfinite(planes[0]))                            # basic layer = point layer = elevation, the first of both lists
    M = xs.size
    out = rec[:lin.size]
    out[:, 0] = xs[lin % M]
    out[:, 1] = ys[lin // M]
    for k, p in enumerate(planes):
        out[:, 2 + k] = p[lin]
    return out


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cells", type=int, nargs="*", default=[202, 1024])
    a = ap.parse_args()
    print("# tools/exp_point_cloud.py: whole-map message + NumPy compaction (A) against get_point_cloud_message (B), alternating on one box; host wall ms, p50 [p10, p90]")
    print("# source_stamp: %s" % bench.source_stamp(), flush=True)
    bad = False
    for cell_n in a.cells:
        m = prepared_map(cell_n)
        M = cell_n - 2
        xs, ys = (t.astype(np.float32) for t in grid_cell_positions((float(m.center[0]), float(m.center[1])), float(np.float32(m.resolution)), M))
        rng = np.random.default_rng(3)
        for fill in FILLS:
            valid = np.zeros((cell_n, cell_n), np.float32)
            valid[1:-1, 1:-1] = rng.random((M, M)) < fill
            m.set_layer_raw("is_valid", valid)
            for tag, layers in LISTS.items():
                L = len(layers)
                buf = np.zeros((L, M, M), np.float32)                        # route A's publisher keeps its buffers between ticks
                rec = np.zeros((M * M, 2 + L), np.float32)
                out = np.zeros(M * M * (2 + L), np.float32)                  # and route B its record buffer
                t = {"a": [], "b": []}
                for k in range(a.warmup + a.ticks):
                    for route in (("a", "b") if k % 2 == 0 else ("b", "a")):      # alternate, and alternate who goes first
                        t0 = time.perf_counter()
                        if route == "a":
                            got_a = compact(m.get_grid_map_message(layers, out=buf), xs, ys, rec)
                        else:
                            got_b = m.get_point_cloud_message(layers, out=out)
                        t1 = time.perf_counter()
                        if k >= a.warmup:
                            t[route].append(1e3 * (t1 - t0))
                same = got_b.width == got_a.shape[0] and got_b.data.tobytes() == got_a.tobytes()
                p50 = {k: float(np.percentile(v, 50)) for k, v in t.items()}
                row = {"cell_n": cell_n, "layers": tag, "fill": fill, "points": int(got_b.width), "ticks": a.ticks, "route_b": m.last_point_cloud_route,
                       "bytes_equal": bool(same), "bytes_d2h_a": 4 * L * M * M, "bytes_d2h_b": 4 + int(got_b.row_step), "bytes_h2d_b": 16 + 8 * M,
                       "b_over_a": round(p50["b"] / p50["a"], 4)}
                for key, v in t.items():
                    row[key + "_ms_p50_p10_p90"] = pct(v)
                print(json.dumps(row), flush=True)
                bad = bad or not same
        m.close()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
