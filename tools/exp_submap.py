#!/usr/bin/env python
"""Single-question experiment: what does a batch of submaps cost at the map's output door?

A planner's tick on a 202^2 (robot scale) and a 1024^2 map whose cells are known and whose `rgb` layer is fused: batches of 1, 4 and
64 requests of 50 x 50 cells each, the shipped publisher's four layers.  Two routes, in ONE process on one box, ALTERNATING tick by
tick on the same map (both only read it):
  A  the only way without the service: get_grid_map_message of the WHOLE map (the publisher keeps its buffer between ticks), then
     per request the geometry and a contiguous copy of each layer's slice on the host
  B  get_submap_messages: the geometry, one upload of the window table, one launch over the windows' tiles, one copy of the packed
     result, one wait
Host wall time per tick: p50 and p10 / p90 of --ticks ticks after --warmup.  After each series B's planes are compared with A's slices
bit for bit (NaN with NaN).  The one condition fixed in advance: at 1024^2 B must not be slower than A in any row (it moves at most
1/400 of A's bytes); the exit status is 1 if it is, or if the planes differ.  At 202^2 both are launch- and wait-bound: whatever comes
is reported.  The first lines carry the source stamp (bench.py: source_stamp); then one JSON line per (map, batch)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elevation_mapping_cupy_amd.elevation_mapping import submap_geometry  # noqa: E402
from tools.exp_grid_map import SHIPPED, pct, prepared_map  # noqa: E402

SIDE = 50


def requests_of(m, n):
    """n requests of SIDE x SIDE cells whose corners lie strictly inside cells, spread over the middle of the map"""
    res = float(np.float32(m.resolution))
    cx, cy = float(m.center[0]), float(m.center[1])
    return [((cx + ((7 * k) % 101 - 50 + 0.3) * res, cy + ((11 * k) % 101 - 50 + 0.3) * res), ((SIDE - 0.8) * res, (SIDE - 0.8) * res)) for k in range(n)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cells", type=int, nargs="*", default=[202, 1024])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 4, 64])
    a = ap.parse_args()
    print("# tools/exp_submap.py: whole-map message + host slices (A) against get_submap_messages (B), alternating on one box; host wall ms, p50 [p10, p90]")
    print("# source_stamp: %s" % bench.source_stamp(), flush=True)
    bad = False
    for cell_n in a.cells:
        m = prepared_map(cell_n)
        M = cell_n - 2
        res = float(np.float32(m.resolution))
        centre = (float(m.center[0]), float(m.center[1]))
        msg = m.get_grid_map_message(SHIPPED)
        L = len(msg.layers)
        buf = np.zeros((L, M, M), np.float32)                                # route A's publisher keeps its buffer between ticks
        for n in a.batches:
            reqs = requests_of(m, n)
            geo = [submap_geometry(centre, M * res, res, M, p, ln) for p, ln in reqs]
            assert all(g is not None and g[2] == SIDE and g[3] == SIDE for g in geo), geo
            out = np.zeros(L * sum(g[2] * g[3] for g in geo), np.float32)     # and route B its packed buffer
            rec = {"a": [], "b": []}
            for k in range(a.warmup + a.ticks):
                for route in (("a", "b") if k % 2 == 0 else ("b", "a")):      # alternate, and alternate who goes first
                    t0 = time.perf_counter()
                    if route == "a":
                        whole = m.get_grid_map_message(SHIPPED, out=buf)
                        slices = []
                        for p, ln in reqs:
                            i0, j0, ni, nj = submap_geometry(centre, M * res, res, M, p, ln)[:4]
                            slices.append([np.ascontiguousarray(d.data.reshape(M, M)[j0:j0 + nj, i0:i0 + ni]) for d in whole.data])
                    else:
                        answers = m.get_submap_messages(reqs, SHIPPED, out=out)
                    t1 = time.perf_counter()
                    if k >= a.warmup:
                        rec[route].append(1e3 * (t1 - t0))
            same = all(ok and same_bits(d.data.reshape(s.shape), s) for (msg_b, ok), sl in zip(answers, slices) for d, s in zip(msg_b.data, sl))
            p50 = {k: float(np.percentile(v, 50)) for k, v in rec.items()}
            row = {"cell_n": cell_n, "batch": n, "window": [SIDE, SIDE], "layers": L, "ticks": a.ticks, "route_b": m.last_submap_route,
                   "planes_equal_bitwise": bool(same), "bytes_d2h_a": 4 * L * M * M, "bytes_d2h_b": 4 * L * n * SIDE * SIDE, "bytes_h2d_b": 32 * n + 16 * 4 * n,
                   "b_over_a": round(p50["b"] / p50["a"], 4), "b_not_slower_than_a": bool(p50["b"] <= p50["a"])}
            for key, v in rec.items():
                row[key + "_ms_p50_p10_p90"] = pct(v)
            print(json.dumps(row), flush=True)
            bad = bad or not same or (cell_n >= 1024 and not row["b_not_slower_than_a"])
        m.close()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
