#!/usr/bin/env python
"""Single-question experiment: what does a PointCloud2 message cost at the map's door?

Messages of 2^20 points (a wavy floor seen from 1.2 m, a few NaN returns) at point_step 16 (xyz + intensity), 22 (Velodyne: xyz,
intensity, ring UINT16, time at offset 18) and 32 (PCL XYZRGB: rgb at 16, padding) on a 1024^2 map, core_param.yaml without the
visibility pass; per frame host wall time from the call to an idle stream (emap_sync), p50 / p90 of --frames frames after --warmup:
  (a) input_pointcloud2(message bytes)                       -- the bytes are uploaded, the cloud is unpacked on the device
  (b) NumPy gather into an (n, cols) float64 matrix + input_pointcloud   -- the node's loop (elevation_mapping_ros.cpp:319-338), vectorised
                                                                (which flatters it), and the route before emap_bind_cloud_message
  (c) input_pointcloud of a ready float32 cloud              -- no gather at all
Every column is moved (typed=False, the reference's behaviour); the channels are not fused (no channel fusion is configured for them),
so the three routes differ only in front of the frame.  Run under `rocprofv3 --kernel-trace --stats -- python tools/exp_pc2_input.py
--only a` for k_cloud_unpack's own time; it reads point_step and writes 12 + 4 Kc bytes a point (printed as bytes_per_point).  One
JSON line per (point_step, route)."""
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

R = np.diag([1.0, -1.0, -1.0]).astype(np.float32)
T = np.array([0.1, -0.05, 1.2], np.float32)
F32, U16 = 7, 4
LAYOUTS = {
    16: [("x", 0, F32, 1), ("y", 4, F32, 1), ("z", 8, F32, 1), ("intensity", 12, F32, 1)],
    22: [("x", 0, F32, 1), ("y", 4, F32, 1), ("z", 8, F32, 1), ("intensity", 12, F32, 1), ("ring", 16, U16, 1), ("time", 18, F32, 1)],
    32: [("x", 0, F32, 1), ("y", 4, F32, 1), ("z", 8, F32, 1), ("rgb", 16, F32, 1)],
}


def message(ps, n, k):
    """the bytes of frame k: n points of a 1024-wide scan pattern over the floor, junk in the bytes no field covers"""
    rng = np.random.default_rng(ps * 100 + k)
    side = int(np.sqrt(n))
    v, u = np.divmod(np.arange(n), side)
    x = ((u + 0.5) / side - 0.5) * 18.0
    y = ((v + 0.5) / side - 0.5) * 18.0
    z = 1.2 - 0.15 * np.sin(0.9 * x + 0.1 * k) * np.cos(0.7 * y)
    z[::1511] = np.nan                                      # missing returns
    pts = rng.integers(0, 256, (n, ps), dtype=np.uint8)
    for name, off, dt, _ in LAYOUTS[ps]:
        if dt == U16:
            col = (np.arange(n) % 64).astype("<u2")
        elif name == "rgb":
            col = rng.integers(0, 1 << 24, n, dtype=np.uint32)
        else:
            col = {"x": x, "y": y, "z": z}.get(name, rng.random(n)).astype("<f4")
        pts[:, off:off + col.dtype.itemsize] = col.view(np.uint8).reshape(n, -1)
    return pts.reshape(-1)


def node_gather(data, ps, n):
    """the node's loop, vectorised: per field the 4 bytes at its offset as a float, widened into the (n, fields) float64 matrix"""
    pts = data.reshape(n, ps)
    out = np.empty((n, len(LAYOUTS[ps])), np.float64)
    for j, (_, off, _, _) in enumerate(LAYOUTS[ps]):
        out[:, j] = np.ascontiguousarray(pts[:, off:off + 4]).view("<f4")[:, 0]
    return out


def run(m, fn, frames, warmup):
    ms = []
    for k in range(warmup + frames):
        m.sync()
        t0 = time.perf_counter()
        fn(k)
        m.sync()
        if k >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.percentile(ms, 50)), float(np.percentile(ms, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cell-n", type=int, default=1024)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    a = ap.parse_args()
    cfg = dict(CORE_PARAM_YAML, enable_visibility_cleanup=False)
    n = a.points
    for ps in (16, 22, 32):
        fields = LAYOUTS[ps]
        names = [f[0] for f in fields]
        msgs = [message(ps, n, k) for k in range(4)]
        ready = [node_gather(d, ps, n).astype(np.float32) for d in msgs]
        kw = dict(fields=fields, width=n, height=1, point_step=ps)
        routes = {
            "a": lambda m: (lambda k: m.input_pointcloud2(msgs[k % 4], R, T.copy(), 0.0, 0.0, **kw)),
            "b": lambda m: (lambda k: m.input_pointcloud(node_gather(msgs[k % 4], ps, n), names, R, T.copy(), 0.0, 0.0)),
            "c": lambda m: (lambda k: m.input_pointcloud(ready[k % 4], names, R, T.copy(), 0.0, 0.0)),
        }
        for name in ("a", "b", "c"):
            if a.only and a.only != name:
                continue
            m = ElevationMap(parameter_from(cfg, a.cell_n))
            p50, p90 = run(m, routes[name](m), a.frames, a.warmup)
            path = m.last_update_path()
            m.close()
            print(json.dumps({"point_step": ps, "points": n, "columns": len(fields), "route": name, "p50_ms": round(p50, 4), "p90_ms": round(p90, 4),
                              "frame_path": path, "frames": a.frames, "bytes_per_point": ps + 12 + 4 * (len(fields) - 3), "cell_n": a.cell_n}), flush=True)


if __name__ == "__main__":
    main()
