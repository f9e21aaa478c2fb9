#!/usr/bin/env python
"""Single-question experiment: what does a depth camera's frame cost at the map's door?

480 x 640 and 720 x 1280 uint16 frames (depth_scale 0.001, a camera 1.2 m above a wavy floor) on a 1024^2 map, core_param.yaml without
the visibility pass; per frame host wall time from the call to an idle stream (emap_sync), p50 / p90 of --frames frames after --warmup:
  (a) input_depth_image                                    -- the images are uploaded, the cloud is produced on the device
  (b) NumPy back-projection + input_pointcloud(float32)    -- the route before emap_bind_depth_image, same commit, same box
  (c) input_pointcloud of a precomputed float32 cloud      -- (b) without the host back-projection
Run under `rocprofv3 --kernel-trace --stats -- python tools/exp_depth_input.py --only a` for k_depth_cloud's own time; its share of
the HBM peak follows from 12 + 4 Kc + input bytes per pixel (printed as bytes_per_pixel).  One JSON line per (shape, route)."""
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

SCALE = np.float32(0.001)
R = np.diag([1.0, -1.0, -1.0]).astype(np.float32)
T = np.array([0.1, -0.05, 1.2], np.float32)


def frame(H, W, k):
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d = 1.2 - 0.15 * np.sin(6 * np.pi * u / W + 0.1 * k) * np.cos(2 * np.pi * v / H)
    raw = np.rint(d / float(SCALE)).astype(np.uint16)
    raw[::37, ::41] = 0                                     # sensor holes
    return raw


def host_backproject(raw, K):
    """the reference's create_pcl_from_image in float32, NaN rows instead of the compaction (what input_pointcloud skips)"""
    H, W = raw.shape
    z = raw.astype(np.float32) * SCALE
    u = np.arange(W, dtype=np.float32)[None, :]
    v = np.arange(H, dtype=np.float32)[:, None]
    x = (u - np.float32(K[0, 2])) * z / np.float32(K[0, 0])
    y = (v - np.float32(K[1, 2])) * z / np.float32(K[1, 1])
    p = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    p[~((z > 0) & (z < 8)).reshape(-1)] = np.nan
    return p


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
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    a = ap.parse_args()
    cfg = dict(CORE_PARAM_YAML, enable_visibility_cleanup=False)
    for H, W in ((480, 640), (720, 1280)):
        K = np.array([[0.8 * W, 0, (W - 1) / 2 + 0.25], [0, 0.8 * W, (H - 1) / 2 - 0.5], [0, 0, 1]])
        raws = [frame(H, W, k) for k in range(8)]
        clouds = [host_backproject(r, K) for r in raws]
        routes = {
            "a": lambda m: (lambda k: m.input_depth_image(raws[k % 8], K, [], R, T.copy(), 0.0, 0.0, depth_scale=float(SCALE))),
            "b": lambda m: (lambda k: m.input_pointcloud(host_backproject(raws[k % 8], K), ["x", "y", "z"], R, T.copy(), 0.0, 0.0)),
            "c": lambda m: (lambda k: m.input_pointcloud(clouds[k % 8], ["x", "y", "z"], R, T.copy(), 0.0, 0.0)),
        }
        for name in ("a", "b", "c"):
            if a.only and a.only != name:
                continue
            m = ElevationMap(parameter_from(cfg, a.cell_n))
            p50, p90 = run(m, routes[name](m), a.frames, a.warmup)
            path = m.last_update_path()
            m.close()
            print(json.dumps({"image": [H, W], "points": H * W, "route": name, "p50_ms": round(p50, 4), "p90_ms": round(p90, 4), "frame_path": path,
                              "frames": a.frames, "bytes_per_pixel": 2 + 12, "cell_n": a.cell_n}), flush=True)


if __name__ == "__main__":
    main()
