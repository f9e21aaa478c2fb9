#!/usr/bin/env python
"""Single-question experiment: what does a camera message cost at the map's door?

Two 480 x 640 messages a camera pipeline publishes next to each other -- an `rgb8` colour image (channels ["rgb"]) and a `32FC1` feature
image (channels ["feat"]) -- on a 202^2 (robot scale) and a 1024^2 map whose cells are known (a flat floor fused first), camera 1.5 m
above the centre looking down.  Two routes, in ONE process on one box, ALTERNATING call by call on two maps in the same state:
  A  the node's host conversion restated in NumPy (bytes -> (H, W, C) -> one float32 plane per channel; the node's cv::split +
     cv2eigen, elevation_mapping_ros.cpp:418-426) + input_image           -- the route before emap_input_image_message
  B  input_image_message(message bytes)                                   -- the bytes are uploaded, one launch does the rest
Per call two host clocks: `call` = until the call returns, `idle` = until the stream is idle (emap_sync) -- work that ends in a device
synchronise.  A counts its conversion (it is work the route needs per message; `convert` reports it alone).  p50 and p10 / p90 of
--frames calls after --warmup.  What is expected, and why: bytes over PCIe fall from 4 n_chan H W (A uploads the float stack) to
H step; launches from 1 + layers to 1; host-device synchronisations from `layers` to 0.  No threshold is asserted.
One JSON line per (map, message, route)."""
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

H, W = 480, 640
R_DOWN = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]], np.float32)
CAM_Z = 1.5


def messages(k):
    rng = np.random.default_rng(k)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    feat = rng.random((H, W), dtype=np.float32)
    return {"rgb8": (rgb.reshape(-1), ["rgb"], 3, np.uint8), "32FC1": (feat.view(np.uint8).reshape(-1), ["feat"], 1, np.float32)}


def node_planes(data, n_chan, dtype):
    """the node's conversion: split into one matrix per channel, each widened to float32"""
    px = data.view(dtype).reshape(H, W, n_chan)
    return [np.ascontiguousarray(px[:, :, c]).astype(np.float32) for c in range(n_chan)]


def prepared_map(cell_n):
    cfg = dict(CORE_PARAM_YAML, enable_visibility_cleanup=False)
    m = ElevationMap(parameter_from(cfg, cell_n))
    m.param.image_channel_fusions = {"rgb": "color", "default": "exponential"}
    rng = np.random.default_rng(7)
    L = cell_n * m.resolution / 2
    n = min(4 * cell_n * cell_n, 1 << 22)
    p = np.empty((n, 3), np.float32)
    p[:, 0] = rng.uniform(-L, L, n); p[:, 1] = rng.uniform(-L, L, n); p[:, 2] = -1.0 + 0.02 * np.sin(3.0 * p[:, 0])
    m.input_pointcloud(p, ["x", "y", "z"], np.eye(3, dtype=np.float32), np.array([0, 0, 1.0], np.float32), 0.0, 0.0)
    m.sync()
    return m


def pct(x):
    return [round(float(np.percentile(x, q)), 4) for q in (50, 10, 90)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cells", type=int, nargs="*", default=[202, 1024])
    a = ap.parse_args()
    msgs = [messages(k) for k in range(4)]
    for cell_n in a.cells:
        ma, mb = prepared_map(cell_n), prepared_map(cell_n)
        # the image's footprint covers the map: focal length so that W pixels span the map's side at CAM_Z
        f = W * CAM_Z / (cell_n * ma.resolution)
        K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)
        D = np.zeros(5, np.float32)
        t = (-R_DOWN @ np.array([0.0, 0.0, CAM_Z])).astype(np.float32)
        for enc in ("rgb8", "32FC1"):
            rec = {"A": {"call": [], "idle": [], "convert": []}, "B": {"call": [], "idle": []}}
            for k in range(a.warmup + a.frames):
                data, channels, n_chan, dtype = msgs[k % 4][enc]
                for route in (("A", "B") if k % 2 == 0 else ("B", "A")):      # alternate, and alternate who goes first
                    m = ma if route == "A" else mb
                    m.sync()
                    t0 = time.perf_counter()
                    if route == "A":
                        planes = node_planes(data, n_chan, dtype)
                        t1 = time.perf_counter()
                        m.input_image(planes, channels, R_DOWN, t, K, D, "radtan", H, W)
                    else:
                        t1 = t0
                        m.input_image_message(data, channels, R_DOWN, t, K, D, height=H, width=W, encoding=enc)
                    t2 = time.perf_counter()
                    m.sync()
                    t3 = time.perf_counter()
                    if k >= a.warmup:
                        rec[route]["call"].append(1e3 * (t2 - t0)); rec[route]["idle"].append(1e3 * (t3 - t0))
                        if route == "A":
                            rec[route]["convert"].append(1e3 * (t1 - t0))
            va = ma.get_image_correspondence()[1]
            same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ma.semantic_map.semantic_map, mb.semantic_map.semantic_map))
            for route in ("A", "B"):
                out = {"cell_n": cell_n, "message": enc, "route": route, "frames": a.frames, "visible_cells": int(va.sum()),
                       "bytes_uploaded": int(4 * n_chan * H * W if route == "A" else data.size), "layers_equal_bitwise": bool(same)}
                for key, v in rec[route].items():
                    out[key + "_ms_p50_p10_p90"] = pct(v)
                print(json.dumps(out), flush=True)
        ma.close(); mb.close()


if __name__ == "__main__":
    main()
