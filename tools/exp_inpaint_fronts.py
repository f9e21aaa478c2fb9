"""Wall time per call of the Inpainting fill: host "telea" (emap_inpaint_telea_u8) against the device "telea_fronts"
(emap_inpaint_telea_fronts_u8), p50 over --calls calls each, both including the host <-> device copies the plugin pays.

Scenes: the 202^2 map of bench.py --workload ref_main after its frames (Parameter defaults, the same seeded 100 000-point cloud and
pose, --frames iterations of input_pointcloud + move_to), quantised as the plugin does; and a 1024^2 map that is >= 90 % unknown.
Prints the fronts count, the launches of S fronts each, and the p50 for S in --steps.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/exp_inpaint_fronts.py`."""
import argparse
import ctypes as ct
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elevation_mapping_cupy_amd import _lib                                  # noqa: E402
from elevation_mapping_cupy_amd.elevation_mapping import ElevationMap        # noqa: E402
from elevation_mapping_cupy_amd.parameter import Parameter                   # noqa: E402

U8P = ct.POINTER(ct.c_uint8)


def ref_main_scene(frames):
    param = Parameter()
    param.update()
    em = ElevationMap(param)
    rng = np.random.default_rng(123)
    R, t = rng.random((3, 3)), rng.random(3)
    points = rng.random((100000, 7))
    for i in range(frames):
        em.input_pointcloud(points[:, :3].copy(), ["x", "y", "z"], R, t.copy(), 0, 0)
        em.move_to(np.array([i * 0.01, i * 0.02, i * 0.01]), R)
    e = np.asarray(em.elevation_map)
    known = e[2] >= 0.5
    h = e[0].astype(np.float32)
    hmin, hmax = float(h[known].min()), float(h[known].max())
    q8 = np.clip((h - hmin) * 255 / (hmax - hmin if hmax > hmin else 1.0), 0, 255).astype(np.uint8)
    return q8, np.ascontiguousarray(~known, np.uint8)


def sparse_scene(n=1024):
    rng = np.random.default_rng(9)
    y, x = np.mgrid[0:n, 0:n]
    img = np.clip(128 + 60 * np.sin(x / 90.0) * np.cos(y / 70.0) + rng.normal(0, 2, (n, n)), 0, 255).astype(np.uint8)
    mask = (rng.uniform(0, 1, (n, n)) > 0.004).astype(np.uint8)
    mask[300:700, 200:900] = 1
    return img, mask


def p50(fn, calls):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--steps", default="4,8,12,16")
    ap.add_argument("--host-calls", type=int, default=50)
    a = ap.parse_args()
    lib = _lib.load()
    ip = ct.c_void_p()
    assert lib.emap_inpainter_create(0, None, ct.byref(ip)) == 0
    for name, (img, mask) in (("202^2 ref_main map", ref_main_scene(a.frames)), ("1024^2 sparse", sparse_scene())):
        out = np.empty_like(img)
        p = lambda x: x.ctypes.data_as(U8P)                                  # noqa: E731
        rows, cols = img.shape
        host = p50(lambda: lib.emap_inpaint_telea_u8(p(img), p(mask), rows, cols, 1, p(out)), a.host_calls)
        n = ct.c_int32(0)
        print("%s: %.1f %% unknown, host telea p50 %.3f ms" % (name, 100.0 * mask.mean(), host), flush=True)
        for s in [int(x) for x in a.steps.split(",")]:
            assert lib.emap_inpainter_set_steps(ip, s) == 0
            dev = p50(lambda: lib.emap_inpaint_telea_fronts_u8(ip, p(img), p(mask), rows, cols, 1, p(out), ct.byref(n)), a.calls)
            print("  telea_fronts S=%2d: fronts %d, launches %d, p50 %.3f ms" % (s, n.value, -(-n.value // s), dev), flush=True)
    lib.emap_inpainter_destroy(ip)


if __name__ == "__main__":
    main()
