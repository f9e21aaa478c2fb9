"""``Inpainting`` plugin (reference EM/plugins/inpainting.py:14-63).

Same semantics around the fill as the reference: mask = ``is_valid < 0.5``, the elevation is quantised to 8 bits over
[h_min, h_max] of the valid cells (``astype("uint8")`` truncation), inpainted with radius 1, de-quantised
(``* (h_max - h_min) / 255 + h_min``), returned as float64.  The fill itself:

* ``method="telea"`` (the reference's default, ``cv2.INPAINT_TELEA``): Telea's fast-marching method, HOST code of ``libemap_hip.so``
  (``emap_inpaint_telea_u8``) -- the reference runs this step on the CPU as well (``cp.asnumpy`` + ``cv2.inpaint``): the algorithm is
  a serial priority-queue march.  OpenCV is an unpinned third-party dependency that is absent here, so this is a restatement of the
  published algorithm and **parity with OpenCV's values is unpinned** (tests/test_inpaint_telea.py pins it against a second,
  line-by-line restatement and checks the properties every implementation must have).
* ``method="front"``: the round-1/2 device-side substitute (``emap_inpaint_u8``: front-by-front distance-weighted mean of the known
  8-neighbours on the MI355X) for maps where a host pass per publish is too slow; needs the owning ElevationMap.
* ``method="telea_fronts"``: Telea's estimator ON THE MI355X (``emap_inpaint_telea_fronts_u8``, csrc/emap_inpaint_fronts.hip): the
  arithmetic of the host ``"telea"`` with radius 1, scheduled by fronts of the L1 distance to the known cells (every cell of a front at
  once) instead of by the serial priority queue -- exactly specified and deterministic, not bit-identical to ``"telea"`` (DESIGN.md §8:
  agreement figures).  Same quantisation around the fill as ``"telea"``.  Its handle is created on first use on the owning
  ElevationMap's device and stream (the manager injects ``emap``), else on the current device's null stream.  The reference has no
  such name and falls back to telea for it (reference plugins/inpainting.py:26-31), so a YAML naming it runs on both.
  This method is also an op of ``emap_plugin_chain`` (``device_op``: ``EMAP_PLUGIN_INPAINT_FRONTS``, csrc/emap_inpaint_chain.hip): in a
  publisher's list (``ElevationMap.get_grid_map_layers``) the range, the 8-bit image, the mask, the fill and the de-quantisation run on
  the map's own cells into a resident plane, bit for bit what ``__call__`` returns, with no copy over PCIe and no wait; ``fronts_run``
  is ``None`` afterwards (nothing waited for it).  ``steps`` (extra parameter, 1 .. 16; 0: the library's default of 16) sets the
  fronts per launch on either route; the result does not depend on it.
* ``method="ns"`` (``cv2.INPAINT_NS``, reference plugins/inpainting.py:33-38): the Navier-Stokes based method in its fast-marching form,
  HOST code as well (``emap_inpaint_ns_u8``): the same march as Telea's, a pixel = the mean of the known pixels within the radius
  weighted along the isophote direction.  Parity with OpenCV's values unpinned like "telea" (tests/test_inpaint_ns.py)."""
from __future__ import annotations

import ctypes as ct
from typing import List

import numpy as np

from .. import _lib
from .._lib import f32p
from .plugin_manager import PluginBase


class Inpainting(PluginBase):
    def __init__(self, cell_n: int = 100, method: str = "telea", emap=None, steps: int = 0, **kwargs):
        super().__init__()
        self.steps = int(steps)                    # "telea_fronts": fronts per launch (0: the library's default)
        self.method = method if method in ("telea", "ns", "front", "telea_fronts") else "telea"      # (the reference falls back to telea for unknown names, :37-38)
        self.cell_n = cell_n
        self.emap = emap
        self.sweeps_run = 0
        self.fronts_run = 0
        self._ip = None                            # emap_inpainter of method "telea_fronts" (created on first use)

    def plugin_inputs(self, plugin_layer_names):
        return ()                                  # elevation and is_valid of the map only: no resident plane has to come back for it

    def device_op(self, layer_names, plugin_layer_names, semantic_layer_names):
        if self.method != "telea_fronts":
            return None                            # "telea" / "ns" are host marches, "front" has its own host door
        return dict(type="inpaint_fronts", src=None, i0=self.steps)

    def __call__(self, elevation_map: np.ndarray, layer_names: List[str], plugin_layers: np.ndarray,
                 plugin_layer_names: List[str], *args) -> np.ndarray:
        known = np.ascontiguousarray(np.asarray(elevation_map[2]) >= 0.5)
        if not known.any() or known.all():
            return elevation_map[0]
        h = np.asarray(elevation_map[0], np.float32)
        h_max, h_min = float(h[known].max()), float(h[known].min())
        span = (h_max - h_min) if h_max > h_min else 1.0
        q8 = np.clip((h - h_min) * 255 / span, 0, 255).astype(np.uint8)            # 8-bit image, truncation like astype("uint8")
        if self.method in ("telea", "ns", "telea_fronts"):
            lib = _lib.load()
            mask = np.ascontiguousarray(~known, np.uint8)
            out8 = np.empty_like(q8)
            p = lambda a: a.ctypes.data_as(ct.POINTER(ct.c_uint8))               # noqa: E731
            if self.method == "telea_fronts":
                n = ct.c_int32(0)
                rc = lib.emap_inpaint_telea_fronts_u8(self._inpainter(lib), p(np.ascontiguousarray(q8)), p(mask), q8.shape[0], q8.shape[1], 1,
                                                      p(out8), ct.byref(n))
                self.fronts_run = n.value
            else:
                fill = lib.emap_inpaint_telea_u8 if self.method == "telea" else lib.emap_inpaint_ns_u8
                rc = fill(p(np.ascontiguousarray(q8)), p(mask), q8.shape[0], q8.shape[1], 1, p(out8))
            if rc != 0:
                raise _lib.EmapError("emap_inpaint_%s_u8 failed (%d)" % (self.method, rc))
            out = out8.astype(np.float32)
        else:
            if self.emap is None:
                raise RuntimeError("Inpainting(method='front') needs the owning ElevationMap (PluginManager(emap=...)): it runs on the device")
            q = q8.astype(np.float32)
            out = np.empty_like(q)
            n = ct.c_int32(0)
            e = self.emap
            e._chk(e._lib.emap_inpaint_u8(e._ctx, f32p(np.ascontiguousarray(q)), f32p(known.astype(np.float32)),
                                          int(2 * self.cell_n), f32p(out), ct.byref(n)))
            self.sweeps_run = n.value
        return (out * np.float32(span) / np.float32(255) + np.float32(h_min)).astype(np.float64)

    def _inpainter(self, lib):
        if self._ip is None:
            if self.emap is not None:
                device, stream = int(self.emap.param.device), int(getattr(self.emap, "stream", 0) or 0)
            else:
                device, stream = -1, 0                  # (-1: the current device)
            h = ct.c_void_p()
            rc = lib.emap_inpainter_create(device, ct.c_void_p(stream or None), ct.byref(h))
            if rc != 0:
                raise _lib.EmapError("emap_inpainter_create failed (%d): no usable HIP device %d" % (rc, device))
            if self.steps and lib.emap_inpainter_set_steps(h, self.steps) != 0:
                lib.emap_inpainter_destroy(h)
                raise _lib.EmapError("Inpainting: steps must lie in 1 .. 16 (got %d)" % self.steps)
            self._ip = h
        return self._ip

    def close(self):
        """Free the device scratch of method "telea_fronts" (a later call creates it again).  The inpainter enqueues on the owning
        ElevationMap's stream only while a call runs, and destroying it does not touch that stream, so closing after the stream is
        gone is safe; a call after the stream is gone is not."""
        ip, self._ip = getattr(self, "_ip", None), None
        if ip is not None and ip.value:
            _lib.load().emap_inpainter_destroy(ip)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
