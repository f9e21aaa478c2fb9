"""``MaxFilter`` plugin: fill invalid cells with the maximum value around them (reference EM/plugins/max_filter.py:12-112).
The sweeps run on the MI355X (``emap_max_filter``: the min-filter sweep kernel with the comparison reversed)."""
from __future__ import annotations

import ctypes as ct
from typing import List

import numpy as np

from .._lib import f32p
from .plugin_manager import PluginBase


class MaxFilter(PluginBase):
    def __init__(self, cell_n: int = 100, dilation_size: int = 5, iteration_n: int = 5, emap=None, **kwargs):
        super().__init__()
        self.iteration_n = int(iteration_n)
        self.dilation_size = int(dilation_size)
        self.width = self.height = cell_n
        self.emap = emap
        self.sweeps_run = 0                # sweeps the last host-route call ran; None after the device route, which does not wait for its counters

    def device_op(self, layer_names, plugin_layer_names, semantic_layer_names):
        if not (0 <= self.dilation_size <= 32 and 0 <= self.iteration_n <= 4096):
            return None
        return dict(type="max_filter", src=None, i0=self.dilation_size, i1=self.iteration_n)

    def plugin_inputs(self, plugin_layer_names):
        return ()

    def __call__(self, elevation_map: np.ndarray, layer_names: List[str], plugin_layers: np.ndarray,
                 plugin_layer_names: List[str], *args) -> np.ndarray:
        if self.emap is None:
            raise RuntimeError("MaxFilter needs the owning ElevationMap (PluginManager(emap=...)): it runs on the device")
        e = self.emap
        out = np.empty((e.cell_n, e.cell_n), np.float32)
        n = ct.c_int32(0)
        if getattr(elevation_map, "device_map", None) is e:
            # the map's own live planes (get_map_with_name_ref): NULL inputs = read elevation / is_valid on the device, only the
            # result crosses PCIe
            e._chk(e._lib.emap_max_filter(e._ctx, None, None, self.dilation_size, self.iteration_n, f32p(out), ct.byref(n)))
        else:
            h = np.ascontiguousarray(elevation_map[0], np.float32)
            v = np.ascontiguousarray(elevation_map[2], np.float32)
            e._chk(e._lib.emap_max_filter(e._ctx, f32p(h), f32p(v), self.dilation_size, self.iteration_n, f32p(out), ct.byref(n)))
        self.sweeps_run = n.value
        return out
