"""``MaxLayerFilter`` plugin (reference EM/plugins/max_layer_filter.py:12-108): per-cell maximum (or minimum) over a list of named
layers after an optional chain per layer -- zeros replaced by a default value or by another layer, ``1 - x``, a scale, a 0/1
threshold.  With none of the layers present: a constant plane of the default value, or the traversability layer."""
from typing import List

import numpy as np

from .plugin_manager import PluginBase


class MaxLayerFilter(PluginBase):
    def __init__(self, cell_n: int = 100, layers: list = ("traversability",), reverse: list = (True,), min_or_max: str = "max",
                 thresholds: list = (False,), scales: list = (1.0,), default_value: float = 0.0, **kwargs):
        super().__init__()
        self.layers, self.reverse, self.min_or_max = list(layers), list(reverse), min_or_max
        self.thresholds, self.scales, self.default_value = list(thresholds), list(scales), default_value

    def __call__(self, elevation_map, layer_names: List[str], plugin_layers, plugin_layer_names: List[str], semantic_map,
                 semantic_layer_names: List[str], *args) -> np.ndarray:
        look = (elevation_map, list(layer_names), plugin_layers, list(plugin_layer_names), semantic_map, list(semantic_layer_names))
        prepared = []
        for it, name in enumerate(self.layers):
            layer = self.get_layer_data(*look, name)
            if layer is None:
                continue
            layer = np.asarray(layer)
            if isinstance(self.default_value, float):
                layer = np.where(layer == 0.0, float(self.default_value), layer)
            elif isinstance(self.default_value, str):
                layer = np.where(layer == 0, self.get_layer_data(*look, self.default_value), layer)
            if self.reverse[it]:
                layer = 1.0 - layer
            if len(self.scales) > it and isinstance(self.scales[it], float):
                layer = layer * float(self.scales[it])
            if isinstance(self.thresholds[it], float):
                layer = np.where(layer > float(self.thresholds[it]), 1, 0)
            prepared.append(layer)
        if not prepared:
            print("No layers are found, returning traversability!")
            if isinstance(self.default_value, float):
                return np.full_like(np.asarray(elevation_map[0]), float(self.default_value))
            return elevation_map[list(layer_names).index("traversability")]
        stack = np.stack(prepared, axis=0)
        return stack.min(axis=0) if self.min_or_max == "min" else stack.max(axis=0)

    def device_op(self, layer_names, plugin_layer_names, semantic_layer_names):
        """``EMAP_PLUGIN_MAX_LAYER``: the per-layer steps and the reduction on the device, the layers that exist in the plugin's order (a
        missing one is skipped, as on the host).  Declined (host route): a layer-name ``default_value``, none of the layers found, a
        found map layer beyond the 7 RAW ones, fewer ``reverse`` / ``thresholds`` entries than layers (the host route raises)."""
        from .._lib import PLUGIN_MIN, PLUGIN_SRC_REVERSE, PLUGIN_SRC_SCALE, PLUGIN_SRC_THRESHOLD, PLUGIN_SRC_ZERO_DEFAULT
        if isinstance(self.default_value, str) or len(self.reverse) < len(self.layers) or len(self.thresholds) < len(self.layers):
            return None
        srcs = []
        for it, name in enumerate(self.layers):
            if name not in layer_names and name not in plugin_layer_names and name not in semantic_layer_names:
                continue
            flags, f0, f1, d0 = 0, 0.0, 0.0, 0.0
            if isinstance(self.default_value, float):
                flags, f0 = flags | PLUGIN_SRC_ZERO_DEFAULT, float(self.default_value)
            if self.reverse[it]:
                flags |= PLUGIN_SRC_REVERSE
            if len(self.scales) > it and isinstance(self.scales[it], float):
                flags, f1 = flags | PLUGIN_SRC_SCALE, float(self.scales[it])
            if isinstance(self.thresholds[it], float):
                flags, d0 = flags | PLUGIN_SRC_THRESHOLD, float(self.thresholds[it])
            q = self.source_entry(name, layer_names, plugin_layer_names, semantic_layer_names, flags=flags, f0=f0, f1=f1, d0=d0)
            if q is None:
                return None
            srcs.append(q)
        if not srcs:
            return None
        return dict(type="max_layer", srcs=srcs, flags=PLUGIN_MIN if self.min_or_max == "min" else 0)

    def plugin_inputs(self, plugin_layer_names):
        if isinstance(self.default_value, str):
            return None
        return [n for n in self.layers if n in plugin_layer_names]
