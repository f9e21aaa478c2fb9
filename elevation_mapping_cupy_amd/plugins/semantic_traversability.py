"""``SemanticTraversability`` plugin (reference EM/plugins/semantic_traversability.py:12-83): votes of named layers -- a layer of type
"traversability" votes where it is AT OR BELOW its threshold, any other type where it is at or above -- and the result is 1 where at
least one layer voted, 0.1 elsewhere.  A layer name that exists nowhere ends the plugin without a layer (the reference returns None)."""
from typing import List

import numpy as np

from .plugin_manager import PluginBase


class SemanticTraversability(PluginBase):
    def __init__(self, cell_n: int = 100, layers: list = ("traversability",), thresholds: list = (0.5,), type: list = ("traversability",), **kwargs):
        super().__init__()
        self.layers = list(layers)
        self.thresholds = np.asarray(thresholds, np.float64)
        self.type = list(type)

    def __call__(self, elevation_map, layer_names: List[str], plugin_layers, plugin_layer_names: List[str], semantic_map,
                 semantic_layer_names: List[str], *args):
        votes = np.zeros(np.asarray(elevation_map[2]).shape, np.float32)
        for it, name in enumerate(self.layers):
            if name in layer_names:
                layer = np.asarray(elevation_map[list(layer_names).index(name)])
            elif name in plugin_layer_names:
                layer = np.asarray(plugin_layers[list(plugin_layer_names).index(name)])
            else:
                print("Layer {} is not in the map, returning traversabiltiy!".format(name))
                return None
            hit = layer <= self.thresholds[it] if self.type[it] == "traversability" else layer >= self.thresholds[it]
            votes += hit
        return np.where(votes <= 0.9, 0.1, 1.0)

    def device_op(self, layer_names, plugin_layer_names, semantic_layer_names):
        """``EMAP_PLUGIN_SEMANTIC_TRAV``: the votes on the device; the thresholds travel as the float64 the host compares with.  Declined
        (host route): a layer that is neither a map layer nor a plugin layer (the host route prints and leaves the layer as it is), no
        layer at all, fewer thresholds or types than layers (the host route raises)."""
        from .._lib import PLUGIN_SRC_AT_MOST
        if not self.layers or len(self.thresholds) < len(self.layers) or len(self.type) < len(self.layers):
            return None
        srcs = []
        for it, name in enumerate(self.layers):
            q = self.source_entry(name, layer_names, plugin_layer_names, (), flags=PLUGIN_SRC_AT_MOST if self.type[it] == "traversability" else 0,
                                  d0=float(self.thresholds[it]))
            if q is None:
                return None
            srcs.append(q)
        return dict(type="semantic_trav", srcs=srcs, flags=0)

    def plugin_inputs(self, plugin_layer_names):
        return [n for n in self.layers if n in plugin_layer_names]
