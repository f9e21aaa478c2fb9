"""``PluginBase`` / ``PluginParams`` / ``PluginManager`` -- the reference's plugin surface
(reference EM/plugins/plugin_manager.py:15-260): YAML keys ``enable, fill_nan, is_height_layer, layer_name,
extra_params[, type]``, discovery = first ``PluginBase`` subclass of module ``plugins.<type>``, call arity dispatch
(5/7/8/9 parameters).  Arrays are NumPy (host copies of device layers); the manager injects ``emap`` (the owning
``ElevationMap``) into plugins that accept it so that they can run their arithmetic on the device.

Resident planes.  A plugin may also describe itself as an op of ``emap_plugin_chain`` (``PluginBase.device_op``: MinFilter, MaxFilter,
SmoothFilter, Erosion, RobotCentricElevation, Inpainting with ``method="telea_fronts"``, and the semantic plugins SemanticFilter,
SemanticTraversability, MaxLayerFilter and FeaturesPca, which read a list of sources -- map layers, plugin planes and semantic layers -- from the
side table of ``emap_plugin_chain_ex``): its output then stays in
a plane the context owns, next plugins and the GridMap launch read it there, and nothing crosses PCIe (``ElevationMap.get_grid_map_layers``).
``PluginManager`` keeps the host array and the planes coherent: per layer it knows which side is newer, downloads a device-newer plane
before the host looks at it (``layers``, ``get_map_with_name``; before a host plugin only the layers its ``plugin_inputs`` names) and
uploads a host-newer layer before a device op reads it."""
from __future__ import annotations

import importlib
import sys
import inspect
from abc import ABC
from dataclasses import dataclass
from inspect import signature
from typing import Dict, List, Optional

import ctypes as ct

import numpy as np
import yaml

from .._lib import (PLUGIN_MAX_OPS, PLUGIN_MAX_PLANES, PLUGIN_OPS, PLUGIN_OPS_EX, PLUGIN_REVERSE, PLUGIN_SRC_LAYER, PLUGIN_SRC_LIMITS, PLUGIN_SRC_PLANE, PLUGIN_SRC_SEMANTIC,
                    PLUGIN_THRESHOLD, EmapPluginOp, EmapPluginSrc, f32p)


@dataclass
class PluginParams:
    name: str
    layer_name: str
    fill_nan: bool = False        # fill nan to invalid region
    is_height_layer: bool = False  # if this is a height layer


class PluginBase(ABC):
    def __init__(self, *args, **kwargs):
        pass

    def __call__(self, elevation_map, layer_names, plugin_layers, plugin_layer_names, semantic_map, semantic_layer_names,
                 *args, **kwargs):
        """layers of elevation_map: 0 elevation, 1 variance, 2 is_valid, 3 traversability, 4 time, 5 upper_bound,
        6 is_upper_bound; return a (cell_n, cell_n) array."""
        pass

    def device_op(self, layer_names, plugin_layer_names, semantic_layer_names):
        """This plugin as an op of ``emap_plugin_chain`` (include/emap_hip.h), or ``None`` when this configuration cannot run on resident
        planes: ``dict(type=<key of _lib.PLUGIN_OPS>, src=None | ("layer", i) | ("plane", k), i0=0, i1=0, flags=0, f0=0.0)`` with ``i`` the
        index in ``layer_names`` and ``k`` the index in ``plugin_layer_names``.  An op that reads several layers (``emap_plugin_chain_ex``)
        returns ``dict(type=<key of _lib.PLUGIN_OPS_EX>, srcs=[<source_entry>, ...], flags=0)`` instead: its sources in the order the plugin stacks them.  The op must
        leave, bit for bit, what ``__call__`` returns."""
        return None

    def plugin_inputs(self, plugin_layer_names):
        """names of the plugin layers ``__call__`` reads; ``None``: unknown, i.e. all of them"""
        return None

    @staticmethod
    def device_source(name, layer_names, plugin_layer_names):
        """``src`` of ``device_op`` for the input layer ``name``: a RAW map layer or a plugin layer; ``None`` for anything else (a semantic
        layer is not a device source)"""
        if name in layer_names:
            return ("layer", layer_names.index(name)) if layer_names.index(name) <= 6 else None
        if name in plugin_layer_names:
            return ("plane", plugin_layer_names.index(name))
        return None

    @staticmethod
    def source_entry(name, layer_names, plugin_layer_names, semantic_layer_names, flags=0, f0=0.0, f1=0.0, d0=0.0):
        """One entry of the side table of ``emap_plugin_chain_ex`` for the input layer ``name``, looked up like ``get_layer_data`` does (map
        layers, then plugin layers, then semantic layers): ``dict(kind=PLUGIN_SRC_LAYER | _PLANE | _SEMANTIC, index=, flags=, f0=, f1=,
        d0=)``, or ``None`` for a name that exists nowhere or a map layer beyond the 7 RAW ones."""
        if name in layer_names:
            kind, index = PLUGIN_SRC_LAYER, list(layer_names).index(name)
            if index > 6:
                return None
        elif name in plugin_layer_names:
            kind, index = PLUGIN_SRC_PLANE, list(plugin_layer_names).index(name)
        elif name in semantic_layer_names:
            kind, index = PLUGIN_SRC_SEMANTIC, list(semantic_layer_names).index(name)
        else:
            return None
        return dict(kind=kind, index=int(index), flags=int(flags), f0=float(f0), f1=float(f1), d0=float(d0))

    def get_layer_data(self, elevation_map, layer_names, plugin_layers, plugin_layer_names, semantic_map,
                       semantic_layer_names, name: str) -> Optional[np.ndarray]:
        if name in layer_names:
            return elevation_map[layer_names.index(name)].copy()
        if name in plugin_layer_names:
            return plugin_layers[plugin_layer_names.index(name)].copy()
        if name in semantic_layer_names:
            return semantic_map[semantic_layer_names.index(name)].copy()
        print(f"Could not find layer {name}!")
        return None


def plugin_chain_plan(names, plugins, plugin_layer_names, layer_names, semantic_layer_names=(), resident=True):
    """How the plugin layers ``names`` (in this order) are computed; needs no context.  ``plugins[k]`` is the plugin behind
    ``plugin_layer_names[k]``.  Returns a list of steps in the order of ``names``: ``("device", name, op)`` -- ``op`` a dict with the fields of
    ``struct emap_plugin_op`` (``type, dst_plane, src_kind, src_index, i0, i1, flags, f0``; plane k = plugin layer k) -- or ``("host", name)``
    for a plugin without ``device_op``, a configuration its ``device_op`` declines (``None``), an op that would read its own plane, a layer
    beyond the 32 planes (``PLUGIN_MAX_PLANES``), or everything with ``resident=False``.  Names that are no plugin layer are left out.

    An op with ``srcs`` (the semantic plugins) also carries ``srcs``, its run of the side table of ``emap_plugin_chain_ex`` as a list of
    ``dict(kind, index, flags, f0, f1, d0)``; the runs of the plan's device steps lie one behind the other: ``src_index`` is the first entry of
    the op's run in that table and ``i0`` its length (``side_table(steps)`` is the table; a chain that holds only some of the ops re-bases
    the runs, ``PluginManager._enqueue``).  Such an op goes to the host when it has more or fewer sources than its type takes
    (``PLUGIN_SRC_LIMITS``), when a source is its own plane or a plane beyond the 32, or when an entry is malformed."""
    plugin_layer_names, layer_names, semantic_layer_names = list(plugin_layer_names), list(layer_names), list(semantic_layer_names)
    steps, table_len = [], 0
    for n in names:
        if n not in plugin_layer_names:
            continue
        k = plugin_layer_names.index(n)
        d = None
        if resident and k < PLUGIN_MAX_PLANES and k < len(plugins):
            d = plugins[k].device_op(layer_names, plugin_layer_names, semantic_layer_names)
        if d is not None:
            src = d.get("src")
            if src is not None and (src[0] not in ("layer", "plane") or (src[0] == "plane" and (src[1] == k or src[1] >= PLUGIN_MAX_PLANES))):
                d = None
        if d is not None and "srcs" in d:
            t = PLUGIN_OPS_EX[d["type"]]
            srcs = [dict(kind=int(q["kind"]), index=int(q["index"]), flags=int(q.get("flags", 0)), f0=float(q.get("f0", 0.0)), f1=float(q.get("f1", 0.0)),
                         d0=float(q.get("d0", 0.0))) for q in d["srcs"]]
            lo, hi = PLUGIN_SRC_LIMITS.get(t, (0, -1))
            bad = not lo <= len(srcs) <= hi
            for q in srcs:
                bad = bad or q["kind"] not in (PLUGIN_SRC_LAYER, PLUGIN_SRC_PLANE, PLUGIN_SRC_SEMANTIC) or q["index"] < 0 \
                    or (q["kind"] == PLUGIN_SRC_LAYER and q["index"] > 6) or (q["kind"] == PLUGIN_SRC_SEMANTIC and q["index"] >= len(semantic_layer_names)) \
                    or (q["kind"] == PLUGIN_SRC_PLANE and (q["index"] == k or q["index"] >= min(PLUGIN_MAX_PLANES, len(plugin_layer_names))))
            if not bad:
                steps.append(("device", n, dict(type=t, dst_plane=k, src_kind=PLUGIN_SRC_LAYER, src_index=table_len, i0=len(srcs), i1=0,
                                                flags=int(d.get("flags", 0)), f0=0.0, srcs=srcs)))
                table_len += len(srcs)
                continue
            d = None
        if d is None:
            steps.append(("host", n))
            continue
        src = d.get("src")
        steps.append(("device", n, dict(type=PLUGIN_OPS[d["type"]], dst_plane=k,
                                        src_kind=PLUGIN_SRC_PLANE if src is not None and src[0] == "plane" else PLUGIN_SRC_LAYER,
                                        src_index=int(src[1]) if src is not None else 0, i0=int(d.get("i0", 0)), i1=int(d.get("i1", 0)),
                                        flags=int(d.get("flags", 0)), f0=float(d.get("f0", 0.0)))))
    return steps


def side_table(steps):
    """the side table of sources of a plan's device steps, in step order (``src_index`` / ``i0`` of the ops point into it)"""
    return [q for st in steps if st[0] == "device" for q in st[2].get("srcs", ())]


def op_source_planes(op):
    """the resident planes an op reads"""
    if "srcs" in op:
        return [q["index"] for q in op["srcs"] if q["kind"] == PLUGIN_SRC_PLANE]
    return [op["src_index"]] if op["src_kind"] == PLUGIN_SRC_PLANE else []


class PluginManager(object):
    def __init__(self, cell_n: int, emap=None, package: str = "elevation_mapping_cupy_amd.plugins"):
        self.cell_n = cell_n
        self.emap = emap
        self.package = package
        self.plugin_params: List[PluginParams] = []
        self.plugins = []
        self._reserved = 0                 # resident planes the context holds (emap_plugin_planes)
        self.layers = np.zeros((0, cell_n, cell_n), np.float32)
        self.layer_names: List[str] = []
        self.plugin_names: List[str] = []

    # ---- the host array and the resident planes ---------------------------------------------------------------------------------------
    # _newer[k]: "host" (the host array holds what the plane does not), "device" (the other way round) or None (the same on both sides)
    @property
    def layers(self):
        """``(n_plugins, cell_n, cell_n)`` float32 on the host.  Planes that are newer on the device are downloaded first, and every plane
        counts as newer on the host afterwards: the caller may write into the array in place, as into the reference's, and the next
        device op that reads a layer uploads it.  (``host_layer`` and ``get_param_with_name`` are the read-only ways.)  The property
        talks to the device: outside ``ElevationMap``'s own methods, hold its ``map_lock`` around it like around any other map access."""
        self._download(range(len(self._newer)))
        self._newer = ["host"] * len(self._newer)
        return self._host

    @layers.setter
    def layers(self, value):
        self._host = value
        # planes the context has never held start as zero there, as this array does in init(); anything else has to be uploaded before use
        fresh = self._reserved == 0 and not np.any(value)
        self._newer = [None if fresh else "host"] * len(value)

    def _call(self, fn, *args):
        self.emap._chk(getattr(self.emap._lib, fn)(self.emap._ctx, *args))

    def _reserve(self):
        n = min(len(self._newer), PLUGIN_MAX_PLANES)
        if n > self._reserved:
            self._call("emap_plugin_planes", n)
            self._reserved = n

    def _download(self, indices):
        for k in indices:
            if self._newer[k] == "device":
                self._call("emap_plugin_plane_read", k, f32p(self._host[k]))
                self._newer[k] = None

    def _upload(self, k):
        if self._newer[k] == "host":
            self._reserve()
            self._staged = np.ascontiguousarray(self._host[k], np.float32)      # (kept until the next upload: never a temporary behind the call)
            self._call("emap_plugin_plane_write", k, f32p(self._staged))
            self._newer[k] = None

    def host_layer(self, name):
        """the host array of ONE layer, to READ (only this plane is downloaded if the device holds the newer one; a write into it is not
        tracked: write through ``layers``)"""
        idx = self.get_layer_index_with_name(name)
        if idx is None:
            return None
        self._download([idx])
        return self._host[idx]

    def _enqueue(self, ops, rotation):
        """one ``emap_plugin_chain`` call -- ``emap_plugin_chain_ex`` when an op brings sources: their runs are laid one behind the other into
        the chain's own side table -- (no wait); the planes it writes are then newer on the device"""
        self._reserve()
        table = (EmapPluginOp * len(ops))()
        srcs = []
        for t, op in zip(table, ops):
            for f, _ in EmapPluginOp._fields_:
                setattr(t, f, op[f])
            if "srcs" in op:
                t.src_index, t.i0 = len(srcs), len(op["srcs"])
                srcs += op["srcs"]
        R = np.ascontiguousarray(np.asarray(rotation if rotation is not None else np.eye(3), np.float32).reshape(-1))
        if any("srcs" in op for op in ops):
            side = (EmapPluginSrc * max(1, len(srcs)))()
            for t, q in zip(side, srcs):
                t.kind, t.index, t.flags, t.reserved, t.f0, t.f1, t.d0 = q["kind"], q["index"], q["flags"], 0, q["f0"], q["f1"], q["d0"]
            self._call("emap_plugin_chain_ex", table, len(ops), f32p(R), side, len(srcs))
        else:
            self._call("emap_plugin_chain", table, len(ops), f32p(R))
        for op in ops:
            self._newer[op["dst_plane"]] = "device"
            p = self.plugins[op["dst_plane"]]
            if hasattr(p, "sweeps_run"):
                p.sweeps_run = None            # nothing waited for the sweeps' counters (MinFilter / MaxFilter on the device route)
            if hasattr(p, "fronts_run"):
                p.fronts_run = None            # nor for the largest front (Inpainting with method "telea_fronts")

    def run_plan(self, steps, host_step, rotation=None):
        """Run the steps of ``plugin_chain_plan`` in order.  Device ops gather in one chain that is enqueued as late as their order allows:
        at the end, before a host plugin that reads (``plugin_inputs``) a plane the chain writes, before an upload a later op needs, or
        when it holds 32 ops (``PLUGIN_MAX_OPS``).  Every plane an op reads -- each plane source of a semantic op -- that is newer on the host goes
        up first, unless an op waiting in the chain writes it.  ``host_step(name)`` runs a host plugin (``update_with_name``).  Returns
        ``{name: "device" | "host"}``."""
        route, pending = {}, []

        def flush():
            if pending:
                self._enqueue(pending, rotation)
                del pending[:]

        for step in steps:
            name = step[1]
            if step[0] == "device":
                op = step[2]
                stale = [p for p in op_source_planes(op) if self._newer[p] == "host" and p not in [q["dst_plane"] for q in pending]]
                if stale:
                    flush()                    # (an op waiting in the chain may read the planes as they are now)
                    for p in sorted(set(stale)):
                        self._upload(p)
                if len(pending) == PLUGIN_MAX_OPS:
                    flush()
                pending.append(op)
                route[name] = "device"
            else:
                inputs = self.plugins[self.layer_names.index(name)].plugin_inputs(self.layer_names)
                written = [self.layer_names[q["dst_plane"]] for q in pending]
                if inputs is None or any(n in written for n in inputs):
                    flush()
                host_step(name)
                route[name] = "host"
        flush()
        return route

    def init(self, plugin_params: List[PluginParams], extra_params: List[Dict]):
        self.plugins = []
        kept = []
        for param, extra_param in zip(plugin_params, extra_params):
            try:
                m = importlib.import_module("." + param.name, package=self.package)
            except ImportError as ex:     # a configured plugin without an implementation here must not take the others down
                print("[WARNING] plugin {} is not available on this backend ({}); layer {} skipped".format(param.name, ex, param.layer_name),
                      file=sys.stderr)
                continue
            kept.append(param)
            for name, obj in inspect.getmembers(m):
                if inspect.isclass(obj) and issubclass(obj, PluginBase) and name != "PluginBase":
                    extra_param = dict(extra_param or {})
                    extra_param["cell_n"] = self.cell_n
                    if "emap" in signature(obj.__init__).parameters:
                        extra_param["emap"] = self.emap
                    self.plugins.append(obj(**extra_param))
        self.plugin_params = kept
        self.layers = np.zeros((len(self.plugins), self.cell_n, self.cell_n), dtype=np.float32)
        self.layer_names = [p.layer_name for p in self.plugin_params]
        self.plugin_names = [p.name for p in self.plugin_params]

    def load_plugin_settings(self, file_path: str):
        print("Start loading plugins...")
        with open(file_path, "r") as f:
            cfg = yaml.safe_load(f) or {}
        plugin_params, extra_params = [], []
        for k, v in cfg.items():
            if v["enable"]:
                plugin_params.append(PluginParams(name=k if "type" not in v else v["type"], layer_name=v["layer_name"],
                                                  fill_nan=v["fill_nan"], is_height_layer=v["is_height_layer"]))
                extra_params.append(v.get("extra_params", {}))
        self.init(plugin_params, extra_params)
        print("Loaded plugins are ", *self.plugin_names)

    def get_layer_names(self):
        return [p.layer_name for p in self.plugin_params]

    def get_plugin_names(self):
        return [p.name for p in self.plugin_params]

    def get_plugin_index_with_name(self, name: str):
        return self.plugin_names.index(name) if name in self.plugin_names else None

    def get_layer_index_with_name(self, name: str):
        return self.layer_names.index(name) if name in self.layer_names else None

    def update_with_name(self, name, elevation_map, layer_names, semantic_map=None, semantic_params=None, rotation=None,
                         elements_to_shift={}):
        idx = self.get_layer_index_with_name(name)
        if idx is None or idx >= len(self.plugins):
            return
        plugin = self.plugins[idx]
        n_param = len(signature(plugin).parameters)        # arity dispatch of the reference (:199-225)
        inputs = plugin.plugin_inputs(self.layer_names)    # the host plugin reads the host array: fetch what it reads and the device holds newer
        self._download(range(len(self._newer)) if inputs is None else [self.layer_names.index(n) for n in inputs if n in self.layer_names])
        args = [elevation_map, layer_names, self._host, self.layer_names]
        if n_param == 5:
            pass
        elif n_param == 7:
            args += [semantic_map, semantic_params]
        elif n_param == 8:
            args += [semantic_map, semantic_params, rotation]
        else:
            args += [semantic_map, semantic_params, rotation, elements_to_shift]
        out = plugin(*args)
        if out is None:                    # (semantic_traversability without its input layer: the reference prints and returns nothing)
            return
        self._host[idx] = np.asarray(out, np.float32)
        self._newer[idx] = "host"

    def get_map_with_name(self, name: str):
        """the layer on the host (all device-newer planes come back first); to read -- in-place writes go through ``layers``"""
        idx = self.get_layer_index_with_name(name)
        if idx is None:
            return None
        self._download(range(len(self._newer)))
        return self._host[idx]

    def get_param_with_name(self, name: str):
        idx = self.get_layer_index_with_name(name)
        return None if idx is None else self.plugin_params[idx]
