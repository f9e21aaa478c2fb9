"""``ElevationMap`` -- host-side mirror of the reference's map object for the point-cloud hot path.

Same method names / argument meaning as the reference class (reference EM/elevation_mapping.py:49-922) so the
ROS wrapper (src/elevation_mapping_wrapper.cpp:173-252) and the reference's tests drive it unchanged; the map
itself lives in HBM inside ``libemap_hip.so`` (C ABI ``include/emap_hip.h``).  NumPy is used for host arrays only;
there is no CuPy, no PyTorch and no CPU compute fallback here.
"""
from __future__ import annotations

import contextlib
import ctypes as ct
import os
import threading
import types
from typing import List

import numpy as np

from . import _lib
from ._lib import (CLOUD_HIDDEN, CLOUD_INDEX, CLOUD_NORMAL_MIN, CLOUD_POINT, CLOUD_TEST, EmapCloudField, EmapCloudMsgDesc, EmapDepthDesc, EmapError, EmapGridLayer, EmapGridLayerEx, EmapGridWindow, EmapPolygonVerdict, EmapImageMsgDesc, EmapImageSpec, EmapParams, EmapStats, EmapStrip,
                   GRID_ADD_Z, GRID_BUILTIN, GRID_FILL_NAN, GRID_MAX_LAYERS, GRID_MAX_WINDOWS, GRID_NORMAL_COLOR, GRID_ORDERS, GRID_PLUGIN, GRID_SEMANTIC, PLANES, POLY_MAP_LAYER, POLY_MAX_BATCH, POLY_MAX_VERTS, POLY_PLUGIN, POLY_SEMANTIC, f32p)
from .parameter import Parameter
from .plugins.plugin_manager import plugin_chain_plan


def _shoelace_area(xy):
    """area of a simple polygon (n, 2)"""
    x, y = np.asarray(xy, np.float64).T
    return 0.5 * abs(float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))))


def _hull_ring(cells):
    """closed counter-clockwise hull ring (k + 1, 2) around integer cells (n, 2), or None when they do not span an area.  The
    reference asks shapely for ``MultiPoint(...).convex_hull`` (absent here); scipy's Qhull yields the same vertex set."""
    if cells.shape[0] < 3:
        return None
    from scipy.spatial import ConvexHull, QhullError
    pts = cells.astype(np.float64)
    try:
        v = ConvexHull(pts).vertices
    except QhullError:              # collinear cells
        return None
    return np.vstack([pts[v], pts[v[:1]]])


def _field(f):
    """(name, offset, datatype, count) of a sensor_msgs/PointField-like object or of such a tuple"""
    if isinstance(f, (tuple, list)):
        name, offset, datatype, count = f
    else:
        name, offset, datatype, count = f.name, f.offset, f.datatype, f.count
    return str(name), int(offset), int(datatype), int(count)


def pointcloud2_descriptor(fields, width, height, point_step, row_step=None, is_bigendian=False, channels=None, typed=False):
    """``(EmapCloudMsgDesc, names)`` of a PointCloud2 layout for ``emap_bind_cloud_message`` (include/emap_hip.h); needs no context.

    ``fields``: sensor_msgs/PointField-like objects or ``(name, offset, datatype, count)`` tuples.  ``channels=None``: every field in
    message order becomes a column and the first three are x, y, z whatever they are called (the node's rule,
    elevation_mapping_ros.cpp:309-313, 333-337); ``channels`` given: the fields named x, y, z and then the named ones.  ``typed=False``:
    every column is the node's 4-byte memcpy (conv 0); ``typed=True``: converted from the field's datatype, except FLOAT32 fields and
    the packed colours ``rgb`` / ``rgba``, which are moved.  ``names``: the columns' names."""
    fs = [_field(f) for f in fields]
    if channels is None:
        cols = fs
    else:
        by_name = {}
        for f in fs:
            by_name.setdefault(f[0], f)
        missing = [n for n in ["x", "y", "z"] + list(channels) if n not in by_name]
        if missing:
            raise ValueError("the message has no field named %s" % ", ".join(map(repr, missing)))
        cols = [by_name[n] for n in ["x", "y", "z"] + list(channels)]
    if not 3 <= len(cols) <= 19:
        raise ValueError("a cloud has x, y, z and at most 16 channels; %d columns selected" % len(cols))
    for name, _, _, count in cols:
        if count != 1:
            raise ValueError("field %r has count %d; only fields of one element can become a column" % (name, count))
    if point_step is None:
        raise ValueError("point_step is required")
    d = EmapCloudMsgDesc()
    d.height, d.width, d.point_step = int(height), int(width), int(point_step)
    d.row_step = int(width) * int(point_step) if row_step is None else int(row_step)
    d.is_bigendian, d.n_cols = int(bool(is_bigendian)), len(cols)
    for c, (name, offset, datatype, _) in enumerate(cols):
        d.offset[c] = offset
        d.conv[c] = datatype if typed and datatype != 7 and name not in ("rgb", "rgba") else 0
    return d, [c[0] for c in cols]


IMAGE_ELEMS = ("8U", "8S", "16U", "16S", "32S", "32F", "64F")      # the OpenCV depth codes 0 .. 6 (emap_image_msg_desc.elem)
IMAGE_ELEM_SIZE = (1, 1, 2, 2, 4, 4, 8)
_NAMED_ENCODINGS = {      # sensor_msgs/image_encodings.h: (element, channels, R <-> B swap -- the node's cvtColor, bgr8 / bgra8 ONLY)
    "mono8": ("8U", 1, False), "mono16": ("16U", 1, False),
    "rgb8": ("8U", 3, False), "rgba8": ("8U", 4, False), "bgr8": ("8U", 3, True), "bgra8": ("8U", 4, True),
    "rgb16": ("16U", 3, False), "rgba16": ("16U", 4, False), "bgr16": ("16U", 3, False), "bgra16": ("16U", 4, False),
}
IMAGE_MAX_SIDE = 8192             # EM_IMGMSG_MAX_SIDE (csrc/emap_launch.h)
IMAGE_MAX_INDEX = 1 << 24         # EM_IMGMSG_MAX_INDEX: H W (x 3 with a colour entry); the reference's float index arithmetic is exact up to here


def image_encoding(encoding):
    """``(elem code, n_chan, swap_rb)`` of a sensor_msgs/Image encoding string: the generic ``8UC1 .. 64FC4`` (a bare ``8UC`` means one
    channel), ``mono8/16`` and the ``rgb / rgba / bgr / bgra`` encodings of 8 and 16 bits.  Only ``bgr8`` / ``bgra8`` are swapped to RGB,
    as the node does (elevation_mapping_ros.cpp:382-386); ``bgr16`` / ``bgra16`` pass as they are.  Anything else (bayer, yuv, unknown
    strings) raises ``ValueError``."""
    enc = str(encoding)
    if enc in _NAMED_ENCODINGS:
        e, n, swap = _NAMED_ENCODINGS[enc]
        return IMAGE_ELEMS.index(e), n, swap
    for code, e in enumerate(IMAGE_ELEMS):
        if enc.startswith(e + "C") and enc[len(e) + 1:] in ("", "1", "2", "3", "4"):
            return code, int(enc[len(e) + 1:] or 1), False
    raise ValueError("image encoding %r is not supported (8UC1 .. 64FC4, mono8/16, rgb/rgba/bgr/bgra 8/16)" % (encoding,))


def image_message_descriptor(encoding, height, width, step=None, is_bigendian=False):
    """``EmapImageMsgDesc`` of a sensor_msgs/Image layout for ``emap_input_image_message`` (include/emap_hip.h); needs no context.
    ``step=None``: tight rows.  Raises ``ValueError`` for everything the entry point would refuse that can be seen here."""
    elem, n_chan, swap = image_encoding(encoding)
    height, width = int(height), int(width)
    if not (1 <= height <= IMAGE_MAX_SIDE and 1 <= width <= IMAGE_MAX_SIDE):
        raise ValueError("image sides must lie in 1 .. %d (%d x %d)" % (IMAGE_MAX_SIDE, height, width))
    tight = width * n_chan * IMAGE_ELEM_SIZE[elem]
    step = tight if step is None else int(step)
    if step < tight:
        raise ValueError("step %d is smaller than width * channels * element size = %d" % (step, tight))
    if height * step >= 1 << 31:
        raise ValueError("height * step must stay below 2^31 bytes")
    if height * width > IMAGE_MAX_INDEX:
        raise ValueError("height * width beyond 2^24 pixels: use input_image")
    d = EmapImageMsgDesc()
    d.height, d.width, d.step, d.elem, d.n_chan = height, width, step, elem, n_chan
    d.is_bigendian, d.swap_rb = int(bool(is_bigendian)), int(swap)
    return d


GRID_BUILTIN_LAYERS = ("elevation", "variance", "traversability", "time", "upper_bound", "is_upper_bound", "normal_x", "normal_y", "normal_z")      # emap_publish_layer's kinds 0 .. 8
GRID_NORMAL_COLOR_LAYERS = ("normal_x", "normal_y", "normal_z", "color")      # what the wrapper appends with enable_normal_color (elevation_mapping_wrapper.cpp:239-251)


def _basic_layers(layers, basic_layers):
    """the wrapper's rule for ``basic_layers=None``: ``["elevation"]`` if it was asked for"""
    if basic_layers is None:
        return ["elevation"] if "elevation" in layers else []
    return list(basic_layers)


def _grid_map_envelope(names, flat, ni, nj, position, lengths, resolution, basic_layers, header, **extra):
    """the duck-typed ``grid_map_msgs/GridMap`` around ``flat`` (``(len(names), ni * nj)``, column-major planes of ``ni x nj`` cells): the header
    both as ``msg.header`` and ``msg.info.header``, the pose at ``position`` with the identity orientation, one ``Float32MultiArray`` per layer
    whose ``data`` is a view of its row of ``flat``; ``extra``: fields only some doors add (``index_in_submap``)"""
    ns = types.SimpleNamespace
    pose = ns(position=ns(x=position[0], y=position[1], z=0.0), orientation=ns(x=0.0, y=0.0, z=0.0, w=1.0))
    info = ns(header=header, resolution=resolution, length_x=lengths[0], length_y=lengths[1], pose=pose)
    data = [ns(layout=ns(dim=[ns(label="column_index", size=nj, stride=ni * nj), ns(label="row_index", size=ni, stride=ni)], data_offset=0),
               data=flat[k]) for k in range(len(names))]
    return ns(header=header, info=info, layers=names, basic_layers=list(basic_layers), data=data, outer_start_index=0, inner_start_index=0, **extra)


def grid_map_descriptor(layers, semantic_layers=(), normal_color=False, slots=None):
    """``(table, names)`` of a GridMap publisher's layer list for ``emap_publish_grid_map`` (include/emap_hip.h); needs no context.

    ``layers``: names of device-resident layers in message order -- the nine built-ins (``GRID_BUILTIN_LAYERS``) and the names in
    ``semantic_layers`` (position = the semantic layer's index).  ``normal_color``: ``normal_x``, ``normal_y``, ``normal_z`` and ``color`` are
    appended as the wrapper appends them (a name already in the list is not added twice); only then is ``color`` a known name, and the
    four names then mean the normal planes and their colour whatever else carries those names.  ``slots``: the plane of the output each
    layer lands in (default: its position).  ``table``: an ``EmapGridLayer`` array.  Raises ``ValueError`` for what the entry point would
    refuse that can be seen here: no layer, more than 32, an unknown name, a name or a slot given twice, a negative slot, a slot list of
    another length."""
    names = [str(n) for n in layers]
    if len(set(names)) != len(names):
        raise ValueError("a layer is named twice: %s" % ", ".join(sorted(n for n in set(names) if names.count(n) > 1)))
    if normal_color:
        names += [n for n in GRID_NORMAL_COLOR_LAYERS if n not in names]
    if not names:
        raise ValueError("no layer asked for")
    if len(names) > GRID_MAX_LAYERS:
        raise ValueError("at most %d layers per launch (%d asked for)" % (GRID_MAX_LAYERS, len(names)))
    slots = list(range(len(names))) if slots is None else [int(x) for x in slots]
    if len(slots) != len(names):
        raise ValueError("%d slots for %d layers" % (len(slots), len(names)))
    if any(x < 0 for x in slots):
        raise ValueError("a slot is negative")
    if len(set(slots)) != len(slots):
        raise ValueError("a slot is named twice")
    semantic_layers = list(semantic_layers)
    table = (EmapGridLayer * len(names))()
    for g, n, slot in zip(table, names, slots):
        if normal_color and n == "color":
            g.kind, g.index = GRID_NORMAL_COLOR, 0
        elif n in GRID_BUILTIN_LAYERS and (n not in semantic_layers or (normal_color and n in GRID_NORMAL_COLOR_LAYERS)):
            g.kind, g.index = GRID_BUILTIN, GRID_BUILTIN_LAYERS.index(n)
        elif n in semantic_layers:
            g.kind, g.index = GRID_SEMANTIC, semantic_layers.index(n)
        else:
            raise ValueError("layer %r is neither a built-in nor one of the semantic layers %s" % (n, semantic_layers))
        g.slot = slot
    return table, names


_SUBMAP_EPS = 10.0 * float(np.finfo(np.float64).eps)      # grid_map_core: 10 * numeric_limits<double>::epsilon()


def submap_geometry(map_position_xy, map_length, resolution, M, position_xy, length_xy):
    """The window of the published index space that a ``get_submap`` request covers (elevation_mapping_ros.cpp:507-553: ``GridMap::getSubmap``),
    in double precision, without a context: ``None`` -- the node's ``isSuccess == false`` -- or ``(i0, j0, ni, nj, submap_position_xy,
    submap_length_xy, index_in_submap)``.

    The map is ``M x M`` cells of ``resolution`` around ``map_position_xy`` with sides ``map_length``; the request is centred at
    ``position_xy`` with sides ``length_xy``, all in the map frame.  Indices are those of element ``(i, j)`` of what
    ``get_map_with_name_ref`` leaves (``M = cell_n - 2``): grid_map's index space with both start indices 0, which holds for the node's map
    because ``get_grid_map`` calls ``setGeometry`` on every tick.  The request is clipped to the map; ``index_in_submap`` is the cell of
    the requested position inside the window.

    grid_map is not available offline: this is a RESTATEMENT of grid_map_core's ``getSubmapInformation`` (``boundPositionToRange``,
    ``getIndexFromPosition``), not pinned by a compiled reference.  The double arithmetic is fragile exactly on cell edges, as there: a
    request whose corner falls on an edge may lose or gain a cell or come back ``None``, so callers and tests keep corners inside cells
    (what the statement gives on edges is recorded in tests/_submap_cases.py, not asserted as grid_map's behaviour).  ``ValueError``: a
    component that is not finite, a negative length, a window size below 1."""
    mp = [float(v) for v in map_position_xy]
    pos = [float(v) for v in position_xy]
    ln = [float(v) for v in length_xy]
    L, res, M = float(map_length), float(resolution), int(M)
    if len(mp) != 2 or len(pos) != 2 or len(ln) != 2:
        raise ValueError("positions and lengths have two components")
    if not all(np.isfinite(v) for v in mp + pos + ln + [L, res]):
        raise ValueError("submap request: a component is not finite")
    if ln[0] < 0.0 or ln[1] < 0.0:
        raise ValueError("submap request: a length is negative")
    if not (L > 0.0 and res > 0.0 and M >= 1):
        raise ValueError("the map needs a positive length, a positive resolution and at least one cell")

    def bound(p):
        out = []
        for a in (0, 1):
            s = p[a] - mp[a] + L / 2.0
            eps = _SUBMAP_EPS * (abs(s) if abs(s) > 1.0 else 1.0)
            if s <= 0.0:
                s = eps
            elif s >= L:
                s = L - eps
            out.append(s + mp[a] - L / 2.0)
        return out

    def index_of(p, length, centre, size):
        idx = []
        for a in (0, 1):
            t = -(p[a] - centre[a] - length[a] / 2.0)
            i = int(-(p[a] - length[a] / 2.0 - centre[a]) / res)      # truncating, like the C++ cast
            if not (0.0 <= t < length[a]) or not (0 <= i < size[a]):
                return None
            idx.append(i)
        return idx

    top_left = index_of(bound([pos[0] + ln[0] / 2.0, pos[1] + ln[1] / 2.0]), (L, L), mp, (M, M))
    bottom_right = index_of(bound([pos[0] - ln[0] / 2.0, pos[1] - ln[1] / 2.0]), (L, L), mp, (M, M))
    if top_left is None or bottom_right is None:
        return None
    size = [bottom_right[a] - top_left[a] + 1 for a in (0, 1)]
    if size[0] < 1 or size[1] < 1:
        raise ValueError("submap request: window size %r is below 1" % (size,))
    sub_len = [size[a] * res for a in (0, 1)]
    corner = [mp[a] + L / 2.0 - res * top_left[a] for a in (0, 1)]
    sub_pos = [corner[a] - sub_len[a] / 2.0 for a in (0, 1)]
    inside = index_of(pos, sub_len, sub_pos, size)
    if inside is None:
        return None
    return top_left[0], top_left[1], size[0], size[1], (sub_pos[0], sub_pos[1]), (sub_len[0], sub_len[1]), (inside[0], inside[1])


def pack_windows(windows, n_layers):
    """``(offsets, total)`` of the packed output of ``emap_publish_grid_windows``: window ``w`` = ``(i0, j0, ni, nj)`` starts at float
    ``offsets[w] = n_layers * sum(ni * nj of the windows before it)``"""
    offsets, total = [], 0
    for _, _, ni, nj in windows:
        offsets.append(total)
        total += int(n_layers) * int(ni) * int(nj)
    return offsets, total


def grid_cell_positions(center_xy, resolution, M):
    """``(x_of_i, y_of_j)``: the float64 positions of the rows ``i`` and the columns ``j`` of the published index space, as grid_map's
    ``getPositionFromIndex`` gives them for a map of ``M x M`` cells of ``resolution`` around ``center_xy`` with both start indices 0:
    ``x(i) = (p_x + (0.5 * L - 0.5 * resolution)) + resolution * (-i)``, ``L = M * resolution``, and ``y(j)`` likewise -- IEEE double, every
    operation rounded on its own.  The conventions are those of ``submap_geometry``: a caller that speaks for a map hands in the float32
    resolution and the float32 centre widened to double.  grid_map is not available offline: a RESTATEMENT, not pinned by a compiled
    reference.  ``ValueError``: a component that is not finite, a resolution that is not positive, ``M < 1``."""
    p = [float(v) for v in center_xy]
    res, M = float(resolution), int(M)
    if len(p) != 2:
        raise ValueError("the centre has two components")
    if not all(np.isfinite(v) for v in p + [res]):
        raise ValueError("cell positions: a component is not finite")
    if not (res > 0.0 and M >= 1):
        raise ValueError("the map needs a positive resolution and at least one cell")
    L = M * res
    off = 0.5 * L - 0.5 * res
    steps = res * (-np.arange(M, dtype=np.float64))
    return (p[0] + off) + steps, (p[1] + off) + steps


POINT_FIELD_FLOAT32 = 7      # sensor_msgs/PointField.FLOAT32


def point_cloud_descriptor(layers, point_layer):
    """``(fields, point_step)`` of the ``sensor_msgs/PointCloud2`` that ``GridMapRosConverter::toPointCloud(map, layers, point_layer, msg)``
    builds (restated: grid_map is not available offline); needs no context.  Fields follow ``layers``: the point layer gives ``x``, ``y``,
    ``z``, a layer named ``color`` gives ``rgb`` (the float's bits as they are), every other layer a field of its own name; all ``FLOAT32``
    (datatype 7), ``count`` 1, offsets 4 apart; ``point_step = 4 * len(fields)``.  ``fields``: namespaces with ``name, offset, datatype, count``.
    ``ValueError``: no layer, a layer named twice, ``point_layer`` not in ``layers`` (a decision: grid_map would emit a cloud without
    coordinates)."""
    names = [str(n) for n in layers]
    if not names:
        raise ValueError("no layer asked for")
    if len(set(names)) != len(names):
        raise ValueError("a layer is named twice: %s" % ", ".join(sorted(n for n in set(names) if names.count(n) > 1)))
    if point_layer not in names:
        raise ValueError("point_layer %r is not one of the layers %s" % (point_layer, names))
    out = []
    for n in names:
        out += ["x", "y", "z"] if n == point_layer else ["rgb" if n == "color" else n]
    fields = [types.SimpleNamespace(name=n, offset=4 * k, datatype=POINT_FIELD_FLOAT32, count=1) for k, n in enumerate(out)]
    return fields, 4 * len(fields)


def _cloud_compact(planes, emit, point_layer, tested, xs, ys, index=False, normals=None, normal_min=None):
    """The host route of the point-cloud output: ``planes`` = ``{name: (M, M) float32 in message order}`` (its ``ravel()`` is the iterator's
    order); a cell passes if every ``tested`` plane is finite there and, with ``normal_min``, ``not (norm < normal_min)`` in double on the
    three ``normals`` planes.  Returns the ``(n, fields)`` float32 records: ``emit`` in order, ``x, y, z`` for the point layer, ``lin`` as an
    int32 behind them with ``index``.  Values are moved, never computed: NaN bits stay."""
    M = xs.size
    ok = np.ones((M, M), bool)
    for n in tested:
        ok &= np.isfinite(planes[n])
    if normal_min is not None:
        nx, ny, nz = (planes[n].astype(np.float64) for n in normals)
        with np.errstate(invalid="ignore"):
            ok &= ~(np.sqrt((nx * nx + ny * ny) + nz * nz) < normal_min)
    lin = np.flatnonzero(ok.ravel())
    j, i = np.divmod(lin, M)
    cols = []
    for n in emit:
        if n == point_layer:
            cols += [xs[i], ys[j]]
        cols.append(planes[n].ravel()[lin])
    rec = np.empty((lin.size, len(cols) + (1 if index else 0)), np.float32)
    for k, c in enumerate(cols):
        rec.view(np.uint32)[:, k] = np.ascontiguousarray(c, np.float32).view(np.uint32)
    if index:
        rec.view(np.int32)[:, -1] = lin
    return rec


def normal_arrow_markers(arrows, frame_id="", stamp=None):
    """The duck-typed ``visualization_msgs/MarkerArray`` of the node's ``normal`` publisher (elevation_mapping_ros.cpp:751-809,
    ``vectorToArrowMarker``) for what ``ElevationMap.get_normal_arrows`` returns: per arrow ``ns "normal"``, ``id`` = the cell's linear
    index, type ARROW (0), action ADD (0), ``points = [start, end]``, ``scale`` 0.01 three times, colour ``(0, 1, 0, 1)``, orientation
    ``w = 1``.  Built here, off the hot path."""
    ns = types.SimpleNamespace
    header = ns(frame_id=str(frame_id), stamp=stamp, seq=0)
    markers = []
    for k, s, e in zip(arrows.ids.tolist(), arrows.starts.tolist(), arrows.ends.tolist()):
        markers.append(ns(header=header, ns="normal", id=k, type=0, action=0,
                          pose=ns(position=ns(x=0.0, y=0.0, z=0.0), orientation=ns(x=0.0, y=0.0, z=0.0, w=1.0)),
                          scale=ns(x=0.01, y=0.01, z=0.01), color=ns(r=0.0, g=1.0, b=0.0, a=1.0),
                          points=[ns(x=s[0], y=s[1], z=s[2]), ns(x=e[0], y=e[1], z=e[2])]))
    return ns(markers=markers)


CAM_CELL_MAX = 65536      # EM_CAM_CELL_MAX (csrc/emap_launch.h): a cap, not a measurement -- 2.6 km at 4 cm cells, far beyond any map


def camera_cell(center, cell_n, resolution, R, t):
    """``(x1, y1, z1)`` of ``input_image``: the camera's cell (float32, integer valued) and its height above the map centre.

    The reference computes ``np.float32(np.uint32(cell_n / 2 + t_cam_map / resolution))`` (elevation_mapping.py:531-534).  For a camera
    more than half a map width on the low side of the centre that cast wraps to about 2**32, and the occlusion walk, which ends only
    by reaching the camera cell, never ends.  DEPARTURE: the index is a SIGNED integer truncated toward zero -- bit for bit the
    reference's value wherever that one is non-negative, the negative index otherwise (the walk then behaves as it does for a camera
    cell beyond the high side) -- and a pose whose index is not finite or exceeds ``CAM_CELL_MAX`` in magnitude raises ``ValueError``
    instead of being launched."""
    R = np.asarray(R, np.float32); t = np.asarray(t, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):      # a pose that is not finite is refused below, not warned about
        t_cam_map = -R.T @ t - center
    cell = []
    for a in (0, 1):
        v = (cell_n / 2) + (t_cam_map[a] / resolution)
        if not np.isfinite(v):
            raise ValueError("camera pose: cell index along axis %d is not finite (%r)" % (a, v))
        i = int(v)                      # toward zero, like the C cast behind np.uint32(...)
        if abs(i) > CAM_CELL_MAX:
            raise ValueError("camera pose: cell index %d along axis %d is beyond +-%d cells" % (i, a, CAM_CELL_MAX))
        cell.append(np.float32(i))
    if not np.isfinite(t_cam_map[2]):
        raise ValueError("camera pose: height is not finite (%r)" % (t_cam_map[2],))
    return cell[0], cell[1], np.float32(t_cam_map[2])


class LazyPlanes:
    """What a plugin receives as ``elevation_map`` / ``semantic_map``: behaves like the reference's ``(L, rows, C)`` array -- ``shape``,
    ``dtype``, ``ndim``, indexing, iteration, arithmetic, ``copy()`` and every other ndarray attribute work -- but a plane only crosses
    PCIe when the plugin actually touches it (the built-in plugins run on the device and never do).  Integer indexing fetches one
    plane; anything else materialises the stack once and delegates to NumPy."""

    def __init__(self, n, fetch, device_map=None, rows=None, cols=None):
        self._n, self._fetch, self._cache, self._full = int(n), fetch, {}, None
        if rows is None and device_map is not None:
            rows, cols = device_map.rows, device_map.cell_n
        self.shape = (self._n, int(rows or 0), int(cols or 0))
        self.dtype = np.dtype(np.float32)
        self.ndim = 3
        self.device_map = device_map          # the ElevationMap whose live core planes these are (built-in plugins read them on the device)

    def __len__(self):
        return self._n

    def _plane(self, k):
        k = int(k)
        if not -self._n <= k < self._n:
            raise IndexError("layer index %d out of range for %d layers" % (k, self._n))
        k %= self._n
        if k not in self._cache:
            self._cache[k] = self._fetch(k)
        return self._cache[k]

    def __getitem__(self, key):
        if isinstance(key, (int, np.integer)):
            return self._plane(key)
        return np.asarray(self)[key]

    def __iter__(self):
        return (self._plane(k) for k in range(self._n))

    def __array__(self, dtype=None, copy=None):
        if self._full is None:
            self._full = (np.stack([self._plane(k) for k in range(self._n)], axis=0) if self._n
                          else np.zeros(self.shape, np.float32))
        return self._full.astype(dtype) if dtype is not None else self._full

    def __getattr__(self, name):              # copy, sum, mean, astype, T, ...: whatever an ndarray offers
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(np.asarray(self), name)

    __hash__ = None


def _forward_operators():
    """arithmetic and comparisons of a LazyPlanes act on the materialised stack, like the reference's cupy array would"""
    def binary(name):
        return lambda self, other: getattr(np.asarray(self), name)(np.asarray(other) if isinstance(other, LazyPlanes) else other)

    def unary(name):
        return lambda self: getattr(np.asarray(self), name)()
    for o in ("add", "radd", "sub", "rsub", "mul", "rmul", "truediv", "rtruediv", "pow", "lt", "le", "gt", "ge", "eq", "ne"):
        setattr(LazyPlanes, "__%s__" % o, binary("__%s__" % o))
    for o in ("neg", "abs"):
        setattr(LazyPlanes, "__%s__" % o, unary("__%s__" % o))


_forward_operators()


class ElevationMap:
    """Core elevation mapping class (MI355X backend)."""

    layer_names_core = ["elevation", "variance", "is_valid", "traversability", "time", "upper_bound", "is_upper_bound"]

    def __init__(self, param: Parameter, strip=None, stream=None):
        """
        Args:
            param: ``Parameter`` (``update()`` is called if ``cell_n`` is unset).
            strip: optional ``(row_begin, row_count, halo_rows)`` for row-strip multi-GPU contexts.
            stream: optional raw ``hipStream_t`` (int) to enqueue on, e.g. ``torch.cuda.current_stream().cuda_stream``.
        """
        if param.cell_n is None:
            param.update()
        self.param = param
        self.data_type = np.float32
        self.resolution = param.resolution
        self.center = np.zeros(3, dtype=np.float32)
        self.base_rotation = np.eye(3, dtype=np.float32)
        self.map_length = param.map_length
        self.cell_n = int(param.cell_n)
        self.map_lock = threading.Lock()
        self.layer_names = list(self.layer_names_core)
        self.initial_variance = param.initial_variance
        self.mean_error = 0.0
        self.additive_mean_error = 0.0
        mode = param.index_mode
        if mode == "auto":
            mode = "reference_fp16" if self.cell_n <= 2049 else "fp32"
        self.index_mode = mode

        # traversability weights: same file format as the reference (elevation_mapping.py:103-104)
        wf = os.path.expandvars(os.path.expanduser(param.weight_file or ""))
        if wf and os.path.isfile(wf):
            param.load_weights(wf)

        # overlap clearance window (reference :88-91) -- recomputed inside the library, kept for API parity
        cell_range = int(np.clip(int(param.overlap_clear_range_xy / self.resolution), 0, self.cell_n))
        self.cell_min = self.cell_n // 2 - cell_range // 2
        self.cell_max = self.cell_n // 2 + cell_range // 2

        self._lib = _lib.load()
        self._strip = None
        if strip is not None:
            self._strip = EmapStrip(int(strip[0]), int(strip[1]), int(strip[2]), 0)
        self.rows = self.cell_n if strip is None else int(strip[1])
        self.row_begin = 0 if strip is None else int(strip[0])
        self._ctx = ct.c_void_p()
        P = _lib.fill_params(param, self.cell_n, mode)
        rc = self._lib.emap_create(ct.byref(P), ct.byref(self._strip) if self._strip is not None else None,
                                   int(param.device), ct.c_void_p(stream or 0), ct.byref(self._ctx))
        if rc != 0:
            self._ctx = ct.c_void_p()
            raise EmapError("emap_create failed with status %d (no usable HIP device / invalid parameters); "
                            "the MI355X backend has no CPU fallback" % rc)
        self._params_struct = P
        self.stream = int(stream or 0)           # (device-side plugins that keep handles of their own enqueue on the same stream)
        self.traversability_buffer = np.full((self.rows, self.cell_n), np.nan, np.float32)

        # managers are optional layers on top of the hot path (built lazily; see semantic_map / plugins)
        self.semantic_map = None
        self.plugin_manager = None
        self._last_plugin_route = {}
        self.last_submap_route = None               # "device" | "host": the route of the last submap call (EMAP_SUBMAP_RESIDENT)
        self.last_point_cloud_route = None          # "device" | "host": the route of the last point-cloud / arrow call (EMAP_CLOUD_RESIDENT)
        self.last_plane_segmentation_route = None   # "device" | "host": the route of the last get_plane_segmentation call (EMAP_PLANES_RESIDENT)
        self.last_planar_terrain_route = None       # the same of the last get_planar_terrain call (EMAP_TERRAIN_RESIDENT)
        self.last_planar_regions_route = None       # the same of the contour stage of the last get_planar_regions / trace_mask call (EMAP_REGIONS_RESIDENT)
        self._mask = self._mask_polygon = None      # safety-polygon service: the mask is built when it is read
        self.last_polygon_route = None              # "device" | "host": the route of the last safety check
        self.untraversable_polygon = None
        from .semantic_map import SemanticMap
        self.semantic_map = SemanticMap(self.param, self)
        # plugins (reference :110-113): same YAML format; a missing file just means "no plugins"
        from .plugins.plugin_manager import PluginManager
        self.plugin_manager = PluginManager(cell_n=self.cell_n, emap=self)
        pf = os.path.expandvars(os.path.expanduser(param.plugin_config_file or ""))
        if pf and os.path.isfile(pf):
            self.plugin_manager.load_plugin_settings(pf)

    # ------------------------------------------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            raise EmapError("libemap_hip call failed (%d): %s" % (rc, self._lib.emap_last_error(self._ctx).decode()))

    def __del__(self):
        try:
            if getattr(self, "_ctx", None) and self._ctx.value:
                self._lib.emap_destroy(self._ctx)
                self._ctx = ct.c_void_p()
        except Exception:
            pass

    def close(self):
        self.__del__()

    def set_scatter_mode(self, mode, bin_stack=0):
        """"auto" | "atomic" | "binned": how count/fuse scatter into the map (bit-identical results).
        ``bin_stack`` (test hook) forces bins of that many stacked 16x64 tiles, as maps beyond 16384 tiles use."""
        self._chk(self._lib.emap_set_scatter_mode(self._ctx, {"auto": 0, "atomic": 1, "binned": 2}[mode] | (int(bin_stack) << 8)))
        self._scatter_mode = mode

    def last_update_path(self):
        """which kernels the last whole frame ran: "atomic" (chain of launches), "binned" (tile kernels) or "small_frame" (one launch,
        robot scale) -- include/emap_hip.h: emap_last_update_path; the results are bit-identical"""
        v = ct.c_int32(-1)
        self._chk(self._lib.emap_last_update_path(self._ctx, ct.byref(v)))
        return {0: "atomic", 1: "binned", 2: "small_frame"}[v.value & 3]

    def small_frame_aborts(self):
        """how many robot-scale frames were re-run on the chain of launches because their single launch aborted a grid barrier (foreign
        work held the GPU) -- include/emap_hip.h: emap_small_frame_aborts; normally 0, the results are the same either way"""
        v = ct.c_uint32(0)
        self._chk(self._lib.emap_small_frame_aborts(self._ctx, ct.byref(v)))
        return int(v.value)

    def last_frame_semantics(self):
        """how the last whole frame fused the channels declared for it (emap_frame_semantics): "in_tile_pass" (32-byte records, fused by
        the tile kernel that fused the heights), "carried" (32-byte records, the stand-alone semantic kernel read the channels from
        them: a launch with heavy-tile parts) or "separate" (the stand-alone kernels on 16-byte records / the atomic path)"""
        v = ct.c_int32(-1)
        self._chk(self._lib.emap_last_update_path(self._ctx, ct.byref(v)))
        return "in_tile_pass" if v.value & 4 else ("carried" if v.value & 8 else "separate")

    def set_ray_mode(self, mode):
        """"auto" | "by_row" | "by_ray": how a SHARDED frame (emap_update_sharded) runs the visibility pass (include/emap_hip.h:
        emap_set_ray_mode; bit-identical results, every rank the same setting)"""
        self._chk(self._lib.emap_set_ray_mode(self._ctx, {"auto": 0, "by_row": 1, "by_ray": 2}[mode]))
        self._ray_mode = {"auto": 0, "by_row": 1, "by_ray": 2}[mode]

    def reload_params(self):
        """Push changed ``self.param`` scalars to the device (kernargs, no recompilation)."""
        P = _lib.fill_params(self.param, self.cell_n, self.index_mode)
        self._chk(self._lib.emap_set_params(self._ctx, ct.byref(P)))
        self._params_struct = P

    # ---- state access ------------------------------------------------------------------------------
    def get_layer_raw(self, name_or_id):
        """Raw device plane as a host ``(rows, cell_n)`` float32 array."""
        pid = PLANES[name_or_id] if isinstance(name_or_id, str) else int(name_or_id)
        out = np.empty((self.rows, self.cell_n), np.float32)
        self._chk(self._lib.emap_get_layer(self._ctx, pid, f32p(out)))
        return out

    @property
    def logical_row_begin(self):
        """first LOGICAL map row of this context's (rows, cell_n) views: 0 for a full map; a strip holds the logical rows
        begin, begin + 1, ... modulo cell_n, and they change with every row shift (the strip keeps its physical rows)"""
        r = ct.c_int32(0)
        self._chk(self._lib.emap_strip_logical_begin(self._ctx, ct.byref(r)))
        return int(r.value)

    def set_layer_raw(self, name_or_id, array):
        pid = PLANES[name_or_id] if isinstance(name_or_id, str) else int(name_or_id)
        a = np.ascontiguousarray(array, np.float32)
        assert a.shape == (self.rows, self.cell_n), a.shape
        self._chk(self._lib.emap_set_layer(self._ctx, pid, f32p(a)))

    @property
    def elevation_map(self):
        """Host copy of the planar ``(7, cell_n, cell_n)`` map (reference attribute, elevation_mapping.py:67)."""
        return np.stack([self.get_layer_raw(k) for k in range(7)], axis=0)

    @elevation_map.setter
    def elevation_map(self, value):
        value = np.asarray(value, np.float32)
        for k in range(7):
            self.set_layer_raw(k, value[k])

    @property
    def normal_map(self):
        return np.stack([self.get_layer_raw(k) for k in (7, 8, 9)], axis=0)

    @normal_map.setter
    def normal_map(self, value):
        value = np.asarray(value, np.float32)
        for j, k in enumerate((7, 8, 9)):
            self.set_layer_raw(k, value[j])

    @property
    def traversability_input(self):
        return self.get_layer_raw(10)

    # ---- reference API -----------------------------------------------------------------------------
    def clear(self):
        """Reset all layers (reference :119-128)."""
        with self.map_lock:
            self._chk(self._lib.emap_clear(self._ctx))
            if self.semantic_map is not None:
                self.semantic_map.clear()
        self.mean_error = 0.0
        self.additive_mean_error = 0.0

    def get_position(self, position):
        position[0][:] = self.center

    def move(self, delta_position):
        """Relative shift (reference :139-152 -- note the sign convention differs from move_to).  The caller's float64 position
        meets the float32 centre in float64, exactly like the reference's array arithmetic (pinned by tests/golden/host_steps.npz)."""
        delta_position = np.asarray(delta_position, np.float64)
        delta_pixel = np.round(delta_position[:2] / self.resolution)
        self.center[:2] += delta_pixel * self.resolution
        self.center[2] += delta_position[2]
        self._shift(delta_pixel, -float(delta_position[2]))

    def move_to(self, position, R):
        """Absolute shift + base rotation update (reference :154-170)."""
        self.base_rotation = np.asarray(R, dtype=np.float32)
        position = np.asarray(position, np.float64)
        delta = position - self.center
        delta_pixel = np.around(delta[:2] / self.resolution)
        self.center[:2] += delta_pixel * self.resolution
        self.center[2] += delta[2]
        self._shift(-delta_pixel, -float(delta[2]))

    def _shift(self, delta_pixel, dz):
        sv = np.asarray(delta_pixel).astype(np.int32)
        with self.map_lock:
            self._chk(self._lib.emap_shift(self._ctx, int(sv[0]), int(sv[1]), ct.c_float(dz)))
            if self.semantic_map is not None and np.abs(sv).sum() != 0:
                self.semantic_map.shift_map_xy(sv)

    def shift_map_xy(self, delta_pixel):
        self._shift(delta_pixel, 0.0)

    def shift_map_z(self, delta_z):
        self._shift(np.zeros(2), float(delta_z))

    def shift_translation_to_map_center(self, t):
        t -= self.center

    def bind_points(self, points_all, strip_pose=None):
        """Upload a host cloud ``(N, 3+K)`` (float32 or float64) and bind it for the next stage calls.  ``strip_pose = (R, t)`` (t
        map-centre relative) on a row-strip context: only the points that can land in this strip's rows under that pose are converted
        and uploaded (include/emap_hip.h: emap_upload_points_strip -- the frame must then use the same pose and must not march its
        rays by row); returns the number of points bound."""
        pts = np.asarray(points_all)
        if pts.dtype == np.float64:
            pts = np.ascontiguousarray(pts)
            dtype = 1
        else:
            pts = np.ascontiguousarray(pts, np.float32)
            dtype = 0
        assert pts.ndim == 2 and pts.shape[1] >= 3
        if strip_pose is not None:
            R, t = self._rt(*strip_pose)
            kept = ct.c_int64(0)
            self._chk(self._lib.emap_upload_points_strip(self._ctx, ct.c_void_p(pts.ctypes.data), ct.c_int64(pts.shape[0]),
                                                         ct.c_int64(pts.shape[1]), dtype, f32p(R), f32p(t), ct.byref(kept)))
            self._n_bound, self._k_bound = int(kept.value), pts.shape[1] - 3
            self._bound_host = None                 # (the bound cloud is a subset: nothing indexes the host copy by point)
            return self._n_bound
        self._chk(self._lib.emap_upload_points(self._ctx, ct.c_void_p(pts.ctypes.data), ct.c_int64(pts.shape[0]),
                                               ct.c_int64(pts.shape[1]), dtype))
        self._n_bound, self._k_bound = pts.shape[0], pts.shape[1] - 3
        self._bound_host = pts
        return self._n_bound

    def strip_point_mask(self, points_all, R, t):
        """which points ``bind_points(points_all, strip_pose=(R, t))`` would upload (bool array; all True on a whole-map context)"""
        pts = np.asarray(points_all)
        dtype = 1 if pts.dtype == np.float64 else 0
        pts = np.ascontiguousarray(pts) if dtype else np.ascontiguousarray(pts, np.float32)
        R, t = self._rt(R, t)
        keep = np.zeros(pts.shape[0], np.uint8)
        self._chk(self._lib.emap_strip_point_mask(self._ctx, ct.c_void_p(pts.ctypes.data), ct.c_int64(pts.shape[0]), ct.c_int64(pts.shape[1]), dtype,
                                                  f32p(R), f32p(t), keep.ctypes.data_as(ct.POINTER(ct.c_uint8))))
        return keep.astype(bool)

    def bind_points_device(self, dev_ptr, n, stride):
        """Bind a device-resident float32 cloud (raw pointer) without copying."""
        self._chk(self._lib.emap_set_points_device(self._ctx, ct.c_void_p(dev_ptr), ct.c_int64(n), ct.c_int64(stride)))
        self._n_bound, self._k_bound = n, stride - 3
        self._bound_host = None

    def bind_points_device_split(self, xyz_ptr, chan_ptr, n, n_chan):
        """Bind a device-resident cloud that is already de-interleaved: xyz ``(n, 3)`` and the extra channels ``(n, n_chan)``, both
        row-major float32 (the layout ``bind_points`` / ``input_pointcloud`` give an uploaded cloud)."""
        self._chk(self._lib.emap_set_points_device_split(self._ctx, ct.c_void_p(xyz_ptr), ct.c_void_p(chan_ptr), ct.c_int64(n), ct.c_int64(n_chan)))
        self._n_bound, self._k_bound = n, n_chan
        self._bound_host = None

    def bind_depth_image(self, depth, K, *, depth_scale=None, rgb=None, features=None, confidence=None, confidence_threshold=0.0,
                         min_depth=0.0, max_depth=8.0, step=1):
        """Upload a depth camera's frame as IMAGES and bind the cloud the device back-projects from them (include/emap_hip.h:
        emap_bind_depth_image; the reference does this on the host, pointcloud_node.py:205-250).  ``depth``: (H, W) float32 metres, or
        uint16 units of ``depth_scale`` metres; ``K``: the 3 x 3 intrinsics; ``rgb``: (H, W, 3) uint8; ``features``: (k, H, W) float32;
        ``confidence``: (H, W) float32.  Every ``step``-th row and column becomes one row of the cloud (NaN where the pixel is not
        valid), its channels colour-then-features; returns the number of rows."""
        depth = np.asarray(depth)
        if depth.dtype == np.uint16:
            if depth_scale is None:
                raise ValueError("a uint16 depth image needs depth_scale (metres per unit)")
            dtype = 1
        else:
            depth, dtype = np.asarray(depth, np.float32), 0
        depth = np.ascontiguousarray(depth)
        if depth.ndim != 2:
            raise ValueError("depth must be an (H, W) image")
        H, W = depth.shape
        Km = np.asarray(K, np.float64).reshape(3, 3)
        d = EmapDepthDesc(H, W, dtype, int(step), int(rgb is not None), 0, Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2],
                          1.0 if depth_scale is None else depth_scale, min_depth, max_depth, confidence_threshold)
        ptr = [None, None, None]
        keep = []
        for k, (img, dt, shape) in enumerate(((rgb, np.uint8, (H, W, 3)), (features, np.float32, None), (confidence, np.float32, (H, W)))):
            if img is None:
                continue
            img = np.ascontiguousarray(img, dt)
            if k == 1:
                if img.ndim == 2:
                    img = img[None]
                shape = (img.shape[0], H, W)
                d.n_features = img.shape[0]
            if img.shape != shape:
                raise ValueError("image of shape %r where %r is expected" % (img.shape, shape))
            keep.append(img)
            ptr[k] = ct.c_void_p(img.ctypes.data)
        n = ct.c_int64(0)
        self._chk(self._lib.emap_bind_depth_image(self._ctx, ct.byref(d), ct.c_void_p(depth.ctypes.data), ptr[0], ptr[1], ptr[2], ct.byref(n)))
        self._n_bound, self._k_bound = int(n.value), int(d.has_rgb) + int(d.n_features)
        self._bound_host = None
        return self._n_bound

    def input_depth_image(self, depth, K, channels: List[str], R, t, position_noise: float, orientation_noise: float, **keywords):
        """``input_pointcloud`` for a depth camera's frame: back-projected on the device (``bind_depth_image``, same keywords) and fused.
        ``channels``: the names of the extra channels, colour then features -- what ``input_pointcloud`` receives as ``channels[3:]``."""
        self.bind_depth_image(depth, K, **keywords)
        self.update_map_with_kernel(None, list(channels), np.asarray(R, np.float32), np.asarray(t, np.float32).copy(),
                                    position_noise, orientation_noise, want_stats=False)

    def bind_pointcloud2(self, cloud, *, fields=None, width=None, height=1, point_step=None, row_step=None, is_bigendian=False,
                         channels=None, typed=False):
        """Upload the BYTES of a sensor_msgs/PointCloud2 message and bind the cloud the device unpacks from them (include/emap_hip.h:
        emap_bind_cloud_message; the reference's node gathers the fields on the host, elevation_mapping_ros.cpp:319-338).  ``cloud``: a
        message-like object (``.data .fields .width .height .point_step .row_step .is_bigendian``; duck-typed, no ROS import) or a
        bytes-like / uint8 array described by the keywords (``width`` defaults to what ``row_step``, or else one of ``height`` equal shares of the data, holds).  ``channels``
        and ``typed``: see ``pointcloud2_descriptor``.  Returns the number of rows; ``bound_channels`` then names the channel columns."""
        if hasattr(cloud, "data") and hasattr(cloud, "fields") and hasattr(cloud, "point_step"):
            data, fields, width, height = cloud.data, cloud.fields, cloud.width, cloud.height
            point_step, row_step, is_bigendian = cloud.point_step, cloud.row_step, cloud.is_bigendian
        else:
            data = cloud
        if fields is None:
            raise ValueError("fields are required with raw message bytes")
        try:
            data = np.frombuffer(data, np.uint8)
        except (TypeError, ValueError):
            data = np.ascontiguousarray(data, np.uint8).reshape(-1)
        if width is None:
            if point_step is None or int(point_step) < 1 or int(height) < 1:
                raise ValueError("point_step and height are required to derive width")
            width = (int(row_step) if row_step is not None else data.size // int(height)) // int(point_step)
        d, names = pointcloud2_descriptor(fields, width, height, point_step, row_step, is_bigendian, channels, typed)
        if d.height >= 1 and d.row_step >= 0 and data.size < d.height * d.row_step:
            raise ValueError("the message holds %d bytes where height * row_step = %d are described" % (data.size, d.height * d.row_step))
        n = ct.c_int64(0)
        self._chk(self._lib.emap_bind_cloud_message(self._ctx, ct.byref(d), ct.c_void_p(data.ctypes.data), ct.byref(n)))
        self._n_bound, self._k_bound = int(n.value), d.n_cols - 3
        self._bound_host = None
        self.bound_channels = names[3:]
        return self._n_bound

    def input_pointcloud2(self, cloud, R, t, position_noise: float, orientation_noise: float, **keywords):
        """``input_pointcloud`` for a PointCloud2 message: unpacked on the device (``bind_pointcloud2``, same keywords) and fused; the
        channel names are the selected fields' names."""
        self.bind_pointcloud2(cloud, **keywords)
        self.update_map_with_kernel(None, list(self.bound_channels), np.asarray(R, np.float32), np.asarray(t, np.float32).copy(),
                                    position_noise, orientation_noise, want_stats=False)

    def bound_points(self):
        """the cloud bound now, read back from the device: ``(xyz (n, 3), chan (n, K))`` float32 (include/emap_hip.h:
        emap_get_bound_points; waits for the stream)"""
        n, k = int(getattr(self, "_n_bound", 0)), int(getattr(self, "_k_bound", 0))
        xyz, chan = np.empty((n, 3), np.float32), np.empty((n, k), np.float32)
        self._chk(self._lib.emap_get_bound_points(self._ctx, ct.c_void_p(xyz.ctypes.data), ct.c_void_p(chan.ctypes.data) if k else None))
        return xyz, chan

    @staticmethod
    def _rt(R, t):
        R = np.ascontiguousarray(np.asarray(R, np.float32).reshape(9))
        t = np.ascontiguousarray(np.asarray(t, np.float32).reshape(3))
        return R, t

    def update_map_with_kernel(self, points_all, channels, R, t, position_noise, orientation_noise, want_stats=True):
        """One frame (reference :316-391).  ``points_all``: host ``(N, 3+K)`` array or ``None`` to reuse the bound
        cloud; ``t`` is shifted to the map centre in place like the reference does (:333)."""
        if points_all is not None:
            self.bind_points(points_all)
        R, t32 = self._rt(R, t)
        with self.map_lock:
            jobs = []
            if self.semantic_map is not None and channels:
                # layers + count plane must exist before the average pass; the sum / colour fusions ride inside the frame
                jobs = self.semantic_map.declare_frame(self, list(channels))
            t32 = t32 - self.center
            try:
                t -= self.center  # reference mutates the caller's array
            except TypeError:
                pass
            st = EmapStats()
            self._chk(self._lib.emap_update(self._ctx, f32p(R), f32p(t32), ct.c_double(position_noise),
                                            ct.c_double(orientation_noise), ct.byref(st) if want_stats else None))
            if want_stats:
                self._take_stats(st)
            if jobs:
                self.semantic_map.finish_frame(self, jobs, R, t32)
        return st if want_stats else None

    def _take_stats(self, st):
        if st.gate_fired:
            self.mean_error = float(st.mean_error)
        self.additive_mean_error = float(st.additive_mean_error)
        self.last_stats = st

    def clear_overlap_map(self, t):
        self._chk(self._lib.emap_overlap_clear(self._ctx, ct.c_float(float(np.asarray(t, np.float32).reshape(3)[2]))))

    def get_additive_mean_error(self):
        st = EmapStats()
        self._chk(self._lib.emap_get_stats(self._ctx, ct.byref(st)))
        self.additive_mean_error = float(st.additive_mean_error)
        return self.additive_mean_error

    def update_variance(self):
        self._chk(self._lib.emap_update_variance(self._ctx))

    def update_time(self):
        self._chk(self._lib.emap_update_time(self._ctx))

    def update_normal(self, dilated_map):
        """normal map from a given (dilated) height plane and the current ``is_valid`` (reference :564-577: ``normal_map *= 0`` + the
        normal filter kernel).  Inside a frame the stencil launch does this on the device planes; this public form takes a host plane:
        it becomes the stencil stage's input, the stage runs, and the two planes the reference's method does not touch (the
        traversability it would also rewrite, the stage's input plane) are put back."""
        with self.map_lock:
            keep_trav, keep_in = self.get_layer_raw("traversability"), self.get_layer_raw("traversability_input")
            try:
                self.set_layer_raw("traversability_input", np.asarray(dilated_map, np.float32))
                self.stage("traversability_normals")
            finally:                                  # whatever the stage did: the two planes the reference's method leaves alone come back
                self.set_layer_raw("traversability", keep_trav)
                self.set_layer_raw("traversability_input", keep_in)

    def update_upper_bound_with_valid_elevation(self):
        m = self.elevation_map
        mask = m[2] > 0.5
        self.set_layer_raw(5, np.where(mask, m[0], m[5]))
        self.set_layer_raw(6, np.where(mask, 0.0, m[6]))

    def input_pointcloud(self, raw_points, channels: List[str], R, t, position_noise: float, orientation_noise: float):
        """Entry point used by the ROS wrapper (reference :434-466).  NaN rows are skipped inside the kernels
        instead of being compacted on the host (:458)."""
        additional_channels = list(channels[3:])
        # asynchronous: nothing is read back per frame (get_additive_mean_error / get_map_with_name_ref synchronise)
        self.update_map_with_kernel(raw_points, additional_channels, np.asarray(R, np.float32),
                                    np.asarray(t, np.float32).copy(), position_noise, orientation_noise, want_stats=False)

    def input_image(self, image, channels: List[str], R, t, K, D, distortion_model: str, image_height: int, image_width: int):
        """Fuse a (multi-channel) camera image into the semantic layers (reference :468-562): every known cell is
        projected into the image, occluded cells are rejected by a Bresenham walk towards the camera, the image is
        sampled per cell."""
        image = np.stack([np.asarray(c) for c in image], axis=0)
        if image.ndim == 2:
            image = image[None]
        image = image.astype(np.float32)
        K = np.asarray(K, np.float32); R = np.asarray(R, np.float32); t = np.asarray(t, np.float32)
        D = np.asarray(D, np.float32).reshape(-1)
        if len(D) < 4:
            D = np.zeros(5, np.float32)
        elif len(D) == 4:
            D = np.concatenate([D, np.zeros(1, np.float32)])
        else:
            D = D[:5].copy()
        if distortion_model != "radtan":
            D = D * 0            # equidistant / plumb_bob: "not implemented yet" in the reference -> no distortion
        P = (K @ np.concatenate([R, t[:, None]], 1)).astype(np.float32)
        x1, y1, z1 = camera_cell(self.center, self.cell_n, self.resolution, R, t)
        with self.map_lock:
            self._chk(self._lib.emap_image_correspondence(
                self._ctx, ct.c_float(x1), ct.c_float(y1), ct.c_float(z1), f32p(np.ascontiguousarray(P.reshape(-1))),
                f32p(np.ascontiguousarray(K.reshape(-1))), f32p(np.ascontiguousarray(D)), ct.c_float(float(image_height)),
                ct.c_float(float(image_width)), f32p(np.ascontiguousarray(self.center, np.float32))))
            self.semantic_map.update_layers_image(self, image, list(channels), image_height, image_width)

    def input_image_message(self, image, channels: List[str], R, t, K=None, D=None, distortion_model: str = "radtan", camera_info=None, **raw):
        """``input_image`` for the BYTES of a sensor_msgs/Image: the message is uploaded as it is and one launch computes the
        correspondence and fuses every channel (include/emap_hip.h: emap_input_image_message; the reference's node converts the message
        to one float matrix per channel on the host, elevation_mapping_ros.cpp:375-446).  ``image``: a message-like object (``.height
        .width .encoding .is_bigendian .step .data``; duck-typed, no ROS import) or a bytes-like / uint8 array described by the keywords
        of the same names.  ``camera_info``: an object with ``.K .D .distortion_model`` used where ``K`` / ``D`` are not given.  The
        planes are the node's: ``bgr8`` / ``bgra8`` arrive as RGB; channel ``j`` of the list samples plane ``j`` and ``rgb`` planes 0, 1, 2,
        exactly as ``update_layers_image`` hands them over; a plane count that does not match the channel list (``rgb`` counts as 3)
        raises ``ValueError`` where the node drops the frame (:428-441).  Returns without waiting for the device."""
        if hasattr(image, "data") and hasattr(image, "encoding"):
            data = image.data
            raw = dict(height=image.height, width=image.width, encoding=image.encoding, is_bigendian=image.is_bigendian, step=image.step)
        else:
            data = image
        unknown = set(raw) - {"height", "width", "encoding", "is_bigendian", "step"}
        if unknown:
            raise TypeError("unexpected keywords: %s" % ", ".join(sorted(unknown)))
        if not all(k in raw for k in ("height", "width", "encoding")):
            raise ValueError("height, width and encoding are required with raw message bytes")
        d = image_message_descriptor(raw["encoding"], raw["height"], raw["width"], raw.get("step"), raw.get("is_bigendian", False))
        try:
            data = np.frombuffer(data, np.uint8)
        except (TypeError, ValueError):
            data = np.ascontiguousarray(data, np.uint8).reshape(-1)
        if data.size < d.height * d.step:
            raise ValueError("the message holds %d bytes where height * step = %d are described" % (data.size, d.height * d.step))
        channels = list(channels)
        planes = sum(3 if c == "rgb" else 1 for c in channels)
        if planes != d.n_chan:
            raise ValueError("the image has %d planes, the channels %s ask for %d" % (d.n_chan, channels, planes))
        if camera_info is not None:
            K = camera_info.K if K is None else K
            D = camera_info.D if D is None else D
            distortion_model = getattr(camera_info, "distortion_model", distortion_model) or distortion_model
        if K is None:
            raise ValueError("K or camera_info is required")
        K = np.asarray(K, np.float32).reshape(3, 3); R = np.asarray(R, np.float32); t = np.asarray(t, np.float32)
        D = np.asarray([] if D is None else D, np.float32).reshape(-1)
        if len(D) < 4:
            D = np.zeros(5, np.float32)
        elif len(D) == 4:
            D = np.concatenate([D, np.zeros(1, np.float32)])
        else:
            D = D[:5].copy()
        if distortion_model != "radtan":
            D = D * 0            # as input_image
        P = (K @ np.concatenate([R, t[:, None]], 1)).astype(np.float32)
        x1, y1, z1 = camera_cell(self.center, self.cell_n, self.resolution, R, t)
        cam = (ct.c_float(x1), ct.c_float(y1), ct.c_float(z1), f32p(np.ascontiguousarray(P.reshape(-1))), f32p(np.ascontiguousarray(K.reshape(-1))),
               f32p(np.ascontiguousarray(D)))
        center = np.ascontiguousarray(self.center, np.float32)
        with self.map_lock:
            entries = self.semantic_map.image_entries(channels)
            if any(e[0] == 1 for e in entries) and 3 * d.height * d.width > IMAGE_MAX_INDEX:
                raise ValueError("3 * height * width beyond 2^24 with a colour channel: use input_image")
            if len(entries) > 4:
                raise ValueError("at most 4 fused channels per image message (%d asked for)" % len(entries))
            if not entries:      # nothing to fuse: the correspondence alone, as input_image computes it
                self._chk(self._lib.emap_image_correspondence(self._ctx, *cam, ct.c_float(float(d.height)), ct.c_float(float(d.width)), f32p(center)))
                return
            specs = (EmapImageSpec * len(entries))()
            for s, (kind, layer, plane, alpha) in zip(specs, entries):
                s.kind, s.layer, s.plane, s.alpha = kind, layer, plane, alpha
            self._chk(self._lib.emap_input_image_message(self._ctx, ct.byref(d), ct.c_void_p(data.ctypes.data), *cam, f32p(center), specs, len(entries)))

    def get_image_correspondence(self):
        """(uv (2, C, C) float32, valid (C, C) bool) of the last input_image call"""
        uv = np.empty((2, self.cell_n, self.cell_n), np.float32); valid = np.empty((self.cell_n, self.cell_n), np.uint8)
        self._chk(self._lib.emap_image_get_correspondence(self._ctx, f32p(uv), valid.ctypes.data_as(ct.c_void_p)))
        return uv, valid.astype(bool)

    input = input_pointcloud  # name used by the C++ wrapper (src/elevation_mapping_wrapper.cpp:173-178)

    # ---- stage-level API (parity tests; same order as update_map_with_kernel) ----------------------
    def stage(self, name, R=None, t=None, **kw):
        L = self._lib
        if name in ("count", "fuse", "rays", "fuse_average"):
            R, t = self._rt(R, t)
            self._chk(getattr(L, "emap_" + name)(self._ctx, f32p(R), f32p(t)))
        elif name == "gate":
            s, c = kw.get("err_sum"), kw.get("err_cnt")
            self._chk(L.emap_set_drift_inputs(self._ctx, ct.c_double(kw.get("position_noise", 0.0)),
                                              ct.c_double(kw.get("orientation_noise", 0.0)),
                                              ct.byref(ct.c_double(s)) if s is not None else None,
                                              ct.byref(ct.c_uint32(c)) if c is not None else None))
        elif name == "overlap":
            self._chk(L.emap_overlap_clear(self._ctx, ct.c_float(float(t))))
        elif name in ("commit", "average", "dilate", "traversability_normals", "post", "update_variance", "update_time"):
            self._chk(getattr(L, "emap_" + name)(self._ctx))
        else:
            raise ValueError(name)

    def stats(self):
        st = EmapStats()
        self._chk(self._lib.emap_get_stats(self._ctx, ct.byref(st)))
        return st

    def point_index(self, R, t):
        """(idx, valid, inside) per bound point -- tail of add_points_kernel (custom_kernels.py:260-262)."""
        R, t = self._rt(R, t)
        n = self._n_bound
        idx, valid, inside = np.empty(n, np.int32), np.empty(n, np.uint8), np.empty(n, np.uint8)
        self._chk(self._lib.emap_point_index(self._ctx, f32p(R), f32p(t), idx.ctypes.data_as(ct.c_void_p),
                                             valid.ctypes.data_as(ct.c_void_p), inside.ctypes.data_as(ct.c_void_p)))
        return idx, valid, inside

    def sync(self):
        self._chk(self._lib.emap_sync(self._ctx))

    # ---- read-back (reference :579-775) ----------------------------------------------------------
    def exists_layer(self, name):
        if name in self.layer_names:
            return True
        if self.semantic_map is not None and name in self.semantic_map.layer_names:
            return True
        if self.plugin_manager is not None and name in self.plugin_manager.layer_names:
            return True
        return False

    def _publish(self, m, fill_nan=False, add_z=False, valid=None):
        m = m.copy()
        if fill_nan:
            m = np.where(valid > 0.5, m, np.nan)
        if add_z:
            m = m + self.center[2]
        return m[1:-1, 1:-1]

    def get_map_with_name_ref(self, name, data):
        """Fill ``data`` (float32, ``(cell_n-2, cell_n-2)``) in place: border stripped, both axes flipped
        (reference :720-775)."""
        if name in GRID_BUILTIN_LAYERS and self._strip is None and isinstance(data, np.ndarray) and data.dtype == np.float32 \
                and data.flags["C_CONTIGUOUS"] and data.shape == (self.cell_n - 2, self.cell_n - 2):
            with self.map_lock:   # strip / NaN fill / +center_z / double flip happen in one device kernel
                self._chk(self._lib.emap_publish_layer(self._ctx, GRID_BUILTIN_LAYERS.index(name), ct.c_float(float(self.center[2])),
                                                       int(bool(self.param.use_only_above_for_upper_bound)), f32p(data)))
            return
        with self.map_lock:
            m = self._stripped_layer(name)
        if m is None:
            print("Layer {} is not in the map".format(name))
            return
        m = np.flip(np.flip(m, 0), 1)
        data[...] = m.astype(np.float32)

    # ---- GridMap message output (include/emap_hip.h: emap_publish_grid_map) -----------------------------------------------------------
    def _grid_launch(self, entries, out, order):
        """``entries``: ``(kind, index, slot[, flags])`` per device layer; ``out``: C-contiguous float32 ``(slots, M, M)``.  At most 32 layers
        per launch: more go in groups of 32.  The caller holds ``map_lock``."""
        entries = [tuple(int(x) for x in e) + (0,) * (4 - len(e)) for e in entries]
        for a in range(0, len(entries), GRID_MAX_LAYERS):
            group = entries[a:a + GRID_MAX_LAYERS]
            table = (EmapGridLayerEx * len(group))()
            for g, (kind, index, slot, flags) in zip(table, group):
                g.kind, g.index, g.slot, g.flags = kind, index, slot, flags
            self._chk(self._lib.emap_publish_grid_map_ex(self._ctx, table, len(group), GRID_ORDERS[order], ct.c_float(float(self.center[2])),
                                                         int(bool(self.param.use_only_above_for_upper_bound)), f32p(out), int(out.shape[0])))

    def publish_grid_layers(self, entries, out, order="rows"):
        """the layer table as it is: ``entries`` = ``(kind, index, slot)`` or ``(kind, index, slot, flags)`` tuples or an ``EmapGridLayer`` /
        ``EmapGridLayerEx`` array (``grid_map_descriptor``), written into ``out`` (float32, C-contiguous, ``(slots, cell_n - 2, cell_n - 2)``);
        slots the table does not name are not written.  Kind ``GRID_PLUGIN``: ``index`` = a resident plugin plane as an ``emap_plugin_chain``
        left it, ``flags`` = ``GRID_FILL_NAN | GRID_ADD_Z``."""
        M = self.cell_n - 2
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.ndim == 3 and out.shape[1:] == (M, M)):
            raise ValueError("out must be a C-contiguous float32 array of shape (slots, %d, %d)" % (M, M))
        if order not in GRID_ORDERS:
            raise ValueError("order must be 'rows' or 'message'")
        entries = [(e.kind, e.index, e.slot, e.flags) if isinstance(e, EmapGridLayerEx) else (e.kind, e.index, e.slot) if isinstance(e, EmapGridLayer)
                   else tuple(e) for e in entries]
        if any(len(e) not in (3, 4) for e in entries):
            raise ValueError("an entry is (kind, index, slot) or (kind, index, slot, flags)")
        with self.map_lock:
            self._grid_launch(entries, out, order)

    @property
    def last_plugin_route(self):
        """``{plugin layer: "device" | "host"}`` of the last ``get_grid_map_layers`` / ``get_grid_map_message`` call: computed by an op of the
        plugin chain into a resident plane, or by the plugin's host route"""
        return dict(self._last_plugin_route)

    def _plugin_host_step(self, name):
        """the host route of one plugin, as ``_stripped_layer`` runs it"""
        sem = self.semantic_map
        self.plugin_manager.update_with_name(
            name, LazyPlanes(7, self.get_layer_raw, device_map=self), self.layer_names,
            LazyPlanes(len(sem.layer_names), sem._layer, rows=self.rows, cols=self.cell_n) if sem is not None else None,
            self.semantic_map.layer_names if self.semantic_map is not None else [],
            self.base_rotation, self.semantic_map.elements_to_shift if self.semantic_map is not None else {})

    def get_grid_map_layers(self, layers, out=None, order="rows", normal_color=False):
        """What the wrapper's ``get_grid_map`` gathers for a publisher (elevation_mapping_wrapper.cpp:213-252), in one call: ``(names,
        array)`` with ``array`` float32 of shape ``(len(names), cell_n - 2, cell_n - 2)``.  ``layers`` keep their order; names for which
        ``exists_layer`` is false are dropped, as there; with ``normal_color`` (the node's ``enable_normal_color``) ``normal_x``, ``normal_y``,
        ``normal_z`` and ``color`` are appended (a name already kept is not added twice).  ``order="rows"``: plane ``k`` is what
        ``get_map_with_name_ref(names[k], ...)`` leaves; ``order="message"``: its transpose stored C-contiguous, i.e. the column-major
        ``Float32MultiArray`` of ``grid_map_msgs/GridMap``.

        Plugin layers are computed in list order, as one ``get_map_with_name_ref`` per layer computes them.  A plugin that describes itself
        as a device op (``PluginBase.device_op``: MinFilter, MaxFilter, SmoothFilter, Erosion, RobotCentricElevation, Inpainting with
        ``method="telea_fronts"``, and the semantic plugins SemanticFilter, SemanticTraversability, MaxLayerFilter and FeaturesPca, which read
        map layers, plugin planes and semantic layers where they lie on the device) joins a chain of launches that is enqueued without a
        wait and leaves its output in a resident plane (``plugins/plugin_manager.py``); the others (Inpainting with a host method, a
        configuration a plugin declines: e.g. a PCA of fewer than 3 or more than 16 layers, a layer-name ``default_value``) take their host
        route and put their plane into ``array`` on the host.  A device FeaturesPca has the host route's definition, not its last bit: a
        colour level may differ by 1 in a few cells.  Then ONE device launch writes every
        built-in, semantic and resident plugin layer, with one copy and one wait (groups of 32 beyond 32 layers).  ``last_plugin_route`` tells
        which route each plugin layer took; ``EMAP_PLUGIN_RESIDENT=0`` in the environment sends every plugin through its host route.  The
        whole call runs under one ``map_lock``."""
        if order not in GRID_ORDERS:
            raise ValueError("order must be 'rows' or 'message'")
        self._require_full_map("get_grid_map_layers")
        with self.map_lock:
            return self._grid_map_layers_locked(layers, out, order, normal_color)

    def _grid_plan(self, layers, normal_color):
        """the layer list of a publisher, filtered, ordered and extended as the wrapper's ``get_grid_map`` does: ``[(name, device entry or
        None)]`` -- ``(kind, index)`` for a built-in, semantic or normal-colour layer, ``None`` for a plugin layer.  Shared by
        ``get_grid_map_layers`` and ``get_submap_layers``; the caller holds ``map_lock``."""
        names = []
        for n in layers:
            if n not in names and self.exists_layer(n):
                names.append(n)
        if normal_color:
            names += [n for n in GRID_NORMAL_COLOR_LAYERS if n not in names]
        sem = self.semantic_map.layer_names if self.semantic_map is not None else []
        plug = self.plugin_manager.layer_names if self.plugin_manager is not None else []
        plan = []                                   # (name, device entry or None)
        for n in names:
            if normal_color and n in GRID_NORMAL_COLOR_LAYERS:
                plan.append((n, (GRID_NORMAL_COLOR, 0) if n == "color" else (GRID_BUILTIN, GRID_BUILTIN_LAYERS.index(n))))
            elif n in GRID_BUILTIN_LAYERS[:6]:
                plan.append((n, (GRID_BUILTIN, GRID_BUILTIN_LAYERS.index(n))))
            elif n in sem:
                plan.append((n, (GRID_SEMANTIC, sem.index(n))))
            elif n in plug:
                plan.append((n, None))
            else:                                   # (is_valid: a layer of the map that get_map_with_name_ref does not publish either)
                print("Layer {} is not in the map".format(n))
        return plan

    def _plugin_steps(self, plan):
        """the ``plugin_chain_plan`` steps of the plugin layers of ``plan`` (the entries without a device source); ``EMAP_PLUGIN_RESIDENT=0``
        in the environment sends every plugin through its host route"""
        pm = self.plugin_manager
        want = [n for n, e in plan if e is None]
        if pm is None or not want:
            return []
        sem = self.semantic_map.layer_names if self.semantic_map is not None else []
        return plugin_chain_plan(want, pm.plugins, pm.layer_names, self.layer_names, sem, resident=os.environ.get("EMAP_PLUGIN_RESIDENT", "1") != "0")

    def _grid_plugins(self, plan, host_plane):
        """the plugin layers of ``plan`` computed in list order, ONCE over the whole map: device-capable plugins as ops of the chain into
        their resident planes, the others on the host -- ``host_plane(name, m)`` takes the published plane (float32, ``(M, M)``, what
        ``get_map_with_name_ref`` leaves).  Sets ``last_plugin_route``; returns the device table ``[(kind, index, position in plan,
        flags)]`` of everything a grid launch can write.  The caller holds ``map_lock``."""
        pm = self.plugin_manager
        plug = pm.layer_names if pm is not None else []

        def host_step(n):                           # the plugin's host route, then _publish and the flips on the host
            self._plugin_host_step(n)
            p = pm.get_param_with_name(n)
            m = self._publish(np.asarray(pm.host_layer(n)), p.fill_nan, p.is_height_layer, self.get_layer_raw(2))
            host_plane(n, np.flip(np.flip(m, 0), 1).astype(np.float32))

        self._last_plugin_route = {}
        if pm is not None and any(e is None for _, e in plan):
            self._last_plugin_route = pm.run_plan(self._plugin_steps(plan), host_step, self.base_rotation)
        device = []
        for slot, (n, e) in enumerate(plan):
            if e is not None:
                device.append((e[0], e[1], slot, 0))
            elif self._last_plugin_route.get(n) == "device":
                p = pm.get_param_with_name(n)
                device.append((GRID_PLUGIN, plug.index(n), slot, (GRID_FILL_NAN if p.fill_nan else 0) | (GRID_ADD_Z if p.is_height_layer else 0)))
        return device

    def _grid_map_layers_locked(self, layers, out, order, normal_color):
        M = self.cell_n - 2
        plan = self._grid_plan(layers, normal_color)
        names = [n for n, _ in plan]
        if out is None:
            out = np.empty((len(names), M, M), np.float32)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.shape == (len(names), M, M)):
            raise ValueError("out must be a C-contiguous float32 array of shape (%d, %d, %d)" % (len(names), M, M))
        slot_of = {n: slot for slot, (n, _) in enumerate(plan)}

        def host_plane(n, m):                       # the layout on the host
            out[slot_of[n]][...] = m.T if order == "message" else m

        device = self._grid_plugins(plan, host_plane)
        if device:
            self._grid_launch(device, out, order)
        return names, out

    # ---- submap service (include/emap_hip.h: emap_publish_grid_windows) -------------------------------------------------------------------
    def _check_windows(self, windows):
        M = self.cell_n - 2
        wins = []
        for w in windows:
            i0, j0, ni, nj = (int(v) for v in w)
            if ni < 1 or nj < 1 or i0 < 0 or j0 < 0 or i0 + ni > M or j0 + nj > M:
                raise ValueError("window %r reaches outside the published map of %d x %d cells or is empty" % ((i0, j0, ni, nj), M, M))
            wins.append((i0, j0, ni, nj))
        return wins

    def _windows_launch(self, device, wins, buf, order):
        """``device``: ``(kind, index, flags)`` per layer (at most 32); ``buf``: flat float32 of the packed size.  ``GRID_MAX_WINDOWS`` windows
        per call: the packed runs of consecutive windows are adjacent, so a longer batch goes in groups.  The caller holds ``map_lock``."""
        table = (EmapGridLayerEx * len(device))()
        for k, (g, (kind, index, flags)) in enumerate(zip(table, device)):
            g.kind, g.index, g.slot, g.flags = kind, index, k, flags
        offsets, total = pack_windows(wins, len(device))
        offsets.append(total)
        for a in range(0, len(wins), GRID_MAX_WINDOWS):
            group = wins[a:a + GRID_MAX_WINDOWS]
            wt = (EmapGridWindow * len(group))()
            for g, (i0, j0, ni, nj) in zip(wt, group):
                g.i0, g.j0, g.ni, g.nj = i0, j0, ni, nj
            lo, hi = offsets[a], offsets[a + len(group)]
            self._chk(self._lib.emap_publish_grid_windows(self._ctx, table, len(device), GRID_ORDERS[order], ct.c_float(float(self.center[2])),
                                                          int(bool(self.param.use_only_above_for_upper_bound)), wt, len(group), f32p(buf[lo:hi]), hi - lo))

    @staticmethod
    def _window_views(buf, wins, n_layers, order):
        offsets, _ = pack_windows(wins, n_layers)
        return [buf[o:o + n_layers * ni * nj].reshape((n_layers, ni, nj) if order == "rows" else (n_layers, nj, ni))
                for o, (_, _, ni, nj) in zip(offsets, wins)]

    def _submap_layers_locked(self, wins, layers, out, order, normal_color):
        M = self.cell_n - 2
        resident = os.environ.get("EMAP_SUBMAP_RESIDENT", "1") != "0"
        plan = self._grid_plan(layers, normal_color)
        names = [n for n, _ in plan]
        L = len(names)
        _, total = pack_windows(wins, L)
        if out is None:
            out = np.empty(total, np.float32)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.ndim == 1 and out.size == total):
            raise ValueError("out must be a C-contiguous float32 array of %d elements (the packed windows)" % total)
        views = self._window_views(out, wins, L, order)
        self.last_submap_route = "device" if resident else "host"
        if not wins or not L:                       # nothing to answer: no plugin runs, nothing is launched
            return names, views

        def put(slot, full):                        # a whole published plane (rows order), sliced on the host
            for v, (i0, j0, ni, nj) in zip(views, wins):
                s = full[i0:i0 + ni, j0:j0 + nj]
                v[slot][...] = s.T if order == "message" else s

        if not resident:                            # A/B: the whole map through get_grid_map_layers, sliced on the host
            _, full = self._grid_map_layers_locked(layers, None, "rows", normal_color)
            for slot in range(L):
                put(slot, full[slot])
            return names, views
        slot_of = {n: slot for slot, (n, _) in enumerate(plan)}
        device = self._grid_plugins(plan, lambda n, m: put(slot_of[n], m))
        if not device:
            return names, views
        if len(device) == L and L <= GRID_MAX_LAYERS:      # every layer from the launch: the packed result IS the output
            self._windows_launch([(k, i, f) for k, i, _, f in device], wins, out, order)
            return names, views
        for a in range(0, len(device), GRID_MAX_LAYERS):   # host-route plugin layers in between, or more than 32 layers: planes are moved into place
            group = device[a:a + GRID_MAX_LAYERS]
            tmp = np.empty(pack_windows(wins, len(group))[1], np.float32)
            self._windows_launch([(k, i, f) for k, i, _, f in group], wins, tmp, order)
            for v, t in zip(views, self._window_views(tmp, wins, len(group), order)):
                for k, (_, _, slot, _) in enumerate(group):
                    v[slot][...] = t[k]
        return names, views

    def published_layers(self):
        """every layer name a GridMap of this map can carry: the six cell layers, the semantic layers and the plugin layers"""
        names = list(GRID_BUILTIN_LAYERS[:6])
        names += [n for n in (self.semantic_map.layer_names if self.semantic_map is not None else []) if n not in names]
        names += [n for n in (self.plugin_manager.layer_names if self.plugin_manager is not None else []) if n not in names]
        return names

    def get_submap_layers(self, windows, layers, out=None, order="rows", normal_color=False):
        """``get_grid_map_layers`` for a batch of WINDOWS of the published map: ``(names, [array per window])``.  ``windows``: ``(i0, j0, ni,
        nj)`` in the index space of ``get_map_with_name_ref`` (``submap_geometry`` makes them from metric requests); window ``w``'s array is
        float32 ``(len(names), ni, nj)`` -- ``get_grid_map_layers(order="rows")[1][:, i0:i0 + ni, j0:j0 + nj]``, bit for bit -- or, with
        ``order="message"``, ``(len(names), nj, ni)``: each plane's transpose stored C-contiguous.  All arrays are views into ONE flat
        buffer (``out``, or a new one), packed window after window.  Names are filtered, ordered and extended as there.

        One ``emap_publish_grid_windows`` call answers the batch (groups of 64 windows beyond 64): only the cells of the windows are read,
        and only the windows travel to the host.  Plugin layers are computed as in ``get_grid_map_layers`` over the whole map -- stencils
        need it -- ONCE per call: a device-capable plugin leaves a resident plane the window launch reads, a host-route plugin's plane is
        sliced on the host (``last_plugin_route``).  ``EMAP_SUBMAP_RESIDENT=0`` in the environment sends the call through
        ``get_grid_map_layers`` and host slices instead; ``last_submap_route`` tells which route ran.  One ``map_lock`` for the call."""
        if order not in GRID_ORDERS:
            raise ValueError("order must be 'rows' or 'message'")
        self._require_full_map("get_submap_layers")
        wins = self._check_windows(windows)
        with self.map_lock:
            return self._submap_layers_locked(wins, list(layers), out, order, normal_color)

    def get_submap_messages(self, requests, layers=None, basic_layers=None, frame_id="", stamp=None, normal_color=False, out=None):
        """The node's ``get_submap`` service (elevation_mapping_ros.cpp:507-553) for a batch of requests in the map frame: ``requests`` =
        ``(position_xy, length_xy)`` pairs; returns a list of ``(msg, success)``.  ``msg`` is the duck-typed ``GridMap`` of
        ``get_grid_map_message`` for the window ``submap_geometry`` gives: ``info.length_x / length_y`` = the window's sides, the pose at
        its centre, ``dim[0] = column_index (nj, ni * nj)``, ``dim[1] = row_index (ni, ni)``, start indices 0, ``msg.index_in_submap`` = the
        cell of the requested position; every ``data`` array of the call is a view into one buffer.  ``layers=None`` or empty: every
        layer the map publishes (``published_layers``: the service's ``request.layers.empty()`` branch).  A request the geometry answers
        with ``None`` -- its centre lies outside the map -- yields ``(a message without layers, False)`` and costs no device work; the
        others are still answered.  The geometry sees what the node's grid map holds: the float32 resolution widened to double, sides of
        ``(cell_n - 2)`` times that, the float32 centre.  A request in another frame is the caller's business (tf)."""
        self._require_full_map("get_submap_messages")
        layers = list(layers) if layers else self.published_layers()
        M = self.cell_n - 2
        res = float(np.float32(self.resolution))
        centre = (float(self.center[0]), float(self.center[1]))
        geo = [submap_geometry(centre, M * res, res, M, p, ln) for p, ln in requests]
        wins = [g[:4] for g in geo if g is not None]
        with self.map_lock:
            names, views = self._submap_layers_locked(wins, layers, out, "message", normal_color)
        basic_layers = _basic_layers(layers, basic_layers)
        answers, views = [], iter(views)
        for g in geo:
            header = types.SimpleNamespace(frame_id=str(frame_id), stamp=stamp, seq=0)
            if g is None:
                answers.append((_grid_map_envelope([], [], 0, 0, (0.0, 0.0), (0.0, 0.0), float(self.resolution), [], header, index_in_submap=None), False))
                continue
            _, _, ni, nj, sub_pos, sub_len, inside = g
            flat = next(views).reshape(len(names), ni * nj)
            answers.append((_grid_map_envelope(list(names), flat, ni, nj, sub_pos, sub_len, float(self.resolution), basic_layers, header,
                                               index_in_submap=inside), True))
        return answers

    def get_submap_message(self, position_xy, length_xy, layers=None, **keywords):
        """``get_submap_messages`` for one request: ``(msg, success)``"""
        return self.get_submap_messages([(position_xy, length_xy)], layers, **keywords)[0]

    # ---- point-cloud output (include/emap_hip.h: emap_publish_point_cloud) ----------------------------------------------------------------
    def _cell_positions(self):
        """what the node's grid map holds: the float32 resolution widened to double, the float32 centre"""
        return grid_cell_positions((float(self.center[0]), float(self.center[1])), float(np.float32(self.resolution)), self.cell_n - 2)

    @staticmethod
    def _cloud_buffer(out, M, point_step):
        """``(uint8 view, capacity in points)`` of the caller's buffer, or of a new one that holds every cell (untouched pages cost nothing)"""
        if out is None:
            return np.empty(M * M * point_step, np.uint8), M * M
        if not (isinstance(out, np.ndarray) and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"] and out.dtype in (np.uint8, np.float32)):
            raise ValueError("out must be a writeable C-contiguous uint8 or float32 array")
        buf = out.reshape(-1).view(np.uint8)
        return buf, buf.size // point_step

    def _cloud_device(self, table, n_dwords, xs, ys, call_flags, normal_min, buf, capacity):
        """one ``emap_publish_point_cloud`` call: ``table`` = ``(kind, index, flags, cloud_flags)`` per entry; returns the number of points.
        ``ValueError`` if ``buf`` is too small: it is left as it was.  The caller holds ``map_lock``."""
        t = (EmapCloudField * len(table))()
        for g, (kind, index, flags, cf) in zip(t, table):
            g.kind, g.index, g.flags, g.cloud_flags = int(kind), int(index), int(flags), int(cf)
        xs32, ys32 = np.ascontiguousarray(xs, np.float32), np.ascontiguousarray(ys, np.float32)
        n, step = ct.c_int64(-1), ct.c_int32(0)
        keep = buf if buf.size else np.empty(1, np.uint8)      # (a pointer the entry point accepts: nothing is written through it at capacity 0)
        rc = self._lib.emap_publish_point_cloud(self._ctx, t, len(t), ct.c_float(float(self.center[2])), int(bool(self.param.use_only_above_for_upper_bound)),
                                                f32p(xs32), f32p(ys32), ct.c_double(float(normal_min)), int(call_flags),
                                                keep.ctypes.data_as(ct.POINTER(ct.c_uint8)), int(capacity), ct.byref(n), ct.byref(step))
        if rc == -1 and n.value > capacity:
            raise ValueError("out holds %d points of %d bytes, the cloud has %d" % (capacity, 4 * n_dwords, n.value))
        self._chk(rc)
        assert step.value == 4 * n_dwords
        return int(n.value)

    def _cloud_host_planes(self, layers, normal_color):
        """the host route's planes: ``get_grid_map_layers(order="message")`` of ``layers`` as a dictionary.  The caller holds ``map_lock``."""
        names, planes = self._grid_map_layers_locked(layers, None, "message", normal_color)
        return dict(zip(names, planes))

    def _any_host_plugin(self, plan):
        return any(s[0] == "host" for s in self._plugin_steps(plan))

    def get_point_cloud_message(self, layers=("elevation",), point_layer="elevation", basic_layers=None, frame_id="", stamp=None, normal_color=False, out=None):
        """The node's ``elevation_map_points`` publisher (elevation_mapping_ros.cpp:501-505: ``GridMapRosConverter::toPointCloud``) without a
        host walk of the map: a duck-typed ``sensor_msgs/PointCloud2`` (``types.SimpleNamespace``, no ROS import) of the VALID cells of the
        published map, in grid_map's iterator order (``lin = j * M + i``: the flat order of ``get_grid_map_layers(order="message")``).  A cell
        is skipped if a basic layer or the point layer is not finite there.  ``fields``, ``point_step``: ``point_cloud_descriptor``; ``height``
        1, ``width`` = the number of points, ``row_step = width * point_step``, ``is_dense`` and ``is_bigendian`` False; ``data`` is a uint8 view
        of exactly ``row_step`` bytes into ``out`` (uint8 or float32, C-contiguous) or a new buffer.  Positions: ``grid_cell_positions`` of
        the float32 resolution and centre, computed in double and rounded to float32; ``z`` is the point layer's float.  grid_map is
        RESTATED here, not pinned by a compiled reference.

        ``layers`` are filtered, ordered and extended as in ``get_grid_map_layers`` (``normal_color``: the normals and ``color``, whose field
        is ``rgb``).  ``basic_layers=None``: the wrapper's rule, ``["elevation"]`` if it was asked for; a basic layer outside ``layers`` is
        tested and not emitted; one the map does not hold is dropped like a layer.  ``ValueError``: ``point_layer`` not in the kept layers (a
        decision: grid_map would emit a cloud without coordinates), an ``out`` that is too small (it is left untouched).

        One ``emap_publish_point_cloud`` call packs the records on the device: three launches, a 4-byte copy of the count, then exactly
        ``row_step`` bytes.  Device-capable plugin layers run in the chain and are read as resident planes; if any layer takes a plugin's
        host route, or the table exceeds 32 entries, or ``EMAP_CLOUD_RESIDENT=0`` is in the environment, the whole call takes the host route:
        ``get_grid_map_layers(order="message")`` and a NumPy compaction, the same bits.  ``last_point_cloud_route`` tells which ran.  One
        ``map_lock`` for the call."""
        self._require_full_map("get_point_cloud_message")
        layers = list(layers)
        basic_layers = _basic_layers(layers, basic_layers)
        M = self.cell_n - 2
        xs, ys = self._cell_positions()
        with self.map_lock:
            asked = layers + [b for b in basic_layers if b not in layers]
            plan = self._grid_plan(asked, normal_color)
            hidden = [n for n, _ in plan if n not in layers and not (normal_color and n in GRID_NORMAL_COLOR_LAYERS)]
            names = [n for n, _ in plan if n not in hidden]
            if point_layer not in names:
                raise ValueError("point_layer %r is not one of the layers %s of this map" % (point_layer, names))
            fields, point_step = point_cloud_descriptor(names, point_layer)
            tested = [n for n, _ in plan if n in basic_layers or n == point_layer]
            buf, capacity = self._cloud_buffer(out, M, point_step)
            resident = os.environ.get("EMAP_CLOUD_RESIDENT", "1") != "0" and len(plan) <= GRID_MAX_LAYERS and not self._any_host_plugin(plan)
            self.last_point_cloud_route = "device" if resident else "host"
            if resident:
                device = self._grid_plugins(plan, None)      # (no host step: checked above)
                table = [(kind, index, flags, (CLOUD_POINT if plan[slot][0] == point_layer else 0) | (CLOUD_TEST if plan[slot][0] in tested else 0)
                          | (CLOUD_HIDDEN if plan[slot][0] in hidden else 0)) for kind, index, slot, flags in device]
                n = self._cloud_device(table, point_step // 4, xs, ys, 0, 0.0, buf, capacity)
            else:
                rec = _cloud_compact(self._cloud_host_planes(asked, normal_color), names, point_layer, tested, xs.astype(np.float32), ys.astype(np.float32))
                n = rec.shape[0]
                if n > capacity:
                    raise ValueError("out holds %d points of %d bytes, the cloud has %d" % (capacity, point_step, n))
                buf[:n * point_step] = rec.reshape(-1).view(np.uint8)
        ns = types.SimpleNamespace
        return ns(header=ns(frame_id=str(frame_id), stamp=stamp, seq=0), height=1, width=n, fields=fields, is_bigendian=False, point_step=point_step,
                  row_step=n * point_step, data=buf[:n * point_step], is_dense=False)

    def get_point_cloud(self, layers=("elevation",), point_layer="elevation", basic_layers=None, normal_color=False, out=None):
        """``get_point_cloud_message`` as ``(field_names, array)``: ``array`` float32 ``(n, len(field_names))``, a view into the message's
        ``data`` (a colour field holds bit patterns)"""
        msg = self.get_point_cloud_message(layers, point_layer, basic_layers, normal_color=normal_color, out=out)
        names = [f.name for f in msg.fields]
        return names, msg.data.view(np.float32).reshape(msg.width, len(names))

    def get_normal_arrows(self, scale=0.1, min_norm=0.1):
        """The node's ``normal`` publisher (elevation_mapping_ros.cpp:751-809) without a host walk: one arrow per cell, in iterator order,
        whose elevation is finite and whose normal is not shorter than ``min_norm`` (``sqrt((nx nx + ny ny) + nz nz) < min_norm`` in double
        skips; a NaN normal is not skipped).  Returns a namespace: ``ids (n,) int32`` -- the cell's linear index ``j * M + i``, the marker
        id --, ``starts (n, 3) float64`` -- the double position ``(x(i), y(j), (double) z)``, not rounded to float -- and ``ends = starts +
        normal * scale``, unfused.  ONE ``emap_publish_point_cloud`` call with the fields elevation (the point layer), ``normal_x``,
        ``normal_y``, ``normal_z`` and the cell index; the double positions are recomputed here from the ids.  ``EMAP_CLOUD_RESIDENT=0``: the
        host route.  ``normal_arrow_markers`` makes the ``MarkerArray``.  ``ValueError``: a ``scale`` or ``min_norm`` that is not finite."""
        self._require_full_map("get_normal_arrows")
        scale, min_norm = float(scale), float(min_norm)
        if not (np.isfinite(scale) and np.isfinite(min_norm)):
            raise ValueError("scale and min_norm must be finite")
        M = self.cell_n - 2
        xs, ys = self._cell_positions()
        normals = ["normal_x", "normal_y", "normal_z"]
        with self.map_lock:
            resident = os.environ.get("EMAP_CLOUD_RESIDENT", "1") != "0"
            self.last_point_cloud_route = "device" if resident else "host"
            if resident:
                table = [(GRID_BUILTIN, 0, 0, CLOUD_POINT)] + [(GRID_BUILTIN, GRID_BUILTIN_LAYERS.index(n), 0, 0) for n in normals]
                buf = np.empty(M * M * 28, np.uint8)
                n = self._cloud_device(table, 7, xs, ys, CLOUD_NORMAL_MIN | CLOUD_INDEX, min_norm, buf, M * M)
                rec = buf[:n * 28].view(np.float32).reshape(n, 7)
            else:
                planes = self._cloud_host_planes(["elevation"], True)      # elevation, the normals (and their colour, not used)
                rec = _cloud_compact(planes, ["elevation"] + normals, "elevation", ["elevation"], xs.astype(np.float32), ys.astype(np.float32),
                                     index=True, normals=normals, normal_min=min_norm)
        ids = rec.view(np.int32)[:, 6].copy()
        starts = np.stack([xs[ids % M], ys[ids // M], rec[:, 2].astype(np.float64)], axis=1)
        ends = starts + rec[:, 3:6].astype(np.float64) * scale
        return types.SimpleNamespace(ids=ids, starts=starts, ends=ends)

    # ---- plane segmentation (include/emap_hip.h: emap_plane_segmentation) -----------------------------------------------------------------
    def get_plane_segmentation(self, layer="elevation", *, kernel_size=3, planarity_opening_filter=0, plane_inclination_threshold_degrees=30.0,
                               local_plane_inclination_threshold_degrees=35.0, plane_patch_error_threshold=0.02, min_number_points_per_label=4,
                               connectivity=4, global_plane_fit_distance_error_threshold=0.025, global_plane_fit_angle_error_threshold_degrees=25.0,
                               normals=False, out=None):
        """The front of convex_plane_decomposition (SlidingWindowPlaneExtractor::runExtraction without RANSAC) on one published layer, without
        the map leaving the device: a plane fitted to the ``kernel_size``^2 window of every cell, planar cells, optionally an opening,
        connected labels, one plane per label (DESIGN.md section 21 holds the contract).  The keywords are the reference's
        ``parameters.yaml`` names and defaults.  Returns a namespace: ``labels`` int32 ``(M, M)`` in the index space of
        ``get_grid_map_layers(order="rows")``, 0 = background (``out``: an array of that kind to fill); ``n_labels``; ``planes``: a structured
        array (``label``, ``n_points``, ``needs_refinement``, ``n_left_out``, ``support`` and ``normal`` 3 x float64, map frame) with one
        row per label that has a plane, ascending; ``normals`` float32 ``(3, M, M)`` with ``normals=True``, else ``None``; ``origin_xy`` (the
        position of cell (0, 0)) and ``resolution``: cell ``(i, j)`` lies at ``origin_xy - (i, j) * resolution``.

        ``layer``: a map layer, a semantic layer or a plugin layer, as ``get_grid_map_layers`` publishes it; a plugin layer runs through the
        plugin chain first and is read as a resident plane -- one that takes its host route is refused (``ValueError``), not downloaded and
        uploaded again.  ``EMAP_PLANES_RESIDENT=0`` in the environment: the whole layer is downloaded and segmented by the host model
        (``plane_segmentation.segment``), the same answer; ``last_plane_segmentation_route`` tells which ran."""
        from . import plane_segmentation as host_model
        self._require_full_map("get_plane_segmentation")
        keywords, angles, lengths = self._plane_keywords(kernel_size, planarity_opening_filter, plane_inclination_threshold_degrees, local_plane_inclination_threshold_degrees,
                                                         plane_patch_error_threshold, min_number_points_per_label, connectivity, global_plane_fit_distance_error_threshold,
                                                         global_plane_fit_angle_error_threshold_degrees)
        kernel_size, opening, min_points, connectivity = (keywords[k] for k in ("kernel_size", "planarity_opening_filter", "min_number_points_per_label", "connectivity"))
        M = self.cell_n - 2
        if out is None:
            out = np.empty((M, M), np.int32)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.int32 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"] and out.shape == (M, M)):
            raise ValueError("out must be a writeable C-contiguous int32 array of shape (%d, %d)" % (M, M))
        xs, ys = self._cell_positions()
        origin, res = (float(xs[0]), float(ys[0])), float(np.float32(self.resolution))
        with self.map_lock:
            plan = self._grid_plan([layer], False)
            if len(plan) != 1:
                raise ValueError("layer %r is not a layer this map publishes" % (layer,))
            resident = os.environ.get("EMAP_PLANES_RESIDENT", "1") != "0"
            self.last_plane_segmentation_route = "device" if resident else "host"
            if not resident:
                _, planes = self._grid_map_layers_locked([layer], None, "rows", False)
                r = host_model.segment(planes[0], res, origin, **keywords)
                out[...] = r.labels
                return types.SimpleNamespace(labels=out, n_labels=r.n_labels, planes=r.planes, normals=r.normals if normals else None, origin_xy=origin, resolution=res)
            if self._any_host_plugin(plan):
                raise ValueError("plugin layer %r takes its host route: it is not resident on the device (get_grid_map_layers computes it on the host)" % (layer,))
            kind, index, _, flags = self._grid_plugins(plan, None)[0]
            src = EmapGridLayerEx(int(kind), int(index), 0, int(flags))
            cos_plane, cos_local, cos_angle = host_model.cosines(*angles)
            P = _lib.EmapPlaneParams(kernel_size, opening, min_points, connectivity, int(bool(self.param.use_only_above_for_upper_bound)), 0, float(self.center[2]), 0.0,
                                     res, origin[0], origin[1], lengths[0], cos_local, cos_plane, lengths[1], cos_angle)
            nrm = np.empty((3, M, M), np.float32) if normals else None
            capacity = 256
            while True:                                 # (a second trip only when more than `capacity` labels have a plane)
                planes = np.zeros(capacity, _lib.PLANE_RECORD_DTYPE)
                n_labels, n_planes = ct.c_int32(0), ct.c_int64(0)
                rc = self._lib.emap_plane_segmentation(self._ctx, ct.byref(src), ct.byref(P), out.ctypes.data_as(ct.POINTER(ct.c_int32)), f32p(nrm) if normals else None,
                                                       planes.ctypes.data_as(ct.POINTER(_lib.EmapPlaneRecord)), capacity, ct.byref(n_labels), ct.byref(n_planes))
                if rc == -1 and n_planes.value > capacity:
                    capacity = int(n_planes.value)
                    continue
                self._chk(rc)
                break
        return types.SimpleNamespace(labels=out, n_labels=int(n_labels.value), planes=planes[:n_planes.value], normals=nrm, origin_xy=origin, resolution=res)

    @staticmethod
    def _plane_keywords(kernel_size, planarity_opening_filter, plane_inclination_threshold_degrees, local_plane_inclination_threshold_degrees, plane_patch_error_threshold,
                        min_number_points_per_label, connectivity, global_plane_fit_distance_error_threshold, global_plane_fit_angle_error_threshold_degrees):
        """the segmentation's keywords, converted and checked: ``(keywords for the host model, the three angles, the two lengths)``"""
        kernel_size, opening, min_points, connectivity = int(kernel_size), int(planarity_opening_filter), int(min_number_points_per_label), int(connectivity)
        if kernel_size not in (3, 5, 7) or connectivity not in (4, 8) or not 0 <= opening <= _lib.PLANE_OPEN_MAX or min_points < 0:
            raise ValueError("kernel_size is 3, 5 or 7, connectivity 4 or 8, planarity_opening_filter 0 .. %d, min_number_points_per_label not negative" % _lib.PLANE_OPEN_MAX)
        angles = [float(a) for a in (plane_inclination_threshold_degrees, local_plane_inclination_threshold_degrees, global_plane_fit_angle_error_threshold_degrees)]
        lengths = [float(plane_patch_error_threshold), float(global_plane_fit_distance_error_threshold)]
        if not all(np.isfinite(v) and v > 0.0 for v in angles + lengths) or any(a > 180.0 for a in angles):
            raise ValueError("thresholds must be positive and finite (angles in degrees, at most 180)")
        keywords = dict(kernel_size=kernel_size, planarity_opening_filter=opening, plane_inclination_threshold_degrees=angles[0],
                        local_plane_inclination_threshold_degrees=angles[1], plane_patch_error_threshold=lengths[0], min_number_points_per_label=min_points,
                        connectivity=connectivity, global_plane_fit_distance_error_threshold=lengths[1], global_plane_fit_angle_error_threshold_degrees=angles[2])
        return keywords, angles, lengths

    # ---- planar terrain (include/emap_hip.h: emap_planar_terrain) --------------------------------------------------------------------------
    def get_planar_terrain(self, layer="elevation", *, preprocess=None, postprocess=None, intermediates=False, normals=False, kernel_size=3,
                           planarity_opening_filter=0, plane_inclination_threshold_degrees=30.0, local_plane_inclination_threshold_degrees=35.0,
                           plane_patch_error_threshold=0.02, min_number_points_per_label=4, connectivity=4, global_plane_fit_distance_error_threshold=0.025,
                           global_plane_fit_angle_error_threshold_degrees=25.0, _locked=False):
        """What convex_plane_decomposition publishes around ``get_plane_segmentation``, without the map leaving the device (DESIGN.md
        section 22 holds the contract): optionally the preprocessing of the layer (``preprocess``: a dict with the reference's
        ``kernelSize`` -- 3 --, ``numberOfRepeats`` -- 1 -- and optionally ``resolution``, which must be the map's; ``{}`` is the reference's
        defaults, ``None`` runs neither the minValues inpainting nor the median), the segmentation of that plane with the keywords of
        ``get_plane_segmentation``, and ``Postprocessing::postprocess`` (``postprocess``: a dict with the keys and defaults of
        Postprocessing.h:7-25; ``None``: the defaults).  Returns ``get_plane_segmentation``'s namespace (``support[2]`` of the planes raised by
        ``extracted_planes_height_offset``) plus float32 ``(M, M)`` planes: ``elevation`` (non-planar cells dilated, everything lifted),
        ``smooth_planar``, ``plane_classification`` (1.0 / 0.0) and ``elevation_before_postprocess``; with ``intermediates=True`` also the
        reference's helper layers ``elevationWithNaN``, ``elevationWithNaN_i``, ``elevationWithNaNClosed`` and
        ``elevationWithNaNClosedDilated``.  Only the planes asked for are copied back.

        ``layer`` as in ``get_plane_segmentation`` (a plugin layer that takes its host route is refused).  ``EMAP_TERRAIN_RESIDENT=0`` in
        the environment: the layer is downloaded and everything is computed by the host model (``planar_terrain.terrain``), the same
        answer; ``last_planar_terrain_route`` tells which ran.  (``_locked``: the caller holds ``map_lock`` -- ``get_planar_regions``.)"""
        from . import plane_segmentation as seg_model
        from . import planar_terrain as host_model
        self._require_full_map("get_planar_terrain")
        keywords, angles, lengths = self._plane_keywords(kernel_size, planarity_opening_filter, plane_inclination_threshold_degrees, local_plane_inclination_threshold_degrees,
                                                         plane_patch_error_threshold, min_number_points_per_label, connectivity, global_plane_fit_distance_error_threshold,
                                                         global_plane_fit_angle_error_threshold_degrees)
        M = self.cell_n - 2
        xs, ys = self._cell_positions()
        origin, res = (float(xs[0]), float(ys[0])), float(np.float32(self.resolution))
        pre, post, _ = host_model.check(M, res, preprocess, postprocess)
        names = host_model.PLANES[:8 if intermediates else 4]
        with (contextlib.nullcontext() if _locked else self.map_lock):
            plan = self._grid_plan([layer], False)
            if len(plan) != 1:
                raise ValueError("layer %r is not a layer this map publishes" % (layer,))
            resident = os.environ.get("EMAP_TERRAIN_RESIDENT", "1") != "0"
            self.last_planar_terrain_route = "device" if resident else "host"
            if not resident:
                _, planes = self._grid_map_layers_locked([layer], None, "rows", False)
                r = host_model.terrain(planes[0], res, origin, preprocess, post, **keywords)
                out = types.SimpleNamespace(labels=r.labels, n_labels=r.n_labels, planes=r.planes, normals=r.normals if normals else None, origin_xy=origin, resolution=res)
                for n in names:
                    setattr(out, n, getattr(r, n))
                return out
            if self._any_host_plugin(plan):
                raise ValueError("plugin layer %r takes its host route: it is not resident on the device (get_grid_map_layers computes it on the host)" % (layer,))
            kind, index, _, flags = self._grid_plugins(plan, None)[0]
            src = EmapGridLayerEx(int(kind), int(index), 0, int(flags))
            cos_plane, cos_local, cos_angle = seg_model.cosines(*angles)
            P = _lib.EmapPlaneParams(keywords["kernel_size"], keywords["planarity_opening_filter"], keywords["min_number_points_per_label"], keywords["connectivity"],
                                     int(bool(self.param.use_only_above_for_upper_bound)), 0, float(self.center[2]), 0.0,
                                     res, origin[0], origin[1], lengths[0], cos_local, cos_plane, lengths[1], cos_angle)
            Q = _lib.EmapTerrainParams(0 if pre is None else 1, 1 if pre is None else pre[0], 0 if pre is None else pre[1], post["nonplanar_horizontal_offset"],
                                       (1 << len(names)) - 1, 0, post["smoothing_dilation_size"], post["smoothing_box_kernel_size"], post["smoothing_gauss_kernel_size"],
                                       post["extracted_planes_height_offset"], post["nonplanar_height_offset"])
            labels = np.empty((M, M), np.int32)
            got = {n: np.empty((M, M), np.float32) for n in names}
            O = _lib.EmapTerrainPlanes()
            for k, n in enumerate(names):
                O.plane[k] = f32p(got[n])
            nrm = np.empty((3, M, M), np.float32) if normals else None
            capacity = 256
            while True:                                 # (a second trip only when more than `capacity` labels have a plane)
                planes = np.zeros(capacity, _lib.PLANE_RECORD_DTYPE)
                n_labels, n_planes = ct.c_int32(0), ct.c_int64(0)
                rc = self._lib.emap_planar_terrain(self._ctx, ct.byref(src), ct.byref(P), ct.byref(Q), labels.ctypes.data_as(ct.POINTER(ct.c_int32)), f32p(nrm) if normals else None,
                                                   planes.ctypes.data_as(ct.POINTER(_lib.EmapPlaneRecord)), capacity, ct.byref(n_labels), ct.byref(n_planes), ct.byref(O))
                if rc == -1 and n_planes.value > capacity:
                    capacity = int(n_planes.value)
                    continue
                self._chk(rc)
                break
        return types.SimpleNamespace(labels=labels, n_labels=int(n_labels.value), planes=planes[:n_planes.value], normals=nrm, origin_xy=origin, resolution=res, **got)

    # ---- planar regions (include/emap_hip.h: emap_planar_regions) --------------------------------------------------------------------------
    def get_planar_regions(self, layer="elevation", *, margin_size=1, **terrain_keywords):
        """``get_planar_terrain`` and, behind it under the same lock, the contour stage of convex_plane_decomposition
        (``ContourExtraction::extractPlanarRegions``) on the labels it left on the device (DESIGN.md section 23 holds the contract): per
        connected piece of a label a boundary polygon with holes and its inset polygons, traced on the x 3 upsampled label image after an
        erosion by ``margin_size`` (the reference's ``marginSize``, 0 .. 14).  ``terrain_keywords``: the keywords of ``get_planar_terrain``.
        Returns that call's namespace plus ``rings`` (a structured array, ``planar_regions.RING_DTYPE``), ``vertices`` int32 ``(n, 2)``
        (x = column, y = row of the upsampled image) and ``regions``: a list in ascending (label, first pixel), each a namespace of
        ``label``, ``plane`` (the label's record), ``transform_plane_to_world`` (4 x 4 float64), ``boundary`` and ``insets`` (a polygon is
        a dict of ``outer`` / ``holes`` in pixels and ``outer_plane`` / ``holes_plane`` in plane coordinates, float64) and ``bbox2d``.

        ``EMAP_REGIONS_RESIDENT=0`` in the environment: the contour stage runs in the host model (``planar_regions.regions``) on the labels
        the terrain call returned, the same answer; ``last_planar_regions_route`` tells which ran."""
        from . import planar_regions as host_model
        margin_size = int(margin_size)
        if not 0 <= margin_size <= _lib.REGION_MARGIN_MAX:
            raise ValueError("margin_size must lie in 0 .. %d" % _lib.REGION_MARGIN_MAX)
        with self.map_lock:
            r = self.get_planar_terrain(layer, _locked=True, **terrain_keywords)
            resident = os.environ.get("EMAP_REGIONS_RESIDENT", "1") != "0"
            self.last_planar_regions_route = "device" if resident else "host"
            if resident and self.last_planar_terrain_route == "device":
                r.rings, r.vertices = self._planar_regions_call(None, 0, 0, 0, margin_size)
            elif resident:                              # the terrain took its host route: its labels are the caller's
                r.rings, r.vertices = self._planar_regions_call(r.labels, r.labels.shape[0], r.n_labels, 0, margin_size)
            else:
                t = host_model.trace_labels(r.labels, r.n_labels, margin_size, 0)
                r.rings, r.vertices = t.rings, t.vertices
        r.regions = host_model.build_regions(r.rings, r.vertices, r.planes, r.resolution, r.origin_xy)
        return r

    def trace_mask(self, mask):
        """The borders of a 0 / 1 mask at its own resolution, traced on the device as ``get_planar_regions`` traces its label images (the
        raw mode of ``emap_planar_regions``): image 0 is the mask, image 1 its erosion by the 3 x 3 cross with the outer rows and columns
        zeroed.  ``mask``: a square integer or bool array of at least 2 x 2.  Returns a namespace of ``rings`` and ``vertices`` as
        ``get_planar_regions`` and ``polygons``: ``planar_regions.assemble`` of them."""
        from . import planar_regions as host_model
        self._require_full_map("trace_mask")
        m = np.ascontiguousarray(mask, np.int32)
        host_model.check_labels(m, 1, 0, 1)
        with self.map_lock:
            resident = os.environ.get("EMAP_REGIONS_RESIDENT", "1") != "0"
            self.last_planar_regions_route = "device" if resident else "host"
            if resident:
                rings, vertices = self._planar_regions_call(m, m.shape[0], 1, 1, 0)
            else:
                t = host_model.trace_labels(m, 1, 0, 1)
                rings, vertices = t.rings, t.vertices
        return types.SimpleNamespace(rings=rings, vertices=vertices, polygons=host_model.assemble(rings, vertices))

    def _planar_regions_call(self, labels, side, n_labels, mode, margin_size):
        """``emap_planar_regions`` with buffers that fit: ``(rings, vertices)``; ``labels`` None: the resident labels"""
        from . import planar_regions as host_model
        self._require_full_map("get_planar_regions")
        P = _lib.EmapRegionParams(int(mode), int(margin_size))
        cap_r, cap_v = 256, 4096
        while True:                                     # (a second trip only when the answer is larger than the buffers)
            rings, verts = np.zeros(cap_r, host_model.RING_DTYPE), np.zeros((cap_v, 2), np.int32)
            n_r, n_v = ct.c_int64(0), ct.c_int64(0)
            rc = self._lib.emap_planar_regions(self._ctx, None if labels is None else labels.ctypes.data_as(ct.POINTER(ct.c_int32)), int(side), int(n_labels), ct.byref(P),
                                               rings.ctypes.data_as(ct.POINTER(_lib.EmapRegionRing)), cap_r, verts.ctypes.data_as(ct.POINTER(ct.c_int32)), cap_v,
                                               ct.byref(n_r), ct.byref(n_v))
            if rc == -1 and (n_r.value > cap_r or n_v.value > cap_v):
                cap_r, cap_v = max(cap_r, int(n_r.value)), max(cap_v, int(n_v.value))
                continue
            self._chk(rc)
            break
        return rings[:n_r.value].copy(), verts[:n_v.value].copy()

    def get_grid_map_message(self, layers, basic_layers=None, frame_id="", stamp=None, normal_color=False, out=None):
        """A duck-typed ``grid_map_msgs/GridMap`` of ``layers`` (``types.SimpleNamespace``, no ROS import): ``info.resolution``,
        ``info.length_x = info.length_y = map_length``, ``info.pose`` at ``(center_x, center_y, 0)`` with the identity orientation, the header
        both as ``msg.header`` (ROS 2) and ``msg.info.header`` (ROS 1), ``layers``, ``basic_layers`` (``None``: the wrapper's rule, ``["elevation"]``
        if it was asked for), and per layer a ``Float32MultiArray`` whose ``data`` is a float32 VIEW into one contiguous buffer filled by
        ``get_grid_map_layers(order="message")``: column-major, ``dim[0] = column_index (M, M * M)``, ``dim[1] = row_index (M, M)``.  ``out``: a
        buffer of the caller's to fill instead of a new one (a publisher that keeps its buffer between ticks), as in ``get_grid_map_layers``."""
        layers = list(layers)
        names, buf = self.get_grid_map_layers(layers, out=out, order="message", normal_color=normal_color)
        M = self.cell_n - 2
        header = types.SimpleNamespace(frame_id=str(frame_id), stamp=stamp, seq=0)
        return _grid_map_envelope(names, buf.reshape(len(names), M * M), M, M, (float(self.center[0]), float(self.center[1])),
                                  (float(self.map_length), float(self.map_length)), float(self.resolution), _basic_layers(layers, basic_layers), header)

    def _require_full_map(self, what):
        if self._strip is not None:
            raise EmapError("%s works on a full map; this context holds the row strip [%d, %d) -- gather the strips first "
                            "(ShardedElevationMap.gather(name) assembles the full plane on every rank)" % (what, self.row_begin, self.row_begin + self.rows))

    def _stripped_layer(self, name):
        """border-stripped, unflipped layer as the reference's get_* accessors return it (:598-680, :740-765)"""
        self._require_full_map("layer read-back (%s)" % name)
        if name == "elevation":
            return self._publish(self.get_layer_raw(0), True, True, self.get_layer_raw(2))
        if name == "variance":
            return self._publish(self.get_layer_raw(1))
        if name == "traversability":
            trav = np.where((self.get_layer_raw(2) + self.get_layer_raw(6)) > 0.5, self.get_layer_raw(3), np.nan)
            self.traversability_buffer[3:-3, 3:-3] = trav[3:-3, 3:-3]
            return self.traversability_buffer[1:-1, 1:-1]
        if name == "time":
            return self._publish(self.get_layer_raw(4))
        if name in ("upper_bound", "is_upper_bound"):
            e = self.elevation_map
            if self.param.use_only_above_for_upper_bound:
                valid = np.logical_or(np.logical_and(e[5] > 0.0, e[6] > 0.5), e[2] > 0.5)
            else:
                valid = np.logical_or(e[2] > 0.5, e[6] > 0.5)
            if name == "upper_bound":
                return np.where(valid, e[5], np.nan)[1:-1, 1:-1] + self.center[2]
            return np.where(valid, e[6], np.nan)[1:-1, 1:-1]
        if name in ("normal_x", "normal_y", "normal_z"):
            return self.get_layer_raw(name)[1:-1, 1:-1]
        if self.semantic_map is not None and name in self.semantic_map.layer_names:
            return self.semantic_map.get_map_with_name(name)
        if self.plugin_manager is not None and name in self.plugin_manager.layer_names:
            self._plugin_host_step(name)
            m = self.plugin_manager.host_layer(name)
            p = self.plugin_manager.get_param_with_name(name)
            return self._publish(np.asarray(m), p.fill_nan, p.is_height_layer, self.get_layer_raw(2))
        return None

    # the reference's per-layer accessors (:598-680): host arrays, border stripped, NOT flipped
    def process_map_for_publish(self, input_map, fill_nan=False, add_z=False, xp=np):
        return self._publish(np.asarray(input_map), fill_nan, add_z, self.get_layer_raw(2) if fill_nan else None)

    def get_elevation(self):
        return self._stripped_layer("elevation")

    def get_variance(self):
        return self._stripped_layer("variance")

    def get_traversability(self):
        return self._stripped_layer("traversability")

    def get_time(self):
        return self._stripped_layer("time")

    def get_upper_bound(self):
        return self._stripped_layer("upper_bound")

    def get_is_upper_bound(self):
        return self._stripped_layer("is_upper_bound")

    def get_normal_maps(self):
        """(3, C-2, C-2), flipped on both axes like the reference (:776-790)"""
        n = self.normal_map[:, 1:-1, 1:-1]
        return np.ascontiguousarray(np.flip(np.flip(n, 1), 2))

    def xp_of_array(self, array):
        return np if isinstance(array, np.ndarray) else None

    def copy_to_cpu(self, array, data, stream=None):
        data[...] = np.asarray(array).astype(np.float32)

    # ---- safety-polygon service (reference :837-897) ---------------------------------------------------------
    def polygon_mask(self, polygon):
        """(cell_n, cell_n) 0/1 mask of the cells inside ``polygon`` ((M, 2) world coordinates, already clipped): the device
        kernel behind get_polygon_traversability (polygon_mask_kernel, custom_kernels.py:509-651)."""
        poly = np.ascontiguousarray(polygon, np.float32)
        mask = np.empty((self.cell_n, self.cell_n), np.float32)
        self._chk(self._lib.emap_polygon_mask(self._ctx, f32p(poly), int(poly.shape[0]), ct.c_float(float(self.center[0])),
                                              ct.c_float(float(self.center[1])), f32p(mask)))
        return mask

    @property
    def mask(self):
        """``(cell_n, cell_n)`` 0/1 mask of the last polygon a safety check clipped (the reference's ``self.mask``).  The device route
        builds no mask: it is computed here, by ``polygon_mask``, when someone looks at it."""
        if self._mask is None and self._mask_polygon is not None:
            with self.map_lock:
                self._mask = self.polygon_mask(self._mask_polygon)
        return self._mask

    @mask.setter
    def mask(self, value):
        self._mask, self._mask_polygon = value, None

    def _clip_polygon(self, poly):
        reach = self.map_length / 2 - self.resolution                  # the polygon is clipped to the map interior (:851-855)
        return np.clip(poly.astype(np.float32), self.center[:2] - reach, self.center[:2] + reach).astype(np.float32)

    def _polygon_checker(self, name):
        """``(kind, index)`` of the checker layer ``name`` where it lies on the device -- a raw map layer, a semantic layer, or a plugin
        layer that an op of the plugin chain computes into its resident plane now (``plugin_chain_plan`` / ``run_plan``, as
        ``get_grid_map_layers``) -- or None: the host route.  The caller holds ``map_lock``."""
        if os.environ.get("EMAP_POLYGON_RESIDENT", "1") == "0":
            return None
        if name in self.layer_names:
            return POLY_MAP_LAYER, self.layer_names.index(name)
        sem = self.semantic_map.layer_names if self.semantic_map is not None else []
        if name in sem:
            return POLY_SEMANTIC, sem.index(name)
        pm = self.plugin_manager
        if pm is not None and name in pm.layer_names:
            steps = plugin_chain_plan([name], pm.plugins, pm.layer_names, self.layer_names, sem,
                                      resident=os.environ.get("EMAP_PLUGIN_RESIDENT", "1") != "0")
            if steps and steps[0][0] == "device":
                pm.run_plan(steps, None, self.base_rotation)
                return POLY_PLUGIN, pm.layer_names.index(name)
        return None

    def _polygons_device(self, clipped, src):
        """one ``emap_polygon_safety`` call for the clipped polygons (at most ``POLY_MAX_BATCH``): the verdict records and, per polygon,
        the risky cells at the ends of each row as (n, 2) indices of the border-stripped view.  The caller holds ``map_lock``."""
        n = len(clipped)
        begin = np.zeros(n + 1, np.int32)
        begin[1:] = np.cumsum([c.shape[0] for c in clipped])
        xy = np.ascontiguousarray(np.concatenate(clipped, axis=0), np.float32)
        rows = self.cell_n - 2
        ext_begin = np.arange(n + 1, dtype=np.int64) * rows
        ext = np.empty((n * rows, 2), np.int32)                         # (room for every row of the map: only a polygon's own rows are written)
        verdicts = (EmapPolygonVerdict * n)()
        thr = np.float32(1.0 - self.param.safe_thresh)                  # what the host route's float32 plane is compared with
        self._chk(self._lib.emap_polygon_safety(
            self._ctx, f32p(xy), begin.ctypes.data_as(ct.POINTER(ct.c_int32)), n, ct.c_float(float(self.center[0])), ct.c_float(float(self.center[1])),
            int(src[0]), int(src[1]), ct.c_float(float(thr)), verdicts, ext.ctypes.data_as(ct.POINTER(ct.c_int32)),
            ext_begin.ctypes.data_as(ct.POINTER(ct.c_int64))))
        cells = []
        for k, v in enumerate(verdicts):
            e = ext[k * rows:k * rows + v.n_rows]
            q = np.nonzero(e[:, 1] >= 0)[0]
            r = q + (v.row_begin - 1)
            lo, hi = e[q, 0] - 1, e[q, 1] - 1
            two = hi > lo
            cells.append(np.concatenate([np.stack([r, lo], 1), np.stack([r[two], hi[two]], 1)]).astype(np.int64))
        return verdicts, cells

    _VERDICT = np.dtype([("is_safe", np.bool_), ("mean_risk", np.float64), ("area", np.float64), ("n_inside", np.int64), ("n_known", np.float64),
                         ("n_risky", np.int64), ("max_risk", np.float32)])

    def _polygons_on_device(self, polys, name):
        """``(verdicts, rings)`` of ``get_polygons_traversability`` by the device route, or None when the batch has to take the host route"""
        if not all(p.ndim == 2 and p.shape[1] == 2 and 1 <= p.shape[0] <= POLY_MAX_VERTS for p in polys):
            return None
        clipped = [self._clip_polygon(p) for p in polys]
        with self.map_lock:
            src = self._polygon_checker(name)
            if src is None:
                return None
            verdicts, cells = [], []
            for a in range(0, len(polys), POLY_MAX_BATCH):
                v, c = self._polygons_device(clipped[a:a + POLY_MAX_BATCH], src)
                verdicts += list(v); cells += c
        out, rings = np.zeros(len(polys), self._VERDICT), [None] * len(polys)
        limit = 1.0 - self.param.safe_min_thresh
        for k, (v, c) in enumerate(zip(verdicts, cells)):
            mean_risk = v.sum_risk / v.sum_valid if v.sum_valid > 0 else 0.0
            safe = v.n_risky <= self.param.max_unsafe_n and float(v.max_risk) <= limit
            if _shoelace_area(clipped[k]) < 0.001:
                print("requested polygon is outside of the map")
                safe = False
            ring = _hull_ring(c)
            if ring is not None:                                        # cell indices of the border-stripped view -> map frame
                ring = self.center[:2].reshape(1, 2) + (ring - self.cell_n / 2.0) * self.resolution
            rings[k] = ring
            out[k] = (safe, mean_risk, _shoelace_area(polys[k]), v.n_inside, v.sum_valid, v.n_risky, v.max_risk)
        self.untraversable_polygon = rings[-1]
        self._mask, self._mask_polygon = None, clipped[-1]
        return out, rings

    def get_polygons_traversability(self, polygons, layer=None):
        """The safety check of ``get_polygon_traversability`` for a BATCH of footprints -- a list of ``(M_i, 2)`` arrays in the map frame --
        against ``layer`` (default: ``param.checker_layer``).  Returns ``(verdicts, rings)``: a structured array with the fields ``is_safe,
        mean_risk, area`` (what ``result`` holds there), ``n_inside`` (cells inside), ``n_known`` (the sum of ``is_valid`` inside),
        ``n_risky`` (cells with risk > 1 - ``safe_thresh``) and ``max_risk``; and per polygon the closed counter-clockwise hull ring around the
        risky cells in the map frame, or ``None`` when they span no area.

        Where the layer lies on the device -- a raw map layer, a semantic layer, or a plugin layer computed into a resident plane -- and no
        polygon has more than 256 vertices, the batch is ONE call of ``emap_polygon_safety`` (groups of 4096 beyond 4096 polygons): the
        statistics are reduced next to the cells, and a verdict record and the risky cells at the ends of each row -- all the hull needs --
        come back; no mask is written, no plane downloaded.  Otherwise every polygon takes the host route.  ``last_polygon_route`` tells
        which; ``EMAP_POLYGON_RESIDENT=0`` in the environment sends everything through the host route."""
        self._require_full_map("get_polygons_traversability")
        name = self.param.checker_layer if layer is None else layer
        polys = [np.asarray(p, np.float64) for p in polygons]
        if not polys:
            return np.zeros(0, self._VERDICT), []
        got = self._polygons_on_device(polys, name)
        self.last_polygon_route = "host" if got is None else "device"
        if got is not None:
            return got
        out, rings = np.zeros(len(polys), self._VERDICT), [None] * len(polys)
        for k, p in enumerate(polys):                                   # the host route, one polygon at a time
            res = np.zeros(3)
            self._polygon_traversability_host(p, res, name)
            out[k] = (bool(res[0]), res[1], res[2], int(self.mask[1:-1, 1:-1].sum())) + self._host_counts
            rings[k] = self.untraversable_polygon
        return out, rings

    def get_polygon_traversability(self, polygon, result):
        """Safety check of a footprint polygon (node service; reference :837-889): ``result`` = (is_safe, mean untraversability of the
        known cells inside, polygon area); the return value is the vertex count of the hull around the cells that are too untraversable
        (``get_untraversable_polygon`` hands it out).

        Where the checker layer lies on the device (``get_polygons_traversability`` says when) the call is a batch of one: the statistics
        are reduced on the device.  ``result[0]``, ``result[2]`` and the vertex count are the host route's values exactly; ``result[1]`` is the
        mean of a double-precision sum in a fixed order, where the host route divides a float32 pairwise sum (which lies further from
        the exact mean); the ring has the host route's vertices in the same counter-clockwise order, but may start at another of them:
        Qhull starts where it likes on a different point set (here the risky cells at the ends of each row, whose hull is that of all of
        them).  Everything else -- a plugin on its host route, an unknown layer, more than 256 vertices, ``EMAP_POLYGON_RESIDENT=0`` --
        takes the host route unchanged.  ``last_polygon_route`` tells which route the call took; ``mask`` is built when it is read."""
        self._require_full_map("get_polygon_traversability")
        got = self._polygons_on_device([np.asarray(polygon, np.float64)], self.param.checker_layer)
        self.last_polygon_route = "host" if got is None else "device"
        if got is None:
            return self._polygon_traversability_host(polygon, result)
        out, rings = got
        result[...] = np.array([out["is_safe"][0], out["mean_risk"][0], out["area"][0]])
        return 0 if rings[0] is None else int(rings[0].shape[0])

    def _polygon_traversability_host(self, polygon, result, layer=None):
        """The host route of ``get_polygon_traversability`` (reference :837-889).  The cell mask comes from the device
        (``emap_polygon_mask`` = the reference's polygon_mask_kernel, bit-exact); the statistics are a few reductions over the
        masked interior: ``result`` = (is_safe, mean untraversability of the known cells inside, polygon area); the return value is
        the vertex count of the hull around the cells that are too untraversable (``get_untraversable_polygon`` hands it out)."""
        self._require_full_map("get_polygon_traversability")
        poly = np.asarray(polygon, np.float64)
        area = _shoelace_area(poly)
        reach = self.map_length / 2 - self.resolution                  # the polygon is clipped to the map interior (:851-855)
        clipped = np.clip(poly.astype(np.float32), self.center[:2] - reach, self.center[:2] + reach).astype(np.float32)
        with self.map_lock:
            self.mask = self.polygon_mask(clipped)
            layer = np.asarray(self.get_layer(self.param.checker_layer if layer is None else layer), np.float32)
            valid = self.get_layer_raw("is_valid")
        inner = (slice(1, -1), slice(1, -1))
        footprint, known = self.mask[inner], valid[inner]
        risk = np.where(known > 0.5, 1.0 - layer[inner], 0.0) * footprint           # unknown cells count as traversable
        n_known = float((known * footprint).sum())
        mean_risk = float(risk.sum()) / n_known if n_known > 0 else 0.0
        too_risky = risk > 1.0 - self.param.safe_thresh
        n_risky, max_risk = int(too_risky.sum()), risk.max()
        safe = n_risky <= self.param.max_unsafe_n and float(max_risk) <= 1.0 - self.param.safe_min_thresh
        if _shoelace_area(clipped) < 0.001:
            print("requested polygon is outside of the map")
            safe = False
        ring = _hull_ring(np.argwhere(too_risky))
        if ring is not None:                                            # cell indices of the border-stripped view -> map frame
            ring = self.center[:2].reshape(1, 2) + (ring - self.cell_n / 2.0) * self.resolution
        self.untraversable_polygon = ring
        self._host_counts = (n_known, n_risky, max_risk)               # (the batch door's extra fields: nothing is reduced twice)
        result[...] = np.array([safe, mean_risk, area])
        return 0 if ring is None else int(ring.shape[0])

    def get_untraversable_polygon(self, untraversable_polygon):
        untraversable_polygon[...] = np.asarray(self.untraversable_polygon)

    # ---- map initialisation from a few known points (reference :899-923, map_initializer.py:25-62) -----------------
    def initialize_map(self, points, method="cubic"):
        """Interpolate the elevation between ``points`` ((M, 3) world x, y, z; e.g. the feet positions) with
        ``scipy.interpolate.griddata`` -- host code in the reference too -- then two dilation passes of radius
        ``dilation_size_initialize`` on the device and upper bound := elevation on valid cells."""
        from scipy.interpolate import griddata
        self._require_full_map("initialize_map")
        self.clear()
        with self.map_lock:
            points = np.array(points, dtype=np.float32)
            # world x, y -> (fractional, truncated) cell indices around the map centre
            indices = ((points[:, :2] - self.center[:2].astype(np.float32).reshape(1, 2)) / self.resolution + self.cell_n / 2).astype(np.int32)
            points[:, :2] = indices.astype(points.dtype)
            points[:, 2] -= self.center[2]
            m = self.elevation_map
            known = np.where(m[2] > 0.5)
            pts_idx = np.vstack([np.stack(known).T, points[:, :2]])
            values = np.hstack([m[0][known], points[:, 2]])
            assert pts_idx.shape[0] > 3, "Initialization points must be more than 3."
            gx, gy = np.mgrid[0:self.cell_n, 0:self.cell_n]
            interpolated = griddata(pts_idx, values, (gx, gy), method=method)
            ok = ~np.isnan(interpolated)
            m[0] = np.nan_to_num(interpolated)
            m[1] = np.where(ok, self.param.initialized_variance, self.initial_variance)
            m[2] = np.where(ok, 1.0, 0.0)
            if self.param.dilation_size_initialize > 0:
                e = np.ascontiguousarray(m[0], np.float32); v = np.ascontiguousarray(m[2], np.float32)
                oe, ov = np.empty_like(e), np.empty_like(v)
                self._chk(self._lib.emap_dilate_planes(self._ctx, f32p(e), f32p(v), int(self.param.dilation_size_initialize), 2, f32p(oe), f32p(ov)))
                m[0], m[2] = oe, ov
            mask = m[2] > 0.5                       # update_upper_bound_with_valid_elevation (:428-432)
            m[5] = np.where(mask, m[0], m[5])
            m[6] = np.where(mask, 0.0, m[6])
            for k in (0, 1, 2, 5, 6):
                self.set_layer_raw(k, m[k])

    def compile_kernels(self):
        """nothing to compile: parameters are kernel arguments of the prebuilt gfx950 library (reference :228-282)"""

    compile_image_kernels = compile_kernels

    def pad_value(self, x, shift_value, idx=None, value=0.0):
        """host helper of the reference's shift (:172-198): fill the band a shift vacated in a (planes, rows, columns) stack.  The map
        itself is shifted on the device (``emap_shift``: circular origin, no copy); this is for callers that shift their own arrays."""
        from .semantic_map import SemanticMap
        SemanticMap.pad_value(None, x, shift_value, idx=idx, value=value)

    def get_normal_ref(self, normal_x_data, normal_y_data, normal_z_data):
        n = self.get_normal_maps()
        normal_x_data[...] = n[0]
        normal_y_data[...] = n[1]
        normal_z_data[...] = n[2]

    def get_layer(self, name):
        """Raw (unflipped, unstripped) layer by name (reference :777-791)."""
        if name in self.layer_names:
            return self.get_layer_raw(self.layer_names.index(name))
        if self.semantic_map is not None and name in self.semantic_map.layer_names:
            return self.semantic_map._layer(self.semantic_map.layer_names.index(name))
        if self.plugin_manager is not None and name in self.plugin_manager.layer_names:
            sem = self.semantic_map
            self.plugin_manager.update_with_name(
                name, LazyPlanes(7, self.get_layer_raw, device_map=self), self.layer_names,
                LazyPlanes(len(sem.layer_names), sem._layer, rows=self.rows, cols=self.cell_n) if sem is not None else None,
                self.semantic_map.layer_names if self.semantic_map is not None else [],
                self.base_rotation, self.semantic_map.elements_to_shift if self.semantic_map is not None else {})
            return self.plugin_manager.get_map_with_name(name)
        print("Layer {} is not in the map, returning traversabiltiy!".format(name))
        return None
