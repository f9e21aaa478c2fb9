"""What the submap service tests share (tests/test_submap_cases.py on the CPU, tests/test_hip_submap.py on the GPU): hand-checked
geometry requests, the NumPy model "slice the full planes" of the packed output of emap_publish_grid_windows, and the window tables
the GPU tests run.

grid_map is absent offline: submap_geometry restates grid_map_core's getSubmapInformation and is NOT pinned by a compiled reference.
The hand values below are worked out on paper for requests whose corners lie strictly inside cells, where the double arithmetic has
no choice to make; what the statement gives ON cell edges is recorded (EDGE_RECORD), not claimed to be grid_map's behaviour."""
import numpy as np

# ---- geometry: a 10 x 10 map of 0.5 m cells around (1.0, -2.0); x spans (-1.5, 3.5), y spans (-4.5, 0.5).  Index i counts down from
# x = 3.5 (cell i covers 3.5 - 0.5 (i + 1) .. 3.5 - 0.5 i), index j counts down from y = 0.5. ---------------------------------------
GEO_MAP = dict(map_position_xy=(1.0, -2.0), map_length=5.0, resolution=0.5, M=10)
# name: (position_xy, length_xy, expected)      expected: None or (i0, j0, ni, nj, submap_position_xy, submap_length_xy, index_in_submap)
GEOMETRY = {
    # corners x 1.8 / 0.8 -> rows 3 .. 5, y -0.9 / -2.9 -> columns 2 .. 6; the window's top-left corner is (2.0, -0.5)
    "interior, ni != nj": ((1.3, -1.9), (1.0, 2.0), (3, 2, 3, 5, (1.25, -1.75), (1.5, 2.5), (1, 2))),
    # x + 0.5 = 3.7 lies beyond the map's upper edge 3.5: clipped to row 0; x - 0.5 = 2.7 -> row 1
    "clipped by one edge": ((3.2, -1.9), (1.0, 0.6), (0, 4, 2, 2, (3.0, -2.0), (1.0, 1.0), (0, 0))),
    # x - 0.5 = -1.7 and y - 0.5 = -4.7 lie beyond the lower edges: clipped to row / column 9
    "clipped by a corner": ((-1.2, -4.2), (1.0, 1.0), (8, 8, 2, 2, (-1.0, -4.0), (1.0, 1.0), (1, 1))),
    # ten times the map: all four edges clip, the window is the map
    "clipped by all four edges": ((1.3, -1.9), (50.0, 50.0), (0, 0, 10, 10, (1.0, -2.0), (5.0, 5.0), (4, 4))),
    # the centre x = 4.1 lies outside the map; the clipped window is row 0 alone (x 3.0 .. 3.5) and does not hold it
    "centre outside the map": ((4.1, -1.9), (1.6, 1.0), None),
}
BAD_REQUESTS = {      # every ValueError that arguments can reach (a window size below 1 cannot be reached with lengths >= 0: bottom_right >= top_left)
    "NaN position": dict(position_xy=(float("nan"), 0.0), length_xy=(1.0, 1.0)),
    "infinite position": dict(position_xy=(0.0, float("inf")), length_xy=(1.0, 1.0)),
    "NaN length": dict(position_xy=(0.0, 0.0), length_xy=(1.0, float("nan"))),
    "infinite length": dict(position_xy=(0.0, 0.0), length_xy=(float("inf"), 1.0)),
    "negative length x": dict(position_xy=(0.0, 0.0), length_xy=(-0.1, 1.0)),
    "negative length y": dict(position_xy=(0.0, 0.0), length_xy=(1.0, -1e-9)),
    "NaN map position": dict(position_xy=(0.0, 0.0), length_xy=(1.0, 1.0), map_position_xy=(0.0, float("nan"))),
    "NaN map length": dict(position_xy=(0.0, 0.0), length_xy=(1.0, 1.0), map_length=float("nan")),
    "zero resolution": dict(position_xy=(0.0, 0.0), length_xy=(1.0, 1.0), resolution=0.0),
    "no cell": dict(position_xy=(0.0, 0.0), length_xy=(1.0, 1.0), M=0),
}
# What the statement gives on cell edges, at M = 32, resolution 0.1 around the origin (recorded from this implementation, in double):
# the whole map comes back whole, a zero-length request at the map centre is the one cell below the centre edge.
EDGE_MAP = dict(map_position_xy=(0.0, 0.0), map_length=32 * 0.1, resolution=0.1, M=32)
EDGE_RECORD = {
    "the whole map": ((0.0, 0.0), (32 * 0.1, 32 * 0.1), (0, 0, 32, 32, (0.0, 0.0), (32 * 0.1, 32 * 0.1), (16, 16))),
    "zero length at the centre": ((0.0, 0.0), (0.0, 0.0), (16, 16, 1, 1, (-0.05, -0.05), (0.1, 0.1), (0, 0))),
}


# ---- the packed layout ----------------------------------------------------------------------------------------------------------------
def packed_size(windows, n_layers):
    return n_layers * sum(ni * nj for _, _, ni, nj in windows)


def pack_slices(full, windows, order):
    """the model: ``full`` = (L, M, M) planes as get_grid_map_layers(order="rows") leaves them; window w's planes are the slices
    [k, i0:i0+ni, j0:j0+nj] -- for "message" their transposes stored contiguous -- one window after the other"""
    parts = []
    for i0, j0, ni, nj in windows:
        s = full[:, i0:i0 + ni, j0:j0 + nj]
        parts.append(np.ascontiguousarray(s.transpose(0, 2, 1) if order == "message" else s).reshape(-1))
    return np.concatenate(parts) if parts else np.empty(0, full.dtype)


def pack_loop(full, windows, order):
    """the header's statement element by element: window w starts at L * sum(ni nj before it), layer k is plane k, element (i, j) lies
    at i * nj + j ("rows") or j * ni + i ("message")"""
    L = full.shape[0]
    flat = np.empty(packed_size(windows, L), full.dtype)
    start = 0
    for i0, j0, ni, nj in windows:
        for k in range(L):
            for i in range(ni):
                for j in range(nj):
                    flat[start + k * ni * nj + (i * nj + j if order == "rows" else j * ni + i)] = full[k, i0 + i, j0 + j]
        start += L * ni * nj
    return flat


# ---- the window tables of the GPU tests (M = cell_n - 2 in 8, 32, 65, 98) ---------------------------------------------------------------
def partition(M):
    """a 3 x 3 partition of the published map into unequal blocks: wherever the circular origin lies, the seam is inside some block"""
    rows, cols = [0, max(1, M // 4), M - 1, M], [0, M // 3 + 1, M - 2, M]
    return [(rows[a], cols[b], rows[a + 1] - rows[a], cols[b + 1] - cols[b]) for a in range(3) for b in range(3)]


def window_sets(M):
    sets = {
        "whole": [(0, 0, M, M)],
        "single cells": [(0, 0, 1, 1), (0, M - 1, 1, 1), (M - 1, 0, 1, 1), (M - 1, M - 1, 1, 1), (M // 2, M // 3, 1, 1)],
        "strips": [(M // 3, 0, 1, M), (0, M // 2, M, 1)],
        "partition": partition(M),
        "overlapping and repeated": [(1, 1, 4, 5), (3, 2, 4, 5), (1, 1, 4, 5)],
        "sixty-four": [((3 * k) % (M - 3), (5 * k) % (M - 2), 1 + k % 3, 1 + k % 2) for k in range(64)],
    }
    if M >= 34:
        sets["astride a tile edge"] = [(31, 2, 3, min(M - 2, 40))]          # i0 = 31, ni = 3: rows 31 | 32 33 of the map, tile rows 0 .. 2 of the window
    if M >= 65:
        sets["5 x 37 and 37 x 5"] = [(7, 20, 5, 37), (20, 7, 37, 5)]      # ni != nj, more than one tile along one axis only
    return sets


def all_windows(M):
    """every window of every set but the 64, in one batch"""
    return [w for name, ws in window_sets(M).items() if name != "sixty-four" for w in ws]
