"""What the point-cloud output tests share (tests/test_cloud_out_cases.py on the CPU, tests/test_hip_cloud_out.py on the GPU): the NumPy
model of GridMapRosConverter::toPointCloud and of the node's normal arrows on message-order planes, a per-cell pure-Python restatement
of grid_map's iterator to check the model against, the validity patterns and the sizes the GPU tests run.

grid_map is absent offline: the iterator (lin = 0 .. M M - 1, index (i, j) = (lin % M, lin / M)), GridMap::isValid, getPosition3 and
getPositionFromIndex are restated from their published definitions and NOT pinned by a compiled reference.  The model is the tests' own:
it shares no code with the package's host route."""
import math

import numpy as np

POISON = 0xA5A5A5A5
# cell_n of the GPU tests: M = 8 (under one tile), 32 (exactly one tile), 33 (one ragged row and column of tiles), 65, 257 (nine tile
# rows: past 256 masks in one column run), and 353: M * ceil(M / 32) = 353 * 12 = 4236 mask words, past the 4096 words (1024 threads x
# 4 words, EM_CLOUD_SCAN_TRIP) that the scan's one workgroup takes in a single trip -- the carry between trips is exercised
SIZES = (10, 34, 35, 67, 259, 355)
SCAN_TRIP = 4096


def mask_words(M):
    return M * ((M + 31) // 32)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def field_names(names, point_layer, hidden=(), index=False):
    out = []
    for n in names:
        if n in hidden:
            continue
        out += ["x", "y", "z"] if n == point_layer else ["rgb" if n == "color" else n]
    return out + (["index"] if index else [])


def model_cloud(planes, names, point_layer, basic, xs, ys, index=False, normal_min=None, hidden=()):
    """``planes[k]``: the (M, M) message-order plane of ``names[k]`` (element (i, j) at [j, i]: ``.ravel()`` is iteration order).  A cell
    passes if the point layer and every ``basic`` layer are finite there and, with ``normal_min``, not (|normal| < normal_min) in double
    (``normal_x / y / z`` must be among ``names``).  ``xs`` / ``ys``: float32 positions of row i / column j.  ``hidden``: tested, not emitted.
    Returns ``(field names, (n, fields) float32 records)``; with ``index`` the last column holds lin as int32 bits."""
    planes = [np.ascontiguousarray(p, np.float32) for p in planes]
    M = planes[0].shape[0]
    by_name = dict(zip(names, planes))
    ok = np.isfinite(by_name[point_layer])
    for b in basic:
        ok = ok & np.isfinite(by_name[b])
    if normal_min is not None:
        nx, ny, nz = (by_name[n].astype(np.float64) for n in ("normal_x", "normal_y", "normal_z"))
        with np.errstate(invalid="ignore"):
            ok = ok & ~(np.sqrt((nx * nx + ny * ny) + nz * nz) < np.float64(normal_min))
    lin = np.nonzero(ok.ravel())[0]
    cols = []
    for n in names:
        if n in hidden:
            continue
        if n == point_layer:
            cols += [np.asarray(xs, np.float32)[lin % M].view(np.uint32), np.asarray(ys, np.float32)[lin // M].view(np.uint32)]
        cols.append(by_name[n].ravel().view(np.uint32)[lin])
    if index:
        cols.append(lin.astype(np.int32).view(np.uint32))
    rec = np.stack(cols, axis=1).astype(np.uint32) if cols else np.empty((lin.size, 0), np.uint32)
    return field_names(names, point_layer, hidden, index), np.ascontiguousarray(rec).view(np.float32)


def loop_cloud(planes, names, point_layer, basic, xs, ys, index=False, normal_min=None, hidden=()):
    """the iterator restated cell by cell: lin = 0 .. M M - 1, (i, j) = (lin % M, lin // M); isValid over the basic layers, getPosition3 on
    the point layer; the norm in Python floats (IEEE double), summed (x x + y y) + z z"""
    M = planes[0].shape[0]
    by_name = dict(zip(names, planes))
    words = []
    n = 0
    for lin in range(M * M):
        i, j = lin % M, lin // M
        if not all(math.isfinite(float(by_name[b][j, i])) for b in basic):
            continue
        if not math.isfinite(float(by_name[point_layer][j, i])):
            continue
        if normal_min is not None:
            x, y, z = (float(by_name[a][j, i]) for a in ("normal_x", "normal_y", "normal_z"))
            s = (x * x + y * y) + z * z
            if (math.sqrt(s) if s == s else float("nan")) < normal_min:
                continue
        for name in names:
            if name in hidden:
                continue
            if name == point_layer:
                words += [np.float32(xs[i]).view(np.uint32), np.float32(ys[j]).view(np.uint32)]
            words.append(np.float32(by_name[name][j, i]).view(np.uint32))
        if index:
            words.append(np.uint32(lin))
        n += 1
    rec = np.array(words, np.uint32).reshape(n, -1) if n else np.empty((0, len(field_names(names, point_layer, hidden, index))), np.uint32)
    return field_names(names, point_layer, hidden, index), rec.view(np.float32)


def positions_loop(center_xy, resolution, M):
    """getPositionFromIndex with both start indices 0, in Python floats: x(i) = (p + (0.5 L - 0.5 res)) + res * (-i)"""
    res = float(resolution)
    L = M * res
    out = []
    for p in center_xy:
        off = 0.5 * L - 0.5 * res
        out.append(np.array([(float(p) + off) + res * float(-i) for i in range(M)], np.float64))
    return out


def model_arrows(elev, nx, ny, nz, xs64, ys64, scale=0.1, min_norm=0.1):
    """message-order planes in, ``(ids int32, starts (n, 3) float64, ends (n, 3) float64)`` out: the arrows of elevation_mapping_ros.cpp:751-809"""
    M = elev.shape[0]
    n64 = [np.ascontiguousarray(a, np.float32).astype(np.float64) for a in (nx, ny, nz)]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(elev) & ~(np.sqrt((n64[0] * n64[0] + n64[1] * n64[1]) + n64[2] * n64[2]) < np.float64(min_norm))
    lin = np.nonzero(ok.ravel())[0]
    starts = np.stack([np.asarray(xs64)[lin % M], np.asarray(ys64)[lin // M], elev.ravel()[lin].astype(np.float64)], axis=1)
    ends = starts + np.stack([a.ravel()[lin] for a in n64], axis=1) * np.float64(scale)
    return lin.astype(np.int32), starts, ends


def loop_arrows(elev, nx, ny, nz, xs64, ys64, scale=0.1, min_norm=0.1):
    M = elev.shape[0]
    ids, starts, ends = [], [], []
    for lin in range(M * M):
        i, j = lin % M, lin // M
        z = float(elev[j, i])
        if not math.isfinite(z):
            continue
        v = [float(a[j, i]) for a in (nx, ny, nz)]
        s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        if (math.sqrt(s) if s == s else float("nan")) < min_norm:
            continue
        st = [float(xs64[i]), float(ys64[j]), z]
        ids.append(lin); starts.append(st); ends.append([st[a] + v[a] * scale for a in range(3)])
    return np.array(ids, np.int32), np.array(starts, np.float64).reshape(-1, 3), np.array(ends, np.float64).reshape(-1, 3)


def same_words(a, b):
    """two float arrays hold the same 32-bit (or 64-bit) words, NaN payloads included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    w = np.uint32 if a.dtype.itemsize == 4 else np.uint64
    return bool((a.view(w) == b.view(w)).all())


# ---- validity patterns: (M, M) bool in the PUBLISHED index space, [i, j] ------------------------------------------------------------------
def validity_patterns(M, seed=11):
    rng = np.random.default_rng(seed + M)
    i, j = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    pats = {
        "none valid": np.zeros((M, M), bool),
        "all valid": np.ones((M, M), bool),
        "two corners": (i == 0) & (j == 0) | (i == M - 1) & (j == M - 1),
        "checkerboard": (i + j) % 2 == 0,
        "random 30 %": rng.random((M, M)) < 0.3,
        "one full column": j == M // 2,                        # between empty ones
        "one full row": i == M // 3,
        "first row tile of every column empty": i >= min(32, M // 2),
    }
    return pats


EXTRA_CASES = ("other field NaN", "+inf elevation", "tested layer NaN")      # run on the "checkerboard" validity


def logical_plane(pub, C, border=0.0):
    """the (C, C) logical plane whose published view (border stripped, both axes flipped) is ``pub`` (M, M), [i, j]"""
    out = np.full((C, C), border, np.float32)
    out[1:C - 1, 1:C - 1] = np.asarray(pub, np.float32)[::-1, ::-1]
    return out


def heights(M):
    """finite, distinct elevations in the published index space, not symmetric under a flip or a transpose"""
    i, j = np.meshgrid(np.arange(M, dtype=np.float32), np.arange(M, dtype=np.float32), indexing="ij")
    return (np.float32(0.25) + np.float32(0.001) * (i * np.float32(M) + j) + np.float32(0.0003) * i).astype(np.float32)


def variances(M):
    i, j = np.meshgrid(np.arange(M, dtype=np.float32), np.arange(M, dtype=np.float32), indexing="ij")
    return (np.float32(0.5) + np.float32(0.002) * (j * np.float32(M) + i)).astype(np.float32)


NAN_PAYLOAD = np.array([0x7FC12345], np.uint32).view(np.float32)[0]      # a NaN whose bits must arrive as they are


def case_state(M, name):
    """``(valid, height, variance)`` published-space planes of a validity pattern or an extra case"""
    pats = validity_patterns(M)
    h, v = heights(M), variances(M)
    if name in pats:
        return pats[name], h, v
    valid = pats["checkerboard"]
    cells = np.argwhere(valid)
    pick = cells[:: max(1, len(cells) // 5)][:5]              # a few valid cells, the first among them
    if name == "other field NaN" or name == "tested layer NaN":
        for a, b in pick[:-1] if len(pick) > 1 else pick:
            v[a, b] = NAN_PAYLOAD
    elif name == "+inf elevation":
        for a, b in pick[:-1] if len(pick) > 1 else pick:
            h[a, b] = np.inf
    else:
        raise KeyError(name)
    return valid, h, v


def all_cases(M):
    return list(validity_patterns(M)) + list(EXTRA_CASES)


def published_planes(M, name, center_z=0.0):
    """message-order planes ``{elevation, variance}`` of a case as the map publishes them: elevation NaN where the cell is not valid"""
    valid, h, v = case_state(M, name)
    e = np.where(valid, h + np.float32(center_z), np.float32(np.nan)).astype(np.float32)
    return {"elevation": np.ascontiguousarray(e.T), "variance": np.ascontiguousarray(v.T)}
