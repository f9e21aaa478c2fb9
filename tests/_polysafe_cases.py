"""The case table of the safety-polygon service on the device (emap_polygon_safety) and a NumPy model of its verdict: the mask of
``oracle.emap_oracle.polygon_mask`` plus the host route's statements (ElevationMap._polygon_traversability_host), with the two sums taken
in float64 in the order the kernels state (emap_polysafe.hip): a thread's four cells in k order, an xor butterfly over the wave's 64
lanes, the four waves in index order, the tiles of the polygon's box row-major.  No device is needed for anything here."""
import numpy as np

from oracle import emap_oracle as eo

RES = 0.04
TILE = 32
# the service's parameters in every test: a cell is risky above 1 - SAFE_THRESH; the maximum may reach 1 - SAFE_MIN_THRESH = 1, so that
# is_safe turns on the COUNT of risky cells alone (the defaults let a single risky cell decide through the maximum)
SAFE_THRESH, SAFE_MIN_THRESH, MAX_UNSAFE_N = 0.5, 0.0, 5
THR32 = np.float32(1.0 - SAFE_THRESH)
RISKY, FINE = np.float32(0.1), np.float32(0.9)      # traversability of a risky cell (risk 0.9) and of the others (risk <= 0.4)


def q16(v):
    return np.float32(np.float16(np.float32(v)))


def poly_cell(C, x, y, cx, cy):
    """cell (row, column) of a world point: get_idx of the reference's polygon kernel in reference_fp16 mode (custom_kernels.py:587-603)"""
    def axis(v, c):
        q = np.float32(q16(v) - q16(c)) / np.float32(RES)
        val = float(q) + 0.5 * float(np.float32(C))
        i = 0 if val != val else int(min(max(val, -2147483648.0), 2147483647.0))
        fi = q16(np.float32(i))
        fi = max(min(fi, q16(np.float32(C - 1))), q16(0.0))
        return int(fi)
    idx = C * axis(x, cx) + axis(y, cy)
    return idx // C, idx % C


def clip_polygon(C, poly, center):
    """ElevationMap._clip_polygon"""
    reach = (C - 2) * RES / 2 - RES
    c = np.asarray(center, np.float32)[:2]
    return np.clip(np.asarray(poly, np.float64).astype(np.float32), c - reach, c + reach).astype(np.float32)


def work_table(C, clipped, center):
    """the polygon's box clipped to the interior and its tiles, row-major: (row0, col0, nrows, ncols, [(tile row, tile col), ...])"""
    clipped = np.asarray(clipped, np.float32)
    mn, mx = clipped.min(axis=0), clipped.max(axis=0)
    r0, c0 = poly_cell(C, mn[0], mn[1], center[0], center[1])
    r1, c1 = poly_cell(C, mx[0], mx[1], center[0], center[1])
    r0, c0, r1, c1 = max(r0, 1), max(c0, 1), min(r1, C - 2), min(c1, C - 2)
    nrows = r1 - r0 + 1 if r1 >= r0 and c1 >= c0 else 0
    ncols = c1 - c0 + 1 if nrows else 0
    ntr, ntc = (nrows + TILE - 1) // TILE, (ncols + TILE - 1) // TILE
    return r0, c0, nrows, ncols, [(tr, tc) for tr in range(ntr) for tc in range(ntc)]


def _butterfly(v):
    """the xor butterfly over 64 lanes: every lane ends with this value"""
    for o in (32, 16, 8, 4, 2, 1):
        v = v[:o] + v[o:2 * o]
    return v[0]


def kernel_order_sum(plane, inside, table):
    """float64 sum of ``plane`` (full map, float32) over the cells of ``inside`` in the kernels' order"""
    r0, c0, nrows, ncols, tiles = table
    total = 0.0
    for tr, tc in tiles:
        v = np.zeros((TILE, TILE), np.float64)                        # [row of the tile][column of the tile]
        rr, cc = r0 + tr * TILE, c0 + tc * TILE
        h, w = min(TILE, r0 + nrows - rr), min(TILE, c0 + ncols - cc)
        v[:h, :w] = np.where(inside[rr:rr + h, cc:cc + w], plane[rr:rr + h, cc:cc + w].astype(np.float64), 0.0)
        thread = np.zeros((8, TILE), np.float64)                      # thread (x, y) holds rows y + 8 k
        for k in range(4):
            thread = thread + v[8 * k:8 * k + 8]
        lanes = thread.reshape(4, 64)                                 # wave = y / 2, lane = (y % 2) * 32 + x
        part = _butterfly(lanes[0])
        for wv in range(1, 4):
            part = part + _butterfly(lanes[wv])
        total = total + part
    return float(total)


def model(mask, layer, valid, table, max_unsafe_n=MAX_UNSAFE_N, safe_thresh=SAFE_THRESH, safe_min_thresh=SAFE_MIN_THRESH):
    """the verdict of one polygon from its (C, C) mask and the (C, C) checker layer and is_valid planes: the host route's statements;
    ``sum_risk`` / ``sum_valid`` / ``mean_risk`` in float64 in the kernels' order"""
    from elevation_mapping_cupy_amd.elevation_mapping import _hull_ring
    inner = (slice(1, -1), slice(1, -1))
    footprint, known = mask[inner], valid[inner]
    with np.errstate(invalid="ignore"):
        risk = np.where(known > 0.5, 1.0 - np.asarray(layer, np.float32)[inner], 0.0) * footprint
    risk = risk.astype(np.float32)
    too_risky = risk > 1.0 - safe_thresh
    max_risk = risk.max()
    inside = np.zeros(mask.shape, bool)
    inside[inner] = footprint > 0
    full_risk = np.zeros(mask.shape, np.float32)
    full_risk[inner] = risk
    sum_valid = kernel_order_sum(valid, inside, table)
    sum_risk = float("nan") if np.isnan(max_risk) else kernel_order_sum(full_risk, inside, table)
    return dict(n_inside=int(footprint.sum()), n_known=float((known * footprint).sum()), n_risky=int(too_risky.sum()), max_risk=np.float32(max_risk),
                sum_valid=sum_valid, sum_risk=sum_risk, mean_risk=sum_risk / sum_valid if sum_valid > 0 else 0.0,
                abs_risk=float(np.abs(risk.astype(np.float64)).sum()),
                is_safe=bool(int(too_risky.sum()) <= max_unsafe_n and float(max_risk) <= 1.0 - safe_min_thresh),
                ring=_hull_ring(np.argwhere(too_risky)), too_risky=too_risky)


def base_planes(C, seed=0):
    """traversability in 0.6 .. 1 (nothing risky) and is_valid with a tenth of the cells unknown"""
    rng = np.random.RandomState(seed)
    trav = (0.6 + 0.4 * rng.rand(C, C)).astype(np.float32)
    valid = (rng.rand(C, C) > 0.1).astype(np.float32)
    return trav, valid


def oracle_params(C):
    return eo.make_params(eo.DEFAULTS, cell_n=C, mode="reference_fp16")


def _known_inside(mask, valid):
    m = np.zeros(mask.shape, bool)
    m[1:-1, 1:-1] = (mask[1:-1, 1:-1] > 0) & (valid[1:-1, 1:-1] > 0.5)
    return np.argwhere(m)


def _outside(mask, valid, known):
    m = np.zeros(mask.shape, bool)
    m[1:-1, 1:-1] = (mask[1:-1, 1:-1] == 0) & ((valid[1:-1, 1:-1] > 0.5) == known)
    return np.argwhere(m)


def _mark(n, step=1):
    def dress(trav, valid, mask):
        for r, c in _known_inside(mask, valid)[::step][:n]:
            trav[r, c] = RISKY
    return dress


def _column(n):
    """n risky cells one below the other: collinear along a column, one per row"""
    def dress(trav, valid, mask):
        cells = _known_inside(mask, valid)
        for r, c in cells:
            run = [(r + k, c) for k in range(n)]
            if all(mask[a, b] > 0 for a, b in run):
                for a, b in run:
                    trav[a, b], valid[a, b] = RISKY, 1.0
                return
        raise AssertionError("no run of %d cells" % n)
    return dress


def _row_pair(trav, valid, mask):
    """2 risky cells in one row"""
    for r, c in _known_inside(mask, valid):
        if mask[r, c + 3] > 0:
            trav[r, c] = trav[r, c + 3] = RISKY
            valid[r, c + 3] = 1.0
            return
    raise AssertionError("no pair")


def _put(value, where):
    def dress(trav, valid, mask):
        cells = {"inside": lambda: _known_inside(mask, valid), "known_outside": lambda: _outside(mask, valid, True),
                 "unknown_outside": lambda: _outside(mask, valid, False)}[where]()
        r, c = cells[len(cells) // 2]
        trav[r, c] = value
    return dress


QUAD = np.array([[-0.6, -0.4], [0.7, -0.5], [0.8, 0.5], [-0.2, 0.9]], np.float64)
# name -> (cell_n, move_to in cells or None, polygon relative to the map centre, dressing of (trav, valid) given the mask, clip)
CASES = {
    "threshold_at": (66, None, QUAD, _mark(MAX_UNSAFE_N, 7), True),
    "threshold_over": (66, None, QUAD, _mark(MAX_UNSAFE_N + 1, 7), True),
    "ragged": (130, None, np.array([[-1.4, -0.9], [1.4, -0.9], [1.4, 0.9], [-1.4, 0.9]], np.float64), _mark(40, 53), True),
    "cut": (130, (20, 25), np.array([[1.2, 1.0], [2.2, 1.1], [2.1, 2.0], [1.3, 1.9]], np.float64), _mark(9, 31), True),
    "hull_0": (66, None, QUAD, _mark(0), True),
    "hull_1": (66, None, QUAD, _mark(1), True),
    "hull_2": (66, None, QUAD, _row_pair, True),
    "hull_4_collinear": (66, None, QUAD, _column(4), True),
    "nan_inside": (66, None, QUAD, _put(np.float32("nan"), "inside"), True),
    "poison": (66, None, QUAD, _put(np.float32("-inf"), "known_outside"), True),
    "no_poison": (66, None, QUAD, _put(np.float32("-inf"), "unknown_outside"), True),
    # not clipped: the box reaches the border rows and columns 0 and C-1 and is cut to the interior 1 .. C-2
    "border": (66, None, np.array([[-1.4, -1.4], [1.4, -1.4], [1.4, 1.4], [-1.4, 1.4]], np.float64), _mark(12, 101), False),
    "big_258": (258, None, np.array([[-4.0, -3.1], [3.5, -4.2], [4.4, 3.0], [0.3, 1.0], [-3.0, 4.5]], np.float64), _mark(30, 977), True),
}


def build(name):
    """(cell_n, centre after the move, clipped polygon, mask, trav, valid, work table) of a case; the planes are in LOGICAL order as
    set_layer_raw takes them AFTER the case's move_to"""
    C, move, poly, dress, clip = CASES[name]
    center = np.zeros(3, np.float32)
    if move is not None:
        center[:2] += np.asarray(move, np.float64) * RES            # ElevationMap.move_to from the origin
    world = poly + center[:2].astype(np.float64)
    clipped = clip_polygon(C, world, center) if clip else world.astype(np.float32)
    mask = eo.polygon_mask(oracle_params(C), clipped, float(center[0]), float(center[1]))
    trav, valid = base_planes(C, seed=len(name))
    dress(trav, valid, mask)
    return C, center, world, clipped, mask, trav, valid, work_table(C, clipped, center)
