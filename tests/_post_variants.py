"""Case table of tests/test_hip_post_variants.py and test_post_variant_cases.py, and -- run as a program -- the child process that
executes every case on the GPU with whatever tile height / kernel the EMAP_POST_* hooks of its environment select
(emap_kernels.hip: post_tile_rows, post_use_dma read them once per process, so one process is one variant):

    python tests/_post_variants.py <out.npz>

The parent builds the same states with state() and compares the recorded arrays with the oracle."""
import sys

import numpy as np

# (cell_n, dilation_size).  66: no tile whose staged region lies inside the map; (66, 20): a region wider than the map; 130: a last tile of
# 2 rows and 2 columns; 202: interior tiles for every tile height; 12 | 13 and 20 | 21: either side of k_post_dma's limit of one lane
# per region row (R + 8 + 2d <= 64) for 32- and 16-row tiles; 32: the launcher halves the tile height until the region fits the LDS.
CASES = [(66, 1), (66, 3), (130, 3), (202, 3), (130, 10), (202, 10), (202, 12), (202, 13), (66, 20), (202, 20), (130, 21), (202, 32)]
SHIFT_B = (37, 5)                 # context B: rows, columns the empty map is moved by before the planes are set
FRAME = dict(C=202, N=20000, seeds=(11, 12), shift=(3, 2))      # the frame case: two whole frames, a move between them
FRAME_KEY = "frame202"
TILE_ROWS = (4, 8, 16, 32)
PT_C = 64                         # tile width of both kernels
SPARSE_MAX_D = 15                 # the kernels search on bit masks only up to this radius (their `sparse` condition)


def case_key(C, d):
    return "c%d_d%d" % (C, d)


def case_seed(C, d):
    return 1000 * C + d


def hole_rectangle(C, d):
    """(r0, c0, side) of the all-hole square: side 2d + 8, so that its centre has no source within the dilation reach.  It lies inside
    the dense half wherever it fits between that half's first column and the border column C - 1; at (66, 20) it does not (48 > 32
    columns) and is centred on the map instead, where its 2d + 1 window stays clear of the flat-index wrap."""
    h, s = C // 2, 2 * d + 8
    if s <= C - 1 - h:
        return (C - s) // 2, h + (C - 1 - h - s) // 2, s
    assert s <= C - 2, (C, d)
    return (C - s) // 2, (C - s) // 2, s


def state(C, d, seed):
    """all seven planes (7, C, C) float32, numpy only: a sparse left half (more than 3/4 holes), a dense right half, busy first and
    last four columns (the reference's flat-index row wrap), valid border cells (keep their value, never a source) and one all-hole
    square whose centre no source reaches.  Two departures from "left half sparse, right half dense, square inside the dense half", both
    forced by the 66-cell maps: hole_rectangle() at (66, 20), and the all-sparse rows below row 26 at (66, 1) and (66, 3)."""
    rng = np.random.default_rng(seed)
    e = np.zeros((7, C, C), np.float32)
    e[5] = rng.uniform(-1, 1, (C, C))
    e[0] = rng.uniform(-1, 1, (C, C)); e[1] = rng.uniform(0.01, 2.0, (C, C)); e[3] = rng.uniform(0, 1, (C, C)); e[4] = rng.uniform(0, 3, (C, C))
    h = C // 2
    uv, uu = rng.uniform(0, 1, (C, C)), rng.uniform(0, 1, (C, C))
    e[2][:, :h] = uv[:, :h] < 0.05; e[6][:, :h] = uu[:, :h] < 0.03
    e[2][:, h:] = uv[:, h:] < 0.6; e[6][:, h:] = uu[:, h:] < 0.1
    if C < PT_C + 6 and d <= SPARSE_MAX_D:
        # a map narrower than a tile's 70-column window: every window spans both halves and none could be 3/4 holes (64 % at most).
        # Below row 26 the sparse density covers the whole width, so that the window of the 32-row tile at row 32 (rows 29 ...) and those
        # of the smaller tiles below it take the bit-mask search -- here with the flat-index wrap on BOTH sides of one tile.
        e[2][26:, h:] = uv[26:, h:] < 0.05; e[6][26:, h:] = uu[26:, h:] < 0.03
    e[2][:, :4] = rng.uniform(0, 1, (C, 4)) < 0.5; e[2][:, -4:] = rng.uniform(0, 1, (C, 4)) < 0.5
    r0, c0, s = hole_rectangle(C, d)
    e[2][r0:r0 + s, c0:c0 + s] = 0; e[6][r0:r0 + s, c0:c0 + s] = 0
    e[2][0, :] = 1; e[2][:, C - 1] = 1
    return e


def window_holes(mask, R):
    """holes (mask < 0.5) the kernels list per tile of R rows, tiles from row 0: the cells of the tile's (R + 6) x 70 window that exist --
    a column beyond the map's edge is the flat index's cell of the neighbouring row"""
    C = mask.shape[0]
    ntx, nty = (C + PT_C - 1) // PT_C, (C + R - 1) // R
    ext = np.zeros((nty * R + 6, ntx * PT_C + 6), np.int64)          # ext[r + 3, c + 3]: 1 = cell (r, c) of the window grid is a hole
    hole = (mask < 0.5).astype(np.int64)
    for c in range(-3, ntx * PT_C + 3):
        if c < 0:
            ext[4:C + 4, c + 3] = hole[:, c + C]                       # row r reads row r - 1
        elif c < C:
            ext[3:C + 3, c + 3] = hole[:, c]
        elif c - C < C:
            ext[2:C + 2, c + 3] = hole[:, c - C]                       # row r reads row r + 1
    return [int(ext[ty * R:ty * R + R + 6, tx * PT_C:tx * PT_C + PT_C + 6].sum()) for ty in range(nty) for tx in range(ntx)]


def frame_inputs():
    import _fixtures as fx
    R, t0 = fx.POSES["rotated"]
    return R, t0, [fx.cloud(FRAME["C"], FRAME["N"], s, dz=dz) for s, dz in zip(FRAME["seeds"], (0.0, -0.03))]


def run_frames(m, is_hip):
    """the frame case on a HIP map or on the oracle (same calls as tests/test_hip_store_paths.py: _post32_case)"""
    R, t0, clouds = frame_inputs()
    res = 0.04
    if not is_hip:
        m.center = np.zeros(3, np.float32)
    for f, p in enumerate(clouds):
        if f:
            m.move(np.array([FRAME["shift"][0] * res, FRAME["shift"][1] * res, 0.0], np.float64))
        t = (t0 + m.center).astype(np.float32)
        if is_hip:
            m.update_map_with_kernel(p, [], R, t, 1.0, 1.0)
        else:
            m.update_map_with_kernel(p, R, (t - m.center).astype(np.float32), 1.0, 1.0)
        m.update_time()


def _record(out, key, hip):
    out[key + "_map"] = hip.elevation_map
    out[key + "_normal"] = hip.normal_map
    out[key + "_trav_in"] = hip.traversability_input


def main(path):
    from _variant_children import child_setup
    weights = child_setup()
    from _util import make_pair
    from oracle import emap_oracle as eo
    out = {}
    for C, d in CASES:
        cfg = dict(eo.YAML, dilation_size=d)
        e = state(C, d, case_seed(C, d))
        key = case_key(C, d)
        a, _ = make_pair(cfg, C, "reference_fp16", weights)                 # context A: origin 0
        a.elevation_map = e
        a.stage("dilate")
        out[key + "_A_dilate"] = a.traversability_input
        a.stage("post")
        _record(out, key + "_A", a)
        a.close()
        b, _ = make_pair(cfg, C, "reference_fp16", weights)                 # context B: the circular origin inside tiles, the stencils in two parts
        res = float(b.resolution)
        b.move(np.array([SHIFT_B[0] * res, SHIFT_B[1] * res, 0.0], np.float64))
        b.elevation_map = e
        b.stage("dilate")
        out[key + "_B_dilate"] = b.traversability_input
        b._chk(b._lib.emap_post_part(b._ctx, 1))                            # rows that need no halo row ...
        b._chk(b._lib.emap_post_part(b._ctx, 2))                            # ... and the two boundary bands: up to three row segments, tile_rows path
        _record(out, key + "_B", b)
        b.close()
    hip, _ = make_pair(eo.YAML, FRAME["C"], "reference_fp16", weights)
    run_frames(hip, True)
    _record(out, FRAME_KEY, hip)
    hip.close()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
