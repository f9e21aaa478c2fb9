"""Case table of tests/test_hip_trip_edges.py and tests/test_trip_cases.py: clouds on a 130-cell map (27 sort tiles of 16 x 64 cells, the
last tile row one usable row high, the last tile column one usable column wide) that put the kernels of the binned frame (emap_binned.hip) and of the
stencil pass (emap_kernels.hip) on either side of the depth of their load batches:

  * OCCUPANCY -- clouds built cell by cell so that chosen tiles hold exactly 0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 4096 and 4097
    records: a tile kernel's workgroup is 1024 threads, k_tile_count and k_tile_fuse request a thread's first record in front of the
    staging and walk the rest of a tile 1024 records at a time (1025, 2049: one record in a further trip), 4096 is the largest tile
    that is not heavy and 4097 the first heavy one (the frames after the first that the host has heard of run the split kernels,
    four records per thread and trip).  Several points share a cell; NaN rows, points beyond the map and points in border cells lie in
    between; the rows are shuffled so that every tile's records come from every chunk.
  * SCATTER -- uniform clouds of 1 ... 6145 points: zero to 2 * SCATTER_U + 1 points per thread of k_bin_scatter's 4096-point chunk
    (512 threads, batches of four), a partial last chunk, with and without carried channel columns.
  * POST -- the stencil staging of k_post requests the wave's rows and POST_KW = 2 pairs of the column walk per thread and turn: the
    walk of a tile of R rows at radius d has (R + 6 + 2 d)(6 + 2 d) pairs for 512 threads.  tests/_post_variants.py's radii give 1, 2 and
    3 pairs per thread for R = 4 (d = 1, 10, 13), R = 8 (d = 3, 10, 12) and R = 32 (d = 1, 3, 10) but only 1 and 3 for R = 16
    (d = 3: 336 pairs, d = 10: 1092); POST_CASES adds d = 5 (32 x 16 = 512 pairs: exactly one per thread) and d = 6 (34 x 18 = 612:
    two for some), run with EMAP_POST_R=16 through tests/_post_variants.py as a child program.  The ROWS of the same loop go U per wave
    and turn, 8 waves: 32 per turn for R = 16 (U = 4), where the two radii give 16 + 6 + 2 d = 32 and 34 region rows, and 48 per turn for
    R = 32 (U = 6), where a second child with EMAP_POST_R=32 gives 48 (exactly one turn) and 50 (rows 48 and 49 in the second turn: one row for
    each of two waves, every other slot of that turn clamped to the last row and dropped).  There the boundary bands of context B (d + 4 = 9 and 10 rows high)
    run 16-row tiles by the host's own rule (emap_post_part), as in tests/test_hip_post_variants.py's table.

Inputs are numpy only.  Run as a program it is the stencil child: python tests/_trip_cases.py <out.npz>."""
import sys

import numpy as np

C = 130
RES = 0.04
TILES_Y, TILES_X = 9, 3
FRAMES = 3
TIME_TICKS = 1
CH = ["x", "y", "z", "s0", "s1", "c0", "rgb"]
FUSIONS = {"rgb": "color", "c0": "class_average", "default": "average"}

# records per tile (tile row, tile column).  Tile row 8 holds cell row 128 only, tile column 2 cell column 128 only (129 is the border).
LIGHT = {
    (0, 0): 1023, (0, 1): 1024, (0, 2): 1,
    (1, 0): 1025, (1, 1): 2047, (1, 2): 0,
    (2, 0): 2048, (2, 1): 2049, (2, 2): 40,
    (3, 0): 4096, (3, 1): 0, (3, 2): 0,
    (4, 0): 1, (4, 1): 973, (4, 2): 5,
    (5, 0): 300, (5, 1): 3000, (5, 2): 0,
    (6, 0): 0, (6, 1): 700, (6, 2): 17,
    (7, 0): 1500, (7, 1): 64, (7, 2): 0,
    (8, 0): 130, (8, 1): 1, (8, 2): 2,
}
HEAVY = dict(LIGHT)
HEAVY[(6, 0)] = 4097
EDGE_COUNTS = (0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 4096)
N_NAN, N_OUTSIDE, N_BORDER = 37, 53, 29

OCCUPANCY = [
    dict(key="open_fp16", layout="light", mode="reference_fp16", rays=False, noise=1.0, sem=False),
    dict(key="shut_fp16", layout="light", mode="reference_fp16", rays=False, noise=0.0, sem=False),
    dict(key="open_fp32", layout="light", mode="fp32", rays=False, noise=1.0, sem=False),
    dict(key="open_fp16_rays", layout="light", mode="reference_fp16", rays=True, noise=1.0, sem=False),
    dict(key="shut_fp32_rays", layout="light", mode="fp32", rays=True, noise=0.0, sem=False),
    dict(key="heavy_open_fp16", layout="heavy", mode="reference_fp16", rays=False, noise=1.0, sem=False),
    dict(key="heavy_open_fp16_rays", layout="heavy", mode="reference_fp16", rays=True, noise=1.0, sem=False),
    dict(key="sem_open_fp16", layout="light", mode="reference_fp16", rays=False, noise=1.0, sem=True),
]
SCATTER_NS = (1, 2, 511, 512, 513, 2047, 2048, 2049, 6145)
SCATTER = [dict(key="n%d%s" % (n, "_ch" if ch else ""), N=n, sem=ch, mode="reference_fp16", rays=False, noise=1.0) for ch in (False, True) for n in SCATTER_NS]
SCATTER_FRAMES = 2

POST_CASES = [(202, 5), (202, 6)]
# child -> the hooks it runs under, and the kernel of each case's five launches: A dilate, A post, B dilate, B part 1, B part 2
POST_CHILDREN = {
    "r16_walk": dict(env={"EMAP_POST_R": "16", "EMAP_POST_DMA": "0"}, kernels=("k_post<16",) * 5),
    "r32_rows": dict(env={"EMAP_POST_R": "32", "EMAP_POST_DMA": "0"}, kernels=("k_post<32",) * 4 + ("k_post<16",)),
}
POST_ROWS_PER_TURN = {16: 8 * 4, 32: 8 * 6}          # waves x U of k_post's staging


def layout(name):
    return {"light": LIGHT, "heavy": HEAVY}[name]


def pose():
    """identity: cell row = floor(x / RES + 65), cell column = floor(y / RES + 65); the sensor one metre above the map's centre"""
    return np.eye(3, dtype=np.float32), np.array([0, 0, 1], np.float32)


def tile_cells(ty, tx):
    """the cells of a tile that take points: inside the map proper (rows and columns 1 ... 128)"""
    rows = [r for r in range(16 * ty, 16 * ty + 16) if 1 <= r <= C - 2]
    cols = [c for c in range(64 * tx, 64 * tx + 64) if 1 <= c <= C - 2]
    return rows, cols


def _xyz(rng, rows, cols, dz):
    """points inside the given cells, a tenth of a cell clear of their edges; heights follow a smooth surface 0.55 ... 0.95 m below the
    sensor (beyond min_valid_distance everywhere) with 2 cm of noise, so that later frames find drift inliers"""
    n = len(rows)
    p = np.empty((n, 3), np.float32)
    p[:, 0] = (rows - C / 2 + rng.uniform(0.1, 0.9, n)) * RES
    p[:, 1] = (cols - C / 2 + rng.uniform(0.1, 0.9, n)) * RES
    p[:, 2] = -0.75 + 0.15 * np.sin(rows * 0.11) * np.cos(cols * 0.07) + rng.uniform(-0.02, 0.02, n) + dz
    return p


def occupancy_cloud(name, frame, sem=False):
    """frame `frame` of a layout: (N, 3) float32, or (N, 7) with two features, a class probability and a packed colour"""
    rng = np.random.default_rng(7000 + 10 * frame + (name == "heavy"))
    rows, cols = [], []
    for (ty, tx), n in sorted(layout(name).items()):
        rr, cc = tile_cells(ty, tx)
        rows.append(np.asarray(rr)[rng.integers(0, len(rr), n)]); cols.append(np.asarray(cc)[rng.integers(0, len(cc), n)])
    good = _xyz(rng, np.concatenate(rows), np.concatenate(cols), -0.01 * frame)
    nan = _xyz(rng, rng.integers(1, C - 1, N_NAN), rng.integers(1, C - 1, N_NAN), 0.0)
    nan[np.arange(N_NAN), rng.integers(0, 3, N_NAN)] = np.nan
    out = _xyz(rng, rng.choice([-7, -1, C, C + 12], N_OUTSIDE), rng.integers(-3, C + 3, N_OUTSIDE), 0.0)       # beyond the map in x (some in y too)
    border = _xyz(rng, rng.choice([0, C - 1], N_BORDER), rng.integers(0, C, N_BORDER), 0.0)                     # in the map, never inside
    border[::2] = border[::2][:, [1, 0, 2]]                                                                     # ... half of them in border columns
    p = np.concatenate([good, nan, out, border])
    p = p[rng.permutation(len(p))]
    return _with_channels(p, rng) if sem else p


def _with_channels(p, rng):
    q = np.empty((len(p), 7), np.float32)
    q[:, :3] = p
    q[:, 3:6] = rng.uniform(0, 1, (len(p), 3))
    q[:, 6] = rng.integers(0, 1 << 24, len(p), dtype=np.uint32).view(np.float32)
    return q


def scatter_cloud(n, frame, sem=False):
    import _fixtures as fx
    p = fx.cloud(C, n, 9000 + 7 * n + frame, dz=-0.02 * frame)
    return _with_channels(p, np.random.default_rng(9500 + 7 * n + frame)) if sem else p


def scatter_pose():
    import _fixtures as fx
    R, t = fx.POSES["rotated"]
    return R, t.copy()


def records_per_tile(orc, p, R, t):
    """{(tile row, tile column): records} of a cloud by the oracle's own index arithmetic: valid points inside the map, per sort tile"""
    idx, valid, inside = orc.point_index(p, R, t)
    idx = idx[(valid != 0) & (inside != 0)].astype(np.int64)
    n = np.bincount((idx // C) // 16 * TILES_X + (idx % C) // 64, minlength=TILES_Y * TILES_X)
    return {(ty, tx): int(n[ty * TILES_X + tx]) for ty in range(TILES_Y) for tx in range(TILES_X)}


def config(case, yaml):
    return dict(yaml, enable_visibility_cleanup=bool(case["rays"]))


def case_frames(case):
    """(R, t, clouds) of an occupancy or scatter case"""
    if "layout" in case:
        R, t = pose()
        return R, t, [occupancy_cloud(case["layout"], f, case["sem"]) for f in range(FRAMES)]
    R, t = scatter_pose()
    return R, t, [scatter_cloud(case["N"], f, case["sem"]) for f in range(SCATTER_FRAMES)]


def main(path):
    """the stencil child: tests/_post_variants.py's program on POST_CASES (its hooks are read once per process)"""
    import _post_variants as pv
    pv.CASES = list(POST_CASES)
    pv.main(path)


if __name__ == "__main__":
    main(sys.argv[1])
