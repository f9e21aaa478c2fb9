"""What the plane-segmentation tests share (tests/test_plane_seg_cases.py on the CPU, tests/test_hip_plane_seg.py on the GPU): the NumPy
model of the device chain -- the stages of elevation_mapping_cupy_amd/plane_segmentation.py composed in the device's order, so that a
lost piece can take a stage's place --, the scenes, the lost-piece variants and independent restatements to check the model against
(numpy.linalg.eigh for the window planes, plain double sums of SlidingWindowPlaneExtractor.cpp:170-199 for the label planes).

Scenes are height planes in published index space.  Three means make a cell not planar, each by a wide margin: no finite height; a
window that mixes floor cells with a 1 m wall (the fitted plane is steeper than 75 degrees); a rough checker of +-5 cm (error test).
``carve(P)`` turns a mask of thin lines into heights whose planar cells are exactly P: floor within one cell of P, a one-cell ring of
wall around it, nothing (NaN) beyond."""
import types

import numpy as np

from elevation_mapping_cupy_amd import plane_segmentation as ps

RES = float(np.float32(0.04))
ORIGIN = (3.14, -1.62)
DEFAULTS = dict(kernel_size=3, planarity_opening_filter=0, plane_inclination_threshold_degrees=30.0, local_plane_inclination_threshold_degrees=35.0,
                plane_patch_error_threshold=0.02, min_number_points_per_label=4, connectivity=4, global_plane_fit_distance_error_threshold=0.025,
                global_plane_fit_angle_error_threshold_degrees=25.0)
# cell_n of the GPU tests: M = 32 (one 32 x 32 tile), 65 (3 x 3 ragged tiles) and 363: ceil(363^2 / 32) = 4118 bit words, past the 4096
# words (EM_CLOUD_SCAN_TRIP) the numbering scan's one workgroup takes in a single trip -- the carry between trips is exercised
SIZES = (34, 67, 365)
BIG_SCENES = ("flat", "checkerboard", "serpentine", "spiral", "pieces")      # the scenes that also run at the largest size
LOST = ("no border merge", "lost arm", "no flatten", "column-major numbering", "rejected label kept", "no dilation")
WALL, ROUGH = np.float32(1.0), np.float32(0.05)


# ---- the model, stage by stage --------------------------------------------------------------------------------------------------------
def params(**over):
    bad = set(over) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **over)


def model(h, P=None, resolution=RES, origin=ORIGIN, lose=None):
    """the device chain a. - g. on one published plane; ``lose``: one of LOST"""
    P = params(**(P or {}))
    cos_plane, cos_local, cos_angle = ps.cosines(P["plane_inclination_threshold_degrees"], P["local_plane_inclination_threshold_degrees"],
                                                 P["global_plane_fit_angle_error_threshold_degrees"])
    thr = float(P["plane_patch_error_threshold"])
    win = ps.window_pass(h, P["kernel_size"], resolution, thr * thr, cos_local)
    planar = ps.opening(win.planar, P["planarity_opening_filter"], dilate=lose != "no dilation")
    root = ps.components(planar, P["connectivity"], merge=lose != "no border merge", flatten=lose != "no flatten", lost_arm=lose == "lost arm")
    labels0, n_labels = ps.numbering(root, column_major=lose == "column-major numbering")
    labels, planes, details = ps.label_planes(h, win.normals, root, labels0, resolution, origin, P["min_number_points_per_label"], cos_plane,
                                              float(P["global_plane_fit_distance_error_threshold"]), cos_angle, reject=lose != "rejected label kept")
    return types.SimpleNamespace(labels=labels, labels0=labels0, n_labels=n_labels, planes=planes, normals=win.normals, planar=planar, window=win,
                                 details=details, root=root, cos=(cos_plane, cos_local, cos_angle), P=P)


def answer(r):
    """the bytes a caller sees"""
    return r.labels.tobytes() + np.int64(r.n_labels).tobytes() + r.planes.tobytes()


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def _dilate(mask, r):
    M = mask.shape[0]
    p = np.pad(mask, r)
    out = np.zeros_like(mask)
    for a in range(2 * r + 1):
        for b in range(2 * r + 1):
            out |= p[a:a + M, b:b + M]
    return out


def carve(P, floor=0.0):
    h = np.full(P.shape, np.nan, np.float32)
    h[_dilate(P, 2)] = np.float32(floor) + WALL
    h[_dilate(P, 1)] = np.float32(floor)
    return h


def serpentine_mask(M):
    """a one-cell-wide path through every tile: the rows 2, 6, 10, ... joined at alternating ends"""
    P = np.zeros((M, M), bool)
    rows = list(range(2, M - 2, 4))
    for k, r in enumerate(rows):
        P[r, 2:M - 2] = True
        if k + 1 < len(rows):
            P[r:r + 5, (M - 3) if k % 2 == 0 else 2] = True
    return P


def comb_mask(M):
    P = np.zeros((M, M), bool)
    P[2, 2:M - 2] = True
    P[2:M - 2, 2:M - 2:4] = True
    return P


def u_mask(M):
    """two arms from the first row, joined only along the last row: the right arm learns its root through the last tile"""
    P = np.zeros((M, M), bool)
    P[2:M - 2, 2] = True
    P[2:M - 2, M - 3] = True
    P[M - 3, 2:M - 2] = True
    return P


def spiral_mask(M):
    P = np.zeros((M, M), bool)
    top, left, bottom, right = 2, 2, M - 3, M - 3
    i, j = top, left
    P[i, j] = True
    while True:
        moved = False
        for di, dj, lim in ((0, 1, lambda: j < right), (1, 0, lambda: i < bottom), (0, -1, lambda: j > left), (-1, 0, lambda: i > top + 4)):
            while lim():
                i, j = i + di, j + dj
                P[i, j] = True
                moved = True
        top, left, bottom, right = top + 4, left + 4, bottom - 4, right - 4
        if not moved or bottom - top < 4 or right - left < 4:
            return P
        while j < left:                                        # on to the next ring
            j += 1
            P[i, j] = True


def pieces(M):
    """small components: roots on a tile border and inside a tile, a single cell, a pair, a collinear triple, a 3-cell corner and a 2 x 2
    block (against min_number_points_per_label = 4), and in an empty corner finite cells whose windows hold 1, 2 and 3 collinear points"""
    P = np.zeros((M, M), bool)
    b = 32 if M > 40 else 16
    P[b, 3:9] = True                                           # root on a tile's first row (at M = 65)
    P[b + 5:b + 10, b] = True                                  # root on a tile's first column
    P[4, 4] = True                                             # one cell
    P[4, 9:11] = True                                          # a pair
    P[4, 15:18] = True                                         # a collinear triple
    P[9, 4] = P[10, 4] = P[10, 5] = True                       # a 3-cell corner
    P[9:11, 10:12] = True                                      # 2 x 2
    P[9:12, 16:21] = True                                      # 3 x 5: a plane
    h = carve(P)
    h[M - 9:, M - 12:] = np.nan
    h[M - 3, M - 3] = 0.25                                     # 1 point
    h[M - 3, M - 8:M - 6] = 0.25                               # 2 points
    h[M - 7, M - 11:M - 8] = 0.25                              # 3 collinear points: the middle eigenvalue is 0
    return h


def scenes(M):
    """name -> (heights float32 (M, M), parameter overrides, properties the CPU tests assert)"""
    i, j = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    flat = np.full((M, M), 0.5, np.float32)
    S = {}
    S["flat"] = (flat, {}, dict(n_labels=1, n_planes=1))
    t = flat.copy(); t[:, M // 2:] += np.float32(0.2)          # a step of 10 x plane_patch_error_threshold
    S["terraces"] = (t, {}, dict(n_labels=2, n_planes=2))
    S["terraces, kernel 5"] = (t, dict(kernel_size=5), dict(n_labels=2, n_planes=2))
    for deg in (20, 32, 45):
        ramp = (np.tan(np.deg2rad(deg)) * RES * i).astype(np.float32)
        S["ramp %d" % deg] = (ramp, {}, dict(n_labels=0 if deg == 45 else 1, n_planes=1 if deg == 20 else 0))
    cb = np.where((i + j) % 2 == 0, np.float32(0.5), np.float32(np.nan)).astype(np.float32)
    S["checkerboard"] = (cb, {}, dict(n_planes=0))
    S["checkerboard, connectivity 8"] = (cb, dict(connectivity=8), dict(n_labels=1, n_planes=1))
    S["serpentine"] = (carve(serpentine_mask(M)), {}, dict(mask=serpentine_mask(M), n_labels=1, n_planes=1))
    S["comb"] = (carve(comb_mask(M)), {}, dict(mask=comb_mask(M), n_labels=1, n_planes=1))
    S["U"] = (carve(u_mask(M)), {}, dict(mask=u_mask(M), n_labels=1, n_planes=1))
    S["spiral"] = (carve(spiral_mask(M)), {}, dict(mask=spiral_mask(M), n_labels=1, n_planes=1))
    S["spiral, connectivity 8"] = (carve(spiral_mask(M)), dict(connectivity=8), dict(n_labels=1))
    S["pieces"] = (pieces(M), {}, dict(n_labels=8, n_planes=4))
    S["pieces, 3 points suffice"] = (pieces(M), dict(min_number_points_per_label=0), dict(n_labels=8, n_planes=6))
    nf = flat.copy(); nf[5, 5] = np.inf; nf[9, 9] = -np.inf; nf[20, 20] = np.nan; nf[0, 0] = np.nan; nf[M - 1, 7] = np.inf
    S["inf and NaN"] = (nf, {}, dict(n_labels=1, n_planes=1))
    S["offset by 50 m"] = ((t + np.float32(50.0)).astype(np.float32), {}, dict(n_labels=2, n_planes=2))
    o = flat.copy(); o[12, 17] += np.float32(0.025)            # one outlier: 2.5 x the distance threshold of this scene
    S["outlier"] = (o, dict(global_plane_fit_distance_error_threshold=0.01), dict(n_labels=1, n_planes=1, needs=[1]))
    rough = np.where((i + j) % 2 == 0, ROUGH, -ROUGH).astype(np.float32)
    br = rough.copy(); br[2:14, 2:14] = 0; br[2:14, 18:30] = 0; br[6:9, 13:19] = 0      # two blocks of planar cells joined by a one-cell bridge (row 7)
    S["bridge"] = (br, dict(plane_patch_error_threshold=0.005), dict(n_labels=1, n_planes=1))
    S["bridge, opening 1"] = (br, dict(plane_patch_error_threshold=0.005, planarity_opening_filter=1), dict(n_labels=2, n_planes=2))
    return S


# ---- independent restatements ---------------------------------------------------------------------------------------------------------
def eigh_window(win):
    """per cell with at least 3 points: LAPACK's eigenvalues (ascending) and smallest eigenvector (z >= 0) of the model's covariance"""
    c = win.cov
    A = np.stack([np.stack([c[0], c[1], c[2]], -1), np.stack([c[1], c[3], c[4]], -1), np.stack([c[2], c[4], c[5]], -1)], -2)
    A = np.where(np.isfinite(A), A, 0.0)
    w, v = np.linalg.eigh(A)
    n0 = v[..., :, 0]
    n0 = np.where(n0[..., 2:3] < 0.0, -n0, n0)
    return w, n0


def double_label_planes(h, labels0, resolution, origin, min_points):
    """computePlaneParametersForLabel's sums (:170-199) in plain double about the map origin, label by label: {label: (n, support, normal)}"""
    M = h.shape[0]
    out = {}
    counts = np.bincount(labels0[np.isfinite(h)].ravel(), minlength=int(labels0.max()) + 1)
    for lab in np.nonzero(counts >= max(min_points, 3))[0]:
        if lab == 0:
            continue
        ii, jj = np.nonzero((labels0 == lab) & np.isfinite(h))
        n = ii.size
        pts = np.stack([origin[0] - ii * resolution, origin[1] - jj * resolution, h[ii, jj].astype(np.float64)], 1)
        mean = pts.sum(0) / n
        cov = pts.T @ pts / n - np.outer(mean, mean)
        w, v = np.linalg.eigh(cov)
        nv = v[:, 0] if w[1] > 1e-8 else np.array([0.0, 0.0, 1.0])
        out[int(lab)] = (n, mean, -nv if nv[2] < 0 else nv)
    return out


def logical_plane(pub, C, border=0.0):
    """the (C, C) logical plane whose published view (border stripped, both axes flipped) is ``pub`` (M, M)"""
    out = np.full((C, C), border, np.float32)
    out[1:C - 1, 1:C - 1] = np.asarray(pub, np.float32)[::-1, ::-1]
    return out
