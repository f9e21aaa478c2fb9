"""What the planar-region tests share (tests/test_planar_region_cases.py on the CPU, tests/test_hip_planar_regions.py on the GPU): the
label scenes of the regions mode, the masks of the raw mode, the lost pieces, and independent restatements to check the model
(elevation_mapping_cupy_amd/planar_regions.py) against -- Upsampling.cpp's loops written out literally, OpenCV's elliptic element from
its formula, per-label erosions and components with scipy.ndimage.

A label scene is ``(labels int32 (M, M), n_labels)``; a mask is int32 (M, M) of 0 and 1."""
import functools

import numpy as np

from elevation_mapping_cupy_amd import planar_regions as pr

# M of the regions mode: U = 22 (one union-find tile), 34 (a tile border at 32), 97 (ragged tiles), 193 (the crack mask past the 4096 words of one
# scan trip: U U / 8 > 4096), 364 (the pixel masks past it: U U / 32 > 4096)
LABEL_SIZES = (8, 12, 33, 65, 122)
RAW_SIZES = (33, 65, 182, 363)
MARGINS = (0, 1, 4)
LOST = {"no border merge": dict(merge=False), "4-connected turn": dict(conn8=False), "frame not zeroed": dict(frame=False),
        "fallback ignored": dict(fallback=False), "edge pixels x 3": dict(edge3=True), "one doubling round short": dict(short=1)}


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def label_scenes(M):
    i, j = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    z = lambda: np.zeros((M, M), np.int32)      # noqa: E731
    S = {}
    L = z(); L[2:M - 2, 2:M - 3] = 1
    S["rectangle inside"] = (L, 1)
    L = z(); L[0:M // 2, M - M // 2 - 1:M] = 1
    S["rectangle flush with two edges"] = (L, 1)
    L = np.ones((M, M), np.int32); L[2:M - 2, 2:M - 2] = 0; L[M // 2 - 1:M // 2 + 1, M // 2 - 1:M // 2 + 1] = 2
    S["ring with an island"] = (L, 2)
    L = z(); L[1:M - 1, 1:M // 2] = 1; L[1:M - 1, M // 2:M - 1] = 2
    S["two labels 4-adjacent"] = (L, 2)
    L = z(); L[1:M // 2, 1:M // 2] = 3; L[M // 2:M - 1, M // 2:M - 1] = 1
    S["two labels diagonal-adjacent"] = (L, 3)
    L = z(); L[1, 1:M - 1] = 1; L[M - 3:M - 1, 1:M - 1] = 2
    S["lines"] = (L, 2)                                        # one cell wide: no region; two cells wide: a region only by the fallback
    S["empty"] = (z(), 0)
    S["full"] = (np.ones((M, M), np.int32), 1)
    L = (((i // 4) * 3 + (j // 5)) % 4).astype(np.int32)
    S["blocks"] = (L, 3)                                       # every label in several pieces, all pieces 4- or diagonal-adjacent to others
    rng = np.random.default_rng(M)
    L = (rng.integers(0, 4, (M // 3 + 1, M // 3 + 1))[i // 3, j // 3]).astype(np.int32)
    L[rng.random((M, M)) < 0.03] = 0
    S["random blocks"] = (L, 5)                                # (labels 4 and 5 do not occur)
    return S


@functools.lru_cache(maxsize=None)
def spiral(M):
    """a one-pixel spiral with one-pixel gaps: ONE border about twice as long as the spiral"""
    X = np.zeros((M, M), np.int32)
    r, c, dr, dc = 0, 0, 0, 1
    X[0, 0] = 1
    inside = lambda a, b: 0 <= a < M and 0 <= b < M      # noqa: E731
    while True:
        for _ in range(2):
            nr, nc, ar, ac = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            if inside(nr, nc) and X[nr, nc] == 0 and (not inside(ar, ac) or X[ar, ac] == 0):
                r, c = nr, nc
                X[r, c] = 1
                break
            dr, dc = dc, -dr
        else:
            return X


def raw_scenes(M):
    i, j = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    rng = np.random.default_rng(100 + M)
    stairs = ((i == j) | (i + j == M - 1) | ((i // 2 == (j + 5) // 2) & (j > 3)) | (((i - 9) // 3 == j // 3) & (i > 9))).astype(np.int32)
    return {"checkerboard": ((i + j) % 2 == 0).astype(np.int32), "spiral": spiral(M).copy(), "staircases": stairs,
            "noise": (rng.random((M, M)) < 0.5).astype(np.int32), "full": np.ones((M, M), np.int32), "empty": np.zeros((M, M), np.int32)}


# ---- independent restatements ---------------------------------------------------------------------------------------------------------
def upsample_loops(image):
    """Upsampling.cpp:12-58, literally"""
    rows, cols = image.shape
    ur, uc = 4 + 3 * (rows - 2), 4 + 3 * (cols - 2)
    out = np.full((ur, uc), -1, image.dtype)

    def column(col_values, target_col):
        for row in range(rows):
            v = col_values[row]
            if row == 0:
                out[0, target_col] = v; out[1, target_col] = v
            elif row + 1 == rows:
                out[ur - 2, target_col] = v; out[ur - 1, target_col] = v
            else:
                t = 2 + 3 * (row - 1)
                out[t, target_col] = v; out[t + 1, target_col] = v; out[t + 2, target_col] = v
    for col in range(cols):
        if col == 0:
            column(image[:, 0], 0); out[:, 1] = out[:, 0]
        elif col + 1 == cols:
            column(image[:, col], uc - 2); out[:, uc - 1] = out[:, uc - 2]
        else:
            t = 2 + 3 * (col - 1)
            column(image[:, col], t); out[:, t + 1] = out[:, t]; out[:, t + 2] = out[:, t + 1]
    return out


def opencv_ellipse(k):
    """getStructuringElement(MORPH_ELLIPSE, (k, k)) from OpenCV's formula (morph.dispatch.cpp): a bool (k, k) matrix"""
    r = c = k // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    elem = np.zeros((k, k), bool)
    for a in range(k):
        dy = a - r
        if abs(dy) <= r:
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) * inv_r2)))
            elem[a, max(c - dx, 0):min(c + dx + 1, k)] = True
    return elem


CROSS3 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)


def erode_label(binary, elem):
    """cv::erode(..., BORDER_REPLICATE) of one label's binary image"""
    from scipy import ndimage as ndi
    h = elem.shape[0] // 2
    return ndi.binary_erosion(np.pad(binary, h, mode="edge"), structure=elem, border_value=1)[h:-h, h:-h]


def same_answer(a, b):
    return a.rings.tobytes() == b.rings.tobytes() and a.vertices.tobytes() == b.vertices.tobytes() and a.rings.shape == b.rings.shape and a.vertices.shape == b.vertices.shape
