"""What the planar-terrain tests share (tests/test_planar_terrain_cases.py on the CPU, tests/test_hip_planar_terrain.py on the GPU): the
scenes, the parameter sets, the lost pieces and independent restatements to check the model
(elevation_mapping_cupy_amd/planar_terrain.py) against -- a literal transcription of grid_map_filters_rsl's minValues sweep
(inpainting.cpp:58-93), a per-cell loop over the shifted window of applyKernelFunction (processing.cpp:158-176).

Scenes are height planes in published index space; the builders of tests/_plane_seg_cases.py (terraces, checkerboard, rough checker,
carve) are reused by import.  Sizes of the smoothing kernels are given in CELLS here and turned into the reference's half widths in
metres by ``post_of``."""
import numpy as np

import _plane_seg_cases as pc
from elevation_mapping_cupy_amd import planar_terrain as pt

RES = pc.RES
# cell_n of the GPU tests: M = 32 (one union-find tile), 33 (a ragged second tile; a kernel of 31 cells fits), 65 (3 x 3 tiles, the last
# ragged), 363 (once: past the 4096 mask words of one scan trip)
SIZES = (34, 35, 67)
BIG = 365
LOST = ("no halo", "clipped window", "rectangle")
NAN = np.float32(np.nan)


def post_of(resolution, kd=None, kb=None, kg=None, **rest):
    """postprocess keywords with the smoothing kernels given in cells (odd); the other keys as they are"""
    out = dict(rest)
    for name, k in (("smoothing_dilation_size", kd), ("smoothing_box_kernel_size", kb), ("smoothing_gauss_kernel_size", kg)):
        if k is not None:
            assert k % 2 == 1
            out[name] = (k // 2) * float(resolution)
            assert pt.kernel_cells(out[name], resolution) == k
    return out


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def hole(M):
    """terraces with a NaN hole that spans four 32 x 32 tiles at M = 65 (rows and columns 20 .. 35 cross 32); its smallest rim value lies
    below the hole's last row, in the tile that holds only 4 x 4 of its cells"""
    h = pc.scenes(M)["terraces"][0].copy()
    a, b = (20, 36) if M >= 48 else (M // 2 - 6, M // 2 + 6)
    h[a:b, a:b] = NAN
    h[a - 3:a, a + 2] = NAN                                    # an arm, so that the component is not a rectangle
    h[b, b - 2] = np.float32(0.125)                            # the rim's minimum
    return h


def nan_edge(M):
    h = pc.scenes(M)["terraces"][0].copy()
    h[0, :] = NAN
    h[:, M - 1] = NAN
    h[5:9, 0] = NAN
    return h


def nan_frame(M):
    """one NaN component that touches all four edges"""
    h = np.full((M, M), 0.5, np.float32)
    h[0, :] = h[M - 1, :] = h[:, 0] = h[:, M - 1] = NAN
    h[M // 2, :] = NAN
    h[1, 2] = np.float32(0.25)                                # on the rim
    return h


def plateau(M):
    """a planar plateau that touches every edge and corner (a cross plus the four corners) above rough ground: the shifted window of
    the sloped dilation shows along every edge"""
    i, j = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    h = np.where((i + j) % 2 == 0, pc.ROUGH, -pc.ROUGH).astype(np.float32)
    c = M // 2
    h[c - 4:c + 5, :] = np.float32(0.5)
    h[:, c - 4:c + 5] = np.float32(0.5)
    for a in (slice(0, 6), slice(M - 6, M)):
        for b in (slice(0, 6), slice(M - 6, M)):
            h[a, b] = np.float32(0.75)
    return h


def hills(M, seed=3):
    """smooth terrain with a little noise and a few holes"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    h = (0.3 * np.sin(i * 0.11) * np.cos(j * 0.07) + 0.002 * rng.standard_normal((M, M))).astype(np.float32)
    h[rng.random((M, M)) < 0.02] = NAN
    return h


def scenes(M):
    """name -> (heights float32 (M, M), segmentation overrides)"""
    S = pc.scenes(M)
    i, j = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    rough = np.where((i + j) % 2 == 0, pc.ROUGH, -pc.ROUGH).astype(np.float32)
    out = {
        "terraces": (S["terraces"][0], {}),
        "checkerboard": (S["checkerboard"][0], {}),
        "checkerboard, connectivity 8": (S["checkerboard"][0], dict(connectivity=8)),
        "bridge": S["bridge"][:2],
        "pieces": (S["pieces"][0], {}),
        "inf and NaN": (S["inf and NaN"][0], {}),
        "hole": (hole(M), {}),
        "NaN edges": (nan_edge(M), {}),
        "NaN frame": (nan_frame(M), {}),
        "all NaN": (np.full((M, M), NAN, np.float32), {}),
        "no planar cell": (rough, {}),
        "plateau": (plateau(M), {}),
        "hills": (hills(M), {}),
    }
    return out


BIG_SCENES = ("hole", "checkerboard")
PRE = dict(kernelSize=3, numberOfRepeats=1)


def parameter_sets(resolution):
    """name -> (preprocess, postprocess): what runs on the scenes of SWEEP_SCENES besides the defaults"""
    P = {}
    for k in (1, 31):
        P["kd %d" % k] = (None, post_of(resolution, kd=k))
        P["kb %d" % k] = (None, post_of(resolution, kb=k))
        P["kg %d" % k] = (None, post_of(resolution, kg=k))
    P["kg 9"] = (None, post_of(resolution, kg=9))
    P["all 31"] = (PRE, post_of(resolution, kd=31, kb=31, kg=31, nonplanar_horizontal_offset=15))
    for k in (3, 5):
        for n in (1, 3):
            P["median %d x %d" % (k, n)] = (dict(kernelSize=k, numberOfRepeats=n), None)
    P["median 9 clamps to 5, resolution given"] = (dict(kernelSize=9, numberOfRepeats=2, resolution=resolution), None)
    P["median 1"] = (dict(kernelSize=1, numberOfRepeats=3), None)
    for o in (0, 1, 15):
        P["offset %d" % o] = (None, dict(nonplanar_horizontal_offset=o))
    P["planes lifted only"] = (None, dict(extracted_planes_height_offset=0.03, nonplanar_height_offset=0.0))
    P["non-planar lifted only"] = (None, dict(extracted_planes_height_offset=0.0, nonplanar_height_offset=0.02))
    P["both lifted"] = (PRE, dict(extracted_planes_height_offset=-0.01, nonplanar_height_offset=0.05))
    P["no lift"] = (None, dict(extracted_planes_height_offset=0.0, nonplanar_height_offset=0.0, nonplanar_horizontal_offset=0))
    return P


SWEEP_SCENES = ("plateau", "hole", "hills")


# ---- independent restatements ---------------------------------------------------------------------------------------------------------
def min_values_sweep(h):
    """the reference's loop, literally (inpainting.cpp:58-93): column outer, row inner, the output read and written in place, until a
    sweep changes nothing"""
    h_in = np.asarray(h, np.float32)
    out = h_in.copy()
    rows, cols = h_in.shape
    has_value, changed = True, True
    while changed and has_value:
        has_value, changed = False, False
        for c in range(cols):
            for r in range(rows):
                if np.isnan(h_in[r, c]):
                    for rr, cc, ok in ((r, c - 1, c > 0), (r, c + 1, c < cols - 1), (r - 1, c, r > 0), (r + 1, c, r < rows - 1)):
                        if ok:
                            v = out[rr, cc]
                            if not np.isnan(v) and (v < out[r, c] or np.isnan(out[r, c])):
                                out[r, c] = v
                                changed = True
                else:
                    has_value = True
    return out


def sloped_loop(h, k, resolution):
    """applyKernelFunction (processing.cpp:158-176) with Postprocessing.cpp:128's function, cell by cell"""
    h = np.asarray(h, np.float32)
    M = h.shape[0]
    off = pt.slope_offsets(k, resolution)
    out = np.empty((M, M), np.float32)
    half = (k - 1) // 2
    for c in range(M):
        for r in range(M):
            cc, cr = max(c - half, 0), max(r - half, 0)
            if cc + k > M:
                cc = M - k
            if cr + k > M:
                cr = M - k
            with np.errstate(invalid="ignore"):
                v = h[cr:cr + k, cc:cc + k] - off
            v = v[np.isfinite(v)]
            out[r, c] = v.max() if v.size else pt.NAN
    return out


def same_words(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    w = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(w) == b.view(w)).all())
