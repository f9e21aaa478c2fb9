"""Host model of the planar terrain on the device (``emap_planar_terrain``, csrc/emap_terrain.hip): NumPy with the
device's arithmetic and operation order, stage by stage.  It is the A/B route of ``ElevationMap.get_planar_terrain``
(``EMAP_TERRAIN_RESIDENT=0``: the source layer is downloaded and everything is computed here) and what the tests compare the device
against, bit for bit.  The stages restate convex_plane_decomposition's GridMapPreprocessing.cpp:14-39 and Postprocessing.cpp:14-146,
grid_map_filters_rsl's inpainting.cpp:25-94 and processing.cpp:145-177, and OpenCV's medianBlur, getStructuringElement(MORPH_ELLIPSE),
dilate / erode, boxFilter and GaussianBlur with BORDER_REPLICATE; neither library is pinned by a compiled reference.  Every plane is
``(M, M)`` in published index space, cell ``(i, j)`` at ``idx = i * M + j``.

Minima, maxima and medians are taken on a float's monotone KEY (``key``): an int32 whose order is the numeric order, -0 below +0, so
that every selecting stage is a function of the bits.  Every NaN a stage computes or makes up is the quiet NaN 0x7fc00000."""
from __future__ import annotations

import math
import types

import numpy as np

from . import plane_segmentation as ps

KERNEL_MAX, OFFSET_MAX, REPEATS_MAX = 31, 15, 8      # EM_TERRAIN_KERNEL_MAX / _OFFSET_MAX / _REPEATS_MAX
NO_KEY = np.int32(0x7fffffff)
NAN = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]
PLANES = ("elevation", "smooth_planar", "plane_classification", "elevation_before_postprocess",
          "elevationWithNaN", "elevationWithNaN_i", "elevationWithNaNClosed", "elevationWithNaNClosedDilated")      # bit k of `want`
PREPROCESS_DEFAULTS = dict(kernelSize=3, numberOfRepeats=1)      # PreprocessingParameters (GridMapPreprocessing.h); resolution: the map's
POSTPROCESS_DEFAULTS = dict(extracted_planes_height_offset=0.0, nonplanar_height_offset=0.02, nonplanar_horizontal_offset=1,
                            smoothing_dilation_size=0.2, smoothing_box_kernel_size=0.1, smoothing_gauss_kernel_size=0.05)      # Postprocessing.h:7-25
GAUSS_FIXED = {1: (1.0,), 3: (0.25, 0.5, 0.25), 5: (0.0625, 0.25, 0.375, 0.25, 0.0625),
               7: (0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125)}


# ---- keys -------------------------------------------------------------------------------------------------------------------------------
def key(x):
    """int32 keys of float32 values that are not NaN: signed order = numeric order, -0 below +0; its own inverse on the bits"""
    b = np.ascontiguousarray(x, np.float32).view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7fffffff))


def unkey(k):
    k = np.ascontiguousarray(k, np.int32)
    return np.where(k >= 0, k, k ^ np.int32(0x7fffffff)).astype(np.int32).view(np.float32)


def _one_nan(x):
    return np.where(np.isnan(x), NAN, x).astype(np.float32)


# ---- parameters -------------------------------------------------------------------------------------------------------------------------
def kernel_cells(size, resolution):
    """kernelSizeInPixels (Postprocessing.cpp:75-77): ``2 * int(round(size / res)) + 1``, std::round (half away from zero)"""
    v = float(size) / float(resolution)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError("a smoothing size must be finite and not negative")
    r = math.floor(v)
    return 2 * int(r + 1 if v - r >= 0.5 else r) + 1


def check(M, resolution, preprocess, postprocess):
    """the caller's two dicts, completed and checked as the device door checks them: ``(pre, post, sizes)`` -- ``pre``: ``None`` or
    ``(median size after the clamp, repeats)``; ``post``: every key of POSTPROCESS_DEFAULTS; ``sizes``: ``(kd, kb, kg)`` in cells"""
    cap = min(int(M), KERNEL_MAX)
    pre = None
    if preprocess is not None:
        bad = set(preprocess) - set(PREPROCESS_DEFAULTS) - {"resolution"}
        if bad:
            raise ValueError("unknown preprocess keys: %s" % sorted(bad))
        if "resolution" in preprocess and abs(float(preprocess["resolution"]) - float(resolution)) > 1e-6:
            raise ValueError("preprocess resolution %r is not the map's %r: resampling is not part of get_planar_terrain" % (preprocess["resolution"], resolution))
        q = dict(PREPROCESS_DEFAULTS, **{k: v for k, v in preprocess.items() if k != "resolution"})
        k, n = max(1, min(int(q["kernelSize"]), 5)), int(q["numberOfRepeats"])      # (GridMapPreprocessing.cpp:21)
        if k % 2 == 0 or k > cap:
            raise ValueError("kernelSize must be odd after its clamp to 1 .. 5 (cv::medianBlur), and at most the map's side")
        if not 0 <= n <= REPEATS_MAX:
            raise ValueError("numberOfRepeats must lie in 0 .. %d" % REPEATS_MAX)
        pre = (k, n)
    bad = set(postprocess or {}) - set(POSTPROCESS_DEFAULTS)
    if bad:
        raise ValueError("unknown postprocess keys: %s" % sorted(bad))
    post = dict(POSTPROCESS_DEFAULTS, **(postprocess or {}))
    post["nonplanar_horizontal_offset"] = int(post["nonplanar_horizontal_offset"])
    for k in POSTPROCESS_DEFAULTS:
        if k != "nonplanar_horizontal_offset":
            post[k] = float(post[k])
            if not math.isfinite(post[k]):
                raise ValueError("%s must be finite" % k)
    if not 0 <= post["nonplanar_horizontal_offset"] <= OFFSET_MAX or 2 * post["nonplanar_horizontal_offset"] + 1 > cap:
        raise ValueError("nonplanar_horizontal_offset must lie in 0 .. %d, its kernel within the map's side" % OFFSET_MAX)
    sizes = tuple(kernel_cells(post[k], resolution) for k in ("smoothing_dilation_size", "smoothing_box_kernel_size", "smoothing_gauss_kernel_size"))
    if any(k > cap for k in sizes):
        raise ValueError("a smoothing kernel must be at most %d cells and at most the map's side (%d): %r" % (KERNEL_MAX, M, sizes))
    return pre, post, sizes


# ---- P1: minValues ------------------------------------------------------------------------------------------------------------------------
def nan_roots(nan):
    """a number in [0, M * M) per 4-connected component of the mask, -1 elsewhere: the device's union-find (any labelling of the same
    partition gives the same fill -- tools/exp_planar_terrain.py puts scipy.ndimage.label here for large maps)"""
    return ps.components(nan, 4)


def inpaint_min(h):
    """the fixed point of minValues (inpainting.cpp:25-94): every NaN cell gets the smallest (by key) of the cells that are not NaN and
    4-adjacent to its 4-connected NaN component; a component without such a cell stays as it is"""
    h = np.ascontiguousarray(h, np.float32)
    M = h.shape[0]
    nan = np.isnan(h)
    root = nan_roots(nan)
    k = key(np.where(nan, np.float32(0.0), h))
    amin = np.full(M * M, NO_KEY, np.int32)
    for sl_c, sl_n in (((slice(None), slice(1, M)), (slice(None), slice(0, M - 1))), ((slice(None), slice(0, M - 1)), (slice(None), slice(1, M))),
                       ((slice(1, M), slice(None)), (slice(0, M - 1), slice(None))), ((slice(0, M - 1), slice(None)), (slice(1, M), slice(None)))):
        on = ~nan[sl_c] & nan[sl_n]
        np.minimum.at(amin, root[sl_n][on], k[sl_c][on])
    got = np.where(nan, amin[np.maximum(root, 0).ravel()].reshape(M, M), NO_KEY)
    return np.where(got != NO_KEY, unkey(np.where(got != NO_KEY, got, 0)), h).astype(np.float32)


# ---- P2: median ---------------------------------------------------------------------------------------------------------------------------
def _windows(h, k):
    M, r = h.shape[0], k // 2
    p = np.pad(h, r, mode="edge")
    return [p[a:a + M, b:b + M] for a in range(k) for b in range(k)]


def median(h, k, repeats=1):
    """cv::medianBlur on a float image, BORDER_REPLICATE, ``repeats`` times: the (k^2 - 1) / 2-th order statistic by key; a window with
    a NaN gives NaN"""
    h = np.ascontiguousarray(h, np.float32)
    if k <= 1:
        return h
    for _ in range(repeats):
        w = np.stack(_windows(h, k))
        nan = np.isnan(w).any(axis=0)
        srt = np.sort(key(np.where(np.isnan(w), np.float32(0.0), w)), axis=0)
        h = np.where(nan, NAN, unkey(srt[(k * k - 1) // 2])).astype(np.float32)
    return h


# ---- Q2 / Q5: the elliptic element ----------------------------------------------------------------------------------------------------------
def ellipse_spans(k):
    """getStructuringElement(MORPH_ELLIPSE, (k, k)): per row the columns ``[lo, hi)``"""
    r = c = k // 2
    out = []
    for a in range(k):
        dy = a - r
        dx = int(np.rint(c * math.sqrt((r * r - dy * dy) / (r * r)))) if r else 0
        out.append((max(c - dx, 0), min(c + dx + 1, k)))
    return out


def ellipse(k, rectangle=False):
    """the element as a bool ``(k, k)`` array (``rectangle``: a test's lost piece)"""
    f = np.zeros((k, k), bool)
    for a, (lo, hi) in enumerate(ellipse_spans(k)):
        f[a, lo:hi] = True
    return np.ones((k, k), bool) if rectangle else f


def morph(h, k, dilate, footprint=None, halo=True):
    """maximum (``dilate``) or minimum over the element of clamp-indexed values, NaN skipped, all NaN: NaN.  ``halo=False``: cells outside
    the map are absent instead of replicated (a test's lost piece)"""
    h = np.ascontiguousarray(h, np.float32)
    M, r = h.shape[0], k // 2
    f = ellipse(k) if footprint is None else footprint
    p = np.pad(h, r, mode="edge") if halo else np.pad(h, r, constant_values=np.nan)
    nan = np.isnan(p)
    ident = np.int32(-0x80000000) if dilate else NO_KEY
    kp = np.where(nan, ident, key(np.where(nan, np.float32(0.0), p)))
    best = np.full((M, M), ident, np.int32)
    any_ = np.zeros((M, M), bool)
    for a in range(k):
        for b in range(k):
            if f[a, b]:
                v = kp[a:a + M, b:b + M]
                best = np.maximum(best, v) if dilate else np.minimum(best, v)
                any_ |= ~nan[a:a + M, b:b + M]
    return np.where(any_, unkey(np.where(any_, best, 0)), NAN).astype(np.float32)


def closing(h, k, **kw):
    return morph(morph(h, k, True, **kw), k, False, **kw)


# ---- Q3: the sloped dilation ----------------------------------------------------------------------------------------------------------------
def slope_offsets(k, resolution):
    """(Postprocessing.cpp:116-125) ``float(double(float(res)) * sqrt(da^2 + db^2))``"""
    res = float(np.float32(resolution))
    d = np.arange(k) - k // 2
    return np.array([[np.float32(res * math.sqrt(float(a * a + b * b))) for b in d] for a in d], np.float32).reshape(k, k)


def corners(M, k, clipped=False):
    """first row of every cell's window (processing.cpp:160-171): moved inwards at an edge, not clipped"""
    c = np.maximum(np.arange(M) - k // 2, 0)
    return c if clipped else np.where(c + k > M, M - k, c)


def sloped_dilation(h, k, resolution, clipped=False):
    """max over the finite ``x - off`` of the SHIFTED k x k window (applyKernelFunction with maxCoeffOfFinites), none finite: NaN.
    ``clipped``: the centred window cut at the border with centred offsets instead (a test's lost piece)"""
    h = np.ascontiguousarray(h, np.float32)
    M, r = h.shape[0], k // 2
    off = slope_offsets(k, resolution)
    best = np.full((M, M), np.int32(-0x80000000), np.int32)
    any_ = np.zeros((M, M), bool)
    ci = corners(M, k)
    for a in range(k):
        for b in range(k):
            if clipped:
                ii, jj = np.arange(M) - r + a, np.arange(M) - r + b
                ok = ((ii >= 0) & (ii < M))[:, None] & ((jj >= 0) & (jj < M))[None, :]
                x = h[np.clip(ii, 0, M - 1)[:, None], np.clip(jj, 0, M - 1)[None, :]]
            else:
                ok = True
                x = h[(ci + a)[:, None], (ci + b)[None, :]]
            with np.errstate(invalid="ignore"):
                v = (x - off[a, b]).astype(np.float32)
            fin = np.isfinite(v) & ok
            best = np.where(fin, np.maximum(best, key(np.where(fin, v, np.float32(0.0)))), best)
            any_ |= fin
    return np.where(any_, unkey(np.where(any_, best, 0)), NAN).astype(np.float32)


# ---- Q4: box mean, Gaussian -----------------------------------------------------------------------------------------------------------------
def gauss_taps(k):
    """getGaussianKernel(k, 0) rounded to float32: the fixed tables up to 7, else sigma = 0.3 ((k - 1) / 2 - 1) + 0.8, normalised in double"""
    if k in GAUSS_FIXED:
        return np.array(GAUSS_FIXED[k], np.float32)
    sigma = 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8
    e = [math.exp(-((a - (k - 1) * 0.5) ** 2) / (2.0 * sigma * sigma)) for a in range(k)]
    s = 0.0
    for v in e:
        s += v
    return np.array([v / s for v in e], np.float64).astype(np.float32)


def blur(h, k, taps=None, columns_outer=False, halo=True):
    """``s = sum_a t[a] * (sum_b t[b] * double(x[clamp(i + a)][clamp(j + b)]))``, rows outer, columns inner, both ascending, in double.
    ``taps=None``: the box, ``float(s * (1.0 / (k * k)))``; else ``float(s)``.  ``columns_outer``: the other summation order (the margin
    check of the tests); ``halo=False``: zeros outside the map (a lost piece)"""
    h = np.ascontiguousarray(h, np.float32)
    M, r = h.shape[0], k // 2
    t = np.ones(k, np.float64) if taps is None else np.asarray(taps, np.float32).astype(np.float64)
    p = (np.pad(h, r, mode="edge") if halo else np.pad(h, r)).astype(np.float64)
    if columns_outer:
        p = p.T
    with np.errstate(invalid="ignore", over="ignore"):
        inner = np.zeros((M + 2 * r, M))
        for b in range(k):
            inner = inner + t[b] * p[:, b:b + M]
        s = np.zeros((M, M))
        for a in range(k):
            s = s + t[a] * inner[a:a + M]
        if columns_outer:
            s = s.T
        out = (s * (1.0 / float(k * k))).astype(np.float32) if taps is None else s.astype(np.float32)
    return _one_nan(out)


# ---- Q5 / Q6 ----------------------------------------------------------------------------------------------------------------------------
def lift(e, m, offset, a, b, footprint=None):
    """dilationInNonplanarRegions (:33-53) and addHeightOffset (:55-65) in float, literally"""
    e, m = np.ascontiguousarray(e, np.float32), np.ascontiguousarray(m, np.float32)
    v = e
    with np.errstate(invalid="ignore", over="ignore"):
        if offset > 0:
            d = morph(e, 2 * offset + 1, True, footprint=footprint)
            v = m * e + (np.float32(1.0) - m) * d
        if a != 0.0 or b != 0.0:
            v = v + np.float32(a + b)
        if b != 0.0:
            v = v - np.float32(b) * m
    return _one_nan(v)


def postprocess(e, labels, resolution, post=None, lose=None):
    """Postprocessing::postprocess on the plane ``e`` and the final labels: a namespace with the planes of PLANES.  ``lose``: a test's
    lost piece -- "no halo", "clipped window", "rectangle"."""
    e = np.ascontiguousarray(e, np.float32)
    M = e.shape[0]
    _, post, (kd, kb, kg) = check(M, resolution, None, post)
    halo = lose != "no halo"
    fp = (lambda k: ellipse(k, rectangle=True)) if lose == "rectangle" else (lambda k: None)
    planar = labels > 0
    m = planar.astype(np.float32)
    w = np.where(planar, e, NAN).astype(np.float32)
    wi = inpaint_min(w)
    closed = closing(wi, kd, footprint=fp(kd), halo=halo)
    dil = sloped_dilation(closed, kd, resolution, clipped=lose == "clipped window")
    smooth = blur(blur(dil, kb, halo=halo), kg, gauss_taps(kg), halo=halo)
    elev = lift(e, m, post["nonplanar_horizontal_offset"], post["extracted_planes_height_offset"], post["nonplanar_height_offset"],
                footprint=fp(2 * post["nonplanar_horizontal_offset"] + 1))
    return types.SimpleNamespace(elevation=elev, smooth_planar=smooth, plane_classification=m, elevation_before_postprocess=e, elevationWithNaN=w,
                                 elevationWithNaN_i=wi, elevationWithNaNClosed=closed, elevationWithNaNClosedDilated=dil, sizes=(kd, kb, kg), post=post)


def terrain(h, resolution, origin_xy, preprocess=None, postprocess_params=None, lose=None, **segmentation_keywords):
    """the whole model on one published height plane: ``plane_segmentation.segment``'s namespace plus the planes of PLANES"""
    h = np.ascontiguousarray(h, np.float32)
    pre, post, _ = check(h.shape[0], resolution, preprocess, postprocess_params)
    e = h
    if pre is not None:
        e = median(inpaint_min(h), pre[0], pre[1])
    seg = ps.segment(e, resolution, origin_xy, **segmentation_keywords)
    out = postprocess(e, seg.labels, resolution, post, lose=lose)
    planes = seg.planes.copy()
    if post["extracted_planes_height_offset"] != 0.0:
        planes["support"][:, 2] += post["extracted_planes_height_offset"]      # (:65-71)
    for k, v in vars(seg).items():
        if not hasattr(out, k):
            setattr(out, k, v)
    out.planes = planes
    return out
