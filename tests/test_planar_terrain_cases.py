"""CPU: the host model of the planar terrain (elevation_mapping_cupy_amd/planar_terrain.py) against independent
restatements -- a literal transcription of the reference's minValues sweep, SciPy's median_filter, grey_dilation / grey_erosion and
label (bit for bit: selecting operators round nothing), uniform_filter / correlate1d in float64 for the two means (a measured
deviation), a per-cell loop over the shifted window --, the element tables, the lost pieces the GPU scenes can tell, the margin
statement on plane_classification, and the C ABI of emap_planar_terrain as far as a machine without a device goes.  Reference:
GridMapPreprocessing.cpp:14-39, Postprocessing.cpp:14-146, inpainting.cpp:25-94, processing.cpp:145-177."""
import ctypes as ct
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import _plane_seg_cases as pc
import _planar_terrain_cases as tc
from conftest import ROOT
from elevation_mapping_cupy_amd import plane_segmentation as ps
from elevation_mapping_cupy_amd import planar_terrain as pt

RES = tc.RES
CSRC = os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc")


def _random_map(rng, M, p_nan):
    h = rng.uniform(-1.0, 1.0, (M, M)).astype(np.float32)
    h[rng.random((M, M)) < p_nan] = np.nan
    return h


# ---- P1 -------------------------------------------------------------------------------------------------------------------------------------
def test_inpainting_is_the_fixed_point_of_the_reference_sweep():
    rng = np.random.default_rng(11)
    maps = [_random_map(rng, M, p) for M, p in zip(rng.integers(3, 24, 30), rng.uniform(0.1, 0.9, 30))]
    single = np.full((9, 9), np.nan, np.float32); single[4, 6] = -0.25
    maps += [np.full((7, 7), np.nan, np.float32), single, tc.nan_frame(13), tc.hole(32), tc.nan_edge(32), np.full((5, 5), 1.5, np.float32)]
    for h in maps:
        assert tc.same_words(pt.inpaint_min(h), tc.min_values_sweep(h)), h.shape
    assert np.isnan(pt.inpaint_min(maps[30])).all() and (pt.inpaint_min(single) == np.float32(-0.25)).all()
    frame = pt.inpaint_min(tc.nan_frame(13))
    assert not np.isnan(frame).any() and frame[0, 0] == np.float32(0.25) and frame[12, 12] == np.float32(0.25)      # one component along all four edges


def test_the_nan_components_are_scipys():
    rng = np.random.default_rng(12)
    for M in (5, 32, 33, 65):
        nan = np.isnan(_random_map(rng, M, 0.55))
        root = ps.components(nan, 4)
        lab, n = ndimage.label(nan)                            # 4-connectivity is the default structure
        assert ((root >= 0) == nan).all()
        pairs = set(zip(root[nan].tolist(), lab[nan].tolist()))
        assert len(pairs) == n == len(set(r for r, _ in pairs))      # a bijection between roots and SciPy's labels


def test_a_minimum_of_signed_zeros_and_infinities_is_taken_on_the_bits():
    h = np.array([[np.nan, 0.0, -0.0], [np.inf, np.nan, -np.inf], [1.0, 2.0, np.nan]], np.float32)
    out = pt.inpaint_min(h)
    assert out[0, 0] == 0.0 and np.signbit(out[0, 0]) == False and out[1, 1] == -np.inf and out[2, 2] == -np.inf      # noqa: E712
    h2 = np.array([[0.0, np.nan, -0.0]], np.float32).repeat(3, 0)
    assert np.signbit(pt.inpaint_min(h2)[:, 1]).all()                    # -0 lies below +0
    k = pt.key(np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32))
    assert (np.diff(k.astype(np.int64)) > 0).all() and tc.same_words(pt.unkey(k), np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32))


# ---- P2 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (3, 5))
def test_the_median_is_scipys(k):
    rng = np.random.default_rng(13)
    for M in (5, 32, 33):
        h = _random_map(rng, M, 0.0)
        want = h
        for n in (1, 2, 3):
            want = ndimage.median_filter(want, size=k, mode="nearest")
            assert tc.same_words(pt.median(h, k, n), want), (M, n)
    h = _random_map(rng, 9, 0.0); h[4, 4] = np.nan
    out = pt.median(h, k)
    r = k // 2
    assert np.isnan(out[4 - r:5 + r, 4 - r:5 + r]).all() and int(np.isnan(out).sum()) == k * k      # a window with a NaN gives NaN
    assert pt.median(h, 1, 5) is not None and tc.same_words(pt.median(h, 1, 5), h)


# ---- Q2 / Q5 --------------------------------------------------------------------------------------------------------------------------------
def test_the_ellipse_tables():
    for k in range(1, 32, 2):
        f = pt.ellipse(k)
        assert (f == f[::-1]).all() and (f == f[:, ::-1]).all() and f[k // 2].all() and f[:, k // 2].all(), k
        r = k // 2
        for a, (lo, hi) in enumerate(pt.ellipse_spans(k)):    # OpenCV multiplies by 1 / r^2 where the contract divides: the same spans up to 31
            dy = a - r
            dx = int(np.rint(r * np.sqrt((r * r - dy * dy) * (1.0 / (r * r))))) if r else 0
            assert (lo, hi) == (max(r - dx, 0), min(r + dx + 1, k)), (k, a)
    assert pt.ellipse(1).tolist() == [[True]]
    assert pt.ellipse(3).astype(int).tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    assert pt.ellipse(5).astype(int).tolist() == [[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]]
    assert [hi - lo for lo, hi in pt.ellipse_spans(11)] == [1, 7, 9, 11, 11, 11, 11, 11, 9, 7, 1]


def test_dilation_erosion_and_closing_are_scipys():
    rng = np.random.default_rng(14)
    for M, k in ((32, 3), (33, 11), (40, 31), (65, 5), (9, 9)):
        h = _random_map(rng, M, 0.0)
        f = pt.ellipse(k)
        assert tc.same_words(pt.morph(h, k, True), ndimage.grey_dilation(h, footprint=f, mode="nearest")), (M, k)
        assert tc.same_words(pt.morph(h, k, False), ndimage.grey_erosion(h, footprint=f, mode="nearest")), (M, k)
        assert tc.same_words(pt.closing(h, k), ndimage.grey_closing(h, footprint=f, mode="nearest")), (M, k)
    h = _random_map(rng, 12, 0.0); h[:, :7] = np.nan
    d = pt.morph(h, 3, True)
    assert np.isnan(d[:, :6]).all() and not np.isnan(d[:, 6:]).any() and (d[:, 6] == h[:, 7]).all()      # NaN is skipped; all NaN: NaN


# ---- Q3 -------------------------------------------------------------------------------------------------------------------------------------
def test_the_sloped_dilation_is_the_per_cell_loop_over_the_shifted_window():
    rng = np.random.default_rng(15)
    for M, k in ((12, 5), (11, 11), (33, 31), (20, 1), (16, 7)):
        h = _random_map(rng, M, 0.3)
        h[0, 0] = np.inf
        assert tc.same_words(pt.sloped_dilation(h, k, RES), tc.sloped_loop(h, k, RES)), (M, k)
    assert np.isnan(pt.sloped_dilation(np.full((8, 8), np.nan, np.float32), 5, RES)).all()
    off = pt.slope_offsets(5, RES)
    assert off[2, 2] == 0 and off[0, 0] == np.float32(float(np.float32(RES)) * np.sqrt(8.0)) and off.dtype == np.float32


# ---- Q4 -------------------------------------------------------------------------------------------------------------------------------------
# the largest deviation of the model's box mean / Gaussian from SciPy's float64 filters on the maps below (heights in [-1, 1)): measured
# 2.910e-08, about 2^-25 -- the rounding of a result below 1 to float32; the double sums differ far below that.
# Asserted at 4 x the measured figure.
BLUR_MEASURED = 2.910e-8


def test_the_box_mean_and_the_gaussian_against_scipy_in_double():
    rng = np.random.default_rng(16)
    worst = 0.0
    for M, k in ((32, 7), (33, 3), (65, 31), (40, 9), (33, 1), (48, 15)):
        h = _random_map(rng, M, 0.0)
        box = ndimage.uniform_filter(h.astype(np.float64), size=k, mode="nearest")
        worst = max(worst, float(np.abs(pt.blur(h, k).astype(np.float64) - box).max()))
        t = pt.gauss_taps(k)
        g = ndimage.correlate1d(ndimage.correlate1d(h.astype(np.float64), t.astype(np.float64), axis=1, mode="nearest"), t.astype(np.float64), axis=0, mode="nearest")
        worst = max(worst, float(np.abs(pt.blur(h, k, t).astype(np.float64) - g).max()))
    print("largest deviation from SciPy's float64 filters: %.3e" % worst)
    assert worst <= 4 * BLUR_MEASURED


def test_the_gaussian_taps():
    for k, want in pt.GAUSS_FIXED.items():
        assert pt.gauss_taps(k).tolist() == list(want)
    for k in range(9, 32, 2):
        t = pt.gauss_taps(k).astype(np.float64)
        sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
        x = np.arange(k) - (k - 1) * 0.5
        e = np.exp(-x * x / (2 * sigma * sigma))
        assert t.dtype == np.float64 and abs(t.sum() - 1.0) < 1e-6 and (t == t[::-1]).all() and np.abs(t - e / e.sum()).max() < 1e-7, k


# ---- parameters -----------------------------------------------------------------------------------------------------------------------------
def test_kernel_sizes_and_refusals():
    res = float(np.float32(0.04))
    _, post, sizes = pt.check(100, res, None, None)
    assert sizes == (11, 7, 3) and post["nonplanar_horizontal_offset"] == 1 and post["nonplanar_height_offset"] == 0.02      # the reference's defaults at 4 cm
    assert pt.kernel_cells(0.0, res) == 1 and pt.kernel_cells(0.5 * res, res) == 3 and pt.kernel_cells(0.49 * res, res) == 1      # round half away
    assert pt.check(100, res, {}, None)[0] == (3, 1) and pt.check(100, res, dict(kernelSize=9), None)[0] == (5, 1) and pt.check(100, res, dict(kernelSize=-2), None)[0] == (1, 1)
    assert pt.check(100, res, dict(resolution=res + 5e-7), None)[0] == (3, 1)
    for pre, post in ((dict(kernelSize=4), None), (dict(kernelSize=2, numberOfRepeats=1), None), (dict(numberOfRepeats=9), None), (dict(numberOfRepeats=-1), None),
                      (dict(resolution=0.05), None), (dict(size=3), None), (None, dict(nonplanar_horizontal_offset=16)), (None, dict(nonplanar_horizontal_offset=-1)),
                      (None, dict(smoothing_dilation_size=16 * res)), (None, dict(smoothing_box_kernel_size=-0.1)), (None, dict(smoothing_gauss_kernel_size=float("nan"))),
                      (None, dict(nonplanar_height_offset=float("inf"))), (None, dict(smoothing=1.0))):
        with pytest.raises(ValueError):
            pt.check(100, res, pre, post)
    with pytest.raises(ValueError):
        pt.check(9, res, None, None)                           # 11 cells do not fit a map of 9
    with pytest.raises(ValueError):
        pt.check(4, res, dict(kernelSize=5), tc.post_of(res, kd=1, kb=1, kg=1))


# ---- the whole model on the GPU scenes ------------------------------------------------------------------------------------------------------
def _run(M, name, pre=None, post=None, lose=None):
    h, over = tc.scenes(M)[name]
    return pt.terrain(h, RES, pc.ORIGIN, pre, post, lose=lose, **pc.params(**over))


def _planes(r):
    return b"".join(getattr(r, n).tobytes() for n in pt.PLANES)


def test_the_scenes_are_what_they_claim():
    M = 65
    r = _run(M, "no planar cell")
    assert r.n_labels == 0 and np.isnan(r.smooth_planar).all() and (r.smooth_planar.view(np.uint32) == 0x7fc00000).all() and (r.plane_classification == 0).all()
    r = _run(M, "all NaN", tc.PRE)
    assert all(np.isnan(getattr(r, n)).all() for n in pt.PLANES if n != "plane_classification")
    r = _run(M, "plateau")
    edge = np.concatenate([r.plane_classification[0], r.plane_classification[-1], r.plane_classification[:, 0], r.plane_classification[:, -1]])
    assert edge.sum() > 40 and all(r.plane_classification[a, b] == 1 for a in (0, M - 1) for b in (0, M - 1))      # planar cells on every edge and corner
    h = tc.hole(M)
    nan = np.isnan(h)
    root = ps.components(nan, 4)
    big = root == root[25, 25]
    tiles = {(int(i) // 32, int(j) // 32) for i, j in zip(*np.nonzero(big))}
    assert tiles == {(0, 0), (0, 1), (1, 0), (1, 1)} and int(big[32:, 32:].sum()) == 16      # four tiles, 4 x 4 cells in the last
    assert (pt.inpaint_min(h)[big] == np.float32(0.125)).all() and h[36, 34] == np.float32(0.125)      # ... which holds the rim's minimum
    r = _run(M, "hole", tc.PRE)
    assert not np.isnan(r.elevation_before_postprocess).any() and tc.same_words(r.elevation_before_postprocess, pt.median(pt.inpaint_min(h), 3, 1))
    r0 = _run(M, "terraces")
    seg = ps.segment(tc.scenes(M)["terraces"][0], RES, pc.ORIGIN, **pc.params())
    assert (r0.labels == seg.labels).all() and r0.planes.tobytes() == seg.planes.tobytes() and tc.same_words(r0.elevation_before_postprocess, tc.scenes(M)["terraces"][0])
    lifted = _run(M, "terraces", None, dict(extracted_planes_height_offset=0.03))
    assert (lifted.planes["support"][:, 2] == seg.planes["support"][:, 2] + 0.03).all() and (lifted.planes["support"][:, :2] == seg.planes["support"][:, :2]).all()
    m = r0.plane_classification == 1
    e = tc.scenes(M)["terraces"][0]
    assert m.any() and not m.all() and tc.same_words(r0.elevation[m], (e[m] + np.float32(0.02)) - np.float32(0.02))      # planar cells: lifted and lowered again
    assert (r0.elevation[~m] >= e[~m] + np.float32(0.02)).all()                                                       # the others: dilated and lifted


@pytest.mark.parametrize("lose", tc.LOST)
def test_a_lost_piece_changes_the_answer_on_the_gpu_scenes(lose):
    """dropping the halo, clipping the sloped window instead of shifting it, a rectangle for the ellipse: the GPU scenes can tell"""
    for M in (32, 33, 65):
        told = [name for name in ("plateau", "hole", "hills", "terraces") if _planes(_run(M, name, lose=lose)) != _planes(_run(M, name))]
        assert "plateau" in told and len(told) >= 2, (lose, M, told)


def test_no_summation_order_moves_a_classification_bit():
    """nothing downstream of the two means is thresholded: with the columns outer in both, plane_classification and every plane but
    smooth_planar keep their bits on every GPU scene, and smooth_planar moves by at most one unit in the last place"""
    for M in (32, 65):
        for name, (h, over) in tc.scenes(M).items():
            r = _run(M, name)
            other = pt.blur(pt.blur(r.elevationWithNaNClosedDilated, r.sizes[1], columns_outer=True), r.sizes[2], pt.gauss_taps(r.sizes[2]), columns_outer=True)
            a, b = r.smooth_planar, other
            assert (np.isnan(a) == np.isnan(b)).all(), name
            ok = np.isfinite(a) & np.isfinite(b)
            assert (np.abs(a[ok].view(np.int32).astype(np.int64) - b[ok].view(np.int32).astype(np.int64)) <= 1).all(), name
            assert tc.same_words(r.plane_classification, (r.labels > 0).astype(np.float32)), name


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_bound_and_additive():
    from elevation_mapping_cupy_amd import _lib
    from elevation_mapping_cupy_amd.csrc import build
    lib = _lib.load()
    assert "emap_planar_terrain" in _lib.SYMBOLS and hasattr(lib, "emap_planar_terrain") and len(lib.emap_planar_terrain.argtypes) == 11
    assert lib.emap_abi_version() == 3 and _lib.ABI_VERSION == 3
    hdr = open(os.path.join(ROOT, "include", "emap_hip.h")).read()
    assert len(re.findall(r"\bint emap_planar_terrain\(", hdr)) == 1
    for cname, cls, size in (("emap_terrain_params", _lib.EmapTerrainParams, 64), ("emap_terrain_planes", _lib.EmapTerrainPlanes, 64)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        declared = [re.sub(r"\[\d+\]", "", f.strip()).lstrip("* ") for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
        assert declared == [f[0] for f in cls._fields_] and ct.sizeof(cls) == size, cname
    assert "EMAP_TERRAIN_KERNEL_MAX = %d, EMAP_TERRAIN_OFFSET_MAX = %d, EMAP_TERRAIN_REPEATS_MAX = %d" % (_lib.TERRAIN_KERNEL_MAX, _lib.TERRAIN_OFFSET_MAX, _lib.TERRAIN_REPEATS_MAX) in hdr
    assert (_lib.TERRAIN_KERNEL_MAX, _lib.TERRAIN_OFFSET_MAX, _lib.TERRAIN_REPEATS_MAX) == (pt.KERNEL_MAX, pt.OFFSET_MAX, pt.REPEATS_MAX) and _lib.TERRAIN_PLANES == pt.PLANES
    launch = open(os.path.join(CSRC, "emap_launch.h")).read()
    for a, b in (("KERNEL_MAX", 31), ("OFFSET_MAX", 15), ("REPEATS_MAX", 8)):
        assert re.search(r"#define EM_TERRAIN_%s %d\b" % (a, b), launch)
    assert "emap_terrain.hip" in build.SOURCES and "emap_api_terrain.hip" in build.SOURCES
    assert "emap_terrain.hip" in open(os.path.join(ROOT, "tools", "kernel_resources.py")).read()


def test_the_host_side_refuses_first_owns_its_buffers_and_reuses_the_union_find():
    src = open(os.path.join(CSRC, "emap_api_terrain.hip")).read()
    body = src[src.index("int emap_planar_terrain("):]
    refusals = [m.start() for m in re.finditer(r"\bCKARG\(|check_layer_entry\(", body)]
    assert len(refusals) >= 20 and max(refusals) < body.index("SF_CHECK()") < body.index("hipSetDevice") < body.index("FLUSH()") < body.index("planeseg_source(") < body.index("hipMemcpyAsync")
    assert "hipMalloc" not in src and "DevBuf" not in src and body.count("hipStreamSynchronize(") == 1      # the context's buffers; one wait besides the segmentation's two
    destroy = open(os.path.join(CSRC, "emap_api.hip")).read()
    assert "hipFree(ctx->terr_buf)" in destroy and "hipHostFree(ctx->terr_pin)" in destroy
    k = open(os.path.join(CSRC, "emap_terrain.hip")).read()
    code = "\n".join(line.split("//")[0] for line in k.splitlines())
    for name in ("k_ps_local", "k_ps_merge", "k_ps_flatten", "ps_union", "ps_find"):
        assert name not in code, name                          # reused through launch_ps_components, not copied
    assert src.count("launch_ps_components(") == 1 and "while (" not in code and "exp(" not in code and "asm" not in code
    seg = open(os.path.join(CSRC, "emap_planeseg.hip")).read()
    assert seg.count("void launch_ps_components(") == 1 and open(os.path.join(CSRC, "emap_launch.h")).read().count("void launch_ps_components(") == 1


def _call(lib, null=(), **over):
    from elevation_mapping_cupy_amd import _lib
    src = _lib.EmapGridLayerEx(0, 0, 0, 0)
    P = _lib.EmapPlaneParams(3, 0, 4, 4, 0, 0, 0.0, 0.0, 0.04, 0.0, 0.0, 0.02, 0.8, 0.85, 0.025, 0.9)
    vals = dict(preprocess=1, median_kernel_size=3, median_repeats=1, nonplanar_horizontal_offset=1, want=15, reserved=0, smoothing_dilation_size=0.2,
                smoothing_box_kernel_size=0.1, smoothing_gauss_kernel_size=0.05, extracted_planes_height_offset=0.0, nonplanar_height_offset=0.02)
    vals.update(over)
    Q = _lib.EmapTerrainParams(**vals)
    labels, rec, planes = np.full(64, -7, np.int32), np.full(64 * 5, 0xA5, np.uint8), np.full((8, 64), -7.0, np.float32)
    O = _lib.EmapTerrainPlanes()
    for k in range(8):
        O.plane[k] = planes[k].ctypes.data_as(ct.POINTER(ct.c_float))
    n_labels, n_planes = ct.c_int32(-7), ct.c_int64(-7)
    rc = lib.emap_planar_terrain(None, None if "source" in null else ct.byref(src), ct.byref(P), None if "terrain" in null else ct.byref(Q),
                                 labels.ctypes.data_as(ct.POINTER(ct.c_int32)), None, rec.ctypes.data_as(ct.POINTER(_lib.EmapPlaneRecord)), 4, ct.byref(n_labels),
                                 ct.byref(n_planes), None if "out" in null else ct.byref(O))
    assert (labels == -7).all() and (rec == 0xA5).all() and (planes == -7.0).all() and n_labels.value == -7 and n_planes.value == -7
    return rc


def test_null_arguments_are_refused_without_a_device():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    assert _call(lib) == -1
    for k in ("source", "terrain", "out"):
        assert _call(lib, null=(k,)) == -1, k
    for over in (dict(preprocess=2), dict(median_kernel_size=4), dict(median_repeats=9), dict(nonplanar_horizontal_offset=16), dict(want=256)):
        assert _call(lib, **over) == -1, over
