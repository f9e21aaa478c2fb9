"""GPU: the plane services behind the plugins at their edges -- k_min_sweep<MAX> (window radii 0 .. 32 incl. the raised-LDS launch,
maps narrower than one tile, holes on the outer ring, 0 sweeps, all-known / all-unknown maps, the device-plane route on a shifted
origin), k_dilate_planes (the flat-index row wrap, the border exclusion), k_erode (windows of 1, 2, 4 and wider than the map, minima
in the corners), k_box3 (1 and 3 passes, constant and NaN planes) and k_inpaint_sweep against a float64 restatement of its arithmetic.
Oracles: oracle/emap_oracle.py (pinned against the compiled reference kernels), scipy.ndimage for the two OpenCV / cupyx substitutes."""
import ctypes as ct

import numpy as np
import pytest

import _fixtures as fx
from _util import make_pair
from oracle import emap_oracle as eo

gpu = pytest.mark.gpu
_CTX = {}


def _f32p(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_float))


def _hip(C):
    """one context per map size for the whole module: the services work on caller planes and leave the map alone"""
    if C not in _CTX:
        _CTX[C] = make_pair(eo.DEFAULTS, C)[0]
    return _CTX[C]


def _same(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


# ---- min / max filter -------------------------------------------------------------------------------------------------------------
def _filter(hip, is_max, e, v, d, iters):
    fn = hip._lib.emap_max_filter if is_max else hip._lib.emap_min_filter
    out = np.empty((hip.cell_n, hip.cell_n), np.float32); n = ct.c_int32(-1)
    if e is None:
        hip._chk(fn(hip._ctx, None, None, d, iters, _f32p(out), ct.byref(n)))
    else:
        e = np.ascontiguousarray(e, np.float32); v = np.ascontiguousarray(v, np.float32)
        hip._chk(fn(hip._ctx, _f32p(e), _f32p(v), d, iters, _f32p(out), ct.byref(n)))
    return out, n.value


def edge_map(C, seed, big_hole):
    """elevation and is_valid with holes along columns 0..2 and C-3..C-1 and rows 0 and C-1 (the outer ring is never a source, and the
    flat-index window of a cell next to it wraps into the neighbouring row), random holes, and optionally a hole wider than two windows"""
    rng = np.random.default_rng(seed)
    e = rng.uniform(-1, 1, (C, C)).astype(np.float32)
    v = (rng.uniform(0, 1, (C, C)) > 0.3).astype(np.float32)
    v[:, :3] = 0; v[:, C - 3:] = 0; v[0] = 0; v[C - 1] = 0
    v[5, 0] = v[0, 7] = v[C - 1, 9] = v[11, C - 1] = 1; e[5, 0] = e[0, 7] = e[C - 1, 9] = e[11, C - 1] = -7.0   # known ring cells: never a source
    if big_hole:
        v[C // 2 - big_hole:C // 2 + big_hole, C // 2 - big_hole:C // 2 + big_hole] = 0
    e[v < 0.5] = 9.0                          # unknown cells hold garbage
    return e, v


@gpu
@pytest.mark.parametrize("is_max", [False, True])
@pytest.mark.parametrize("C,d", [(130, 0), (130, 16), (130, 27), (130, 32), (34, 16), (34, 32), (66, 5)])
def test_min_max_filter_radii_and_narrow_maps(C, d, is_max):
    """d >= 27 needs more than 64 KB of dynamic LDS (the raised-LDS launch); C = 34 < 64 = one tile wider than the map, where the
    window of every cell wraps rows on both sides; d = 0 fills nothing and runs every sweep"""
    hip = _hip(C)
    e, v = edge_map(C, 3 * d + C, big_hole=min(d + 3, C // 2 - 4) if d else 6)
    iters = 3
    got, n = _filter(hip, is_max, e, v, d, iters)
    want, sweeps = (eo.max_filter if is_max else eo.min_filter)(C, d, iters, e, v)
    print("C=%d d=%d max=%d: sweeps %d, filled %d, open %d" % (C, d, is_max, sweeps, int((~np.isnan(want)).sum() - (v > 0.5).sum()), int(np.isnan(want).sum())))
    assert n == sweeps and _same(got, want)
    if d == 0:
        assert sweeps == iters and np.array_equal(np.isnan(want), v < 0.5)
    else:
        assert (~np.isnan(want)).sum() > (v > 0.5).sum() + 100
        assert (want == -7.0).sum() == 4 and not (want == 9.0).any()        # ring cells never spread, garbage under holes is never read
        assert sweeps >= 2 or C == 34                                       # the big hole is wider than two windows


@gpu
@pytest.mark.parametrize("is_max", [False, True])
@pytest.mark.parametrize("C,d", [(34, 2), (66, 5)])
def test_min_max_filter_degenerate_maps_and_sweep_counts(C, d, is_max):
    hip = _hip(C)
    ref = eo.max_filter if is_max else eo.min_filter
    rng = np.random.default_rng(C + d)
    e = rng.uniform(-1, 1, (C, C)).astype(np.float32)
    ones, zeros = np.ones((C, C), np.float32), np.zeros((C, C), np.float32)
    # all known: the first sweep finds nothing open; the later ones are copies
    got, n = _filter(hip, is_max, e, ones, d, 4)
    assert n == 1 == ref(C, d, 4, e, ones)[1] and np.array_equal(got, e)
    # all unknown: every sweep runs, nothing is ever filled
    got, n = _filter(hip, is_max, e, zeros, d, 4)
    assert n == 4 == ref(C, d, 4, e, zeros)[1] and np.isnan(got).all()
    # no sweep at all: the input through the mask
    e2, v2 = edge_map(C, 5, big_hole=0)
    got, n = _filter(hip, is_max, e2, v2, d, 0)
    want, sweeps = ref(C, d, 0, e2, v2)
    assert n == 0 == sweeps and _same(got, want) and np.array_equal(np.isnan(got), v2 < 0.5)
    # a hole that closes exactly on the last sweep allowed, and one sweep short of it
    e3, v3 = edge_map(C, 6, big_hole=C // 2 - 4)
    _, n_close = ref(C, d, 64, e3, v3)
    assert 2 <= n_close < 64
    for iters, closed in ((n_close, True), (n_close - 1, False), (n_close + 1, True)):
        got, n = _filter(hip, is_max, e3, v3, d, iters)
        want, sweeps = ref(C, d, iters, e3, v3)
        assert n == sweeps == min(iters, n_close) and _same(got, want) and (not np.isnan(want).any()) == closed, (iters, n, sweeps)


@gpu
@pytest.mark.parametrize("is_max", [False, True])
def test_min_max_filter_device_route_on_a_shifted_origin(is_max, weights):
    """NULL host pointers = the map's own elevation / is_valid planes, de-interleaved on the device through the circular origin: after
    a move_to with a shift in both axes the device route, the host route and the oracle agree"""
    C, d, iters = 66, 2, 3
    hip, _ = make_pair(eo.DEFAULTS, C, "reference_fp16", weights)
    R, t = fx.POSES["rotated"]
    hip.input_pointcloud(fx.cloud(C, 3000, 2), ["x", "y", "z"], R, t.copy(), 0.0, 0.0)
    hip.move_to(np.array([7 * 0.04, -11 * 0.04, 0.03]), np.eye(3))
    m = hip.elevation_map
    known = int((m[2] > 0.5).sum())
    assert 300 < known < C * C - 300 and np.allclose(hip.center, [7 * 0.04, -11 * 0.04, 0.03])
    on_device, n_dev = _filter(hip, is_max, None, None, d, iters)
    from_host, n_host = _filter(hip, is_max, m[0], m[2], d, iters)
    want, sweeps = (eo.max_filter if is_max else eo.min_filter)(C, d, iters, m[0], m[2])
    assert n_dev == n_host == sweeps
    assert _same(from_host, want) and _same(on_device, want)


# ---- dilation of caller planes ----------------------------------------------------------------------------------------------------
def _dilate_oracle(C, d, iterations, plane, mask):
    for _ in range(iterations):          # out of place, the mask carried along (eo_dilate reports only the cells it filled)
        plane, filled = eo.dilate_plane(C, d, plane, mask)
        mask = np.where(filled > 0.5, np.float32(1), mask).astype(np.float32)
    return plane, mask


def dilate_planes(C, kind):
    rng = np.random.default_rng(C)
    plane = rng.uniform(1, 2, (C, C)).astype(np.float32)
    mask = np.zeros((C, C), np.float32)
    if kind == "wrap":       # known cells ONLY at column C-2 of two rows: the holes at columns 0.. of the NEXT row are their flat-index neighbours
        mask[5, C - 2] = mask[12, C - 2] = 1
    elif kind == "ring":     # known cells on the outer ring only: they are never a source, so nothing spreads
        mask[0, 4:9] = mask[C - 1, 3] = mask[6, 0] = mask[9, C - 1] = 1
    else:
        mask[rng.uniform(0, 1, (C, C)) < 0.03] = 1
    return plane, mask


@gpu
@pytest.mark.parametrize("kind", ["wrap", "ring", "sparse"])
@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("d", [0, 1, 8])
@pytest.mark.parametrize("C", [34, 66])
def test_dilate_planes_wrap_and_border(C, d, iterations, kind):
    hip = _hip(C)
    plane, mask = dilate_planes(C, kind)
    out = np.empty_like(plane); om = np.empty_like(mask)
    hip._chk(hip._lib.emap_dilate_planes(hip._ctx, _f32p(plane), _f32p(mask), d, iterations, _f32p(out), _f32p(om)))
    want, wm = _dilate_oracle(C, d, iterations, plane, mask)
    assert np.array_equal(om, wm) and np.array_equal(out, want)
    if kind == "ring" or d == 0:
        assert np.array_equal(om, mask) and np.array_equal(out, plane)
    if kind == "wrap" and d == 8:
        # the reference's quirk: j = i + C * dy + dx runs off the row's end into the next row, so (6, 1) takes its value from (5, C-2), 3
        # flat cells before it, although the two are a map width apart
        assert om[6, 1] == 1 and out[6, 1] == plane[5, C - 2] and om[13, 0] == 1
    if kind == "sparse" and d:
        assert om.sum() > mask.sum() + 50


# ---- erosion ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("corner", [(0, 0), (0, 33), (33, 0), (33, 33)])
@pytest.mark.parametrize("k", [1, 2, 4, 63])
def test_erode_window_sizes_and_corner_minima(k, corner):
    from scipy import ndimage
    C = 34
    hip = _hip(C)
    q = np.random.default_rng(k).integers(10, 256, (C, C)).astype(np.float32)
    q[corner] = 1.0                                       # the global minimum sits in a corner
    for iterations in (0, 1, 2):
        out = np.empty_like(q)
        hip._chk(hip._lib.emap_erode(hip._ctx, _f32p(q), k, iterations, _f32p(out)))
        want = q
        for _ in range(iterations):
            want = ndimage.minimum_filter(want, size=k, mode="constant", cval=np.inf)     # offsets -k//2 .. k-k//2-1 = cv2's anchor (k//2, k//2)
        assert np.array_equal(out, want), (k, corner, iterations)
        if iterations == 0 or k == 1:
            assert np.array_equal(out, q)
        else:
            # the corner minimum reaches exactly the cells whose window holds it: offsets -(k//2) .. k-k//2-1 per iteration, cut at the map's
            # edge (k = 2 looks one cell up and left only, so a minimum in the last row and column stays where it is)
            a, b = (k // 2) * iterations, (k - k // 2 - 1) * iterations
            span = [min(x + a, C - 1) - max(x - b, 0) + 1 for x in corner]
            assert (out == 1.0).sum() == span[0] * span[1] and out[corner] == 1.0, (k, corner, iterations)


# ---- smoothing ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("passes", [1, 3])
def test_box3_small_map_constant_and_nan(passes):
    C = 34
    hip = _hip(C)

    def smooth(a):
        out = np.empty_like(a)
        hip._chk(hip._lib.emap_smooth_filter(hip._ctx, _f32p(np.ascontiguousarray(a)), passes, _f32p(out)))
        return out
    a = np.random.default_rng(passes).normal(0, 1, (C, C)).astype(np.float32)
    assert np.allclose(smooth(a), eo.smooth_filter(a, passes), rtol=1e-6, atol=1e-6)       # float32 output of a double-accumulated 3-tap mean
    const = np.full((C, C), np.float32(0.7321), np.float32)
    assert np.array_equal(smooth(const), const)             # 3 c / 3 is exact in double, so the constant comes back bit for bit
    for r, c in ((0, 0), (17, 20), (33, 5)):
        b = a.copy(); b[r, c] = np.nan
        nan = np.isnan(smooth(b))
        want = np.zeros((C, C), bool)
        want[max(r - passes, 0):r + passes + 1, max(c - passes, 0):c + passes + 1] = True      # its 3 x 3 neighbourhood per pass, no further
        assert np.array_equal(nan, want), (r, c)
        assert np.array_equal(smooth(b)[~want], smooth(a)[~want])      # (scipy's running sum would carry the NaN down the line: no oracle here)


# ---- inpainting substitute (method="front") -------------------------------------------------------------------------------------------
W_DIAG = float(np.float32(0.70710678))        # the kernel's float32 diagonal weight


def inpaint_fixture(C=66):
    """8-bit image with holes: a block, a hole that touches two borders and scattered pixels"""
    rng = np.random.default_rng(21)
    xx, yy = np.meshgrid(np.arange(C), np.arange(C), indexing="ij")
    img = np.rint(127 + 90 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.uniform(-20, 20, (C, C))).clip(0, 255).astype(np.float32)
    known = rng.uniform(0, 1, (C, C)) > 0.2
    known[20:33, 25:41] = False
    known[:6, :9] = False
    known[C - 4:, C - 7:] = False
    img[~known] = 0.0
    return img, known


def inpaint_restatement(img, known, max_sweeps):
    """k_inpaint_sweep in float64: Jacobi sweeps, every open pixel with a known 8-neighbour becomes the weighted mean of those
    (weights 1 and 1/sqrt 2), rounded half to even and clamped to 0 .. 255.  Returns (values, sweeps run, exact means of the filled
    pixels at the sweep that filled them)."""
    C = img.shape[0]
    val, msk = img.astype(np.float64), known.copy()
    exact = np.full(img.shape, np.nan)
    sweeps = 0
    while sweeps < max_sweeps:
        pv, pm = np.pad(val, 1), np.pad(msk, 1)
        s = np.zeros_like(val); w = np.zeros_like(val)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if dr or dc:
                    wt = W_DIAG if dr and dc else 1.0
                    nm = pm[1 + dr:1 + dr + C, 1 + dc:1 + dc + C]
                    s += np.where(nm, wt * pv[1 + dr:1 + dr + C, 1 + dc:1 + dc + C], 0.0); w += np.where(nm, wt, 0.0)
        fill = ~msk & (w > 0)
        mean = np.divide(s, w, out=np.zeros_like(s), where=w > 0)
        exact[fill] = mean[fill]
        val = np.where(fill, np.clip(np.rint(mean), 0, 255), val); msk = msk | fill
        sweeps += 1
        if msk.all():
            break
    return val, sweeps, exact


def _near_half(exact):
    frac = exact - np.floor(exact)
    return np.abs(frac - 0.5) < 1e-3


def test_inpaint_fixture_has_few_means_near_a_half_integer():
    """CPU: the restatement alone -- at most 1 % of the filled pixels have an exact mean within 1e-3 of a half-integer (where float32
    and float64 may round to different sides), the hole closes, and it takes several fronts"""
    img, known = inpaint_fixture()
    val, sweeps, exact = inpaint_restatement(img, known, 200)
    filled = ~known
    near = _near_half(exact[filled])
    print("filled %d, near a half-integer %d, sweeps %d" % (filled.sum(), near.sum(), sweeps))
    assert filled.sum() > 800 and 5 <= sweeps < 200 and not np.isnan(exact[filled]).any()
    assert near.sum() <= 0.01 * filled.sum()
    assert val[filled].min() >= 0 and val[filled].max() <= 255 and np.array_equal(val[known], img[known])


def _assert_inpaint_equal(out, val, exact, known):
    """equal, except +-1 where the exact weighted mean lies within 1e-3 of a half-integer (float32 products of the diagonal weight can
    land on the other side of the tie there); such pixels are at most 1 % of the filled ones"""
    filled = ~known & ~np.isnan(exact)
    diff = np.abs(out.astype(np.float64) - val)
    loose = filled & _near_half(np.where(filled, exact, 0.0))
    print("differing pixels %d, pixels near a half-integer %d of %d filled" % (int((diff != 0).sum()), int(loose.sum()), int(filled.sum())))
    assert loose.sum() <= 0.01 * (~known).sum()
    assert not diff[~loose].any() and diff[loose].max(initial=0.0) <= 1


@gpu
def test_inpaint_sweep_matches_its_float64_restatement():
    img, known = inpaint_fixture()
    C = img.shape[0]
    hip = _hip(C)
    out = np.empty_like(img); n = ct.c_int32(-1)
    k32 = known.astype(np.float32)
    hip._chk(hip._lib.emap_inpaint_u8(hip._ctx, _f32p(img), _f32p(k32), 2 * C, _f32p(out), ct.byref(n)))
    val, sweeps, exact = inpaint_restatement(img, known, 2 * C)
    assert n.value == sweeps
    _assert_inpaint_equal(out, val, exact, known)
    # fewer sweeps than fronts: the front stops where it is, the rest stays open (and keeps the input's value)
    hip._chk(hip._lib.emap_inpaint_u8(hip._ctx, _f32p(img), _f32p(k32), 2, _f32p(out), ct.byref(n)))
    val2, sweeps2, exact2 = inpaint_restatement(img, known, 2)
    assert n.value == sweeps2 == 2 and np.isnan(exact2[~known]).sum() > 100
    _assert_inpaint_equal(out, val2, exact2, known)
