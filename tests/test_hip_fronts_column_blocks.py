"""GPU: the column pass of the fronts pipeline's distance transform in row blocks with a carry (k_fr_dt_cols_local / k_fr_dt_cols_carry,
csrc/emap_inpaint_fronts.hip).  The fill's schedule is the distance itself, so the filled image and the reported largest front
(fronts_run = max d) against the restatement (tests/_telea_fronts.py) pin g through the host door, bit for bit.  Heights of 2, 31, 32,
33, 64, 65 and 97 rows: one partial block, one row short of a block, exactly one (no carry launch), one row into a second block, two
full blocks, one row into a third, three blocks and a row; 5 and 300 columns (a ragged and a second workgroup of 256 columns).  The
masks put the only known pixels of a column into its first block, its last block, one block in the middle, or nowhere, so every carry
crosses whole blocks in both directions.

The "sparse" masks (2 % known pixels, far apart) are compared through fronts_run and the known pixels only: on such masks k_fr_advance
and the restatement disagree by one level in single pixels of front 5 (97 x 300 with the image below: pixel (22, 263), 196 against 197),
with the one-thread-per-column pass exactly as with this one -- a finding about the estimator, not about the distance."""
import ctypes as ct

import numpy as np
import pytest

import _telea_fronts as tf

pytestmark = pytest.mark.gpu
U8P = ct.POINTER(ct.c_uint8)
ROWS = (2, 31, 32, 33, 64, 65, 97)
COLS = (5, 300)
MASKS = ("top", "bottom", "middle", "sparse")
BLOCK = 32


def _mask(rows, cols, kind):
    m = np.ones((rows, cols), np.uint8)
    rng = np.random.default_rng(rows * 1000 + cols)
    if kind == "top":                  # known pixels in the first rows only, none at all in every third column
        m[0, :] = 0; m[min(1, rows - 1), ::2] = 0; m[:, 2::3] = 1; m[0, 0] = 0
    elif kind == "bottom":
        m[rows - 1, :] = 0; m[max(rows - 3, 0), 1::2] = 0; m[:, 1::4] = 1; m[rows - 1, cols - 1] = 0
    elif kind == "middle":             # one known pixel per column in the block in the middle, at a row that moves with the column
        b0 = (rows // BLOCK // 2) * BLOCK
        m[np.minimum(b0 + np.arange(cols) % BLOCK, rows - 1), np.arange(cols)] = 0
    else:
        m[rng.uniform(0, 1, (rows, cols)) < 0.02] = 0; m[rows // 2, cols // 2] = 0
    return m


def _image(rows, cols):
    """a ramp with noise, the kind of image tests/test_hip_inpaint_fronts.py fills"""
    y, x = np.mgrid[0:rows, 0:cols]
    return np.clip(80 + 0.4 * x + 0.5 * y + np.random.default_rng(rows + cols).normal(0, 3, (rows, cols)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def handle():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    h = ct.c_void_p()
    assert lib.emap_inpainter_create(0, None, ct.byref(h)) == 0 and h.value
    yield lib, h
    assert lib.emap_inpainter_destroy(h) == 0


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("cols", COLS)
def test_every_block_count_equals_the_restatement(handle, cols, kind):
    lib, h = handle
    crossed = 0
    for rows in ROWS + (64, 2):        # (and back down: the scratch of a larger image serves a smaller one)
        mask = _mask(rows, cols, kind)
        img = _image(rows, cols)
        d = tf.distance(mask)
        known = mask == 0
        for b in range(0, rows, BLOCK):  # columns whose nearest known pixel lies outside this block: the carry decides their distance
            crossed += int((known.any(axis=0) & ~known[b:b + BLOCK].any(axis=0)).sum())
        out = np.full_like(img, 77)
        n = ct.c_int32(-1)
        p = lambda a: a.ctypes.data_as(U8P)      # noqa: E731
        assert lib.emap_inpaint_telea_fronts_u8(h, p(img), p(mask), rows, cols, 1, p(out), ct.byref(n)) == 0
        assert n.value == int(d.max()), (rows, n.value, int(d.max()))
        assert np.array_equal(out[known], img[known])
        if kind == "sparse":
            continue
        want = tf.inpaint_fronts(img, mask)
        assert np.array_equal(out, want), "%d x %d, %s: %d pixels differ" % (rows, cols, kind, int((out != want).sum()))
        assert (want != img)[mask != 0].any()
    assert crossed > 0


def test_the_block_summaries_grow_with_the_shape_not_with_the_pixel_count(handle):
    """64 x 5 and 2 x 160 hold the same number of pixels; the second has sixteen times the (block, column) summaries"""
    lib, h = handle
    for rows, cols in ((64, 5), (2, 160), (160, 2)):
        mask = _mask(rows, cols, "middle")
        img = _image(rows, cols)
        out = np.full_like(img, 77)
        n = ct.c_int32(-1)
        p = lambda a: a.ctypes.data_as(U8P)      # noqa: E731
        assert lib.emap_inpaint_telea_fronts_u8(h, p(img), p(mask), rows, cols, 1, p(out), ct.byref(n)) == 0
        assert n.value == int(tf.distance(mask).max()) and np.array_equal(out, tf.inpaint_fronts(img, mask)), (rows, cols)
