"""CPU: the contract of the Inpainting plugin's method "telea_fronts" (tests/_telea_fronts.py restates it; the device must equal that
restatement bit for bit, tests/test_hip_inpaint_fronts.py) -- what every inpainting must do, its agreement with the host Telea
(oracle/telea.py), and that it is closer to the host Telea than the existing device method "front"."""
import numpy as np
import pytest

import _telea_fronts as tf
from oracle import telea
from test_inpaint_telea import _case


def _agreement(got, want, mask):
    dd = np.abs(got.astype(int) - want.astype(int))[mask != 0]
    return float((dd == 0).mean()), float((dd <= 2).mean()), float(dd.mean())


def test_properties():
    img, mask = _case(7, n=40)
    out = tf.inpaint_fronts(img, mask)
    assert np.array_equal(out[mask == 0], img[mask == 0])                   # known pixels are never touched
    flat = np.full((20, 20), 117, np.uint8); m = np.zeros((20, 20), np.uint8); m[5:15, 6:13] = 1
    assert np.array_equal(tf.inpaint_fronts(flat * (m == 0), m), flat)      # a constant image is reproduced
    y, x = np.mgrid[0:24, 0:24]
    ramp = (40 + 4 * x).astype(np.uint8); m = np.zeros((24, 24), np.uint8); m[8:16, 8:16] = 1
    filled = tf.inpaint_fronts(np.where(m == 0, ramp, 0).astype(np.uint8), m)
    err = np.abs(filled.astype(int) - ramp.astype(int))[m != 0]
    assert err.max() <= 14 and err.mean() <= 5                               # the 32-level ramp across the hole
    assert np.array_equal(tf.inpaint_fronts(img, np.zeros_like(mask)), img)              # nothing to fill
    assert np.array_equal(tf.inpaint_fronts(img, np.ones_like(mask)), img)               # no known pixel
    with pytest.raises(ValueError):
        tf.inpaint_fronts(img, mask, radius=2)
    with pytest.raises(ValueError):
        tf.inpaint_fronts(np.zeros((1, 9), np.uint8), np.ones((1, 9), np.uint8))


@pytest.mark.parametrize("seed", [1, 2, 7])
def test_agreement_with_host_telea(seed):
    img, mask = _case(seed)
    exact, within2, mean = _agreement(tf.inpaint_fronts(img, mask), telea.inpaint_telea(img, mask, 1), mask)
    assert exact >= 0.45 and within2 >= 0.70 and mean <= 2.2, (exact, within2, mean)


@pytest.mark.parametrize("seed", [1, 2, 7])
def test_closer_to_host_telea_than_the_front_rule(seed):
    img, mask = _case(seed)
    host = telea.inpaint_telea(img, mask, 1)
    e_f, _, m_f = _agreement(tf.inpaint_fronts(img, mask), host, mask)
    e_r, _, m_r = _agreement(tf.inpaint_front_rule(img, mask), host, mask)
    assert e_f > e_r and m_f < m_r, (e_f, e_r, m_f, m_r)


@pytest.mark.parametrize("seed,shape,frac", [(1, (9, 13), 0.5), (2, (2, 2), 0.5), (3, (2, 7), 0.6), (4, (12, 5), 0.85), (5, (16, 16), 0.3)])
def test_vectorised_equals_loops(seed, shape, frac):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, shape).astype(np.uint8)
    mask = (rng.uniform(0, 1, shape) < frac).astype(np.uint8)
    mask[0, 0] = 0
    if shape[0] > 4:
        mask[1:4, :] = 1                                                  # a band several fronts deep, touching both side borders
    assert np.array_equal(tf.inpaint_fronts(img, mask), tf.inpaint_fronts_loops(img, mask))


def test_vectorised_equals_loops_on_the_cases():
    img, mask = _case(2)
    assert np.array_equal(tf.inpaint_fronts(img, mask), tf.inpaint_fronts_loops(img, mask))


def test_distance_is_the_bfs_front_index():
    rng = np.random.default_rng(11)
    mask = (rng.uniform(0, 1, (37, 23)) < 0.9).astype(np.uint8)
    d = tf.distance(mask)
    ys, xs = np.nonzero(mask == 0)
    want = np.min(np.abs(np.arange(37)[:, None, None] - ys) + np.abs(np.arange(23)[None, :, None] - xs), axis=2)
    assert np.array_equal(d, want)
    assert (tf.distance(np.ones((4, 5), np.uint8)) == tf.INF).all()


def test_large_sparse_map_runs_in_seconds():
    """the restatement is usable as the device's yardstick at 1024^2 (no timing is asserted: the test only has to finish)"""
    rng = np.random.default_rng(0)
    n = 1024
    img = rng.integers(0, 256, (n, n)).astype(np.uint8)
    mask = np.ones((n, n), np.uint8); mask[400:460, 500:620] = rng.uniform(0, 1, (60, 120)) > 0.5
    out = tf.inpaint_fronts(img, mask)
    assert np.array_equal(out[mask == 0], img[mask == 0])


def test_library_exports_the_fronts_entry_points_and_rejects_bad_arguments():
    import ctypes as ct
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    for n in ("emap_inpainter_create", "emap_inpainter_destroy", "emap_inpainter_set_steps", "emap_inpaint_telea_fronts_u8"):
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    assert lib.emap_inpaint_telea_fronts_u8(None, None, None, 4, 4, 1, None, None) == -1       # (checked before any device call)
    assert lib.emap_inpainter_create(0, None, None) == -1
    assert lib.emap_inpainter_set_steps(None, 8) == -1
    assert lib.emap_inpainter_destroy(None) == 0
    h = ct.c_void_p()
    assert lib.emap_inpainter_create(10 ** 6, None, ct.byref(h)) == -1 and not h.value           # no such device


def test_plugin_keeps_the_method_name():
    """the plugin routes "telea_fronts" to the device fill (unknown names fall back to "telea", as in the reference)"""
    from elevation_mapping_cupy_amd.plugins.inpainting import Inpainting
    assert Inpainting(cell_n=8, method="telea_fronts").method == "telea_fronts"
    assert Inpainting(cell_n=8, method="no_such_method").method == "telea"
    assert Inpainting(cell_n=8).method == "telea"
