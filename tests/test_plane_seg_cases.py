"""CPU: the host model of the plane segmentation (elevation_mapping_cupy_amd/plane_segmentation.py, composed in tests/_plane_seg_cases.py)
against independent yardsticks, and the scenes the GPU tests run (tests/test_hip_plane_seg.py) against the conditions that make a
bit-for-bit comparison meaningful.  DESIGN.md section 21 quotes the figures asserted here.

1. components: the same partition as scipy.ndimage.label (the only test that needs scipy).
2. window planes: eigenvalues and normals against numpy.linalg.eigh -- model against LAPACK, both on this CPU.  Measured over every
   scene: eigenvalues 8.0e-16 of the largest eigenvalue, normals 9.9e-14 per component where the two smallest eigenvalues are apart;
   asserted at 4 x.  The same run fixes the sweep count: 3 sweeps reach these figures, 2 do not (4.4e-8, 1.7e-4), so EM_PLANE_SWEEPS = 4.
3. label planes: the fixed-point moments about the anchor against plain double sums about the map origin (:170-199).  Measured: the
   normals 4.0e-4 degrees apart, the support vectors 7.0e-7 m; asserted at 4 x.
4. margins: a condition on the INPUTS.  No cell's planar bit, no label's verdict hangs on the last bits of a double.  For the window
   error the condition is counted where the error can decide the bit -- cells whose normal passes the inclination test or lies within
   2 degrees of it: the fitted error of a window across a step of 10 x the threshold at 4 cm cells lies at 1.03 x the threshold^2
   whatever one does (the cell is not planar by 33 degrees of inclination), so an unconditional count cannot be zero on the terraces.
   A ramp AT 32 degrees is 2 degrees from the 30 degree limit up to the float rounding of its heights: "within 2 degrees" is
   counted with 1e-3 degrees of slack.
5. every lost piece changes the answer on at least one scene."""
import re
import os

import numpy as np
import pytest

import _plane_seg_cases as pc
from conftest import ROOT
from elevation_mapping_cupy_amd import plane_segmentation as ps

EIGENVALUE_DEV, NORMAL_DEV = 8.0e-16, 9.9e-14                # measured (check 2), asserted at 4 x
LABEL_ANGLE_DEV_DEG, LABEL_SUPPORT_DEV_M = 4.0e-4, 7.0e-7   # measured (check 3: heights enter in steps of 2^-13 m), asserted at 4 x
_cache = {}


def _runs():
    """every scene at the small sizes, BIG_SCENES at the largest: computed once"""
    if not _cache:
        for C in pc.SIZES:
            M = C - 2
            for name, (h, over, props) in pc.scenes(M).items():
                if C == pc.SIZES[-1] and name not in pc.BIG_SCENES:
                    continue
                _cache[(M, name)] = (h, over, props, pc.model(h, over))
    return _cache


def test_the_scenes_are_what_they_claim():
    for (M, name), (h, over, props, r) in _runs().items():
        if "mask" in props:
            assert (r.planar == props["mask"]).all(), (M, name)      # a one-cell-wide line really is one
        if "n_labels" in props:
            assert r.n_labels == props["n_labels"], (M, name, r.n_labels)
        if "n_planes" in props:
            assert len(r.planes) == props["n_planes"], (M, name, len(r.planes))
        if "needs" in props:
            assert r.planes["needs_refinement"].tolist() == props["needs"], (M, name)
        else:
            assert not r.planes["needs_refinement"].any(), (M, name)
        assert r.labels.dtype == np.int32 and r.labels.max() <= r.n_labels and (r.planes["label"][1:] > r.planes["label"][:-1]).all()
    cb = _runs()[(32, "checkerboard")][3]
    assert cb.n_labels == int(cb.planar.sum()) > 32 * 32 // 2 - 8 and cb.details.slots == 0      # one label a cell, not one slot
    r32 = _runs()[(32, "ramp 32")][3]
    assert r32.planar.all() and (r32.labels == 0).all() and (r32.labels0 == 1).all()             # locally planar, the label rejected
    pieces = _runs()[(65, "pieces")][3]
    w = pieces.window
    assert ((w.n == 1) & w.centre).any() and ((w.n == 2) & w.centre).any() and ((w.n >= 3) & w.centre & (w.err > 1e29)).any()      # n < 3, and 3 collinear points
    roots = np.nonzero(pieces.root.ravel() == np.arange(65 * 65))[0]
    assert any(r // 65 % 32 == 0 for r in roots) and any(r % 65 % 32 == 0 for r in roots) and any(r // 65 % 32 and r % 65 % 32 for r in roots)


def test_components_are_scipys_partition():
    ndi = pytest.importorskip("scipy.ndimage")
    for (M, name), (h, over, props, r) in _runs().items():
        conn = pc.params(**over)["connectivity"]
        want, n = ndi.label(r.planar, structure=np.ones((3, 3), int) if conn == 8 else None)
        got = pc.ps.numbering(r.root)[0]
        assert n == r.n_labels, (M, name)
        pairs = np.unique(np.stack([want.ravel(), got.ravel()]), axis=1)
        assert pairs.shape[1] == n + (1 if (want == 0).any() else 0), (M, name)      # a bijection of labels
        # and the numbering: the first cell of a raster scan gets the next number (scipy numbers the same way)
        assert (want == got).all(), (M, name)


def test_window_planes_against_lapack():
    worst_w = worst_n = 0.0
    for (M, name), (h, over, props, r) in _runs().items():
        win = r.window
        ok = win.centre & (win.n >= 3)
        w, n0 = pc.eigh_window(win)
        scale = np.maximum(np.abs(w[..., 2]), 1e-300)
        worst_w = max([worst_w] + [float((np.abs(win.w[k] - w[..., k]) / scale)[ok].max()) for k in range(3)])
        apart = ok & (w[..., 1] > 1e-8) & ((w[..., 1] - w[..., 0]) > 1e-6 * scale)
        if apart.any():
            worst_n = max([worst_n] + [float(np.abs(win.normal[k] - n0[..., k])[apart].max()) for k in range(3)])
    print("window planes against eigh: eigenvalues %.3g of the largest, normals %.3g" % (worst_w, worst_n))
    assert worst_w <= 4 * EIGENVALUE_DEV and worst_n <= 4 * NORMAL_DEV
    src = open(os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc", "emap_launch.h")).read()
    assert int(re.search(r"#define EM_PLANE_SWEEPS (\d+)", src).group(1)) == ps.SWEEPS == 4      # one count for the device and the model
    assert int(re.search(r"#define EM_PLANE_Q_BITS (\d+)", src).group(1)) == ps.Q_BITS and float(re.search(r"#define EM_PLANE_Q_RANGE ([\d.]+)", src).group(1)) == ps.Q_RANGE


def test_the_sweep_count_is_the_smallest_that_agrees_plus_one():
    def dev(sweeps):
        worst = 0.0
        for (M, name), (h, over, props, r) in _runs().items():
            if M > 100:
                continue
            P = pc.params(**over)
            win = ps.window_pass(h, P["kernel_size"], pc.RES, P["plane_patch_error_threshold"] ** 2, r.cos[1], sweeps=sweeps)
            ok = win.centre & (win.n >= 3)
            w, _ = pc.eigh_window(win)
            scale = np.maximum(np.abs(w[..., 2]), 1e-300)
            worst = max([worst] + [float((np.abs(win.w[k] - w[..., k]) / scale)[ok].max()) for k in range(3)])
        return worst
    assert dev(ps.SWEEPS - 2) > 1e-9 and dev(ps.SWEEPS - 1) <= 4 * EIGENVALUE_DEV


def test_fixed_point_label_planes_against_plain_double_sums():
    worst_angle = worst_support = 0.0
    seen = 0
    for (M, name), (h, over, props, r) in _runs().items():
        P = r.P
        want = pc.double_label_planes(h, r.labels0, pc.RES, pc.ORIGIN, P["min_number_points_per_label"])
        kept = {lab: v for lab, v in want.items() if v[2][2] > r.cos[0]}
        assert sorted(kept) == r.planes["label"].tolist(), (M, name)
        for rec in r.planes:
            n, support, normal = kept[int(rec["label"])]
            assert n == rec["n_points"] and rec["n_left_out"] == 0
            worst_angle = max(worst_angle, float(np.degrees(np.arccos(min(1.0, abs(float(np.dot(normal, rec["normal"]))))))))
            worst_support = max(worst_support, float(np.abs(support - rec["support"]).max()))
            seen += 1
    print("label planes, fixed point against double: %.3g degrees, %.3g m over %d planes" % (worst_angle, worst_support, seen))
    assert seen > 40 and worst_angle <= 4 * LABEL_ANGLE_DEV_DEG and worst_support <= 4 * LABEL_SUPPORT_DEV_M


def test_cells_beyond_the_fixed_point_range_are_left_out_and_counted():
    M = 8
    h = np.zeros((M, M), np.float32)
    h[4:, :] = 40.0                                                            # farther than 32 m from the anchor (0, 0)
    root = np.zeros((M, M), np.int64)                                          # one component, given (no window pass joins such cells)
    labels, planes, _ = ps.label_planes(h, np.zeros((3, M, M), np.float32), root, np.ones((M, M), np.int32), pc.RES, pc.ORIGIN, 4, 0.5, 1e9, -1.0)
    assert planes["n_points"].tolist() == [32] and planes["n_left_out"].tolist() == [32] and abs(planes["support"][0][2]) < 1e-12


def test_no_scene_hangs_on_the_last_bits():
    slack = 1e-3
    for (M, name), (h, over, props, r) in _runs().items():
        P, w = r.P, r.window
        thr2 = P["plane_patch_error_threshold"] ** 2
        local, plane, glob = (P[k] for k in ("local_plane_inclination_threshold_degrees", "plane_inclination_threshold_degrees", "global_plane_fit_angle_error_threshold_degrees"))
        fitted = w.centre & (w.n >= 3) & (w.err < 1e29)
        angle = np.degrees(np.arccos(np.clip(w.normal[2], -1.0, 1.0)))
        near_err = fitted & (w.err > thr2 / 4) & (w.err < 4 * thr2) & (angle < local + 2)
        near_angle = fitted & (np.abs(angle - local) < 2 - slack) & (w.err < 4 * thr2)
        middle = w.centre & (w.n >= 3) & (w.w[1] > 1e-8 / 4) & (w.w[1] < 4e-8)      # the test on the middle eigenvalue
        assert int(near_err.sum()) == 0 and int(near_angle.sum()) == 0 and int(middle.sum()) == 0, (M, name)
        if r.details.slots:
            la = np.degrees(np.arccos(np.clip(r.details.normal_z, -1.0, 1.0)))
            assert int((np.abs(la - plane) < 2 - slack).sum()) == 0, (M, name, la)
            assert not ((r.details.w[1] > 1e-8 / 4) & (r.details.w[1] < 4e-8)).any()
            d, a = r.details.max_dist / P["global_plane_fit_distance_error_threshold"], np.degrees(np.arccos(np.clip(r.details.min_dot, -1.0, 1.0))) / glob
            assert int(((d > 0.5) & (d < 2)).sum()) == 0 and int(((a > 0.5) & (a < 2)).sum()) == 0, (M, name, d, a)


def test_every_lost_piece_changes_an_answer():
    base = {k: pc.answer(v[3]) for k, v in _runs().items() if k[0] < 100}
    for lose in pc.LOST:
        hit = [k for k in base if pc.answer(pc.model(_runs()[k][0], _runs()[k][1], lose=lose)) != base[k]]
        assert hit, lose
        print("%-24s changes %d of %d answers, e.g. %r" % (lose, len(hit), len(base), hit[0]))
    # the U is the scene the lost arm is about; a single tile has no border to merge
    u = _runs()[(65, "U")]
    assert pc.answer(pc.model(u[0], u[1], lose="lost arm")) != base[(65, "U")]
    one = _runs()[(32, "serpentine")]
    assert pc.answer(pc.model(one[0], one[1], lose="no border merge")) == base[(32, "serpentine")]
