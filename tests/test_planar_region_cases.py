"""CPU: the host model of the planar regions (elevation_mapping_cupy_amd/planar_regions.py) against independent
restatements -- scipy.ndimage's components and erosions, Upsampling.cpp's loops written out, OpenCV's elliptic element from its formula
-- on the scenes of tests/_planar_region_cases.py and on random binary images up to 13 x 13, and the lost pieces: each must change the
answer on at least one scene.  Reference: ContourExtraction.cpp:28-128, Upsampling.cpp:12-68, PlanarRegion.cpp:5-50."""
import numpy as np
import pytest
from scipy import ndimage as ndi

import _planar_region_cases as rc
from elevation_mapping_cupy_amd import planar_regions as pr

EIGHT = np.ones((3, 3), bool)


def _random_masks(n=300, seed=5):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        U = int(rng.integers(2, 14))
        yield (rng.random((U, U)) < rng.choice([0.25, 0.5, 0.75])).astype(np.int32)


def _masks():
    yield from _random_masks()
    for M in (33, 65):
        yield from rc.raw_scenes(M).values()


def _chain(X, ring, raw, succ):
    """the cyclic sequence of distinct consecutive owners of a ring, walked crack by crack from its smallest crack"""
    start = int(np.searchsorted(raw, ring["crack"]))
    assert raw[start] == ring["crack"]
    owners, k = [], start
    while True:
        owners.append(int(raw[k] >> 2))
        k = int(succ[k])
        if k == start:
            break
    chain = [o for n, o in enumerate(owners) if n == 0 or o != owners[n - 1]]
    if len(chain) > 1 and chain[-1] == chain[0]:
        chain.pop()
    return chain


def test_the_successor_map_is_a_permutation_and_its_rings_are_the_borders():
    for X in _masks():
        U = X.shape[0]
        raw, succ = pr.successors(X)
        assert np.array_equal(np.sort(succ), np.arange(len(raw)))
        t = pr.trace_labels(X, 1, mode=1)
        rings = t.rings[t.rings["image"] == 0]
        n_comp = ndi.label(X, structure=EIGHT)[1]
        bg, n_bg = ndi.label(np.pad(X, 1) == 0)                   # 4-connected; the component of the padded frame is no hole
        assert len(rings) == n_comp + n_bg - 1 and int((rings["is_hole"] == 0).sum()) == n_comp
        assert (np.diff(rings["crack"]) > 0).all() and (t.vertices >= 0).all() and (t.vertices < U).all()
        assert int(t.rings["n_vertices"].sum()) == len(t.vertices) and np.array_equal(t.rings["first_vertex"], np.cumsum(t.rings["n_vertices"]) - t.rings["n_vertices"])
        P = np.pad(X, 1)
        edge = (X != 0) & ((P[:-2, 1:-1] == 0) | (P[2:, 1:-1] == 0) | (P[1:-1, :-2] == 0) | (P[1:-1, 2:] == 0))
        seen = np.zeros(U * U, bool)
        for r in rings:
            chain = _chain(X, r, raw, succ)
            seen[chain] = True
            q = np.array(chain + chain[:1])
            assert (np.abs(np.diff(q // U)) <= 1).all() and (np.abs(np.diff(q % U)) <= 1).all()      # consecutive chain pixels are 8-neighbours
            v = t.vertices[r["first_vertex"]:r["first_vertex"] + r["n_vertices"]]
            if len(chain) == 1:
                assert r["n_vertices"] == 1
            steps = [(chain[n] // U - chain[n - 1] // U, chain[n] % U - chain[n - 1] % U) for n in range(len(chain))]      # the step INTO pixel n
            want = [chain[n] for n in range(len(chain)) if len(chain) == 1 or steps[n] != steps[(n + 1) % len(chain)]]
            assert [int(y) * U + int(x) for x, y in v] == want
            if not r["is_hole"]:
                assert v[0][1] * U + v[0][0] == r["root"] == np.flatnonzero(ndi.label(X, structure=EIGHT)[0].ravel() == ndi.label(X, structure=EIGHT)[0].ravel()[r["root"]])[0]
        assert np.array_equal(seen.reshape(U, U), edge)


def test_a_rectangle_gives_its_corners_and_a_line_its_ends():
    X = np.zeros((9, 9), np.int32)
    X[2:6, 3:8] = 1
    t = pr.trace_labels(X, 1, mode=1)
    assert t.vertices[:4].tolist() == [[3, 2], [3, 5], [7, 5], [7, 2]]      # down the left side first
    assert t.rings["n_vertices"].tolist() == [4, 4] and t.vertices[4:].tolist() == [[4, 3], [4, 4], [6, 4], [6, 3]]      # the inset: one pixel in
    X = np.zeros((5, 5), np.int32)
    X[2, 1:4] = 1
    assert pr.trace_labels(X, 1, mode=1).vertices.tolist() == [[1, 2], [3, 2]]
    X = np.zeros((5, 5), np.int32)
    X[3, 3] = 1
    t = pr.trace_labels(X, 1, mode=1)
    assert t.vertices.tolist() == [[3, 3]] and t.rings["n_vertices"].tolist() == [1]


def test_the_upsampling_rule_is_the_reference_loops():
    rng = np.random.default_rng(1)
    for M in (2, 3, 4, 7, 12):
        L = rng.integers(0, 5, (M, M)).astype(np.int32)
        assert np.array_equal(pr.upsample(L), rc.upsample_loops(L))
        assert pr.upsample(L).shape == (3 * M - 2, 3 * M - 2)


def test_the_elliptic_element_is_opencvs_and_holds_the_cross():
    for margin in range(pr.MARGIN_MAX + 1):
        k = 2 * (1 + margin) + 1
        elem = np.zeros((k, k), bool)
        for a, b in pr.ellipse_offsets(k):
            elem[a + k // 2, b + k // 2] = True
        assert np.array_equal(elem, rc.opencv_ellipse(k)), k
        assert all(elem[k // 2 + a, k // 2 + b] for a, b in pr.CROSS)
    assert np.array_equal(rc.opencv_ellipse(3), rc.CROSS3)


@pytest.mark.parametrize("margin", rc.MARGINS)
def test_the_all_label_erosions_and_the_local_fallback(margin):
    """per label with scipy: the margin erosion, the cross erosion, and 'the margin route yields no inset component of >= 2 pixels'"""
    elem = rc.opencv_ellipse(2 * (1 + margin) + 1)
    for M in (8, 12, 33):
        for name, (L, n) in rc.label_scenes(M).items():
            up = pr.upsample(L)
            Am, Ac = pr.erode(up, pr.ellipse_offsets(elem.shape[0])), pr.erode(up, pr.CROSS)
            A, B = pr.images(L, n, margin)
            for lab in range(1, n + 1):
                b = up == lab
                m, c = rc.erode_label(b, elem), rc.erode_label(b, rc.CROSS3)
                assert np.array_equal(Am == lab, m) and np.array_equal(Ac == lab, c), (name, M, lab)
                ins = pr.zero_frame(rc.erode_label(m, rc.CROSS3).astype(np.int32))
                lab8, k = ndi.label(ins, structure=EIGHT)
                keeps = k > 0 and int(np.bincount(lab8.ravel())[1:].max()) >= 2
                assert np.array_equal(A == lab, m if keeps else c), (name, M, lab, keeps)
                assert np.array_equal(B == lab, pr.zero_frame(rc.erode_label(A == lab, rc.CROSS3).astype(np.int32)) == 1), (name, M, lab)
            assert ((Am == 0) | (Am == Ac)).all()              # A_m is a subset of A_c


def test_components_are_label_pure_and_insets_lie_in_their_boundary():
    for M in (12, 33):
        for margin in rc.MARGINS:
            for name, (L, n) in rc.label_scenes(M).items():
                t = pr.trace_labels(L, n, margin)
                for X, roots in ((t.A, t.roots_a), (t.B, t.roots_b)):
                    lab8, k = ndi.label(X != 0, structure=EIGHT)
                    for c in range(1, k + 1):
                        sel = lab8 == c
                        assert len(np.unique(X[sel])) == 1 and (roots[sel] == np.flatnonzero(sel.ravel())[0]).all(), (name, M)
                assert ((t.B == 0) | (t.B == t.A)).all()
                ins = t.rings[t.rings["image"] == 1]
                assert (ins["boundary"] == t.roots_a.ravel()[ins["root"]]).all() and (ins["boundary"] >= 0).all()


def test_the_regions_of_the_scenes():
    M = 12
    S = rc.label_scenes(M)
    t = pr.trace_labels(*S["lines"], 1)
    got = pr.assemble(t.rings, t.vertices)
    assert [g["label"] for g in got] == [2]                    # one cell wide: no region; two cells wide: one
    t0 = pr.trace_labels(*S["lines"], 1, fallback=False)
    assert pr.assemble(t0.rings, t0.vertices) == []            # ... and only by the fallback
    t = pr.trace_labels(*S["ring with an island"], 0)
    got = pr.assemble(t.rings, t.vertices)
    assert [g["label"] for g in got] == [1, 2] and len(got[0]["boundary"]["holes"]) == 1 and len(got[0]["insets"]) == 1 and len(got[0]["insets"][0]["holes"]) == 1
    t = pr.trace_labels(*S["empty"], 1)
    assert len(t.rings) == 0 and t.vertices.shape == (0, 2) and pr.assemble(t.rings, t.vertices) == []
    t = pr.trace_labels(*S["blocks"], 0)
    got = pr.assemble(t.rings, t.vertices)
    keys = [(g["label"], g["root"]) for g in got]
    assert keys == sorted(keys) and len(keys) > 3 and len(set(k[0] for k in keys)) == 3      # several pieces per label, ascending (label, root)


def test_every_lost_piece_changes_the_answer_somewhere():
    for what, kw in rc.LOST.items():
        changed = False
        for M in (12, 33):
            for margin in (1,):
                for L, n in rc.label_scenes(M).values():
                    changed = changed or not rc.same_answer(pr.trace_labels(L, n, margin), pr.trace_labels(L, n, margin, **kw))
            if "edge" not in what:
                for X in rc.raw_scenes(M + 32).values():
                    changed = changed or not rc.same_answer(pr.trace_labels(X, 1, mode=1), pr.trace_labels(X, 1, mode=1, **kw))
        assert changed, what
    X = rc.spiral(65)
    full, short = pr.trace_labels(X, 1, mode=1), pr.trace_labels(X, 1, mode=1, short=1)
    assert len(full.rings) == 1 and not rc.same_answer(full, short)      # the longest border needs every doubling round


def test_the_frame_of_a_region():
    T = pr.transform_plane_to_world([0.0, 0.0, 2.0], [1.0, 2.0, 3.0])      # z up: y = z x unitX = unitY, x = y x z = unitX
    assert T.tolist() == [[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]]
    for n in ([0.1, -0.2, 0.9], [1.0, 1e-5, 1e-5], [0.0, 0.0, 1.0]):      # the second: the crossTolerance branch
        T = pr.transform_plane_to_world(n, [0.5, -0.25, 0.125])
        R = T[:3, :3]
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(R), 1.0) and np.allclose(R[:, 2], np.asarray(n) / np.linalg.norm(n))
        assert T[:3, 3].tolist() == [0.5, -0.25, 0.125] and T[3].tolist() == [0, 0, 0, 1]
    T = pr.transform_plane_to_world([0.1, -0.2, 0.9], [0.5, -0.25, 0.125])
    px = np.array([[4, 7], [0, 0]])
    got = pr.to_plane(px, T, 0.04 / 3.0, (1.0, 2.0))
    for (x, y), g in zip(px, got):                             # the point of the plane above the pixel, in the plane's frame
        w = np.array([1.0 - 0.04 / 3.0 * y, 2.0 - 0.04 / 3.0 * x, 0.0])
        w[2] = T[2, 3] - (T[0, 2] * (w[0] - T[0, 3]) + T[1, 2] * (w[1] - T[1, 3])) / T[2, 2]
        local = np.linalg.solve(T, np.append(w, 1.0))
        assert np.allclose(local[:2], g, atol=1e-12) and abs(local[2]) < 1e-12


def test_the_model_refuses_what_the_device_refuses():
    ok = np.zeros((4, 4), np.int32)
    for bad in (dict(labels=np.zeros((1, 1), np.int32)), dict(labels=np.zeros((3, 4), np.int32)), dict(margin_size=15), dict(margin_size=-1), dict(mode=2),
                dict(labels=ok + 2, n_labels=1), dict(labels=ok - 1), dict(labels=ok + 2, mode=1), dict(n_labels=-1)):
        kw = dict(labels=ok, n_labels=1, margin_size=1, mode=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            pr.trace_labels(kw["labels"], kw["n_labels"], kw["margin_size"], kw["mode"])
    assert 4 * (3 * pr.SIDE_MAX - 2) ** 2 < 2 ** 31 <= 4 * (3 * (pr.SIDE_MAX + 1) - 2) ** 2 and 4 * pr.RAW_SIDE_MAX ** 2 < 2 ** 31 <= 4 * (pr.RAW_SIDE_MAX + 1) ** 2
