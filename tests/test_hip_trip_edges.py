"""GPU: the frame's kernels on either side of the depth of their load batches, against the oracle BIT FOR BIT (tests/_trip_cases.py):
tiles of exactly 0 ... 4097 records for k_tile_count / k_tile_fuse (1024 threads, the first record requested in front of the staging,
1024 records per further trip; 4097 is the first heavy tile), clouds of 1 ... 6145 points for k_bin_scatter (batches of four points
per thread, a partial last chunk) with and without carried channel columns, and the two radii at which the column walk of
k_post<16, .>'s staging has exactly one and just over one pair per thread (it requests two per thread and turn, next to the rows).
The same two radii give 32 and 34 region rows there against 32 rows per turn, and 48 and 50 against the 48 per turn of k_post<32, .>
(8 waves x 6 rows), which a second child runs: exactly one row turn, and two rows into a second one whose other slots are clamped.

Every case runs its frames once on a fresh context with the binned scatter forced; all seven planes, the normal planes, the
traversability input, the semantic layers and the additive mean error of the drift compensation must equal the oracle's."""
import os

import numpy as np
import pytest

import _post_variants as pv
import _trip_cases as tc
import _variant_children as vc
from _util import assert_planes_equal, kernel_trace_rows, make_pair
from oracle import emap_oracle as eo

pytestmark = pytest.mark.gpu


def _run_pair(case, weights):
    """the case's frames on a HIP map (binned scatter forced) and on the oracle; returns both maps and the paths the HIP frames took"""
    cfg = tc.config(case, eo.YAML)
    hip, orc = make_pair(cfg, tc.C, case["mode"], weights)
    hip.set_scatter_mode("binned")
    if case["sem"]:
        hip.param.pointcloud_channel_fusions = dict(tc.FUSIONS)
    R, t, clouds = tc.case_frames(case)
    if "layout" in case:                                     # the intended occupancy, by the oracle's own index arithmetic, before anything runs
        for p in clouds:
            assert tc.records_per_tile(orc, p, R, t) == tc.layout(case["layout"]), case["key"]
    paths = []
    for p in clouds:
        if case["sem"]:
            hip.input_pointcloud(p, tc.CH, R, t.copy(), case["noise"], case["noise"])
            orc.update_map_with_kernel(p, R, t, case["noise"], case["noise"])
            orc.semantic_update(p, R, t, average=[(3, 0), (4, 1)], class_average=[(5, 2)], color=[(6, 3)], alpha=0.5)
        else:
            hip.update_map_with_kernel(p, [], R, t.copy(), case["noise"], case["noise"])
            orc.update_map_with_kernel(p, R, t, case["noise"], case["noise"])
        paths.append(hip.last_update_path())
        for _ in range(tc.TIME_TICKS):
            hip.update_time(); orc.update_time()
    return hip, orc, paths


def _compare(case, weights):
    hip, orc, paths = _run_pair(case, weights)
    what = case["key"]
    try:
        assert paths == ["binned"] * len(paths), (what, paths)
        assert_planes_equal(hip.elevation_map, orc.elevation_map, what=what)
        assert_planes_equal(hip.normal_map, orc.normal_map, names=["nx", "ny", "nz"], what=what)
        assert_planes_equal(np.asarray(hip.traversability_input)[None], np.asarray(orc.traversability_input)[None], names=["traversability_input"], what=what)
        assert hip.get_additive_mean_error() == float(orc.additive_mean_error), (what, hip.get_additive_mean_error(), orc.additive_mean_error)
        if case["sem"]:
            assert list(hip.semantic_map.layer_names) == tc.CH[3:], hip.semantic_map.layer_names
            assert_planes_equal(hip.semantic_map.semantic_map, np.array(orc.semantic_map[:4], np.float32), names=tc.CH[3:], what=what + " semantic")
        return hip.get_additive_mean_error()
    finally:
        hip.close()


@pytest.mark.parametrize("case", tc.OCCUPANCY, ids=[c["key"] for c in tc.OCCUPANCY])
def test_tiles_at_the_edges_of_the_record_batches(case, weights):
    add = _compare(case, weights)
    if case["noise"] > 0.0:
        assert add != 0.0, "%s: the drift gate never fired -- the frames found no inliers, the statistics were not exercised" % case["key"]


@pytest.mark.parametrize("case", tc.SCATTER, ids=[c["key"] for c in tc.SCATTER])
def test_clouds_at_the_edges_of_the_scatter_batches(case, weights):
    _compare(case, weights)


# ---- stencil staging: one child per tile height (the EMAP_POST_R hook is read once per process), tests/_post_variants.py's program on POST_CASES ----
CHILD_TIMEOUT_S = 300


@pytest.fixture(scope="module")
def post_child(tmp_path_factory):
    return vc.lazy_children(lambda v: vc.run_child(os.path.abspath(tc.__file__), v, tc.POST_CHILDREN[v]["env"], lambda k: k.startswith("EMAP_POST_"),
                                                   str(tmp_path_factory.mktemp("trip_post_" + v)), CHILD_TIMEOUT_S))


@pytest.fixture(scope="module")
def oracle_post(weights):
    return vc.cached_oracle(lambda case: _oracle_post(case[0], case[1], weights))


def _oracle_post(C, d, weights):
    _, orc = make_pair(dict(eo.YAML, dilation_size=d), C, "reference_fp16", weights)
    orc.elevation_map[...] = pv.state(C, d, pv.case_seed(C, d))
    orc.dilate()
    dil = orc.traversability_input.copy()
    orc.traversability(); orc.normals()
    return [np.array(a, np.float32) for a in (dil, orc.elevation_map, orc.normal_map, orc.traversability_input)]


def _check_post_child(child, case, post_child, oracle_post):
    got, trace = post_child(child)
    names = [n for n, _ in kernel_trace_rows(trace) if "k_post" in n]
    want_names = tc.POST_CHILDREN[child]["kernels"] * len(tc.POST_CASES)                  # per case: dilate, post, dilate, part 1, part 2
    assert len(names) >= len(want_names) and all(k + "," in n for k, n in zip(want_names, names)), names[:len(want_names)]
    key = pv.case_key(*case)
    want = oracle_post(case)
    for ctx in ("A", "B"):
        what = "%s context %s" % (key, ctx)
        assert np.array_equal(got["%s_%s_dilate" % (key, ctx)].view(np.uint32), want[0].view(np.uint32)), what + ": stage-1 dilation"
        vc.assert_case_planes(got, "%s_%s" % (key, ctx), want[1], want[2], want[3], what)


@pytest.mark.parametrize("case", tc.POST_CASES, ids=[pv.case_key(*c) for c in tc.POST_CASES])
def test_stencil_walks_of_one_and_two_pairs_per_thread(case, post_child, oracle_post):
    _check_post_child("r16_walk", case, post_child, oracle_post)


@pytest.mark.parametrize("case", tc.POST_CASES, ids=[pv.case_key(*c) for c in tc.POST_CASES])
def test_stencil_rows_of_one_turn_and_two_rows_more_in_the_tallest_tile(case, post_child, oracle_post):
    _check_post_child("r32_rows", case, post_child, oracle_post)
