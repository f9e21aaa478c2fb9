"""GPU: the deferred stencil pass.  A whole-map frame on the binned path leaves its stencil pass pending and the next such frame runs it
in ONE launch with its own histogram (k_post_hist<MODE, 16 | 32>); every other call into the library launches a pending pass first.

One child process per tile height (EMAP_POST_R is read once per process; EMAP_POST_DMA=0 keeps the plain k_post, the only stencil
kernel that is deferred) plays every sequence of tests/_post_deferred.py three ways -- deferral on and the planes read at the end,
deferral on and the planes read after every step, EMAP_POST_DEFER=0 -- on 202^2 (interior tiles) and 130^2 maps (a last tile of 2 rows
by 2 columns), dilation 3, both index modes, clouds of 1, 4097 and 20 000 points with NaN rows.  The seven map planes, the three normal
planes and the dilated input are compared bit for bit between the three ways and with the oracle, and the counter of fused launches
proves which path ran: a passing comparison without it would prove nothing."""
import os

import numpy as np
import pytest

import _post_deferred as pd
import _variant_children as vc
from _util import make_pair

pytestmark = pytest.mark.gpu

VARIANTS = {"r16": {"EMAP_POST_R": "16", "EMAP_POST_DMA": "0"}, "r32": {"EMAP_POST_R": "32", "EMAP_POST_DMA": "0"}}
CHILD_TIMEOUT_S = 240      # some 60 contexts of at most 202^2 cells with two to five small frames each: seconds; the rest is start-up
CASES = [(name, m) for name, (maps, _, _) in pd.SEQUENCES.items() for m in maps]
PLANES = ("_map", "_normal", "_trav_in")


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """variant -> the child's recorded arrays: started the first time a test needs it, never twice; after a child that ended badly
    none is started (tests/_variant_children.py)"""
    def run(v):
        drop = lambda k: k.startswith("EMAP_POST_")
        return vc.run_child(os.path.abspath(pd.__file__), v, VARIANTS[v], drop, str(tmp_path_factory.mktemp("defer_" + v)), CHILD_TIMEOUT_S, tracer=None)[0]
    return vc.lazy_children(run)


def _oracle_planes(key, weights):
    name, m = key
    C, mode = pd.MAPS[m]
    if name.startswith("two_contexts"):
        k = int(name[-1])
        opts, steps = {}, [(s[0], s[1] + 100 * k, s[2]) for s in pd.TWO_CONTEXTS]
    else:
        _, opts, steps = pd.SEQUENCES[name]
    _, orc = make_pair(pd.config(opts), C, mode, weights)
    pd.play_oracle(orc, steps)
    out = tuple(np.array(a, np.float32) for a in (orc.elevation_map, orc.normal_map, orc.traversability_input))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def oracle(weights):
    return vc.cached_oracle(lambda key: _oracle_planes(key, weights))


def _same_three_ways(got, name, m):
    ref = pd.key_of(name, m, "off")
    for way in ("end", "each"):
        for pl in PLANES:
            a, b = got[pd.key_of(name, m, way) + pl], got[ref + pl]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s on map %s: %s differs between '%s' and EMAP_POST_DEFER=0" % (name, m, pl, way)


@pytest.mark.parametrize("case", CASES, ids=["%s_%s" % c for c in CASES])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_sequences_three_ways_and_the_oracle(variant, case, children, oracle):
    got = children(variant)
    name, m = case
    _same_three_ways(got, name, m)
    want = oracle(case)
    for way in pd.WAYS:
        vc.assert_case_planes(got, pd.key_of(name, m, way), want[0], want[1], want[2], "%s %s on map %s, way '%s'" % (variant, name, m, way))
    fused = {way: int(got[pd.key_of(name, m, way) + "_fused"][0]) for way in pd.WAYS}
    print("%s %s map %s: fused launches %r, paths %s" % (variant, name, m, fused, got[pd.key_of(name, m, "end") + "_paths"]))
    assert fused["off"] == 0, fused
    assert fused["end"] == pd.FUSED_END[name], fused
    # read after every step: a read launches the pending pass, so only frames with NOTHING between them fuse -- none does here
    assert fused["each"] == 0, fused


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_back_to_back_frames_fuse_all_but_the_first(variant, children):
    """the counter equals the number of binned frames minus one"""
    got = children(variant)
    for m in pd.SEQUENCES["four_frames"][0]:
        paths = str(got[pd.key_of("four_frames", m, "end") + "_paths"]).split(",")
        assert paths == ["binned"] * 4, paths
        assert int(got[pd.key_of("four_frames", m, "end") + "_fused"][0]) == len(paths) - 1


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_small_frame_between_binned_frames_launches_the_pending_pass(variant, children):
    got = children(variant)
    paths = str(got[pd.key_of("small_between", "a", "end") + "_paths"]).split(",")
    assert paths == ["binned", "small_frame", "binned", "binned"], paths


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_two_contexts_alternating(variant, children, oracle):
    got = children(variant)
    for k in range(2):
        name = "two_contexts%d" % k
        _same_three_ways(got, name, "a")
        want = oracle((name, "a"))
        vc.assert_case_planes(got, pd.key_of(name, "a", "end"), want[0], want[1], want[2], "%s %s" % (variant, name))
        assert int(got[pd.key_of(name, "a", "end") + "_fused"][0]) == len(pd.TWO_CONTEXTS) - 1
        assert int(got[pd.key_of(name, "a", "off") + "_fused"][0]) == 0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_stage_timing_keeps_every_frame_whole(variant, children):
    got = children(variant)
    for way in pd.WAYS:
        assert int(got[pd.key_of("timing", "b", way) + "_fused"][0]) == 0
        ms = got[pd.key_of("timing", "b", way) + "_stage_ms"]
        assert np.all(np.isfinite(ms)) and ms[:3].sum() > 0 and ms[9] > 0, ms      # hist + scan + scatter, and the stencil stage ("post")
