"""GPU: the pending stencil pass, taken along lean.  A frame that runs the pass of the frame before it in its histogram launch
(k_post_hist<MODE, 16 | 32, OUT>) lets it write only what the frame reads -- traversability, and the normals in front of a visibility
pass -- or, reading nothing, launches no stencil workgroup; the pass stays owed until a full one has run (emap_api.hip: count_impl).

One child process per tile height (as tests/test_hip_post_deferred.py forces them) plays every sequence of tests/_post_lean.py four ways
-- default, EMAP_POST_LEAN=0, EMAP_POST_DEFER=0, and with traversability_input and the normals read after every step -- on 202^2 and
130^2 maps (a last tile of 2 rows), dilation 3, both index modes, clouds on the binned path.  The seven map planes, the three normal
planes and traversability_input are compared bit for bit among the four ways and with the oracle; bits 16 and 32 of
emap_last_update_path and the counter of fused launches are asserted for every frame of every way: a passing comparison that never
ran lean would prove nothing."""
import os

import numpy as np
import pytest

import _post_deferred as pd
import _post_lean as pl
import _variant_children as vc
from _util import make_pair

pytestmark = pytest.mark.gpu

VARIANTS = {"r16": {"EMAP_POST_R": "16", "EMAP_POST_DMA": "0"}, "r32": {"EMAP_POST_R": "32", "EMAP_POST_DMA": "0"}}
CHILD_TIMEOUT_S = 240      # some 70 contexts of at most 202^2 cells with four to seven small frames each: seconds; the rest is start-up
CASES = [(name, m) for name, (maps, _, _) in pl.SEQUENCES.items() for m in maps]
PLANES = ("_map", "_normal", "_trav_in")


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    def run(v):
        drop = lambda k: k.startswith("EMAP_POST_")
        return vc.run_child(os.path.abspath(pl.__file__), v, VARIANTS[v], drop, str(tmp_path_factory.mktemp("lean_" + v)), CHILD_TIMEOUT_S, tracer=None)[0]
    return vc.lazy_children(run)


def _oracle_planes(key, weights):
    name, m = key
    C, mode = pl.MAPS[m]
    _, opts, steps = pl.SEQUENCES[name]
    _, orc = make_pair(pd.config(opts), C, mode, weights)
    pl.play_oracle(orc, steps)
    out = tuple(np.array(a, np.float32) for a in (orc.elevation_map, orc.normal_map, orc.traversability_input))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def oracle(weights):
    return vc.cached_oracle(lambda key: _oracle_planes(key, weights))


def test_the_table_of_expected_bits_covers_every_frame():
    """CPU-side sanity of the table itself (no child is started)"""
    for name, (_, _, steps) in pl.SEQUENCES.items():
        assert len(pl.LEAN_BITS[name]) == sum(s[0] == "frame" for s in steps), name
    assert any(16 in b for b in pl.LEAN_BITS.values()) and any(32 in b for b in pl.LEAN_BITS.values())


@pytest.mark.parametrize("case", CASES, ids=["%s_%s" % c for c in CASES])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_sequences_four_ways_and_the_oracle(variant, case, children, oracle):
    got = children(variant)
    name, m = case
    ref = pd.key_of(name, m, "off")
    for way in ("lean", "full", "each"):
        for p in PLANES:
            a, b = got[pd.key_of(name, m, way) + p], got[ref + p]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s on map %s: %s differs between '%s' and EMAP_POST_DEFER=0" % (name, m, p, way)
    want = oracle(case)
    for way in pl.WAYS:
        vc.assert_case_planes(got, pd.key_of(name, m, way), want[0], want[1], want[2], "%s %s on map %s, way '%s'" % (variant, name, m, way))
    bits = {way: [int(b) & 48 for b in got[pd.key_of(name, m, way) + "_bits"]] for way in pl.WAYS}
    fused = {way: int(got[pd.key_of(name, m, way) + "_fused"][0]) for way in pl.WAYS}
    print("%s %s map %s: bits %r, fused launches %r, paths %s" % (variant, name, m, bits, fused, got[pd.key_of(name, m, "lean") + "_paths"]))
    expect = pl.LEAN_BITS[name]
    assert bits["lean"] == expect, bits                                        # lean where expected, owed without a launch where expected
    for way in ("full", "off", "each"):
        assert bits[way] == [0] * len(expect), (way, bits)                     # never with EMAP_POST_LEAN=0, never without a pending pass
    for f in pl.RAY_FRAMES.get(name, []):
        assert all(bits[way][f] & 32 == 0 for way in pl.WAYS), bits            # a visibility pass reads the normals: the pass is never skipped
    # the counter of fused launches: lean launches count, a pass left owed without a launch does not; EMAP_POST_LEAN=0 launches both kinds in full
    assert fused["lean"] == sum(b == 16 for b in expect), fused
    assert fused["full"] == sum(b != 0 for b in expect), fused
    assert fused["off"] == 0 and fused["each"] == 0, fused
    # the low bits still say which kernels ran: the decoders of the package mask them
    low = [int(b) & 3 for b in got[pd.key_of(name, m, "lean") + "_bits"]]
    assert low == [{"atomic": 0, "binned": 1, "small_frame": 2}[p] for p in str(got[pd.key_of(name, m, "lean") + "_paths"]).split(",")], low
