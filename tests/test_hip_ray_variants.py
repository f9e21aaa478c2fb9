"""GPU: every variant of the visibility pass the ray launcher can select on a whole-map context (emap_kernels.hip: launch_rays_t,
launch_rays_i, ray_lds_window), against the oracle BIT FOR BIT on SMALL maps (tests/_ray_variants.py: sensor in the middle, on a
128-column piece boundary of the bitmap, in two corners and outside the map, a map width that is no multiple of 64, maps on which the
reach window is refused, both index modes, clouds of exactly 131 071 and 131 072 points, a moved map).

The launcher chooses the workgroup shape from the cloud size, the bitmap's place (LDS / global memory) from EMAP_RAY_LMAP or -- unhooked
-- from a host-mapped word k_ray_apply writes asynchronously, the part of the bitmap an LDS launch stages from the sensor pose
(EMAP_RAY_WINDOW=0: all of it), and the index method from a host proof (EMAP_RAY_IDX=1: the table).  The hooks are read once per
process, so every variant is one child process (tests/_ray_variants.py as a program), started once, one after another, each under its
own time limit and under `rocprofv3 --kernel-trace` -- the trace is what proves which instantiation the values are credited to, and its
lds_size column what proves that a window was applied (a hook that silently fell back, or a window that was never used, would pass
every value test).

Template arguments of k_rays: <MODE, STATS, IDX, STRIP, BLOCK, LMAP, LPR>.  The twelve instantiations these cases can reach are
k_rays<0, S, 2|1, false, 512, true|false, 1> (S = false | true), k_rays<1, false, 0, false, 512, true|false, 1> and
k_rays<0, false, 2|1, false, 256, false, 4>.  k_rays<0, ., 0, ...> (reference_fp16 with the defining arithmetic) is compiled but
unreachable on affordable maps: it needs a half -> index table that cannot be built or does not fit, i.e. more than 65 535 cells per side.
STRIP = true (row strips, by-ray windows) is the subject of the strip tests.  The expectation below is a decision table derived by hand and
kept as literals on purpose: it is not recomputed from a copy of the launcher's arithmetic."""
import os

import numpy as np
import pytest

import _ray_variants as rv
import _variant_children as vc
from _util import kernel_trace_rows

pytestmark = pytest.mark.gpu

VARIANTS = {
    "default": {},
    "lds_window": {"EMAP_RAY_LMAP": "1"},
    "lds_whole": {"EMAP_RAY_LMAP": "1", "EMAP_RAY_WINDOW": "0"},
    "global": {"EMAP_RAY_LMAP": "0"},
    "table_lds": {"EMAP_RAY_IDX": "1", "EMAP_RAY_LMAP": "1"},
    "table_global": {"EMAP_RAY_IDX": "1", "EMAP_RAY_LMAP": "0"},
}
HOOKS = ("EMAP_RAY_LMAP", "EMAP_RAY_WINDOW", "EMAP_RAY_IDX")
CHILD_TIMEOUT_S = 300      # per child: 17 contexts of at most 384^2 cells, two frames each, take seconds; the rest is start-up under the tracer
RAY_BLOCK = 512            # the launcher's workgroup size for clouds of 131 072 points and more, as a literal

# variant -> the bitmap's place in the large-cloud kernels: True = LDS, False = global memory, None = either (unhooked, the choice
# follows a word the previous frame's k_ray_apply writes asynchronously)
LMAP = {"default": None, "lds_window": True, "lds_whole": True, "global": False, "table_lds": True, "table_global": False}
# variant -> index method per case, in the order of rv.CASES: centre384 rot384 piece_lo piece_lo-1 two_pieces corner_a corner_b outside
# narrow200 rows_only200 refused300 whole128 | fp32_corner fp32_centre | n131072 n131071 stats384.  2 = the float formula (the host
# proved it exact on every one of these reference_fp16 maps), 1 = the half -> index table (forced), 0 = the defining arithmetic (fp32).
IDX = {
    "default":      (2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0, 0, 2, 2, 2),
    "lds_window":   (2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0, 0, 2, 2, 2),
    "lds_whole":    (2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0, 0, 2, 2, 2),
    "global":       (2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0, 0, 2, 2, 2),
    "table_lds":    (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1),
    "table_global": (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1),
}


def name_of(mode, stats, idx, strip, block, lmap, lpr):
    b = ("false", "true")
    return "k_rays<%d, %s, %d, %s, %d, %s, %d>" % (mode, b[stats], idx, b[strip], block, b[lmap], lpr)


def expected_names(variant, key):
    """the legal dispatch names of one frame of one case: one name, or two where the bitmap's place is not determined"""
    case = rv.case_of(key)
    mode = {"reference_fp16": 0, "fp32": 1}[case["mode"]]
    stats, idx = bool(case.get("stats")), IDX[variant][rv.KEYS.index(key)]
    if key == rv.SMALL_CLOUD_KEY:
        return {name_of(mode, stats, idx, False, 256, False, 4)}
    places = (True, False) if LMAP[variant] is None else (LMAP[variant],)
    return {name_of(mode, stats, idx, False, RAY_BLOCK, p, 1) for p in places}


def reachable_instantiations():
    return {n for v in VARIANTS for k in rv.KEYS for n in expected_names(v, k)}


def _run_child(variant, tmp):
    arrays, trace = vc.run_child(os.path.abspath(rv.__file__), variant, VARIANTS[variant], HOOKS, tmp, CHILD_TIMEOUT_S)
    rows = [(c, l) for c, l in ((vc.canonical_kernel_name(n, {"k_rays": "ibibibi"}), l) for n, l in kernel_trace_rows(trace)) if c]
    return arrays, rows


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """variant -> (recorded arrays, [(k_rays dispatch name, lds_size)] in start order): one child per variant, started the first time a
    test needs it, never twice; after a child that ended badly none is started (tests/_variant_children.py)"""
    return vc.lazy_children(lambda v: _run_child(v, str(tmp_path_factory.mktemp("rays_" + v))))


@pytest.fixture(scope="module")
def oracle(weights):
    """case key -> (elevation_map, normal_map, traversability_input, visits per frame) of the oracle, computed once"""
    return vc.cached_oracle(lambda key: rv.oracle_run(rv.case_of(key), weights))


@pytest.mark.parametrize("key", rv.KEYS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_values_equal_the_oracle(variant, key, children, oracle):
    got, _ = children(variant)
    want = oracle(key)
    what = "%s %s" % (variant, key)
    vc.assert_case_planes(got, key, want[0], want[1], want[2], what)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_visit_count_equals_the_oracle(variant, children, oracle):
    """ray_visits (the figure bench.py divides by for visits / s) counts what the oracle counts: samples that enter a new cell which is
    not a border cell (custom_kernels.py:209-211).  Both counting sites state that; here the numbers are compared, frame by frame."""
    got, _ = children(variant)
    for key in [c["key"] for c in rv.CASES if c.get("stats")]:
        want = oracle(key)[3]
        have = [int(v) for v in got[key + "_ray_visits"]]
        print("%s %s: ray_visits per frame %r, oracle %r" % (variant, key, have, want))
        assert have == want, "%s %s: ray_visits per frame %r, oracle %r" % (variant, key, have, want)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_hooks_selected_the_expected_kernels(variant, children):
    """two k_rays dispatches per case (one per frame), in case order"""
    _, rows = children(variant)
    names = [n for n, _ in rows]
    print("variant %s: k_rays dispatches: %s" % (variant, sorted(set(names))))
    assert len(names) == 2 * len(rv.KEYS), "variant %s: %d k_rays dispatches instead of two per case: %r" % (variant, len(names), names)
    wrong = {}
    for i, key in enumerate(rv.KEYS):
        legal = expected_names(variant, key)
        traced = names[2 * i:2 * i + 2]
        if not all(n in legal for n in traced):
            wrong[key] = (traced, sorted(legal))
    assert not wrong, "variant %s: (traced, legal) dispatches differ: %r" % (variant, wrong)


@pytest.mark.parametrize("key", [k for k in rv.KEYS if k != rv.SMALL_CLOUD_KEY])
def test_the_reach_window_was_applied(key, children):
    """lds_size of the same dispatch in three children, relative comparisons only: where the case has a window the windowed launch needs
    strictly less LDS than the whole-bitmap launch, where the window is refused they need the same, and the global-memory launch needs
    less than both"""
    i = rv.KEYS.index(key)
    lds = {v: [l for _, l in children(v)[1][2 * i:2 * i + 2]] for v in ("lds_window", "lds_whole", "global")}
    print("%s: lds_size per frame %r" % (key, lds))
    for f in range(2):
        win, whole, glob_ = lds["lds_window"][f], lds["lds_whole"][f], lds["global"][f]
        if rv.case_of(key)["window"] is not None:
            assert win < whole, (key, f, lds)
        else:
            assert win == whole, (key, f, lds)
        assert glob_ < win and glob_ < whole, (key, f, lds)
