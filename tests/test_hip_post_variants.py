"""GPU: every tile height of the two fused stencil kernels, k_post<R, STAGE> and k_post_dma<R, STAGE> (emap_kernels.hip: launch_post),
against the oracle BIT FOR BIT on SMALL maps with adversarial states (tests/_post_variants.py: sparse and dense halves, busy edge
columns for the reference's flat-index row wrap, valid border cells, a hole no source reaches, radii 1 ... 32, a region wider than
the map, partial last tiles, the circular origin inside tiles, the boundary-band launch of emap_post_part).

Without a hook a map of at most 512^2 cells runs k_post<4, .> and nothing else.  The launcher's test hooks EMAP_POST_R, EMAP_POST_DMA
and EMAP_POST_DMA_LDS_KB are read once per process, so every variant is one child process (tests/_post_variants.py as a program),
started once, one after another, each under its own time limit and under `rocprofv3 --kernel-trace` -- the trace is what proves that the
hook selected the kernel the values are credited to (a hook that silently fell back to k_post<4> would pass every value test).

The twelve instantiations the launcher can reach are k_post<4|8|16|32, 0|1> and k_post_dma<16|32, 0|1>; k_post_dma<4|8, .> are compiled
but unreachable (post_use_dma requires R >= 16).  The expectation below is a decision table derived by hand from post_tile_rows,
post_use_dma and the LDS formulas and kept as literals on purpose: it is not recomputed from a copy of the launcher's arithmetic."""
import os
import re

import numpy as np
import pytest

import _post_variants as pv
import _variant_children as vc
from _util import kernel_trace_rows, make_pair
from oracle import emap_oracle as eo

pytestmark = pytest.mark.gpu

VARIANTS = {
    "default": {},
    "r8": {"EMAP_POST_R": "8", "EMAP_POST_DMA": "0"},
    "r16": {"EMAP_POST_R": "16", "EMAP_POST_DMA": "0"},
    "r32": {"EMAP_POST_R": "32", "EMAP_POST_DMA": "0"},
    "dma16": {"EMAP_POST_R": "16", "EMAP_POST_DMA_LDS_KB": "150"},
    "dma32": {"EMAP_POST_R": "32", "EMAP_POST_DMA_LDS_KB": "150"},
}
CHILD_TIMEOUT_S = 300      # per child: 26 contexts of at most 202^2 cells and some 60 small launches take seconds; the rest is start-up under the tracer

# variant -> dilation radius -> (kernel of the whole-map launches: dilate, post, part 1; kernel of the boundary bands: part 2).
# The bands' tile height is the smallest of 4, 8, 16, 32 that reaches d + 4 rows, used only when it is below the variant's own.
EXPECTED = {
    "default": {d: ("k_post<4", "k_post<4") for d in (1, 3, 10, 12, 13, 20, 21, 32)},
    "r8": {d: ("k_post<8", "k_post<8") for d in (1, 3, 10, 12, 13, 20, 21, 32)},
    "r16": {1: ("k_post<16", "k_post<8"), 3: ("k_post<16", "k_post<8"), 10: ("k_post<16", "k_post<16"), 12: ("k_post<16", "k_post<16"),
            13: ("k_post<16", "k_post<16"), 20: ("k_post<16", "k_post<16"), 21: ("k_post<16", "k_post<16"), 32: ("k_post<16", "k_post<16")},
    "r32": {1: ("k_post<32", "k_post<8"), 3: ("k_post<32", "k_post<8"), 10: ("k_post<32", "k_post<16"), 12: ("k_post<32", "k_post<16"),
            13: ("k_post<32", "k_post<32"), 20: ("k_post<32", "k_post<32"), 21: ("k_post<32", "k_post<32"), 32: ("k_post<16", "k_post<16")},
    "dma16": {1: ("k_post_dma<16", "k_post<8"), 3: ("k_post_dma<16", "k_post<8"), 10: ("k_post_dma<16", "k_post_dma<16"),
              12: ("k_post_dma<16", "k_post_dma<16"), 13: ("k_post_dma<16", "k_post_dma<16"), 20: ("k_post_dma<16", "k_post_dma<16"),
              21: ("k_post<16", "k_post<16"), 32: ("k_post<16", "k_post<16")},
    "dma32": {1: ("k_post_dma<32", "k_post<8"), 3: ("k_post_dma<32", "k_post<8"), 10: ("k_post_dma<32", "k_post_dma<16"),
              12: ("k_post_dma<32", "k_post_dma<16"), 13: ("k_post<32", "k_post<32"), 20: ("k_post<32", "k_post<32"),
              21: ("k_post<32", "k_post<32"), 32: ("k_post<16", "k_post<16")},
}


def expected_sequence(variant):
    """dispatch names of the child's k_post* launches in launch order, all cases: A-dilate, A-post, B-dilate, B-part 1, B-part 2"""
    seq = []
    for _, d in pv.CASES:
        full, bands = EXPECTED[variant][d]
        seq += [full + ", 1>", full + ", 0>", full + ", 1>", full + ", 0>", bands + ", 0>"]
    return seq


def reachable_instantiations():
    return {name for v in VARIANTS for name in expected_sequence(v)}


def _kernel_names(trace_dir):
    """the dispatches of a rocprofv3 kernel trace in start order"""
    return [n for n, _ in kernel_trace_rows(trace_dir)]


def _run_child(variant, tmp):
    arrays, trace = vc.run_child(os.path.abspath(pv.__file__), variant, VARIANTS[variant], lambda k: k.startswith("EMAP_POST_"), tmp, CHILD_TIMEOUT_S)
    names = [m.group(1) for m in (re.match(r"void (k_post(?:_dma)?<\d+, [01]>)", n) for n in _kernel_names(trace)) if m]
    return arrays, names


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """variant -> (recorded arrays, k_post* dispatch names): one child per variant, started the first time a test needs it, never twice;
    after a child that ended badly none is started (tests/_variant_children.py)"""
    return vc.lazy_children(lambda v: _run_child(v, str(tmp_path_factory.mktemp("post_" + v))))


def _oracle_case(key, weights):
    if key == pv.FRAME_KEY:
        _, orc = make_pair(eo.YAML, pv.FRAME["C"], "reference_fp16", weights)
        pv.run_frames(orc, False)
        dil = None
    else:
        C, d = next(c for c in pv.CASES if pv.case_key(*c) == key)
        _, orc = make_pair(dict(eo.YAML, dilation_size=d), C, "reference_fp16", weights)
        orc.elevation_map[...] = pv.state(C, d, pv.case_seed(C, d))
        orc.dilate()
        dil = orc.traversability_input.copy()
        orc.traversability(); orc.normals()
    out = tuple(None if a is None else np.array(a, np.float32) for a in (dil, orc.elevation_map, orc.normal_map, orc.traversability_input))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def oracle(weights):
    """case key -> the oracle's arrays, computed once: (stage-1 dilation, elevation_map, normal_map, traversability_input)"""
    return vc.cached_oracle(lambda key: _oracle_case(key, weights))


def _check(got, key, want, what):
    vc.assert_case_planes(got, key, want[1], want[2], want[3], what)


@pytest.mark.parametrize("case", pv.CASES, ids=[pv.case_key(*c) for c in pv.CASES])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_values_equal_the_oracle(variant, case, children, oracle):
    got, _ = children(variant)
    key = pv.case_key(*case)
    want = oracle(key)
    for ctx in ("A", "B"):
        what = "%s %s context %s" % (variant, key, ctx)
        assert np.array_equal(got["%s_%s_dilate" % (key, ctx)].view(np.uint32), want[0].view(np.uint32)), what + ": stage-1 dilation"
        _check(got, "%s_%s" % (key, ctx), want, what)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_values_of_whole_frames_equal_the_oracle(variant, children, oracle):
    """the stencil launch as emap_update issues it: two frames with rays, a move by (3, 2) cells between them"""
    got, _ = children(variant)
    _check(got, pv.FRAME_KEY, oracle(pv.FRAME_KEY), "%s frames" % variant)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_hooks_selected_the_expected_kernels(variant, children):
    _, names = children(variant)
    want = expected_sequence(variant)
    head, tail = names[:len(want)], names[len(want):]
    per_case = {pv.case_key(*c): (head[5 * i:5 * i + 5], want[5 * i:5 * i + 5]) for i, c in enumerate(pv.CASES)}
    wrong = {k: v for k, v in per_case.items() if v[0] != v[1]}
    print("variant %s: k_post* dispatches: %s" % (variant, sorted(set(names))))
    assert not wrong, "variant %s: (traced, expected) dispatches of dilate, post, dilate, part 1, part 2 differ: %r" % (variant, wrong)
    assert EXPECTED[variant][3][0] + ", 0>" in tail, "variant %s: the frames' stencil launches were %r" % (variant, tail)
