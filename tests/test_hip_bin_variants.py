"""GPU: every variant of the tile-binned scatter its launchers can select (emap_binned.hip: launch_bin_hist, launch_bin_scatter,
launch_tile_count, launch_bin_fuse, launch_tile_semantic; emap_api.hip: ensure_bins, count_impl, frame_sem_begin), against the oracle
BIT FOR BIT on SMALL maps (tests/_bin_variants.py: uniform clouds, clouds of 1, 2 and 3 slabs of k_bin_scan's matrix, heavy tiles that
want more parts than the launch has room for, more heavy bins than there are slots, a tile beyond the clamp of 128 parts, the staged
entry points, carried semantic channels with and without parts, row strips).

The hooks EMAP_SPLIT, EMAP_SPLIT_CAP, EMAP_BIN_STRIP, EMAP_BIN_CHUNK, EMAP_SEM_CARRY, EMAP_HIST_BLOCK and EMAP_SCATTER_BLOCK are read
once per process, so every variant is one child process (tests/_bin_variants.py as a program), started once, one after another, each
under its own time limit and under `rocprofv3 --kernel-trace`: the trace proves which instantiations the values are credited to and
how many workgroups ran (a hook that silently fell back, or extra workgroups that were never launched, would pass every value test).

Template arguments: k_bin_hist<MODE, BLK, STRIP>, k_bin_scatter<MODE, BLK, STRIP, CH>, k_tile_count<SPLIT, RS>,
k_tile_fuse<AVG, RAYS, SPLIT, RS, SEM>, k_tile_semantic<SPLIT, RS>.  The decision table below (expected_frame and the literals it
reads) is derived by hand from the launchers and kept as literals on purpose: it is not recomputed from a copy of their arithmetic.

  * MODE: 0 reference_fp16, 1 fp32.  BLK: 1024 (hist) and 512 (scatter) unless EMAP_HIST_BLOCK / EMAP_SCATTER_BLOCK say otherwise.
  * STRIP: strip contexts without a visibility pass, unless EMAP_BIN_STRIP=0.
  * CH = true, RS = 2: whole frames that declare at most four averaged / colour channel columns, no visibility pass, unless
    EMAP_SEM_CARRY=0.
  * SPLIT = the launch holds extra workgroups: k_tile_count runs in the frame (whole and sharded frames: the drift gate is open; staged count: always)
    and EMAP_SPLIT is not 0 and the cap is above zero.  EMAP_SPLIT_CAP forces the cap; unforced it is what the last finished scan of
    the context reported through a host-mapped word (+ 25 % + 8), 0 on a fresh context: frame 0 never splits, a later frame with a
    heavy tile before it may legally show either instantiation.
  * k_tile_count runs when the gate is open (staged: always).  AVG: whole frames and sharded frames (strips); false on the staged path.
  * SEM = true (last_frame_semantics() == "in_tile_pass") exactly on carrying frames without parts in the launch; a carrying frame with
    parts runs k_tile_semantic<true, 2> behind the tile kernel ("carried"); a declaring frame that does not carry runs
    k_tile_semantic<SPLIT, 1> ("separate").

Compiled but unreachable from these cases: k_bin_scatter<1, ., false, true> (no fp32 case declares channels here: the MODE and CH
branches of the kernel are independent, tests/test_hip_frame_semantics.py runs fp32 carrying frames); k_tile_fuse<true, false, false, 2,
false> and k_tile_semantic<false, 2> (32-byte records exist only in frames with a declaration, and those fuse in the tile kernel unless
the launch holds parts); k_tile_fuse<false, false, ., 2, false> (the staged count stage never carries channels)."""
import os
from collections import Counter

import numpy as np
import pytest

import _bin_variants as bv
import _variant_children as vc
from _util import assert_planes_equal, kernel_trace_grid_rows

pytestmark = pytest.mark.gpu

VARIANTS = {
    "default": {},
    "split_off": {"EMAP_SPLIT": "0"},
    "cap8": {"EMAP_SPLIT_CAP": "8"},
    "cap128": {"EMAP_SPLIT_CAP": "128"},
    "blocks_a": {"EMAP_HIST_BLOCK": "256", "EMAP_SCATTER_BLOCK": "1024"},
    "blocks_b": {"EMAP_HIST_BLOCK": "512", "EMAP_SCATTER_BLOCK": "256"},
    "chunk256": {"EMAP_BIN_CHUNK": "256"},
    "plain": {"EMAP_BIN_STRIP": "0", "EMAP_SEM_CARRY": "0"},
}
HOOKS = ("EMAP_SPLIT", "EMAP_SPLIT_CAP", "EMAP_BIN_STRIP", "EMAP_BIN_CHUNK", "EMAP_SEM_CARRY", "EMAP_HIST_BLOCK", "EMAP_SCATTER_BLOCK")
CHILD_TIMEOUT_S = 300      # per child, as the stencil and ray variant tests: GPU work is seconds, the rest is start-up under the tracer

# ---- the decision table (literals) ------------------------------------------------------------------------------------------------
HIST_BLOCK = {"default": 1024, "split_off": 1024, "cap8": 1024, "cap128": 1024, "blocks_a": 256, "blocks_b": 512, "chunk256": 1024, "plain": 1024}
SCATTER_BLOCK = {"default": 512, "split_off": 512, "cap8": 512, "cap128": 512, "blocks_a": 1024, "blocks_b": 256, "chunk256": 512, "plain": 512}
STRIP_KERNELS = {"default": True, "split_off": True, "cap8": True, "cap128": True, "blocks_a": True, "blocks_b": True, "chunk256": True, "plain": False}
CARRIES = {"default": True, "split_off": True, "cap8": True, "cap128": True, "blocks_a": True, "blocks_b": True, "chunk256": True, "plain": False}
# "on": extra workgroups in every launch of a frame whose k_tile_count runs; "off": never; "follows": the cap follows the need word
SPLIT_RULE = {"default": "follows", "split_off": "off", "cap8": "on", "cap128": "on", "blocks_a": "follows", "blocks_b": "follows", "chunk256": "follows", "plain": "follows"}
EXTRA_CAP = {"cap8": 8, "cap128": 128}

# workgroups of k_bin_hist and k_bin_scatter on the block-count cases, by hand from ensure_bins (T = 16 tiles, TB = 17):
#   EMAP_BIN_CHUNK=256: B = ceil(N / 256) = 1024, 1025, 1172, 2049 -> whole rounds of 256: 1024, 1024, 1024, 2048 -> chunk = ceil(N / B)
#   = 256, 257, 293, 257 -> whole units of 1024: 1024 -> ceil(N / 1024) = 256, 257, 293, 513: one slab of 256 matrix rows, two with one
#   row in the second, two with a partial wave row, three.
#   unhooked (2048 points per workgroup below 1 M points): B = 128, 129, 147, 257 -> 257 becomes 256 (whole rounds) -> chunk = 2048, 2033,
#   2041, 2049 -> whole units of 1024: 2048, 2048, 2048, 3072 -> ceil(N / chunk) = 128, 129, 147, 171.  (524 289 points: one point more
#   than 256 chunks of 2048 hold, so the chunk grows by a unit and 171 workgroups remain -- not 256.)
HIST_WGS = {
    "chunk256": {262144: 256, 262145: 257, 300000: 293, 524289: 513},
    "default": {262144: 128, 262145: 129, 300000: 147, 524289: 171},
}
# ... and on the strip cases (N = 27 000 and 50 000): strip kernels stage whole units of 4096 points per workgroup (7 and 13), the plain
# kernels on a strip context 2048 (14 and 25)
STRIP_HIST_WGS = {"default": {27000: 7, 50000: 13}, "plain": {27000: 14, 50000: 25}}

B = ("false", "true")


def hist_name(mode, blk, strip):
    return "k_bin_hist<%d, %d, %s>" % (mode, blk, B[strip])


def scatter_name(mode, blk, strip, ch):
    return "k_bin_scatter<%d, %d, %s, %s>" % (mode, blk, B[strip], B[ch])


def count_name(split, rs):
    return "k_tile_count<%s, %d>" % (B[split], rs)


def fuse_name(avg, rays, split, rs, sem):
    return "k_tile_fuse<%s, %s, %s, %d, %s>" % (B[avg], B[rays], B[split], rs, B[sem])


def semantic_name(split, rs):
    return "k_tile_semantic<%s, %d>" % (B[split], rs)


def expected_frame(variant, key, f):
    """the legal dispatch sequences of frame f of a case (one context): [(names in launch order, last_frame_semantics() or None)] -- one
    entry, or two where the cap follows the need word and a heavy tile came before"""
    case = bv.case_of(key)
    mode = {"reference_fp16": 0, "fp32": 1}[case["mode"]]
    kind, rule = case["kind"], SPLIT_RULE[variant]
    counts = kind == "staged" or case["noise"] > 0.01                         # k_tile_count in the frame
    if not counts or rule == "off":
        splits = (False,)
    elif rule == "on":
        splits = (True,)
    else:
        splits = (False, True) if case["heavy_from"] is not None and f > case["heavy_from"] else (False,)
    strip = kind == "strip" and STRIP_KERNELS[variant]
    ch = kind == "sem" and not case["rays"] and CARRIES[variant]
    rs = 2 if ch else 1
    out = []
    for s in splits:
        seq = [hist_name(mode, HIST_BLOCK[variant], strip), "k_bin_scan", scatter_name(mode, SCATTER_BLOCK[variant], strip, ch)]
        if counts:
            seq.append(count_name(s, rs))
        sem = ch and not s
        seq.append(fuse_name(kind != "staged", bool(case["rays"]), s, rs, sem))
        how = None
        if kind == "sem":
            how = "in_tile_pass" if sem else ("carried" if ch else "separate")
            if not sem:
                seq.append(semantic_name(s, rs))
        out.append((tuple(seq), how))
    return out


def reachable_instantiations(deterministic_only=False):
    out = set()
    for v in VARIANTS:
        for c in bv.CASES:
            for f in range(c["frames"]):
                legal = expected_frame(v, c["key"], f)
                if deterministic_only and len(legal) > 1:
                    continue
                for seq, _ in legal:
                    out.update(seq)
    return out


TYPES = {"k_bin_hist": "iib", "k_bin_scan": "", "k_bin_scatter": "iibb", "k_tile_count": "bi", "k_tile_fuse": "bbbib", "k_tile_semantic": "bi"}


def _run_child(variant, tmp):
    arrays, trace = vc.run_child(os.path.abspath(bv.__file__), variant, VARIANTS[variant], HOOKS, tmp, CHILD_TIMEOUT_S)
    rows = [(c, g // w) for c, g, w in ((vc.canonical_kernel_name(n, TYPES), g, w) for n, _, g, w in kernel_trace_grid_rows(trace)) if c]
    return arrays, _segments(variant, rows)


def _segments(variant, rows):
    """case key -> frames -> [(name, workgroups)]: the six kernels' dispatches cut at every k_bin_hist (one per frame and context; a
    strip case's 2 x frames segments are its two ranks interleaved and stay one list per case)"""
    cuts = [i for i, (n, _) in enumerate(rows) if n.startswith("k_bin_hist")] + [len(rows)]
    assert cuts[0] == 0 or not rows, "variant %s: tile kernels in front of the first k_bin_hist: %r" % (variant, rows[:cuts[0]])
    want = sum(c["frames"] * (bv.WORLD if c["kind"] == "strip" else 1) for c in bv.CASES)
    assert len(cuts) - 1 == want, "variant %s: %d k_bin_hist dispatches instead of one per frame and context (%d)" % (variant, len(cuts) - 1, want)
    out, k = {}, 0
    for c in bv.CASES:
        if c["kind"] == "strip":
            n = c["frames"] * bv.WORLD
            out[c["key"]] = [rows[cuts[k]:cuts[k + n]]]
        else:
            n = c["frames"]
            out[c["key"]] = [rows[cuts[k + f]:cuts[k + f + 1]] for f in range(n)]
        k += n
    return out


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """variant -> (recorded arrays, dispatches per case and frame): one child per variant, started the first time a test needs it, never
    twice; after a child that ended badly none is started (tests/_variant_children.py)"""
    return vc.lazy_children(lambda v: _run_child(v, str(tmp_path_factory.mktemp("bins_" + v))))


@pytest.fixture(scope="module")
def oracle(weights):
    """case key -> the oracle's arrays (bv.oracle_run), computed once, read-only"""
    return vc.cached_oracle(lambda key: bv.oracle_run(bv.case_of(key), weights))


SINGLE = [k for k in bv.KEYS if bv.case_of(k)["kind"] != "strip"]
STRIPS = [k for k in bv.KEYS if bv.case_of(k)["kind"] == "strip"]
SEMANTIC = [k for k in bv.KEYS if bv.case_of(k)["kind"] == "sem"]


@pytest.mark.parametrize("key", SINGLE)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_values_equal_the_oracle(variant, key, children, oracle):
    got, _ = children(variant)
    want = oracle(key)
    what = "%s %s" % (variant, key)
    frames = bv.case_of(key)["frames"]
    if bv.case_of(key)["kind"] != "staged":
        assert list(got[key + "_path"]) == ["binned"] * frames, (what, got[key + "_path"])
    vc.assert_case_planes(got, key, want["map"], want["normal"], want["trav_in"], what)
    assert float(got[key + "_add"][0]) == float(want["add"][0]), (what, got[key + "_add"], want["add"])


@pytest.mark.parametrize("key", STRIPS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_strips_equal_the_oracles_rows(variant, key, children, oracle):
    got, _ = children(variant)
    want = oracle(key)
    C = bv.case_of(key)["C"]
    rows = got[key + "_rows"]
    assert int(rows[:, 1].sum()) == C and len(rows) == bv.WORLD
    for r, (r0, n) in enumerate(rows):
        what = "%s %s: strip at row %d" % (variant, key, r0)
        assert_planes_equal(got["%s_r%d_map" % (key, r)], want["map"][:, r0:r0 + n], what=what)
        assert_planes_equal(got["%s_r%d_normal" % (key, r)], want["normal"][:, r0:r0 + n], names=["nx", "ny", "nz"], what=what)
        assert float(got[key + "_add"][r]) == float(want["add"][0]), (what, got[key + "_add"], want["add"])


@pytest.mark.parametrize("key", SEMANTIC)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_semantic_layers(variant, key, children, oracle):
    """bit for bit the layers of the `plain` child (16-byte records, channels gathered by point index, the stand-alone kernel): the sums
    are exact in any grouping (emap_binned.hip), so carrying, fusing in the tile kernel and sharing sums between parts change no bit;
    against the oracle with the tolerances of tests/test_hip_frame_semantics.py"""
    got, base, want = children(variant)[0][key + "_sem"], children("plain")[0][key + "_sem"], oracle(key)["sem"]
    what = "%s %s" % (variant, key)
    assert_planes_equal(got, base, names=bv.CH[3:], what=what + " against plain")
    assert np.allclose(got[:3], want[:3], atol=1e-6, rtol=1e-5), what
    assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32)), what
    assert int((got[3].view(np.uint32) != 0).sum()) > 1000 and int((got[0] != 0).sum()) > 1000, what


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_hooks_selected_the_expected_kernels(variant, children):
    got, seg = children(variant)
    wrong, seen = {}, Counter()
    for key in SINGLE:
        case = bv.case_of(key)
        for f in range(case["frames"]):
            traced = tuple(n for n, _ in seg[key][f])
            seen.update(traced)
            legal = expected_frame(variant, key, f)
            hit = [how for seq, how in legal if seq == traced]
            if not hit:
                wrong[(key, f)] = (traced, [seq for seq, _ in legal])
            elif case["kind"] == "sem" and got[key + "_sempath"][f] != hit[0]:
                wrong[(key, f)] = ("last_frame_semantics() = %s" % got[key + "_sempath"][f], hit[0])
    for key in STRIPS:                          # two ranks interleave: the multiset of names of the whole case
        case = bv.case_of(key)
        traced = Counter(n for n, _ in seg[key][0])
        seen.update(traced)
        legal = Counter()
        for f in range(case["frames"]):
            (seq, _), = expected_frame(variant, key, f)
            for n in seq:
                legal[n] += bv.WORLD
        if traced != legal:
            wrong[key] = (dict(traced), dict(legal))
    print("variant %s: dispatches: %s" % (variant, sorted(seen.items())))
    assert not wrong, "variant %s: (traced, legal) dispatches differ: %r" % (variant, wrong)


@pytest.mark.parametrize("variant", ["cap8", "cap128"])
@pytest.mark.parametrize("key", ["sem_stack4", "sem_slots1100"])
def test_carried_channels_feed_the_split_semantic_kernel(variant, key, children):
    got, seg = children(variant)
    for f in range(bv.case_of(key)["frames"]):
        names = [n for n, _ in seg[key][f]]
        assert names[-1] == "k_tile_semantic<true, 2>" and got[key + "_sempath"][f] == "carried", (variant, key, f, names, got[key + "_sempath"])


def _tile_grids(seg, key):
    """per frame: the workgroups of the frame's k_tile_count and k_tile_fuse dispatches, in launch order"""
    return [[(n.split("<")[0], g) for n, g in frame if n.startswith(("k_tile_count", "k_tile_fuse"))] for frame in seg[key]]


@pytest.mark.parametrize("key", SINGLE)
def test_forced_caps_add_exactly_their_workgroups(key, children):
    """relative comparisons only: the same dispatch of the same case has 8 x sub (128 x sub) workgroups more under EMAP_SPLIT_CAP=8
    (128) than under EMAP_SPLIT=0 -- none where the gate is host-decidably shut (no k_tile_count: nothing may be split)"""
    case = bv.case_of(key)
    sub = max(1, case["stack"])
    base = _tile_grids(children("split_off")[1], key)
    for variant in ("cap8", "cap128"):
        grids = _tile_grids(children(variant)[1], key)
        print("%s: workgroups under split_off %r, under %s %r" % (key, base, variant, grids))
        extra = 0 if key == "gate_shut" else EXTRA_CAP[variant] * sub
        want = [[(n, g + extra) for n, g in frame] for frame in base]
        assert grids == want and all(len(frame) == (1 if key == "gate_shut" else 2) for frame in base), (key, variant, grids, want)


@pytest.mark.parametrize("variant", ["chunk256", "default"])
def test_point_pass_workgroups_equal_the_literals(variant, children):
    _, seg = children(variant)
    for n in bv.BLOCK_NS:
        for f, frame in enumerate(seg["blocks%d" % n]):
            got = {name.split("<")[0]: g for name, g in frame if name.startswith(("k_bin_hist", "k_bin_scatter"))}
            print("%s: %d points, frame %d: %r" % (variant, n, f, got))
            assert got == {"k_bin_hist": HIST_WGS[variant][n], "k_bin_scatter": HIST_WGS[variant][n]}, (variant, n, f, got)


@pytest.mark.parametrize("variant", ["default", "plain"])
def test_strip_point_pass_workgroups_equal_the_literals(variant, children):
    _, seg = children(variant)
    for key in STRIPS:
        n = bv.case_of(key)["N"]
        got = sorted({g for name, g in seg[key][0] if name.startswith(("k_bin_hist", "k_bin_scatter"))})
        print("%s %s: %r" % (variant, key, got))
        assert got == [STRIP_HIST_WGS[variant][n]], (variant, key, got)


def test_the_table_reaches_every_instantiation_the_launchers_can_select(children):
    """what the eight traces showed, together, is what the table says is reachable and pinned (a single legal sequence)"""
    seen = set()
    for v in VARIANTS:
        for frames in children(v)[1].values():
            for frame in frames:
                seen.update(n for n, _ in frame)
    pinned = reachable_instantiations(deterministic_only=True)
    assert pinned <= seen <= reachable_instantiations(), (sorted(pinned - seen), sorted(seen - reachable_instantiations()))
