"""The pending stencil pass taken along with POST_OUT_TRAV: the drift gate gets a flag byte per cell, not the traversability word.

Without a visibility pass the pass a frame takes along in its histogram launch (k_post_hist<MODE, 16 | 32, 2>) has one reader: the test
traversability > traversability_inlier of the drift statistics (k_tile_count).  It writes that predicate as one byte per cell into a flag
plane, "use the word you hold" for the 3-cell border it does not decide, and no word into the hot half; the frame's k_tile_count is the
form that reads the plane (k_tile_count_flags<SPLIT, RS>).  The word stays stale until the next full pass (emap_api.hip: count_impl).

One child process per tile height, and one with extra workgroups in every tile launch (EMAP_SPLIT_CAP=8: the SPLIT instantiations),
plays the sequences of tests/_post_flags.py five ways -- default, EMAP_POST_FLAGS=0, EMAP_POST_LEAN=0, EMAP_POST_DEFER=0, and with the
traversability plane read after every step -- on 202^2 and 130^2 maps (partial tiles; C no multiple of 64), both index modes, the gate
open in every frame, under `rocprofv3 --kernel-trace`: runs of lean frames with nothing read in between, a shifted map (origin (5, 37):
37 % 64 != 0), a heavy tile, frames with 32-byte records, traversability_inlier changed between lean frames, and border cells with
traversability on both sides of the threshold.  The seven map planes, the normals, traversability_input, additive_mean_error and, for
the frames that ask for statistics, err_sum and err_cnt are compared bit for bit among the five ways and with the oracle; bits 16 / 32
of emap_last_update_path are asserted for every frame of every way, the counter of fused launches once per sequence (reading it
launches an owed pass, so it cannot be read between the frames of a lean run: the per-frame bits say which frames fused), and the trace
says which instantiations ran how often.

A comparison in which the traversability test decides nothing would pass with any flag plane.  So the parent plays every sequence on
the ORACLE first, takes traversability_inlier from the oracle's traversability plane and asserts, before a child is started: in every
lean frame, of the cells that receive a point which passes the other three inlier conditions, at least 20 % lie on each side of the
threshold, and the frame's err_cnt differs from the count with every cell passing and from the count with none passing."""
import json
import os

import numpy as np
import pytest

import _post_deferred as pd
import _post_flags as pf
import _variant_children as vc
from _util import assert_planes_equal, kernel_trace_grid_rows

R16 = {"EMAP_POST_R": "16", "EMAP_POST_DMA": "0"}
VARIANTS = {"r16": R16, "r32": {"EMAP_POST_R": "32", "EMAP_POST_DMA": "0"}, "r16_cap8": dict(R16, EMAP_SPLIT_CAP="8")}
ALL_CASES = [(name, m) for name, (maps, _) in pf.SEQUENCES.items() for m in maps]
CASES = {"r16": ALL_CASES, "r32": ALL_CASES, "r16_cap8": [c for c in ALL_CASES if c[0] in ("heavy", "rs2")]}
PAIRS = [(v, c) for v in VARIANTS for c in CASES[v]]
CHILD_TIMEOUT_S = 300      # at most 120 contexts of at most 202^2 cells with four to six frames of 30 000 points: seconds; the rest is start-up and the tracer
HOOKS = ("EMAP_SPLIT_CAP", "EMAP_SPLIT", "EMAP_SPLIT_POOL", "EMAP_BIN_CHUNK", "EMAP_SMALL_FRAME")
TYPES = {"k_tile_count_flags": "bi", "k_tile_count": "bi", "k_post_hist": "iii"}
MIN_SIDE = 0.2             # share of the candidate cells on each side of the threshold


def _play_oracle(case, weights):
    """the sequence on the oracle: the planes, the statistics and thresholds the child is compared with / configured by, and per frame
    what the traversability test had to decide (scene)"""
    from oracle import emap_oracle as eo
    name, m = case
    C, mode = pf.MAPS[m]
    orc = eo.OracleMap(eo.make_params(pd.config({}), cell_n=C, mode=mode, weights=weights))
    R, t = pd.pose()
    pending, thr, stats, scene, border_set = 0.5, [], [], [], False
    i, j = np.meshgrid(np.arange(C), np.arange(C), indexing="ij")
    ring = (i < 3) | (i >= C - 3) | (j < 3) | (j >= C - 3)
    for s in pf.SEQUENCES[name][1]:
        if s[0] in pf.FRAME_STEPS:
            p = pf.cloud(C, s[1], s[2], s[0])
            keep = orc.P.traversability_inlier
            orc.P.traversability_inlier = -1.0                      # every cell passes (traversability = exp(-x) >= 0, the border holds 1 or the checkerboard)
            n_pts, inl_all, _, cnt_all = orc.count(p, R, t)
            orc.P.traversability_inlier = 2.0                       # none passes
            cnt_none = orc.count(p, R, t)[3]
            cand = inl_all > 0                                      # cells with a point that passes the other three conditions
            trav = orc.elevation_map[3].astype(np.float64)
            if pending is not None and cand.any():
                keep = float(np.quantile(trav[cand], pending))
                thr.append(keep); pending = None
            orc.P.traversability_inlier = keep
            above = trav > keep
            tiles = np.add.reduceat(np.add.reduceat(n_pts.astype(np.int64), np.arange(0, C, 16), axis=0), np.arange(0, C, 64), axis=1)
            scene.append(dict(cand=int(cand.sum()), above=int((cand & above).sum()), cnt_all=int(cnt_all), cnt_none=int(cnt_none),
                              ring_above=int((cand & ring & above).sum()), ring_below=int((cand & ring & ~above).sum()), border_set=border_set,
                              max_tile=int(tiles.max()), undecided=pending is not None))
            orc.update_map_with_kernel(p, R, t, 1.0, 1.0)
            scene[-1].update(err_cnt=int(orc.last["err_cnt"]), fired=bool(orc.last["gate_fired"]))
            stats.append((float(orc.last["err_sum"]), int(orc.last["err_cnt"]), bool(orc.last["gate_fired"])))
        elif s[0] == "thr":
            pending = s[1]
        elif s[0] == "border":
            orc.elevation_map[3] = pf.border_plane(orc.elevation_map[3]); border_set = True
        else:
            pd.play_oracle(orc, [s])
    out = dict(map=np.array(orc.elevation_map, np.float32), normal=np.array(orc.normal_map, np.float32), trav_in=np.array(orc.traversability_input, np.float32),
               add=float(orc.additive_mean_error), stats=stats, thr=thr, scene=scene)
    for k in ("map", "normal", "trav_in"):
        out[k].setflags(write=False)
    return out


@pytest.fixture(scope="module")
def oracle(weights):
    return vc.cached_oracle(lambda case: _play_oracle(case, weights))


def _assert_scene(case, want):
    """the condition that keeps the comparison from passing vacuously, from the oracle alone"""
    name, _ = case
    steps = pf.SEQUENCES[name][1]
    frames = [s for s in steps if s[0] in pf.FRAME_STEPS]
    n_thr = 1 + sum(s[0] == "thr" for s in steps)
    assert len(want["thr"]) == n_thr and len(set(want["thr"])) == n_thr, (case, want["thr"])
    assert all(0.0 < x < 1.0 for x in want["thr"]), (case, want["thr"])
    lean = [f for f, b in enumerate(pf.LEAN_BITS[name]) if b == 16]
    assert lean, case
    for f in lean:
        sc = want["scene"][f]
        what = "%s frame %d: %r" % (case, f, sc)
        assert not sc["undecided"] and sc["cand"] >= 500, what
        assert MIN_SIDE * sc["cand"] <= sc["above"] <= (1.0 - MIN_SIDE) * sc["cand"], what
        assert sc["err_cnt"] != sc["cnt_all"] and sc["err_cnt"] != sc["cnt_none"] and sc["err_cnt"] >= 100, what
        if sc["border_set"]:
            assert sc["ring_above"] >= 5 and sc["ring_below"] >= 5, what      # border cells on both sides, answered by the word they hold
        if frames[f][0] == "heavy":
            assert sc["max_tile"] > 4096 + 1000, what                           # a tile beyond the split threshold
    assert any(want["scene"][f]["fired"] for f in lean) and want["add"] != 0.0, case


def test_the_tables_cover_every_frame():
    """CPU-side sanity of the tables themselves (no child is started)"""
    for name, (maps, steps) in pf.SEQUENCES.items():
        assert len(pf.LEAN_BITS[name]) == sum(s[0] in pf.FRAME_STEPS for s in steps), name
        assert set(maps) <= set(pf.MAPS)
    assert {pf.MAPS[m] for _, m in ALL_CASES} == {(202, "reference_fp16"), (130, "fp32"), (130, "reference_fp16"), (202, "fp32")}
    assert sum(b.count(16) >= 3 and 0 not in b[1:] for b in pf.LEAN_BITS.values()) >= 3      # runs of lean frames with nothing in between
    for v in VARIANTS:
        assert set(CASES[v]) <= set(ALL_CASES) and CASES[v]
    a = pf.border_plane(np.full((130, 130), 0.5, np.float32))
    assert a[3:-3, 3:-3].min() == 0.5 and a[3:-3, 3:-3].max() == 0.5 and set(np.unique(a[:3])) == {np.float32(0.01), np.float32(0.99)}


@pytest.mark.parametrize("case", ALL_CASES, ids=["%s_%s" % c for c in ALL_CASES])
def test_the_scenes_give_the_traversability_test_something_to_decide(case, oracle):
    _assert_scene(case, oracle(case))


@pytest.fixture(scope="module")
def children(tmp_path_factory, oracle):
    def run(v):
        tmp = str(tmp_path_factory.mktemp("flags_" + v))
        plan = []
        for case in CASES[v]:
            want = oracle(case)
            _assert_scene(case, want)                     # before anything runs on the device
            plan.append(dict(name=case[0], map=case[1], thr0=want["thr"][0], thr=want["thr"][1:]))
        path = os.path.join(tmp, "plan.json")
        with open(path, "w") as f:
            json.dump(plan, f)
        drop = lambda k: k.startswith("EMAP_POST_") or k in HOOKS
        arrays, trace = vc.run_child(os.path.abspath(pf.__file__), v, dict(VARIANTS[v], EMAP_TEST_FLAGS_PLAN=path), drop, tmp, CHILD_TIMEOUT_S)
        names = [vc.canonical_kernel_name(n, TYPES) for n, _, _, _ in kernel_trace_grid_rows(trace)]
        return arrays, [n for n in names if n]
    return vc.lazy_children(run)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,case", PAIRS, ids=["%s-%s_%s" % (v, c[0], c[1]) for v, c in PAIRS])
def test_sequences_five_ways_and_the_oracle(variant, case, children, oracle):
    got, _ = children(variant)
    name, m = case
    want = oracle(case)
    ref = pf.key_of(name, m, "off")
    for way in pf.WAYS:
        key, what = pf.key_of(name, m, way), "%s %s on map %s, way '%s'" % (variant, name, m, way)
        for p in ("_map", "_normal", "_trav_in", "_add"):
            a, b = got[key + p], got[ref + p]
            assert a.tobytes() == b.tobytes(), "%s: %s differs from EMAP_POST_DEFER=0" % (what, p)
        sa, sb = got[key + "_stats"], got[ref + "_stats"]
        assert sa.tobytes() == sb.tobytes(), "%s: err_sum / err_cnt / gate differ from EMAP_POST_DEFER=0: %r %r" % (what, sa, sb)
        vc.assert_case_planes(got, key, want["map"], want["normal"], want["trav_in"], what)
        assert float(got[key + "_add"][0]) == want["add"], (what, got[key + "_add"], want["add"])
        steps = [s for s in pf.SEQUENCES[name][1] if s[0] in pf.FRAME_STEPS]
        for f, (s, st) in enumerate(zip(steps, want["stats"])):
            if len(s) > 3 and s[3]:
                e_sum, e_cnt, fired = got[key + "_stats"][f]
                print("%s frame %d: err_sum %r (oracle %r), err_cnt %d (oracle %d)" % (what, f, e_sum, st[0], e_cnt, st[1]))
                assert int(e_cnt) == st[1] and bool(fired) == st[2], (what, f)
                assert abs(e_sum - st[0]) <= 1e-6 * max(1.0, st[1]), (what, f)      # (the bound of tests/test_hip_parity.py: fixed-point sums against the oracle's double)
                sc = want["scene"][f]
                assert int(e_cnt) != sc["cnt_all"] and int(e_cnt) != sc["cnt_none"], (what, f, sc)
    bits = {way: [int(b) & 48 for b in got[pf.key_of(name, m, way) + "_bits"]] for way in pf.WAYS}
    fused = {way: int(got[pf.key_of(name, m, way) + "_fused"][0]) for way in pf.WAYS}
    print("%s %s map %s: bits %r, fused launches %r" % (variant, name, m, bits, fused))
    expect = pf.LEAN_BITS[name]
    for way in ("flags", "word"):
        assert bits[way] == expect, (way, bits)
        assert fused[way] == expect.count(16), (way, fused)
    for way in ("full", "off", "each"):
        assert bits[way] == [0] * len(expect), (way, bits)
    assert fused["full"] == expect.count(16) and fused["off"] == 0 and fused["each"] == 0, fused
    assert str(got[pf.key_of(name, m, "flags") + "_paths"]).split(",") == ["binned"] * len(expect)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_trace_names_the_flag_kernels(variant, children):
    """the lean frames of the default way ran k_post_hist<., ., 2> and the k_tile_count that reads the flag plane, those of EMAP_POST_FLAGS=0
    k_post_hist<., ., 3> and the k_tile_count that reads the word, as often as the tables say"""
    _, names = children(variant)
    R = int(VARIANTS[variant]["EMAP_POST_R"])
    lean = {mode: sum(pf.LEAN_BITS[n].count(16) for n, m in CASES[variant] if pf.MAPS[m][1] == mode) for mode in ("reference_fp16", "fp32")}
    seen = {n: names.count(n) for n in set(names)}
    print("variant %s: dispatches %r" % (variant, sorted(seen.items())))
    for k, mode in enumerate(("reference_fp16", "fp32")):
        for out in (0, 2, 3):                        # full (EMAP_POST_LEAN=0) | flag plane (default) | word (EMAP_POST_FLAGS=0)
            assert seen.get("k_post_hist<%d, %d, %d>" % (k, R, out), 0) == lean[mode], (mode, out, seen)
        assert not any(n.startswith("k_post_hist<%d, %d, 1>" % (k, R)) for n in seen), seen      # (no visibility pass in these sequences)
    flags = {n: c for n, c in seen.items() if n.startswith("k_tile_count_flags")}
    assert sum(flags.values()) == sum(lean.values()), flags
    rs2 = sum(1 for n, m in CASES[variant] if n == "rs2")                       # one lean frame with 32-byte records per rs2 case
    assert sum(c for n, c in flags.items() if n.endswith(", 2>")) == rs2, flags
    if variant == "r16_cap8":
        assert set(flags) == {"k_tile_count_flags<true, 1>", "k_tile_count_flags<true, 2>"}, flags
    else:
        assert {"k_tile_count_flags<false, 1>", "k_tile_count_flags<false, 2>"} <= set(flags), flags
