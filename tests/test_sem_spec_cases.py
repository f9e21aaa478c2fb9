"""CPU: the case table of tests/test_hip_semantic_specs.py (tests/_sem_specs.py) really reaches the branches it was built for -- checked
with numpy and the oracle alone, so that no case silently stops reaching its branch.  The per-group decisions of k_tile_semantic and the
host-side choices are restated once in tests/_sem_specs.py (each cites the source lines it mirrors); here the table as a whole must take
every value of every decision, in both channel-matrix layouts where the layout matters, and the clouds must give the kernels the
records those branches need (counted from the oracle's point_index)."""
import numpy as np
import pytest

import _sem_specs as ss
from oracle import emap_oracle as eo


def _decisions(case):
    """every (spec, record form) the stand-alone tile kernel can meet in the case: dicts of _sem_specs.group_decisions"""
    out = []
    if case["scatter"] != "binned":
        return out
    c0 = ss.carried_c0(case)
    if c0 < 0 or case["cloud"] == "heavy":           # (a carrying frame without heavy-tile parts fuses in k_tile_fuse: no groups)
        out += ss.group_decisions(ss.SPECS[case["spec"]], case["layout"], c0)
    if case["after"]:
        out += ss.group_decisions(ss.AFTER[case["after"]], case["layout"], c0)
    return out


def test_the_table_is_what_the_issue_lists():
    assert len(ss.KEYS) == len(set(ss.KEYS)) == 57
    for s in ss.SPECS:
        if s == "abi_frame":
            continue
        paths = {(c["scatter"], c["rays"], c["cloud"]) for c in ss.CASES if c["spec"] == s}
        assert paths >= {("atomic", False, "base"), ("binned", False, "base"), ("binned", True, "base"), ("binned", False, "heavy")}, s
    for s in ("bayes3", "six_sums"):
        assert ss.case_of(s + "_stack4")["stack"] == 4 and ss.case_of(s + "_fp32")["mode"] == "fp32"
    assert {c["layout"] for c in ss.CASES if c["spec"] == "row_end"} == {"upload", "rows", "split"}
    assert all(ss.case_of(s + "_rows")["layout"] == "rows" for s in ("spread", "six_sums"))
    for c in ss.CASES:
        assert c["C"] <= 202 and c["N"] <= 150001 and c["frames"] == 3
        assert (c["C"], c["N"]) == ((202, 150001) if c["cloud"] == "heavy" else (200, 59999))
        assert c["C"] % 16 and c["C"] % 64 and c["C"] > 3 * 64 and c["C"] > 12 * 16      # partial edge tiles, several tiles per direction
        s = ss.SPECS[c["spec"]]
        assert len(s["sums"]) <= 16 and len(s["colours"]) <= 4
        if len(s["colours"]) > 1:
            assert c["N"] % len(s["colours"]) != 0
        layers = [l for _, _, l in ss.all_sums(c)] + [l for _, l in s["colours"]]
        assert len(set(layers)) == len(layers) and 0 not in layers and max(layers) == ss.n_layers(c) - 1
    assert len(ss.SPECS["sixteen"]["sums"]) == 16 and len(ss.SPECS["colours4"]["colours"]) == 4          # the bounds of emap_sem_spec
    assert {k for _, k, _ in ss.SPECS["mixed_group"]["sums"]} == {0, 1, 2, 3} and len(ss.SPECS["mixed_group"]["sums"]) == 4
    # members of a group stand next to each other (the GPU test runs a group in one test, this file keeps one oracle run at a time)
    groups = [ss.group_of(c) for c in ss.CASES]
    assert all(groups.index(g) + groups.count(g) - 1 == len(groups) - 1 - groups[::-1].index(g) for g in set(groups))


def test_row_end_windows_fit_exactly_and_overrun_by_one_in_both_layouts():
    for layout in ("upload", "rows", "split"):
        (fit,) = ss.group_decisions(ss.SPECS["row_end"], layout, -1)
        (over,) = ss.group_decisions(ss.SPECS["row_end_over"], layout, -1)
        assert fit["fit"] == 0 and fit["wide"] and over["fit"] == 1 and not over["wide"], layout
    assert ss.chan_view("upload", 11) == ss.chan_view("split", 11) == (3, 8) and ss.chan_view("rows", 11) == (0, 11)


def test_the_table_takes_every_value_of_every_decision():
    seen = {}
    for c in ss.CASES:
        view = "rows" if c["layout"] == "rows" else "matrix"
        for d in _decisions(c):
            for k in ("ride", "inrec"):
                seen.setdefault(k, set()).add(d[k])
            if not d["inrec"]:
                seen.setdefault(("wide", view), set()).add(d["wide"])
                seen.setdefault(("fit", view), set()).add(d["fit"])
        s = ss.SPECS[c["spec"]]
        seen.setdefault("carry", set()).add(ss.carry_eligible(s, c["rays"]))
        if c["cloud"] == "heavy" or c["stack"] == 4:
            seen.setdefault("split", set()).add(ss.sem_split_possible(s))
            if ss.sem_split_possible(s) and c["scatter"] == "binned":
                seen.setdefault("split_phases", set()).add(ss.phases(s))
                if ss.phases(s) > 1:
                    seen.setdefault("split_ride", set()).add(len(s["colours"]) == 1)
            assert (c["spec"] in ss.SPLIT_KERNEL_ON_HEAVY or c["spec"] == "abi_frame") == ss.sem_split_possible(s)
    assert seen["ride"] == seen["inrec"] == seen["carry"] == seen["split"] == {False, True}
    for view in ("matrix", "rows"):
        assert seen[("wide", view)] == {False, True}, view
        assert {0, 1, None} <= seen[("fit", view)], view                # wide by exact fit, not wide by an overrun of one, not wide by span
    assert seen["split_phases"] >= {1, 2, 4} and seen["split_ride"] == {False, True}
    # the two ABI specs behind a carrying frame: one mixed group that is gathered; one group read from the record and one gathered
    a = ss.group_decisions(ss.AFTER["abi_after"], "upload", 3)
    b = ss.group_decisions(ss.AFTER["abi_after2"], "upload", 3)
    assert [(d["inrec"], d["wide"]) for d in a] == [(False, False)] and [(d["inrec"], d["wide"]) for d in b] == [(True, True), (False, False)]
    assert ss.carried_c0(ss.case_of("abi_after")) == 3


def test_expected_paths():
    assert [ss.expected_frame(ss.case_of("row_end_binned"), f) for f in range(3)] == [("binned", "in_tile_pass")] * 3
    assert [ss.expected_frame(ss.case_of("row_end_heavy"), f)[1] for f in range(3)] == ["in_tile_pass", "carried", "carried"]
    assert [ss.expected_frame(ss.case_of("abi_after_heavy"), f)[1] for f in range(3)] == ["in_tile_pass", "carried", "carried"]
    for key in ("row_end_rays", "spread_binned", "six_sums_heavy", "bayes3_stack4", "colours3_heavy"):
        assert {ss.expected_frame(ss.case_of(key), f) for f in range(3)} == {("binned", "separate")}, key
    assert ss.expected_frame(ss.case_of("sixteen_atomic"), 1) == ("atomic", "separate")
    # colour_only carries where no visibility pass runs (one column): its stand-alone colour loop runs behind the other frames
    assert ss.expected_frame(ss.case_of("colour_only_binned"), 0) == ("binned", "in_tile_pass")
    assert [ss.expected_frame(ss.case_of("colour_only_heavy"), f)[1] for f in range(3)] == ["in_tile_pass", "carried", "carried"]


@pytest.fixture(scope="module")
def oracle():
    done = {}

    def get(case):
        g = ss.group_of(case)
        if g not in done:
            eo.set_threads(8)
            try:
                done.clear()                      # one group at a time
                done[g] = ss.oracle_run(case, eo)
            finally:
                eo.set_threads(1)
        return done[g]

    return get


def _groups():
    first = {}
    for c in ss.CASES:
        first.setdefault(ss.group_of(c), c["key"])
    return list(first.values())


@pytest.mark.parametrize("key", _groups())
def test_clouds_reach_the_tiles_and_the_layers(key, oracle):
    case = ss.case_of(key)
    C, N = case["C"], case["N"]
    R, t, clouds = ss.case_inputs(case)
    assert all(p.shape == (N, ss.SPECS[case["spec"]]["ncols"]) and p.dtype == np.float32 for p in clouds)
    orc = eo.OracleMap(eo.make_params(ss.case_config(case, eo.YAML), cell_n=C, mode=case["mode"]))
    tx = (C + 63) // 64
    ks = sorted({len(ss.SPECS[case["spec"]]["colours"])} | {sum(1 for _, k, _ in ss.all_sums(case) if k == kind) for kind in (ss.CBAY, ss.BINF)})
    for f, p in enumerate(clouds):
        idx, valid, inside = orc.point_index(p, R, t)
        ok = (valid != 0) & (inside != 0)
        cell = idx[ok].astype(np.int64)
        tiles = np.bincount((cell // C) // 16 * tx + (cell % C) // 64, minlength=tx * ((C + 15) // 16))
        assert len(tiles) == 52 and 1 <= int((tiles == 0).sum()) <= 12, (key, f, int((tiles == 0).sum()))      # whole tiles without any record
        if case["cloud"] == "heavy":
            assert int(tiles.max()) > ss.SPLIT_CAP, (key, f)
            sq = ss.squeezed(N)
            for K in ks:
                if K > 1:                          # the compact decode id * K + q < N cuts through both shares of the cloud
                    lo = np.arange(N) < N // K
                    for share in (sq, ~sq):
                        assert int((ok & share & lo).sum()) > 1000 and int((ok & share & ~lo).sum()) > 1000, (key, f, K)
        else:
            assert int(tiles.max()) <= ss.SPLIT_CAP
            for stack in {c["stack"] for c in ss.CASES if ss.group_of(c) == ss.group_of(case)} - {0}:
                bins = np.bincount((cell // C) // (16 * stack) * tx + (cell % C) // 64)
                assert int(bins.max()) > ss.SPLIT_CAP, (key, f, stack)          # stacked bins of the same cloud are heavy
    ref = oracle(case)
    last, first = ref["sem"][-1], ref["sem"][0]
    written = [l for _, _, l in ss.all_sums(case)] + [l for _, l in ss.SPECS[case["spec"]]["colours"]]
    for l in written:
        assert int((last[l].view(np.uint32) != 0).sum()) >= 500, (key, l)
    assert not last[0].any()
    for _, k, l in ss.all_sums(case):
        if k == ss.CAVG:                           # the prev != 0 branch matters
            assert int((first[l] != last[l]).sum()) >= 500, (key, l)
        if k == ss.CBAY:
            assert int((ref["alpha"][-1][l] != ref["alpha"][0][l]).sum()) >= 500 and float(ref["alpha"][-1][l].max()) > 2.0
            # cells of whole empty tiles keep their prior and are renormalised all the same
            assert int(((ref["alpha"][-1][l] == ss.priors(case)[0][l]) & (ss.priors(case)[0][l] > 0)).sum()) >= 500
        if k == ss.BINF:
            assert np.array_equal(last[l], ss.priors(case)[1][l])
    if len(ss.SPECS[case["spec"]]["colours"]) > 1:    # the launch size of color_average_kernel: only the first C * C / K cells get a colour
        K = len(ss.SPECS[case["spec"]]["colours"])
        for q, (_, l) in enumerate(ss.SPECS[case["spec"]]["colours"]):
            flat = np.flatnonzero(last[l].view(np.uint32))
            assert int(flat.max()) * K + q < C * C <= (int(flat.max()) + 8 * C) * K, (key, l)


def test_inputs_are_deterministic():
    for key in ("bayes3_heavy", "colours3_binned"):
        a, b = ss.case_inputs(ss.case_of(key)), ss.case_inputs(ss.case_of(key))
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[2], b[2]))
        assert not np.array_equal(a[2][0], a[2][1])
