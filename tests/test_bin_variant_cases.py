"""CPU: the inputs of tests/test_hip_bin_variants.py really reach what that file is about -- checked with numpy and the oracle alone, so
that the GPU tests cannot pass vacuously.  Records per sort bin are counted as bin_of() (emap_binned.hip) defines them, from the
oracle's point_index (tests/_bin_variants.py: records_per_bin); a bin is heavy above 4096 records and then wants ceil(n / 4096) - 1
extra parts, at most 127.  Measured here (frame by frame): heavy202 four heavy tiles wanting 3 + 3 + 8 + 8, then 2 + 3 + 8 + 8;
heavy400_stack2 four heavy bins wanting 1, 2-3, 11 and 14; slots1100 and sem_slots1100 17 heavy bins of 36 (5116 ... 5609 records);
parts_clamp 689 324 and 715 159 records in one tile; sem_stack4 five heavy bins, one extra part each; the block-count cases 12 to 14
heavy tiles of 16."""
import numpy as np
import pytest

import _bin_variants as bv
from oracle import emap_oracle as eo

SPLIT_MAX_SLOTS = 1024            # emap_device.h, as literals
SEM_SPLIT_SLOTS = 128             # emap_launch.h


@pytest.fixture(scope="module")
def records():
    done = {}

    def get(key):
        if key not in done:
            eo.set_threads(8)
            try:
                done[key] = bv.records_per_bin(bv.case_of(key))
            finally:
                eo.set_threads(1)
            print("%s: largest bin per frame %r, wanted extra parts per frame %r" % (
                key, [int(n.max()) for n in done[key]], [sorted(int(x) for x in bv.wanted_parts(n) if x) for n in done[key]]))
        return done[key]

    return get


@pytest.mark.parametrize("key", ["uniform202", "uniform202_rays", "fp32_202"])
def test_uniform_cases_have_no_heavy_bin(key, records):
    for n in records(key):
        assert int(n.max()) <= bv.SPLIT_CAP and int(n.sum()) > 10000, (key, int(n.max()))


@pytest.mark.parametrize("key", ["heavy202", "heavy202_rays", "staged_heavy", "gate_shut"])
def test_heavy202_wants_more_than_a_cap_of_8_and_less_than_128(key, records):
    for n in records(key):
        want = bv.wanted_parts(n)
        assert 8 < int(want.sum()) <= 128 and int((want > 0).sum()) >= 2, (key, want[want > 0])


def test_heavy400_has_one_bin_that_wants_more_than_a_cap_of_8_holds(records):
    assert bv.case_of("heavy400_stack2")["stack"] == 2
    for n in records("heavy400_stack2"):
        want = bv.wanted_parts(n)
        assert int(want.max()) > 8 and int((want > 0).sum()) >= 2 and int(want.sum()) <= 128, want[want > 0]


@pytest.mark.parametrize("key", ["slots1100", "sem_slots1100"])
def test_slot_cases_have_more_heavy_bins_than_slots(key, records):
    case = bv.case_of(key)
    sub = case["stack"]
    assert sub == 64
    for n in records(key):
        heavy = int((n > bv.SPLIT_CAP).sum())
        assert heavy > SPLIT_MAX_SLOTS // sub == 16, (key, heavy)                # the 17th finds no slot
        assert heavy * 1 <= 128 and int(bv.wanted_parts(n).sum()) > 8            # ... and a cap of 8 is short, one of 128 ample
        if key == "sem_slots1100":
            assert (heavy - 1) * sub >= SEM_SPLIT_SLOTS                           # at least one heavy bin's slot lies at or beyond the semantic scratch


def test_parts_clamp_holds_more_than_128_parts_in_one_tile(records):
    case = bv.case_of("parts_clamp")
    assert case["stack"] == 0
    for n in records("parts_clamp"):
        assert int(n.max()) > 128 * bv.SPLIT_CAP == 524288 and int((n > 0).sum()) == 1, (int(n.max()), int((n > 0).sum()))
        assert int(bv.wanted_parts(n).max()) == 127
    R, t, clouds = bv.case_inputs(case)
    for p in clouds:                  # beyond min_valid_distance (0.5 m) of the sensor whatever the height: the squeezed points stay valid
        assert float(np.hypot(p[:, 0], p[:, 1]).min()) > 0.7


@pytest.mark.parametrize("key", ["sem_stack4", "sem_stack4_rays"])
def test_semantic_stack_case_has_a_heavy_bin_in_every_frame(key, records):
    for n in records(key):
        assert int((n > bv.SPLIT_CAP).sum()) >= 1 and int(bv.wanted_parts(n).sum()) <= 8, n[n > bv.SPLIT_CAP]


def test_heavy_from_column_is_what_the_oracle_counts(records):
    for case in bv.CASES:
        if case["kind"] == "strip":
            continue
        first = next((f for f, n in enumerate(records(case["key"])) if int(n.max()) > bv.SPLIT_CAP), None)
        assert first == case["heavy_from"], (case["key"], first)


@pytest.mark.parametrize("key", [k for k in bv.KEYS if bv.case_of(k)["kind"] == "strip"])
def test_every_rank_owns_points_in_every_chunk(key):
    """... of 4096 points (strip kernels: 7 / 13 chunks) and of 2048 (plain kernels on the strip context: 14 / 25), and no bin of a
    strip is heavy"""
    import test_hip_bin_variants as tv
    from elevation_mapping_cupy_amd.sharded import strip_rows
    case = bv.case_of(key)
    C, N = case["C"], case["N"]
    orc = eo.OracleMap(bv.oracle_params(case, None))
    R, t, clouds = bv.case_inputs(case)
    for p in clouds:
        idx, valid, inside = orc.point_index(p, R, t)
        ok = (valid != 0) & (inside != 0)
        row = idx.astype(np.int64) // C
        for rank in range(bv.WORLD):
            r0, r1 = strip_rows(C, bv.WORLD, rank)
            own = ok & (row >= r0) & (row < r1)
            for variant, chunk in (("default", 4096), ("plain", 2048)):
                chunks = tv.STRIP_HIST_WGS[variant][N]
                assert (chunks - 1) * chunk < N <= chunks * chunk
                per = np.add.reduceat(own.astype(np.int64), np.arange(0, N, chunk))
                assert len(per) == chunks and int(per.min()) >= 1, (key, rank, variant, per)
            col = (idx.astype(np.int64) % C)[own]
            bins = np.bincount((row[own] - r0) // 16 * ((C + 63) // 64) + col // 64)
            assert int(bins.max()) <= bv.SPLIT_CAP


def test_block_count_cases_sit_on_the_slab_boundaries():
    import test_hip_bin_variants as tv
    assert [bv.case_of("blocks%d" % n)["N"] for n in bv.BLOCK_NS] == [262144, 262145, 300000, 524289]
    assert all(bv.case_of("blocks%d" % n)["C"] == 128 and not bv.case_of("blocks%d" % n)["rays"] for n in bv.BLOCK_NS)
    slabs = lambda b: (b + 255) // 256      # noqa: E731  (k_bin_scan: slabs of 256 matrix rows)
    assert [slabs(tv.HIST_WGS["chunk256"][n]) for n in bv.BLOCK_NS] == [1, 2, 2, 3]
    assert [tv.HIST_WGS["chunk256"][n] % 8 for n in bv.BLOCK_NS] == [0, 1, 5, 1]          # B = 8 q + r of bin_chunk_of_block
    assert [slabs(tv.HIST_WGS["default"][n]) for n in bv.BLOCK_NS] == [1, 1, 1, 1]
    for v in tv.HIST_WGS:
        for n, b in tv.HIST_WGS[v].items():
            assert (b - 1) * 1024 < n                                                      # every workgroup has points (chunks are whole units of 1024)


def test_inputs_are_deterministic():
    for case in bv.CASES:
        a, b = bv.case_inputs(case), bv.case_inputs(case)
        assert len(a[2]) == case["frames"] in (2, 3)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[2], b[2]))
        assert all(p.shape == (case["N"], 7 if case["cloud"][0] == "semantic" else 3) and p.dtype == np.float32 for p in a[2])
        assert not np.array_equal(a[2][0], a[2][1])


def test_the_tables_name_every_hook_variant_and_case_once():
    import test_hip_bin_variants as tv
    assert len(bv.KEYS) == len(set(bv.KEYS)) == 20
    names = ["default", "split_off", "cap8", "cap128", "blocks_a", "blocks_b", "chunk256", "plain"]
    assert list(tv.VARIANTS) == names
    for table in (tv.HIST_BLOCK, tv.SCATTER_BLOCK, tv.STRIP_KERNELS, tv.CARRIES, tv.SPLIT_RULE):
        assert sorted(table) == sorted(names)
    used = sorted({h for env in tv.VARIANTS.values() for h in env})
    assert used == sorted(tv.HOOKS) and len(tv.HOOKS) == 7
    assert tv.VARIANTS["default"] == {} and len({tuple(sorted(e.items())) for e in tv.VARIANTS.values()}) == 8
    assert sorted(tv.SINGLE + tv.STRIPS) == sorted(bv.KEYS) and set(tv.SEMANTIC) == {"sem_stack4", "sem_stack4_rays", "sem_slots1100"}
    for v in names:
        for key in bv.KEYS:
            for f in range(bv.case_of(key)["frames"]):
                assert 1 <= len(tv.expected_frame(v, key, f)) <= 2


def test_the_expectation_names_every_reachable_instantiation():
    """literal list of what the launchers can select on these contexts (see the docstring of tests/test_hip_bin_variants.py for the
    compiled instantiations that are not among them)"""
    import test_hip_bin_variants as tv
    b = ("false", "true")
    want = {"k_bin_scan"}
    want |= {"k_bin_hist<%d, %d, %s>" % (m, blk, s) for m in (0, 1) for blk in (256, 512, 1024) for s in b}
    want |= {"k_bin_scatter<%d, %d, %s, false>" % (m, blk, s) for m in (0, 1) for blk in (256, 512, 1024) for s in b}
    want |= {"k_bin_scatter<0, %d, false, true>" % blk for blk in (256, 512, 1024)}
    want |= {"k_tile_count<%s, %d>" % (s, rs) for s in b for rs in (1, 2)}
    want |= {"k_tile_fuse<true, true, %s, 1, false>" % s for s in b} | {"k_tile_fuse<true, false, %s, 1, false>" % s for s in b}
    want |= {"k_tile_fuse<false, false, %s, 1, false>" % s for s in b}
    want |= {"k_tile_fuse<true, false, false, 2, true>", "k_tile_fuse<true, false, true, 2, false>"}
    want |= {"k_tile_semantic<false, 1>", "k_tile_semantic<true, 1>", "k_tile_semantic<true, 2>"}
    assert tv.reachable_instantiations() == want and len(want) == 43
    # ... each of them pinned by a frame with a single legal sequence (the frames whose cap follows the need word add none)
    assert tv.reachable_instantiations(deterministic_only=True) == want
