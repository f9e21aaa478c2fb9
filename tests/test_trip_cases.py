"""CPU: the case table of tests/test_hip_trip_edges.py says what it claims (tests/_trip_cases.py) -- the clouds put exactly the listed
numbers of records into the sort tiles by the oracle's own index arithmetic, every count at an edge of the record batches occurs, the
clouds carry rows that are no records, and the stencil radii give the walk lengths their comment states."""
import numpy as np
import pytest

import _trip_cases as tc
from oracle import emap_oracle as eo


@pytest.fixture(scope="module")
def orc():
    return eo.OracleMap(eo.make_params(eo.YAML, cell_n=tc.C, mode="reference_fp16", weights=None))


@pytest.mark.parametrize("name", ["light", "heavy"])
def test_every_frame_holds_the_listed_records_per_tile(name, orc):
    R, t = tc.pose()
    want = tc.layout(name)
    assert len(want) == tc.TILES_Y * tc.TILES_X == 27
    for f in range(tc.FRAMES):
        for sem in (False, True):
            p = tc.occupancy_cloud(name, f, sem)
            assert p.dtype == np.float32 and p.shape[1] == (7 if sem else 3)
            assert tc.records_per_tile(orc, p, R, t) == want, (name, f, sem)
            assert len(p) == sum(want.values()) + tc.N_NAN + tc.N_OUTSIDE + tc.N_BORDER
            assert int(np.isnan(p[:, :3]).any(axis=1).sum()) == tc.N_NAN
        q = tc.occupancy_cloud(name, f)
        assert np.array_equal(q.view(np.uint32), tc.occupancy_cloud(name, f, True)[:, :3].view(np.uint32)), "the channel cloud has the same points"
    a, b = tc.occupancy_cloud(name, 0), tc.occupancy_cloud(name, 1)
    assert not np.array_equal(a, b)


def test_the_edge_counts_occur_and_only_the_heavy_layout_has_a_heavy_tile():
    assert set(tc.EDGE_COUNTS) <= set(tc.LIGHT.values()) and max(tc.LIGHT.values()) == 4096
    assert sorted(tc.HEAVY.values())[-2:] == [4096, 4097]
    assert {k: v for k, v in tc.HEAVY.items() if v != tc.LIGHT[k]} == {(6, 0): 4097}


def test_several_points_share_a_cell_and_tiles_are_spread_over_the_cloud():
    R, t = tc.pose()
    p = tc.occupancy_cloud("light", 0)
    o = eo.OracleMap(eo.make_params(eo.YAML, cell_n=tc.C, mode="reference_fp16", weights=None))
    idx, valid, inside = o.point_index(p, R, t)
    ok = (valid != 0) & (inside != 0)
    assert np.bincount(idx[ok]).max() >= 4
    tile = (idx // tc.C) // 16 * tc.TILES_X + (idx % tc.C) // 64
    rows_of_3_0 = np.flatnonzero(ok & (tile == 3 * tc.TILES_X))
    assert rows_of_3_0.min() < 4096 < rows_of_3_0.max(), "the 4096-record tile draws on more than one chunk of the cloud"


def test_scatter_sizes_straddle_the_batches_of_a_chunk():
    # 512 threads x batches of 4 = 2048 points per turn, 4096 per chunk
    assert tc.SCATTER_NS == (1, 2, 511, 512, 513, 2047, 2048, 2049, 6145)
    assert len(tc.SCATTER) == 18 and sum(c["sem"] for c in tc.SCATTER) == 9
    for c in tc.SCATTER:
        p = tc.scatter_cloud(c["N"], 0, c["sem"])
        assert p.shape == (c["N"], 7 if c["sem"] else 3)


def test_stencil_radii_give_one_and_two_pairs_per_thread():
    pairs = {d: (16 + 6 + 2 * d) * (6 + 2 * d) for _, d in tc.POST_CASES}
    assert pairs == {5: 512, 6: 612}
    assert [-(-n // 512) for n in pairs.values()] == [1, 2]


def test_stencil_radii_give_one_row_turn_and_one_row_more():
    rows = {R: [R + 6 + 2 * d for _, d in tc.POST_CASES] for R in (16, 32)}
    assert rows == {16: [32, 34], 32: [48, 50]}
    assert tc.POST_ROWS_PER_TURN == {16: 32, 32: 48}
    for R in (16, 32):                   # exactly one turn, and one row / two rows into the second
        assert [divmod(n, tc.POST_ROWS_PER_TURN[R]) for n in rows[R]] == [(1, 0), (1, 2)]
    assert [k for k, v in tc.POST_CHILDREN.items() if v["kernels"][1] == "k_post<32"] == ["r32_rows"]
