"""CPU: the submap service's host side without a device -- submap_geometry against hand values (tests/_submap_cases.py: requests whose
corners lie strictly inside cells), every ValueError, the packed layout of emap_publish_grid_windows in both orders against a
per-element loop, and the window tables the GPU tests (tests/test_hip_submap.py) run."""
import numpy as np
import pytest

import _grid_cases as gc
import _submap_cases as sc
from elevation_mapping_cupy_amd.elevation_mapping import pack_windows, submap_geometry


def _same(got, want):
    if want is None:
        return got is None
    if got is None:
        return False
    return tuple(got[:4]) == tuple(want[:4]) and tuple(got[6]) == tuple(want[6]) and \
        np.allclose(got[4], want[4], rtol=0, atol=1e-12) and np.allclose(got[5], want[5], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", sorted(sc.GEOMETRY))
def test_the_geometry_gives_the_hand_values(name):
    position, length, want = sc.GEOMETRY[name]
    got = submap_geometry(position_xy=position, length_xy=length, **sc.GEO_MAP)
    assert _same(got, want), (name, got, want)
    if got is not None:
        i0, j0, ni, nj, sub_pos, sub_len, inside = got
        assert all(isinstance(v, int) for v in (i0, j0, ni, nj) + tuple(inside))
        assert 0 <= i0 and 0 <= j0 and i0 + ni <= sc.GEO_MAP["M"] and j0 + nj <= sc.GEO_MAP["M"]
        assert 0 <= inside[0] < ni and 0 <= inside[1] < nj


def test_the_hand_cases_are_the_ones_asked_for():
    g = {k: v[2] for k, v in sc.GEOMETRY.items()}
    assert g["interior, ni != nj"][2] != g["interior, ni != nj"][3]
    assert g["clipped by one edge"][0] == 0 and g["clipped by one edge"][1] > 0
    assert g["clipped by a corner"][0] + g["clipped by a corner"][2] == 10 and g["clipped by a corner"][1] + g["clipped by a corner"][3] == 10
    assert g["clipped by all four edges"][:4] == (0, 0, 10, 10) and sc.GEOMETRY["clipped by all four edges"][1] == (50.0, 50.0)      # 10 x the map
    assert g["centre outside the map"] is None
    res, top = sc.GEO_MAP["resolution"], (3.5, 0.5)
    for name, (p, ln, _) in sc.GEOMETRY.items():                               # every corner lies strictly inside a cell: 0.05 m or more from an edge
        for a in (0, 1):
            for corner in (p[a] + ln[a] / 2, p[a] - ln[a] / 2, p[a]):
                f = ((top[a] - corner) / res) % 1.0
                assert 0.09 < f < 0.91, (name, a, corner)


@pytest.mark.parametrize("name", sorted(sc.BAD_REQUESTS))
def test_every_bad_request_raises(name):
    kw = dict(sc.GEO_MAP, **sc.BAD_REQUESTS[name])
    with pytest.raises(ValueError):
        submap_geometry(**kw)


@pytest.mark.parametrize("name", sorted(sc.EDGE_RECORD))
def test_what_the_statement_gives_on_cell_edges_is_recorded(name):
    """a record of this restatement's double arithmetic, not of grid_map's: corners ON cell edges"""
    position, length, want = sc.EDGE_RECORD[name]
    got = submap_geometry(position_xy=position, length_xy=length, **sc.EDGE_MAP)
    assert _same(got, want), (name, got, want)


@pytest.mark.parametrize("order", gc.ORDERS)
def test_the_packed_layout_at_m_5(order):
    M, L = 5, 3
    full = np.arange(L * M * M, dtype=np.float32).reshape(L, M, M) + 0.5
    windows = [(0, 0, 5, 5), (1, 2, 3, 2), (4, 0, 1, 5), (0, 4, 5, 1), (2, 2, 1, 1), (1, 2, 3, 2)]
    want = sc.pack_loop(full, windows, order)
    got = sc.pack_slices(full, windows, order)
    assert got.shape == want.shape == (sc.packed_size(windows, L),) and (got == want).all()
    offsets, total = pack_windows(windows, L)
    assert total == want.size and offsets == [0, 75, 93, 108, 123, 126]
    for o, (i0, j0, ni, nj) in zip(offsets, windows):                           # a window's planes: shape (L, ni, nj) or (L, nj, ni)
        planes = want[o:o + L * ni * nj].reshape((L, ni, nj) if order == "rows" else (L, nj, ni))
        s = full[:, i0:i0 + ni, j0:j0 + nj]
        assert (planes == (s if order == "rows" else s.transpose(0, 2, 1))).all()
    if order == "message":
        assert not (got == sc.pack_slices(full, windows, "rows")).all()


@pytest.mark.parametrize("C", gc.SIZES)
def test_the_window_tables_of_the_gpu_tests(C):
    M = C - 2
    sets = sc.window_sets(M)
    for name, ws in sets.items():
        for i0, j0, ni, nj in ws:
            assert ni >= 1 and nj >= 1 and i0 >= 0 and j0 >= 0 and i0 + ni <= M and j0 + nj <= M, (name, (i0, j0, ni, nj))
    count = np.zeros((M, M), np.int32)
    for i0, j0, ni, nj in sets["partition"]:
        count[i0:i0 + ni, j0:j0 + nj] += 1
    assert (count == 1).all() and len(sets["partition"]) == 9                  # every published cell exactly once
    assert len({(ni, nj) for _, _, ni, nj in sets["partition"]}) >= 6          # unequal blocks
    assert len(sets["sixty-four"]) == 64 and len(sc.all_windows(M)) <= 64
    assert sets["overlapping and repeated"][0] == sets["overlapping and repeated"][2]
    assert ("5 x 37 and 37 x 5" in sets) == (M >= 65) and ("astride a tile edge" in sets) == (M >= 34)
    if M >= 34:
        i0, _, ni, _ = sets["astride a tile edge"][0]
        assert i0 == 31 and ni == 3
