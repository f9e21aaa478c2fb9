"""CPU: the restatements the GPU test of the GridMap message output compares with (tests/_grid_cases.py) and the refusals of
grid_map_descriptor.  grid_map is absent offline: layout and colour are checked against per-element loops and hand values."""
import numpy as np
import pytest

import _grid_cases as gc


@pytest.mark.parametrize("M", [3, 5])
def test_the_message_layout_is_column_major(M):
    rows = np.arange(M * M, dtype=np.float32).reshape(M, M) * 1.5 - 2.0
    got = gc.message_plane(rows)
    assert got.flags["C_CONTIGUOUS"] and got.dtype == np.float32
    assert np.array_equal(got, gc.message_plane_loop(rows))
    assert not np.array_equal(got, rows)                                  # (the case can tell a missing transpose)
    flat = got.reshape(-1)
    (l0, s0, st0), (l1, s1, st1) = gc.message_layout(M)
    assert (l0, s0, st0, l1, s1, st1) == ("column_index", M, M * M, "row_index", M, M)
    for i in range(M):
        for j in range(M):
            assert flat[j * st1 + i] == rows[i, j]


def _bits(nx, ny, nz):
    return int(gc.normal_color(np.float32([nx]), np.float32([ny]), np.float32([nz])).view(np.uint32)[0])


def test_the_normal_colour_on_hand_values():
    assert _bits(0.0, 0.0, 1.0) == 0x007F7FFF
    assert _bits(1.0, -1.0, 0.0) == 0x00FF0000
    assert _bits(-1.0, 1.0, 0.5) == 0x0000FF7F                             # 127.5 truncates
    assert _bits(-1.0, -1.0, -1.0) == 0xFFFFFF01                           # b = -255: two's complement, the low 32 bits
    one_below, one_above = np.nextafter(np.float32(1.0), np.float32(0.0)), np.nextafter(np.float32(1.0), np.float32(2.0))
    assert _bits(-1.0, -1.0, one_below) == 254                              # 255 - 255 * 2^-24 rounds to 255 - 2^-16
    assert _bits(-1.0, -1.0, one_above) == 255
    assert _bits(one_below, -1.0, 0.0) == 0x00FF0000                        # (1 - 2^-24 + 1) / 2 rounds to 1 in float32


def test_the_normal_colour_around_integer_boundaries():
    """every component of the pattern the GPU test uses, by a scalar loop: the float64 product of a float32 and 255 is exact, so one
    rounding to float32 is the float32 product"""
    n = gc.normal_pattern(10)
    got = gc.normal_color(n[0], n[1], n[2]).view(np.uint32).reshape(-1)
    near = 0
    for k, (x, y, z) in enumerate(zip(*(a.reshape(-1) for a in n))):
        c = [np.float32((float(x) + 1.0) / 2.0), np.float32((float(y) + 1.0) / 2.0), z]
        scaled = [np.float32(float(v) * 255.0) for v in c]
        near += sum(abs(float(s) - round(float(s))) < 1e-4 for s in scaled)
        r, g, b = (int(s) for s in scaled)                                  # int(): toward zero
        assert got[k] == ((r << 16) | (g << 8) | b) & 0xFFFFFFFF, (k, x, y, z)
    assert near >= 40                                                       # the pattern does sit on the boundaries
    for a in range(3):
        assert all((n[a] == v).any() for v in (-1.0, 0.0, 1.0))


def test_the_descriptor():
    from elevation_mapping_cupy_amd import _lib
    from elevation_mapping_cupy_amd.elevation_mapping import GRID_BUILTIN_LAYERS, grid_map_descriptor
    assert tuple(GRID_BUILTIN_LAYERS) == gc.BUILTINS
    table, names = grid_map_descriptor(["elevation", "rgb", "normal_y"], ["s0", "rgb"], normal_color=True)
    assert names == ["elevation", "rgb", "normal_y", "normal_x", "normal_z", "color"]
    assert [(g.kind, g.index, g.slot) for g in table] == [(0, 0, 0), (1, 1, 1), (0, 7, 2), (0, 6, 3), (0, 8, 4), (2, 0, 5)]
    table, names = grid_map_descriptor(["time", "s0"], ["s0"], slots=[4, 1])
    assert [(g.kind, g.index, g.slot) for g in table] == [(0, 3, 4), (1, 0, 1)] and names == ["time", "s0"]
    assert isinstance(table[0], _lib.EmapGridLayer)
    table, names = grid_map_descriptor([], normal_color=True)
    assert names == ["normal_x", "normal_y", "normal_z", "color"]


@pytest.mark.parametrize("args, kw", [
    (([],), {}),                                                            # no layer
    ((["elevation", "ghost"],), {}),                                        # unknown name
    ((["color"],), {}),                                                     # the colour exists only with normal_color
    ((["rgb"],), {}),                                                       # a semantic name that is not configured
    ((["elevation", "time", "elevation"],), {}),                            # a name twice
    ((["elevation", "time"],), {"slots": [0]}),                             # slot list of another length
    ((["elevation", "time"],), {"slots": [1, 1]}),                          # a slot twice
    ((["elevation", "time"],), {"slots": [0, -1]}),                         # a negative slot
    ((["s%d" % k for k in range(33)], ["s%d" % k for k in range(33)]), {}), # more than 32
    ((["s%d" % k for k in range(29)], ["s%d" % k for k in range(29)]), {"normal_color": True}),   # 33 with the appended four
])
def test_the_descriptor_refuses(args, kw):
    from elevation_mapping_cupy_amd.elevation_mapping import grid_map_descriptor
    with pytest.raises(ValueError):
        grid_map_descriptor(*args, **kw)
