"""CPU: the PointCloud2 input's case table, restatement, scene and bindings (tests/_pc2_cases.py; the GPU side is tests/test_hip_pc2.py).

The table must reach both k_cloud_unpack instantiations, every datatype and every alignment class; the restatement must be the node's
loop (elevation_mapping_ros.cpp:319-338) where every column is moved; the scene must feed the frame: conditions on the INPUTS of the
GPU tests, checked where no GPU is needed.  The bindings are checked as far as a machine without a device allows."""
import ctypes as ct
import struct
from collections import Counter

import numpy as np
import pytest

import _depth_cases as dc
import _pc2_cases as pc
from oracle import emap_oracle as eo

DESC = [(c, pc.descriptor(c)[0]) for c in pc.CASES]


def test_the_table_reaches_every_instantiation_datatype_and_alignment_class():
    assert len({pc.case_key(c) for c in pc.CASES}) == len(pc.CASES)
    inst = Counter(pc.aligned4(d) for _, d in DESC)
    assert inst[True] >= 10 and inst[False] >= 10, inst
    # both instantiations by rows (row_step > width * point_step) and as one row of n points
    assert {(pc.aligned4(d), d.row_step == d.width * d.point_step) for _, d in DESC} == {(a, t) for a in (False, True) for t in (False, True)}
    conv = Counter(d.conv[c] for _, d in DESC for c in range(d.n_cols))
    assert set(conv) == set(range(9)) - {7}, conv          # (FLOAT32 fields are moved: typed=True leaves them conv 0)
    assert {d.conv[c] for _, d in DESC if pc.aligned4(d) for c in range(d.n_cols)} >= {0, 6}      # a 4-byte integer on the dword path
    n = [d.height * d.width for _, d in DESC]
    assert {x % 4 for x in n} == {0, 1, 2, 3}
    assert set(n) >= {1, 2, 3, 5, 63, 64, 65, 127, 129, 255, 256, 257, 1023, 1025, 4097}
    assert {(d.n_cols - 3) % 4 for _, d in DESC} == {0, 1, 2, 3}
    assert {d.n_cols - 3 for _, d in DESC} >= {0, 1, 2, 3, 4, 5, 16}
    assert {d.point_step % 4 for _, d in DESC} == {0, 1, 2, 3}
    assert {d.offset[c] % 4 for _, d in DESC for c in range(d.n_cols)} == {0, 1, 2, 3}
    assert {d.point_step for _, d in DESC} >= {12, 13, 16, 20, 22, 32, 48, 256}
    # every tile size is straddled: fewer points than a tile, exactly one, one more, several tiles
    for T in (64, 256, 512, 1024):
        rows = [d.width if d.row_step != d.width * d.point_step else d.height * d.width for _, d in DESC if pc.tile(d.point_step) == T]
        assert any(r < T for r in rows) and any(r > T for r in rows) and any(r % T not in (0,) and r > 2 * T for r in rows), (T, sorted(set(rows)))
    assert {pc.tile(ps) for ps in range(1, 257)} == {64, 128, 256, 512, 1024} and all(pc.tile(ps) * ps <= 16384 for ps in range(1, 257))
    # where a tile's bytes start, modulo the 16-byte loads: inside a row of tight points every tile starts on 16 (T * point_step is a
    # multiple of 64), so the other classes come from rows: dword-aligned ones, odd ones, and rows of several tiles
    by_rows = [d for _, d in DESC if d.row_step != d.width * d.point_step]
    starts = {(r * d.row_step) % 16 for d in by_rows for r in range(d.height)}
    assert starts >= {0, 4, 8, 12} and len({s for s in starts if s % 2}) >= 4, starts
    assert {pc.aligned4(d) for d in by_rows if d.width > 2 * pc.tile(d.point_step)} == {False, True}
    # the organised cloud of the issue, padded and tight, both settings
    org = [(c["row_pad"], c["typed"]) for c in pc.CASES if (c["layout"], c["height"], c["width"]) == ("22", 3, 37)]
    assert sorted(org) == [(0, False), (0, True), (6, False), (6, True)]
    # the typed layout: all eight datatypes, the FLOAT64 4- but not 8-aligned, its edges in the message
    lay = pc.LAYOUTS["typed47"]
    assert {f[2] for f in lay["fields"]} == set(range(1, 9))
    off64 = [f[1] for f in lay["fields"] if f[2] == pc.FLOAT64][0]
    assert off64 % 4 == 0 and off64 % 8 == 4


def test_the_typed_edges_convert_as_the_contract_says():
    c = [c for c in pc.CASES if c["layout"] == "typed47" and c["typed"] and c["width"] == 129][0]
    data, kw, cols = pc.message(c)
    d, names = pc.descriptor(c)
    xyz, chan = pc.unpack(data, d)
    f64 = chan[:, names.index("f64") - 3]
    inf = np.float32(np.inf)
    tiny = np.float32(2.0 ** -149)
    assert f64[0] == inf and f64[1] == -inf and f64[2] == inf                       # overflow; FLT_MAX + half an ulp
    assert f64[3] == np.float32(1e-40) and 0 < f64[3] < np.finfo(np.float32).tiny   # a float32 subnormal is kept
    assert f64[4] == -tiny and f64[5] == 0 and f64[6] == 2 * tiny and f64[7] == tiny      # ties at the bottom go to even
    assert f64[8] == 1 and f64[9] == np.float32(1 + 2.0 ** -22) and f64[10] == np.float32(1 + 2.0 ** -23)
    assert np.isnan(f64[11]) and np.signbit(f64[12]) and f64[12] == 0 and f64[14] == np.finfo(np.float32).max
    u32 = chan[:, names.index("u32") - 3]
    assert u32[:6].tolist() == [2.0 ** 24, 2.0 ** 24 + 4, 2.0 ** 24 + 2, 2.0 ** 25, 2.0 ** 25 + 8, 2.0 ** 25 + 4]      # on ties (to even), exact, off a tie
    assert u32[6] == 2.0 ** 32 and u32[7] == 2.0 ** 32 and u32[8] == 2.0 ** 32 - 256
    i32 = chan[:, names.index("i32") - 3]
    assert i32[0] == -2.0 ** 31 and i32[1] == 2.0 ** 31 and i32[2] == -2.0 ** 24 and i32[5] == 2.0 ** 31 - 128 and i32[6] == 2.0 ** 31
    small = {nm: chan[:3, names.index(nm) - 3].tolist() for nm in ("i8", "u8", "i16", "u16")}
    assert small == {"i8": [-128.0, 127.0, 0.0], "u8": [0.0, 255.0, 0.0], "i16": [-32768.0, 32767.0, 0.0], "u16": [0.0, 65535.0, 0.0]}
    # the moved FLOAT32 column keeps NaN payloads and subnormal patterns
    assert chan[:7, names.index("f32") - 3].view(np.uint32).tolist() == pc._F32_BITS.tolist()


@pytest.mark.parametrize("c", [c for c in pc.CASES if not c["typed"] and c["height"] * c["width"] <= 130], ids=pc.case_key)
def test_moved_columns_are_the_nodes_loop(c):
    """typed=False: the reference's gather, restated literally -- one 4-byte read per point and field at i * point_step + offset (the
    node ignores row_step; it is given the tight rows it assumes), widened to float64, cast back by input_pointcloud"""
    data, kw, cols = pc.message(c)
    d, names = pc.descriptor(c)
    xyz, chan = pc.unpack(data, d)
    H, W, ps, rs = d.height, d.width, d.point_step, d.row_step
    raw = np.frombuffer(data, np.uint8).reshape(H, rs)
    tight = raw[:, :W * ps].tobytes()
    n = H * W
    points = np.zeros((n, d.n_cols), np.float64)
    for i in range(n):
        for j in range(d.n_cols):
            points[i, j] = struct.unpack_from("<f", tight, i * ps + d.offset[j])[0]
    got = np.concatenate([xyz, chan], axis=1)
    want = points.astype(np.float32)
    nan = np.isnan(want)                                      # (a signalling NaN is quieted on its way through float64 in the reference; here its bits are kept)
    assert (np.isnan(got) == nan).all()
    assert (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all()


def test_pack_and_unpack_are_inverse_and_the_padding_is_junk():
    c = [c for c in pc.CASES if c["layout"] == "22" and c["row_pad"] == 6 and c["typed"]][0]
    data, kw, cols = pc.message(c)
    d, names = pc.descriptor(c)
    assert d.row_step == 22 * 37 + 6 and len(data) == 3 * d.row_step
    xyz, chan = pc.unpack(data, d)
    for k, nm in enumerate("xyz"):
        assert (xyz[:, k].view(np.uint32) == cols[nm]).all()
    assert (chan[:, 1] == cols["ring"].astype(np.float32)).all() and (chan[:, 2].view(np.uint32) == cols["time"]).all()
    raw = np.frombuffer(data, np.uint8).reshape(3, d.row_step)
    assert len(np.unique(raw[:, 22 * 37:])) > 8               # the row padding is not zeros


@pytest.mark.parametrize("colour", [False, True])
def test_the_scene_feeds_the_frame(colour):
    xyz, chan, names = pc.scene_cloud(60, 80, colour)
    n = xyz.shape[0]
    assert n == 4800 and chan.shape == (n, 4 if colour else 0)
    data, kw = pc.scene_message(xyz, chan, names, "rgbf32" if colour else "xyz22u")
    from elevation_mapping_cupy_amd.elevation_mapping import pointcloud2_descriptor
    d, got_names = pointcloud2_descriptor(kw["fields"], kw["width"], kw["height"], kw["point_step"], kw["row_step"])
    assert got_names == ["x", "y", "z"] + names
    x2, c2 = pc.unpack(data, d)
    assert x2.tobytes() == xyz.tobytes() and c2.tobytes() == chan.tobytes()
    ok = ~np.isnan(xyz).any(axis=1)
    assert ok.sum() * 2 >= n and not ok.all()
    om = eo.OracleMap(eo.make_params(eo.YAML, cell_n=66))
    om.update_map_with_kernel(np.ascontiguousarray(np.concatenate([xyz, chan], axis=1)), dc.CAM_R, dc.CAM_T.copy(), 0.0, 0.0)
    fused = int(om.last["cnt"].sum())
    assert fused * 2 >= n, (fused, n)


# ---- bindings, as far as a machine without a device goes ----------------------------------------------------------------------------
def test_the_entry_point_is_bound_and_exported():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    assert "emap_bind_cloud_message" in _lib.SYMBOLS and hasattr(lib, "emap_bind_cloud_message")
    assert ct.sizeof(_lib.EmapCloudMsgDesc) == 176
    assert [f[0] for f in _lib.EmapCloudMsgDesc._fields_] == ["height", "width", "point_step", "row_step", "is_bigendian", "n_cols", "offset", "conv"]
    assert _lib.EmapCloudMsgDesc.offset.size == 76 and _lib.EmapCloudMsgDesc.conv.size == 76
    import os
    import re
    from conftest import ROOT
    h = open(os.path.join(ROOT, "include", "emap_hip.h")).read()
    body = re.search(r"typedef struct emap_cloud_msg_desc \{(.*?)\} emap_cloud_msg_desc;", h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    header = [re.sub(r"\[.*\]", "", f.strip()) for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert header == [f[0] for f in _lib.EmapCloudMsgDesc._fields_]


def test_a_null_context_is_refused_without_a_device():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    d, _ = pc.descriptor(pc.CASES[0])
    data = np.zeros(64, np.uint8)
    n = ct.c_int64(-7)
    assert lib.emap_bind_cloud_message(None, ct.byref(d), ct.c_void_p(data.ctypes.data), ct.byref(n)) == -1 and n.value == -7


class _Field:
    def __init__(self, name, offset, datatype, count=1):
        self.name, self.offset, self.datatype, self.count = name, offset, datatype, count


def test_fields_channels_and_typed_give_the_expected_descriptor():
    from elevation_mapping_cupy_amd.elevation_mapping import pointcloud2_descriptor as desc
    F = pc.LAYOUTS["22"]["fields"]
    d, names = desc(F, 37, 3, 22, 820)
    assert (d.height, d.width, d.point_step, d.row_step, d.is_bigendian, d.n_cols) == (3, 37, 22, 820, 0, 6)
    assert names == ["x", "y", "z", "intensity", "ring", "time"]
    assert list(d.offset)[:6] == [0, 4, 8, 12, 16, 18] and list(d.conv) == [0] * 19 and list(d.offset)[6:] == [0] * 13
    d, names = desc([_Field(*f[:3]) for f in F], 37, 3, 22, typed=True)      # objects as well as tuples; row_step defaults to tight rows
    assert d.row_step == 22 * 37 and list(d.conv)[:6] == [0, 0, 0, 0, pc.UINT16, 0]
    # the node's rule: the first three fields are x, y, z whatever they are called
    d, names = desc([("a", 8, 7, 1), ("b", 0, 7, 1), ("c", 4, 7, 1), ("w", 12, 8, 1)], 5, 1, 20, typed=True)
    assert names == ["a", "b", "c", "w"] and list(d.offset)[:4] == [8, 0, 4, 12] and list(d.conv)[:4] == [0, 0, 0, 8]
    # channels: the fields NAMED x, y, z first, then the named ones in the given order
    d, names = desc([("z", 8, 7, 1), ("time", 18, 7, 1), ("x", 0, 7, 1), ("ring", 16, 4, 1), ("y", 4, 7, 1)], 5, 1, 22, channels=["ring", "time"], typed=True)
    assert names == ["x", "y", "z", "ring", "time"] and list(d.offset)[:5] == [0, 4, 8, 16, 18] and list(d.conv)[:5] == [0, 0, 0, 4, 0]
    d, names = desc(F, 5, 1, 22, channels=[])
    assert d.n_cols == 3 and names == ["x", "y", "z"]
    # rgb / rgba stay moved whatever datatype the message claims for them
    d, _ = desc([("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1), ("rgb", 12, 6, 1), ("rgba", 16, 6, 1), ("t", 20, 6, 1)], 5, 1, 24, typed=True)
    assert list(d.conv)[:6] == [0, 0, 0, 0, 0, 6]
    d, _ = desc(F, 5, 1, 22, is_bigendian=True)
    assert d.is_bigendian == 1
    with pytest.raises(ValueError):
        desc(F[:3] + [("normal", 12, 7, 3)], 5, 1, 24)                  # a selected field with count != 1
    desc(F[:3] + [("normal", 12, 7, 3)], 5, 1, 24, channels=[])         # ... which is fine when it is not selected
    with pytest.raises(ValueError):
        desc(F, 5, 1, 22, channels=["nope"])
    with pytest.raises(ValueError):
        desc(F[:2], 5, 1, 22)                                           # fewer than three columns
    with pytest.raises(ValueError):
        desc([("f%d" % k, 4 * k, 7, 1) for k in range(20)], 5, 1, 80)   # more than 3 + 16


def test_the_compat_package_offers_the_same_class():
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        from elevation_mapping_cupy.elevation_mapping import ElevationMap as Compat
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))
    for m in ("bind_pointcloud2", "input_pointcloud2", "bound_points"):
        assert callable(getattr(Compat, m))
