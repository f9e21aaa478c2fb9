"""GPU: the HIP path against the oracle, BIT FOR BIT, wherever the store paths of the frame's writing kernels branch:
  * k_bin_hist / k_bin_scatter hand workgroup b the chunk rho(b) of the cloud (emap_binned.hip: bin_chunk_of_block) -- forced-binned
    clouds of 1 workgroup, fewer than 8 and a number that is no multiple of 8, on a whole-map context (plain kernels) and on row strips
    without a visibility pass (strip kernels: staging records per chunk);
  * k_tile_fuse writes the two cell halves through (st16_wt, emap_device.h): every binned frame here, with and without pending map
    moves, on tiles that are cut by the map's edge (widths 202, 130, 1030);
  * the stencil pass behind them on maps of 512 and more 32 x 64 tiles (k_post<32, .>): column origins shifted by 1, 2, 3 (the wrap of
    the circular origin then lies inside the last column tile) and by 100 (inside a middle tile), row origins shifted with them (row
    segments that end inside a wave's four rows), and a map width that is no multiple of 64 (a partial last column tile).  These are the
    cases in which a 16-byte-per-lane store path of k_post has fast and fallback waves in one launch; that path was built, measured
    slower than the 4-byte stores and taken out again -- the cases stay as the pin for the next attempt.
k_post_dma and the other tile heights of k_post are covered by tests/test_hip_post_variants.py (small maps, launcher hooks, one
process per variant).  No test asserts a timing or a placement."""
import threading

import numpy as np
import pytest

import _fixtures as fx
from _util import assert_planes_equal, make_pair
from oracle import emap_oracle as eo

pytestmark = pytest.mark.gpu

NORAYS = dict(eo.YAML, enable_visibility_cleanup=False)


@pytest.fixture(autouse=True)
def _oracle_threads():
    eo.set_threads(8)
    yield
    eo.set_threads(1)


# 2048 points per workgroup below 1 M points (emap_api.hip: bin geometry): 1, 5 and 14 workgroups
@pytest.mark.parametrize("N", [1500, 10000, 27000])
def test_binned_whole_map_by_block_count(N, weights):
    C = 202
    hip, orc = make_pair(NORAYS, C, "reference_fp16", weights)
    hip.set_scatter_mode("binned")
    R, t = fx.POSES["rotated"]
    for f, dz in enumerate((0.0, -0.03)):
        p = fx.cloud(C, N, 40 + f, dz=dz)
        hip.update_map_with_kernel(p, [], R, t.copy(), 1.0, 1.0)
        orc.update_map_with_kernel(p, R, t, 1.0, 1.0)
        assert hip.last_update_path() == "binned"
        for _ in range(3):
            hip.update_time(); orc.update_time()
    assert_planes_equal(hip.elevation_map, orc.elevation_map, what="%d points" % N)
    assert_planes_equal(hip.normal_map, orc.normal_map, names=["nx", "ny", "nz"], what="%d points" % N)
    assert hip.get_additive_mean_error() == float(orc.additive_mean_error)


# strips stage 4096 points per workgroup at least: 1, 7 and 13 workgroups
@pytest.mark.parametrize("N", [3000, 27000, 50000])
def test_binned_strips_by_block_count(N, weights):
    import torch
    from elevation_mapping_cupy_amd.configs import parameter_from
    from elevation_mapping_cupy_amd.sharded import ShardedElevationMap
    from _torch_strips import TorchStripEngine
    from test_hip_strips import ThreadComm
    C, world = 130, 2
    cfg = dict(eo.DEFAULTS); cfg.update(NORAYS)
    R, t = fx.POSES["rotated"]
    clouds = [fx.cloud(C, N, 50 + f, dz=dz) for f, dz in enumerate((0.0, -0.03))]
    _, orc = make_pair(NORAYS, C, "reference_fp16", weights)
    for p in clouds:
        orc.update_map_with_kernel(p, R, t, 1.0, 1.0)
        for _ in range(3):
            orc.update_time()
    dev = torch.device("cuda", 0)
    shared = {"bar": threading.Barrier(world), "sums": [None] * world, "send": [None] * world}
    out, errs = [None] * world, []

    def run(rank):
        try:
            eng = TorchStripEngine(parameter_from(cfg, C, "reference_fp16", weights), rank, world, 0, dev)
            eng.map.set_scatter_mode("binned")
            sm = ShardedElevationMap(eng, ThreadComm(rank, world, shared), False, cfg["enable_overlap_clearance"])
            for p in clouds:
                eng.bind_points(p)
                sm.update(R, t, 1.0, 1.0)
                for _ in range(3):
                    eng.update_time()
            eng.sync()
            out[rank] = (eng.map.row_begin, eng.map.rows, eng.map.elevation_map, eng.map.normal_map, eng.map.get_additive_mean_error())
        except Exception as e:  # pragma: no cover
            errs.append(e)
            shared["bar"].abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [x.start() for x in th]; [x.join() for x in th]
    assert not errs, errs
    want, want_n = np.ascontiguousarray(orc.elevation_map, np.float32), np.ascontiguousarray(orc.normal_map, np.float32)
    assert sum(rows for _, rows, _, _, _ in out) == C
    for r0, rows, m, nm, add in out:
        assert_planes_equal(m, want[:, r0:r0 + rows], what="strip at row %d, %d points" % (r0, N))
        assert_planes_equal(nm, want_n[:, r0:r0 + rows], names=["nx", "ny", "nz"], what="strip at row %d, %d points" % (r0, N))
        assert add == float(orc.additive_mean_error)


def _post32_case(C, shift, weights):
    """two binned frames on a map of >= 512 stencil tiles of 32 rows, the second after a move by `shift` cells along both axes (no z
    offset: every plane stays bit-comparable); the stencil outputs of both frames are compared"""
    N = 60000
    assert ((C + 63) // 64) * ((C + 31) // 32) >= 512
    hip, orc = make_pair(NORAYS, C, "reference_fp16", weights)
    hip.set_scatter_mode("binned")
    orc.center = np.zeros(3, np.float32)
    R, t0 = fx.POSES["rotated"]
    res = float(hip.resolution)

    def frame(f, dz):
        p = fx.cloud(C, N, 60 + f, dz=dz)
        hip.update_map_with_kernel(p, [], R, (t0 + hip.center).astype(np.float32), 1.0, 1.0)
        orc.update_map_with_kernel(p, R, (t0 + hip.center - orc.center).astype(np.float32), 1.0, 1.0)
        for _ in range(2):
            hip.update_time(); orc.update_time()

    def check(what):
        assert_planes_equal(hip.elevation_map, orc.elevation_map, what=what)
        assert_planes_equal(hip.normal_map, orc.normal_map, names=["nx", "ny", "nz"], what=what)
        assert_planes_equal(np.asarray(hip.traversability_input)[None], np.asarray(orc.traversability_input)[None], names=["traversability_input"], what=what)

    frame(0, 0.0)
    check("C = %d, origin 0" % C)
    if shift:
        v = np.array([shift * res, shift * res, 0.0], np.float64)
        hip.move(v); orc.move(v)
        assert np.array_equal(hip.center, orc.center)
        frame(1, -0.03)
        check("C = %d, origin shifted by %d" % (C, shift))
        v = np.array([-res, -res, 0.0], np.float64)           # ... and back by one: the other sign of the alignment
        hip.move(v); orc.move(v)
        frame(2, -0.05)
        check("C = %d, origin shifted by %d - 1" % (C, shift))


@pytest.mark.parametrize("shift", [1, 2, 3, 100])
def test_post32_with_shifted_origin(shift, weights):
    _post32_case(1024, shift, weights)


@pytest.mark.parametrize("C,shift", [(1030, 0), (1030, 3)])
def test_post32_width_no_multiple_of_64(C, shift, weights):
    _post32_case(C, shift, weights)
