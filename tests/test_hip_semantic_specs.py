"""GPU: every RGB / semantic point-fusion spec and gather branch of tests/_sem_specs.py against the oracle, frame by frame (the table
and what each case was built to hit: tests/_sem_specs.py; that the cases reach it: tests/test_sem_spec_cases.py).  Which code runs in
k_tile_semantic, k_sem_sum / k_sem_color / k_sem_finalize depends on the spec and on the cloud's layout alone: no environment hook, no
child process.  The specs go through the C ABI (emap_frame_semantics, emap_semantic_update), so that channel order and layers are what
the table says."""
import ctypes as ct

import numpy as np
import pytest

import _sem_specs as ss
from _util import assert_planes_equal, make_pair
from oracle import emap_oracle as eo

pytestmark = pytest.mark.gpu

def _ctypes_spec(spec):
    from elevation_mapping_cupy_amd._lib import EmapSemSpec
    s = EmapSemSpec()
    s.alpha = 0.5
    s.n_sum, s.n_col = len(spec["sums"]), len(spec["colours"])
    for i, (c, k, l) in enumerate(spec["sums"]):
        s.sum_chan[i], s.sum_kind[i], s.sum_layer[i] = c, k, l
    for i, (c, l) in enumerate(spec["colours"]):
        s.col_chan[i], s.col_layer[i] = c, l
    return s


class _Device:
    """device copies of host arrays through the HIP runtime (as test_device_cloud_layouts_agree of tests/test_hip_semantic.py makes them),
    freed by close().  close() leaves the context with a dangling cloud pointer: call it only once the frame's results were read back
    (that synchronises), and bind the next cloud or close the context before anything reads points again."""

    def __init__(self):
        self.hip = ct.CDLL("libamdhip64.so")
        self.kept = []

    def put(self, a):
        a = np.ascontiguousarray(a, np.float32)
        d = ct.c_void_p()
        assert self.hip.hipMalloc(ct.byref(d), ct.c_size_t(a.nbytes)) == 0
        assert self.hip.hipMemcpy(d, ct.c_void_p(a.ctypes.data), ct.c_size_t(a.nbytes), 1) == 0
        self.kept.append(d)
        return d.value

    def close(self):
        for d in self.kept:
            self.hip.hipFree(d)
        self.kept = []


def _bind(hip, dev, layout, p):
    N, ncols = p.shape
    if layout == "upload":
        hip.bind_points(p)
    elif layout == "rows":
        hip.bind_points_device(dev.put(p), N, ncols)
    else:
        hip.bind_points_device_split(dev.put(p[:, :3]), dev.put(p[:, 3:]), N, ncols - 3)


def _check_layers(case, sem, get_alpha, ref, f):
    """the layers after frame f against the oracle's"""
    what = "%s frame %d" % (case["key"], f)
    want, want_alpha = ref["sem"][f], ref["alpha"][f]
    spec = ss.SPECS[case["spec"]]
    for _, l in spec["colours"]:
        assert np.array_equal(sem[l].view(np.uint32), want[l].view(np.uint32)), "%s: packed colour layer %d differs in %d cells" % (
            what, l, int((sem[l].view(np.uint32) != want[l].view(np.uint32)).sum()))
    assert not sem[0].any(), what
    bayes = [l for _, k, l in ss.all_sums(case) if k == ss.CBAY]
    for _, k, l in ss.all_sums(case):
        if k == ss.BINF:
            assert np.array_equal(sem[l].view(np.uint32), want[l].view(np.uint32)), "%s: bayesian_inference layer %d" % (what, l)
        else:
            d = np.abs(sem[l].astype(np.float64) - want[l])
            assert np.allclose(sem[l], want[l], atol=1e-6, rtol=1e-5), "%s: layer %d (kind %d), max |d| = %g in %d cells" % (
                what, l, k, float(d.max()), int((d > 1e-6 + 1e-5 * np.abs(want[l])).sum()))
        if k == ss.CBAY:
            a = get_alpha(l)
            assert np.allclose(a, want_alpha[l], atol=1e-5, rtol=1e-5), "%s: pseudo-counts of layer %d, max |d| = %g" % (
                what, l, float(np.abs(a.astype(np.float64) - want_alpha[l]).max()))
    if bayes:
        tot = np.sum([sem[l].astype(np.float64) for l in bayes], axis=0)
        assert np.allclose(tot[tot > 0], 1.0, atol=1e-6), what
        assert int((tot > 0).sum()) > 1000


def _run_case(case, ref):
    """the case's frames on a fresh context, every frame checked against the oracle run `ref`; returns the layers after the last frame"""
    from elevation_mapping_cupy_amd._lib import f32p
    key = case["key"]
    hip, _ = make_pair(ss.case_config(case, eo.YAML), case["C"], case["mode"])
    dev = _Device()
    try:
        hip.set_scatter_mode(case["scatter"], case["stack"])
        for l in range(ss.n_layers(case)):
            hip.semantic_map.add_layer("l%d" % l)
        alpha, layer = ss.priors(case)
        for l, a in alpha.items():
            hip.semantic_map.set_alpha(l, a)
        for l, a in layer.items():
            hip.semantic_map.set_layer(l, a)
        spec = _ctypes_spec(ss.SPECS[case["spec"]])
        after = _ctypes_spec(ss.AFTER[case["after"]]) if case["after"] else None
        R, t, clouds = ss.case_inputs(case)
        seen = []
        for f, p in enumerate(clouds):
            _bind(hip, dev, case["layout"], p)
            # (keep_counts: a call behind the frame needs the accepted counts a frame that fuses in its tile pass would not leave)
            hip._chk(hip._lib.emap_frame_semantics(hip._ctx, ct.byref(spec), 1 if after is not None else 0))
            hip.update_map_with_kernel(None, [], R, t.copy(), ss.NOISE, ss.NOISE)
            seen.append((hip.last_update_path(), hip.last_frame_semantics()))
            if after is not None:
                Rf, tf = hip._rt(R, t)
                hip._chk(hip._lib.emap_semantic_update(hip._ctx, f32p(Rf), f32p(tf), ct.byref(after)))
            for _ in range(ss.TIME_TICKS):
                hip.update_time()
            sem = hip.semantic_map.semantic_map          # (synchronises: the device clouds of this frame may go)
            dev.close()
            print("%s frame %d: %s / %s" % (key, f, *seen[-1]))
            assert seen[-1] == ss.expected_frame(case, f), (key, f, seen)
            _check_layers(case, sem, hip.semantic_map.get_alpha, ref, f)
        # a semantic pass must not disturb the heights it shares LDS with
        assert_planes_equal(hip.elevation_map, ref["map"], what=key)
    finally:
        dev.close()
        hip.close()
    return sem


# One test per group of the table (cases that fuse the same clouds into the same map state, tests/_sem_specs.py: group_of): the group's
# oracle run is computed once and its members are compared among themselves inside the test, whatever pytest selects or reorders.
GROUPS = {}
for _c in ss.CASES:
    GROUPS.setdefault(ss.group_of(_c), []).append(_c["key"])


@pytest.mark.parametrize("keys", list(GROUPS.values()), ids=["+".join(k) for k in GROUPS.values()])
def test_spec_cases_against_the_oracle(keys):
    cases = [ss.case_of(k) for k in keys]
    ref = ss.oracle_run(cases[0], eo)
    exact = {l for _, l in ss.SPECS[cases[0]["spec"]]["colours"]} | {l for _, k, l in ss.all_sums(cases[0]) if k == ss.BINF}
    written = [l for _, _, l in ss.all_sums(cases[0])] + [l for _, l in ss.SPECS[cases[0]["spec"]]["colours"]]
    done = []
    for case in cases:
        sem = _run_case(case, ref)
        # the paths, stacks and layouts of one group among themselves: the binned forms to the bit; the atomic path adds in another order
        for other, osem in done:
            what = "%s vs %s" % (case["key"], other["key"])
            if other["scatter"] == case["scatter"] == "binned":
                assert_planes_equal(sem, osem, names=["layer %d" % l for l in range(len(sem))], what=what)
            else:
                for l in written:
                    if l in exact:
                        assert np.array_equal(sem[l].view(np.uint32), osem[l].view(np.uint32)), (what, l)
                    else:
                        assert np.allclose(sem[l], osem[l], atol=1e-6, rtol=1e-6), (what, l)
        done.append((case, sem))
