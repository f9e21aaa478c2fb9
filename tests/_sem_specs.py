"""Case table of tests/test_hip_semantic_specs.py and tests/test_sem_spec_cases.py: RGB / semantic point-fusion specs (emap_sem_spec) and
cloud layouts chosen for the branches of k_tile_semantic (emap_binned.hip), k_sem_sum / k_sem_color / k_sem_finalize (emap_semantic.hip)
and the host-side choice between them (emap_api_semantic.hip).  Numpy only; the oracle runs in the two test files.

A spec: `ncols` columns of the cloud, `sums` = [(cloud column, kind, layer)], `colours` = [(cloud column, layer)]; kinds as in
emap_device.h (0 average, 1 class_average, 2 class_bayesian, 3 bayesian_inference).  The columns of kinds 2 / 3 are shifted by -0.2
(some theta < 0), the layers of kind 2 start from pseudo-count priors, those of kind 3 from a prior layer (the reference leaves it as
it is).  Layer 0 of every spec is written by nothing.

A case: key, spec, C, N, mode, rays, scatter ("atomic" | "binned") and stack, layout ("upload" | "rows" = emap_set_points_device |
"split" = emap_set_points_device_split), cloud ("base" = uniform with the piling of fx.semantic_cloud | "heavy" = the squeeze of
heavy202 in tests/_bin_variants.py, by index pattern), frames.  `after` (the ABI cases): a second spec that one emap_semantic_update
call fuses behind every frame."""
import numpy as np

RES = 0.04
TIME_TICKS = 3
NOISE = 1.0                       # position / orientation noise of every frame: the drift gate is open, heavy tiles are split
SPLIT_CAP = 4096                  # records per part (emap_device.h), as a literal
SEM_GROUP = 4                     # channels per LDS pass of k_tile_semantic (emap_binned.hip)
AVG, CAVG, CBAY, BINF = 0, 1, 2, 3
SQUEEZE = (0.1, (1.2, 0.8))       # heavy202: scale about the sensor, move by (dx, dy) metres


def _spec(ncols, sums, colours):
    """sums: [(column, kind)], colours: [column]; layers n ... 1 in that order (layer 0 stays untouched)"""
    n = len(sums) + len(colours)
    return dict(ncols=ncols, sums=[(c, k, n - i) for i, (c, k) in enumerate(sums)],
                colours=[(c, n - len(sums) - i) for i, c in enumerate(colours)])


SPECS = {
    "spread": _spec(10, [(3, AVG), (9, AVG), (5, CAVG)], [6]),
    "row_end": _spec(11, [(7, AVG), (8, AVG), (9, AVG), (10, AVG)], []),
    "row_end_over": _spec(11, [(8, AVG), (9, AVG), (10, AVG)], []),
    "colour_only": _spec(4, [], [3]),
    "colours2": _spec(6, [(3, AVG)], [4, 5]),
    "colours3": _spec(7, [(3, AVG)], [4, 5, 6]),
    "colours4": _spec(8, [(3, AVG)], [4, 5, 6, 7]),
    "six_sums": _spec(10, [(3, AVG), (4, AVG), (5, CAVG), (6, AVG), (7, CAVG), (8, AVG)], [9]),
    "sixteen": _spec(19, [(3 + k, AVG if k % 2 == 0 else CAVG) for k in range(16)], []),
    "bayes3": _spec(11, [(8, CBAY), (4, CBAY), (10, CBAY), (9, BINF), (3, BINF)], [6]),
    "mixed_group": _spec(7, [(3, AVG), (4, CBAY), (5, CAVG), (6, BINF)], []),
    # the ABI cases: what the frame declares (and carries: columns 3 ... 6 travel in the 32-byte records) ...
    "abi_frame": _spec(11, [(3, AVG), (4, AVG)], [6]),
}
# ... and what one emap_semantic_update call fuses behind it, into further layers.  abi_after is ONE group of four: it reaches beyond the
# carried window and is gathered from the cloud through the records' point index.  abi_after2 has two groups: the first lies inside
# the window (read from the record), the second outside (gathered).
AFTER = {
    "abi_after": dict(ncols=11, sums=[(4, AVG, 4), (5, AVG, 5), (8, CAVG, 6), (9, CAVG, 7)], colours=[]),
    "abi_after2": dict(ncols=11, sums=[(4, AVG, 4), (5, AVG, 5), (3, AVG, 6), (4, AVG, 7), (8, CAVG, 8), (9, CAVG, 9)], colours=[]),
}
SPLIT_KERNEL_ON_HEAVY = ("six_sums", "sixteen", "spread", "row_end", "row_end_over")      # sem_split_possible(); the others run the unsplit kernel behind a split sort


def _case(key, spec, path, **kw):
    c = dict(key=key, spec=spec, C=200, N=59999, mode="reference_fp16", rays=False, scatter="binned", stack=0, layout="upload",
             cloud="base", frames=3, after=None)
    if path == "atomic":
        c.update(scatter="atomic")
    elif path == "binned_rays":
        c.update(rays=True)
    elif path == "heavy":
        c.update(C=202, N=150001, cloud="heavy")
    else:
        assert path == "binned"
    c.update(kw)
    return c


# cases that share (spec, cloud, mode, rays) compute the same layers and stand next to each other: the atomic form first
CASES = []
for _s in ("spread", "row_end", "row_end_over", "colour_only", "colours2", "colours3", "colours4", "six_sums", "sixteen", "bayes3", "mixed_group"):
    CASES += [_case(_s + "_atomic", _s, "atomic"), _case(_s + "_binned", _s, "binned")]
    if _s in ("bayes3", "six_sums"):
        CASES += [_case(_s + "_stack4", _s, "binned", stack=4)]
    if _s in ("spread", "six_sums"):
        CASES += [_case(_s + "_rows", _s, "binned", layout="rows")]
    CASES += [_case(_s + "_rays", _s, "binned_rays")]
    if _s in ("row_end", "row_end_over"):      # (the stand-alone kernel on 16-byte records: where the 16-byte window of the gather is decided)
        CASES += [_case(_s + "_rays_rows", _s, "binned_rays", layout="rows")]
    if _s == "row_end":
        CASES += [_case(_s + "_rays_split", _s, "binned_rays", layout="split")]
    if _s in ("bayes3", "six_sums"):
        CASES += [_case(_s + "_fp32", _s, "binned", mode="fp32")]
    CASES += [_case(_s + "_heavy", _s, "heavy")]
for _a in ("abi_after", "abi_after2"):
    CASES += [_case(_a, "abi_frame", "binned", after=_a), _case(_a + "_heavy", "abi_frame", "heavy", after=_a)]
KEYS = [c["key"] for c in CASES]


def case_of(key):
    return CASES[KEYS.index(key)]


def group_of(case):
    """cases of one group fuse the same clouds into the same map state: equal layers whatever the path, stack or layout"""
    return (case["spec"], case["after"], case["cloud"], case["C"], case["N"], case["mode"], case["rays"])


def case_config(case, yaml):
    cfg = dict(yaml, enable_visibility_cleanup=bool(case["rays"]))
    assert cfg["enable_overlap_clearance"] and cfg["enable_drift_compensation"]
    return cfg


def all_sums(case):
    """(column, kind, layer) of everything a frame of the case fuses, the call behind the frame included"""
    return SPECS[case["spec"]]["sums"] + (AFTER[case["after"]]["sums"] if case["after"] else [])


def n_layers(case):
    s = SPECS[case["spec"]]
    return 1 + max([l for _, _, l in all_sums(case)] + [l for _, l in s["colours"]])


def squeezed(N):
    """which points of a heavy cloud are squeezed: 60 % by index pattern, so that the decode boundary N / K of the compact kernels
    cuts through both shares"""
    return np.arange(N) % 5 < 3


def case_inputs(case):
    """(R, t, [cloud per frame]); t is relative to the map's centre, which never moves"""
    import _fixtures as fx
    R, t = fx.POSES["rotated"]
    s = SPECS[case["spec"]]
    C, N, seed = case["C"], case["N"], 100 * (sorted(SPECS).index(case["spec"]) + 1)
    sums = all_sums(case)
    clouds = []
    for f in range(case["frames"]):
        p = fx.cloud(C, N, seed + f, dz=-0.03 * f, extra=s["ncols"] - 3)
        rng = np.random.default_rng(5000 + seed + f)
        for c, _ in s["colours"]:
            p[:, c] = rng.integers(0, 1 << 24, N, dtype=np.uint32).view(np.float32)
        for c in sorted({c for c, k, _ in sums if k >= CBAY}):
            p[:, c] -= np.float32(0.2)
        if case["cloud"] == "heavy":
            m = squeezed(N)
            scale, (dx, dy) = SQUEEZE
            p[m, :2] *= np.float32(scale)
            p[m, 0] += np.float32(dx); p[m, 1] += np.float32(dy)
        else:
            k = p[1::3].shape[0]
            p[:3 * k:3, :2] = p[1::3, :2]             # pile points up so that cells see several points (fx.semantic_cloud)
        clouds.append(p)
    return R, t.copy(), clouds


def priors(case):
    """{layer: plane}: pseudo-counts of the class_bayesian layers (30 % of the cells empty), and {layer: plane}: previous contents of the
    bayesian_inference layers (half of the cells empty)"""
    C = case["C"]
    rng = np.random.default_rng(78)
    alpha, layer = {}, {}
    for _, k, l in all_sums(case):
        if k == CBAY:
            a = rng.uniform(0, 2, (C, C)).astype(np.float32)
            a[rng.uniform(0, 1, (C, C)) < 0.3] = 0.0
            alpha[l] = a
        elif k == BINF:
            a = rng.uniform(0, 1, (C, C)).astype(np.float32)
            a[rng.uniform(0, 1, (C, C)) < 0.5] = 0.0
            layer[l] = a
    return alpha, layer


def oracle_kwargs(spec):
    """the spec as OracleMap.semantic_update takes it (class_bayesian / bayesian_inference in spec order: their position is the q of
    the compact decode)"""
    by = {k: [(c, l) for c, kk, l in spec["sums"] if kk == k] for k in (AVG, CAVG, CBAY, BINF)}
    return dict(average=by[AVG], class_average=by[CAVG], class_bayesian=by[CBAY], bayesian_inference=by[BINF], color=list(spec["colours"]), alpha=0.5)


def oracle_run(case, eo):
    """the case on the oracle `eo` (oracle.emap_oracle): per frame the semantic layers and the pseudo-counts, the map after the last
    frame; read-only arrays"""
    orc = eo.OracleMap(eo.make_params(case_config(case, eo.YAML), cell_n=case["C"], mode=case["mode"]))
    R, t, clouds = case_inputs(case)
    L, C = n_layers(case), case["C"]
    orc.semantic_map = np.zeros((L, C, C), np.float32)
    orc.semantic_alpha = np.zeros((L, C, C), np.float32)
    alpha, layer = priors(case)
    for l, a in alpha.items():
        orc.semantic_alpha[l] = a
    for l, a in layer.items():
        orc.semantic_map[l] = a
    sem, alp = [], []
    for p in clouds:
        orc.update_map_with_kernel(p, R, t, NOISE, NOISE)
        orc.semantic_update(p, R, t, **oracle_kwargs(SPECS[case["spec"]]))
        if case["after"]:
            orc.semantic_update(p, R, t, **oracle_kwargs(AFTER[case["after"]]))
        for _ in range(TIME_TICKS):
            orc.update_time()
        sem.append(orc.semantic_map.copy()); alp.append(orc.semantic_alpha.copy())
    out = dict(sem=sem, alpha=alp, map=np.array(orc.elevation_map, np.float32))
    for a in sem + alp + [out["map"]]:
        a.setflags(write=False)
    return out


# ---- the decisions of the device code, restated -------------------------------------------------------------------------------------
def chan_view(layout, ncols):
    """(col0, stride) of the channel matrix (emap_api.hip: emap_upload_points :508-509, emap_set_points_device_split :570-571,
    emap_set_points_device :578-579)"""
    return (0, ncols) if layout == "rows" else (3, ncols - 3)


def carry_eligible(spec, rays):
    """frame_sem_begin (emap_api_semantic.hip:104-108): the frame's sort may carry the channels in 32-byte records"""
    if rays or len(spec["sums"]) > 4 or len(spec["colours"]) > 1 or not spec["sums"] + spec["colours"]:
        return False
    if any(k > CAVG for _, k, _ in spec["sums"]):
        return False
    cols = [c for c, _, _ in spec["sums"]] + [c for c, _ in spec["colours"]]
    return max(cols) - min(cols) < 4


def carried_c0(case):
    """first column of the carried window of the case's frames (emap_api_semantic.hip:110), -1: 16-byte records"""
    s = SPECS[case["spec"]]
    if case["scatter"] != "binned" or not carry_eligible(s, case["rays"]):
        return -1
    return min([c for c, _, _ in s["sums"]] + [c for c, _ in s["colours"]])


def sem_split_possible(spec):
    """emap_binned.hip:1137"""
    return len(spec["sums"]) > 0 and not any(k == CBAY for _, k, _ in spec["sums"]) and len(spec["colours"]) <= 1


def group_decisions(spec, layout, cc0):
    """per channel group of k_tile_semantic (emap_binned.hip:971-986): dict(ride, inrec, wide, fit), fit = (first column of the 16-byte
    window - col0 + 4) - stride for a group within four columns (0: the window ends exactly at the row's end, 1: it overruns by one),
    None otherwise.  cc0 >= 0: 32-byte records that carry columns [cc0, cc0 + 4)."""
    col0, stride = chan_view(layout, spec["ncols"])
    ride = len(spec["colours"]) == 1 and len(spec["sums"]) > 0
    out = []
    for g0 in range(0, len(spec["sums"]), SEM_GROUP):
        cols = [c for c, _, _ in spec["sums"][g0:g0 + SEM_GROUP]]
        if ride and g0 == 0:
            cols.append(spec["colours"][0][0])
        cmin, cmax = min(cols), max(cols)
        inrec = cc0 >= 0 and cmin >= cc0 and cmax < cc0 + 4
        if inrec:
            cmin = cc0
        fit = cmin - col0 + 4 - stride if cmax - cmin < 4 and cmin >= col0 else None
        out.append(dict(ride=ride and g0 == 0, inrec=inrec, wide=inrec or (fit is not None and fit <= 0), fit=fit))
    return out


def phases(spec):
    return (len(spec["sums"]) + SEM_GROUP - 1) // SEM_GROUP


def heavy_in(case, f):
    """a sort bin of frame f holds more than 4096 records (tests/test_sem_spec_cases.py checks it against the oracle's point_index)"""
    return case["cloud"] == "heavy" or case["stack"] == 4


def expected_frame(case, f):
    """(emap_last_update_path, last_frame_semantics) of frame f.  A frame that carries fuses in the tile pass unless its launch has
    heavy-tile parts -- which the scan of the frame BEFORE asks for (emap_api.hip: count_impl), so never in the first frame."""
    if case["scatter"] == "atomic":
        return "atomic", "separate"
    if carried_c0(case) < 0:
        return "binned", "separate"
    return "binned", ("carried" if f > 0 and heavy_in(case, f - 1) else "in_tile_pass")
