"""What the tests of the plugin chain past the 256-workgroup clamp of its map-wide reductions share (tests/test_chain_large_cases.py on
the CPU, tests/test_hip_chain_large.py on the GPU): the sizes, the dressed start states, the configuration, the pieces of a map a faulty
stride loop or final fold would lose, and the host route's arithmetic with such a piece left out of a reduction.

Three reductions clamp their first stage to 256 workgroups of 256 threads and stride over the rest of the map: the erosion's lo / hi /
has-NaN (csrc/emap_plugchain.hip: k_range_parts -> k_range_final, logical index), the inpainting's known-height range and counts
(csrc/emap_inpaint_chain.hip: k_inp_range_parts -> k_inp_range_final, PHYSICAL index) and the PCA's means, moments and score range
(csrc/emap_pca.hip, logical index).  As in tests/_plug_cases.py the yardstick of every value on the GPU is the plugins' host route on a
TWIN map; the dressing below makes a lost piece change that value."""
import numpy as np

import _grid_cases as gc
import _inpaint_chain_cases as ic
import _plug_cases as pc
import _semplug_cases as sc

F32 = np.float32
LARGE = (256, 257, 363)      # 65 536 cells: every part, no second pass; 66 049: 513 cells of a second pass; 131 769: a third, ragged pass
BLOCK, PARTS = 256, 256      # EM_BLOCK; ER_PARTS = EM_INP_PARTS = EM_PCA_PARTS
HEAD = BLOCK * PARTS         # the cells of pass 0
ORDERS = gc.ORDERS
_entry = pc._entry


# ---- the pieces ---------------------------------------------------------------------------------------------------------------------------
def last_part_cell(C):
    """the last cell that part 255 (the last partial record) reduces: 65 535 at 256 and 257 (pass 0), 131 071 at 363 (pass 1)"""
    L = C * C
    i = np.arange(L)
    return int(i[(i % HEAD) // BLOCK == PARTS - 1].max())


def pieces(C):
    """flat boolean masks of the cells a faulty reduction would lose: "a" every pass behind the first, "b" the ragged last block alone
    (257: one cell, 363: 185 cells), "c" the last part record alone"""
    L = C * C
    i = np.arange(L)
    return {"a": i >= HEAD, "b": i >= (L // BLOCK) * BLOCK, "c": (i % HEAD) // BLOCK == PARTS - 1}


# ---- the erosion's sources ------------------------------------------------------------------------------------------------------------------
ERO_LO, ERO_HI = F32(-0.25), F32(1.5)      # outside the rest of the layer (0 .. 1): losing either changes the quantiser's span for every cell


def erosion_extremes(C, which):
    """(flat logical index of the unique minimum, of the unique maximum).
    "map" (the traversability layer): the minimum in the first cell of pass 1, the maximum in the last cell -- at 257 the single cell of
    the ragged block, at 363 a cell of pass 2; at 256 cell 0 and the last cell, which is part 255's.
    "plane" (a plugin plane): the minimum in the last cell, the maximum in the last cell of part 255, so that a final fold that drops the
    last record is visible past the clamp as well (at 257 that part has cells of pass 0 only); at 256 the last cell and cell 0."""
    L = C * C
    if which == "map":
        return (HEAD if L > HEAD else 0), L - 1
    return L - 1, (last_part_cell(C) if L > HEAD else 0)


def erosion_layer(C, which):
    x = np.random.default_rng(11 if which == "map" else 12).uniform(0.0, 1.0, C * C).astype(F32)
    lo, hi = erosion_extremes(C, which)
    x[lo], x[hi] = ERO_LO, ERO_HI
    return x.reshape(C, C)


EROSIONS = [("ero_map_f", "map", False), ("ero_map_r", "map", True), ("ero_plane_f", "plane", False), ("ero_plane_r", "plane", True)]
ERO_K, ERO_IT = 3, 1


def erosion_restated(layer, reverse, lose=None):
    """plugins/erosion.py on the host (tests/_plug_cases.py: erosion_quantise / erode_loop / erosion_dequantise) with the cells `lose` left
    out of lo / hi; the uint8 cast wraps, as the device's does, where a value leaves 0 .. 255 under a wrong range"""
    x = np.asarray(layer, F32)
    if reverse:
        x = F32(1) - x
    kept = x.reshape(-1) if lose is None else x.reshape(-1)[~lose]
    lo, hi = kept.min(), kept.max()
    assert hi > lo
    span = F32(np.float64(hi) - np.float64(lo))
    q = (np.trunc((x - lo) * F32(255) / span).astype(np.int64) & 255).astype(F32)
    return pc.erosion_dequantise(pc.erode_loop(q, ERO_K, ERO_IT), lo, hi, reverse)


# ---- the PCA's features ---------------------------------------------------------------------------------------------------------------------
PCA_PATTERNS = {"pca3": ["^feat_[0-2]$"], "pca5": ["^feat_[0-4]$"], "pca16": ["^feat_.*$"]}
PCA_WIDTHS = {"pca3": 3, "pca5": 5, "pca16": 16}
DIRECT_ORDER = [5, 0, 3, 1, 6, 2, 4]                        # a table handed to emap_plugin_chain_ex directly: seven features, out of order
RATIO_FLOOR = 1.65                                          # tests/test_semplug_cases.py


def corner_cells(C):
    """(the cell that holds CORNER, the cell that holds -CORNER): the last cell of the map -- the ragged block of 257 and 363 -- and the
    last cell of part 255; at 256, where those are one cell, cell 0"""
    L = C * C
    return L - 1, (last_part_cell(C) if L > HEAD else 0)


def features(C):
    """(16, C, C): sc.feature_layers with, in features 0 .. 2, the cells behind pass 0 overwritten by values near the clip:
    +-0.98 (seven in ten positive), 0.96 in four cells of ten and 0 elsewhere, -0.94 in three of twenty and 0 elsewhere, drawn
    independently -- three variances that fall like the undressed ones, and means off the undressed ones, so that the means and the
    moments of a reduction that stops behind pass 0 are other numbers.  Two cells hold opposite corners of the clip cube in those three
    features (corner_cells; corner): the far ends of one score, so that the score range loses an end with either of them."""
    feat = sc.feature_layers(C).reshape(16, -1).copy()
    n = C * C - HEAD
    if n > 0:
        u = np.random.default_rng(31 + C).uniform(0.0, 1.0, (3, n))
        feat[0, HEAD:] = np.where(u[0] < 0.7, 0.98, -0.98)
        feat[1, HEAD:] = np.where(u[1] < 0.4, 0.96, 0.0)
        feat[2, HEAD:] = np.where(u[2] < 0.15, -0.94, 0.0)
    plus, minus = corner_cells(C)
    feat[:3, plus], feat[:3, minus] = corner(feat), -corner(feat)
    return feat.reshape(16, C, C)


def corner(feat):
    """the corner of the clip cube that lies farthest along the third principal axis of features 0 .. 2 (+-1 each): feature 2 seldom
    reaches the clip, so a cell in that corner is alone at the end of the third score"""
    x = np.clip(np.asarray(feat, F32)[:3].reshape(3, -1), -1, 1).astype(np.float64)
    v = np.linalg.eigh(np.cov(x))[1][:, 0]
    return np.where(v < 0, F32(-1), F32(1)).astype(F32)


def pca_stacks(C):
    """name -> (F, C, C): the stacks of the three configured PCA layers and of the direct table"""
    f = features(C)
    out = {n: f[:w] for n, w in PCA_WIDTHS.items()}
    out["direct"] = f[DIRECT_ORDER]
    return out


def pca_lossy(sources, lose_mean=None, lose_moments=None, lose_range=None):
    """sc.pca_restated with the cells `lose_*` (flat masks) left out of one reduction: the means (the sum of the kept cells over the
    count of ALL cells, as k_pca_mean_final divides), the centred moments, or lo / hi of the scores; levels wrap like the device's
    `& 255` where a score leaves the range"""
    src = np.asarray(sources, F32)
    shape = src.shape[1:]
    x = np.clip(src, F32(-1), F32(1)).reshape(len(src), -1).T.astype(np.float64)
    keep = lambda lose: slice(None) if lose is None else ~lose      # noqa: E731
    d = x - x[keep(lose_mean)].sum(axis=0) / len(x)
    dm = d[keep(lose_moments)]
    w, v = np.linalg.eigh(dm.T @ dm)
    vecs = v[:, np.argsort(-w, kind="stable")[:3]].T
    big = np.argmax(np.abs(vecs), axis=1)
    sign = np.where(vecs[np.arange(3), big] < 0, -1.0, 1.0)
    scores = d @ (vecs * sign[:, None]).T
    lo, hi = scores[keep(lose_range)].min(axis=0), scores[keep(lose_range)].max(axis=0)
    span = np.where(hi > lo, hi - lo, 1.0)
    lev = (np.trunc((scores - lo) / span * 255).astype(np.int64) & 255).astype(np.uint32).reshape(shape + (3,))
    return ((lev[..., 0] << np.uint32(16)) | (lev[..., 1] << np.uint32(8)) | lev[..., 2]).view(F32)


def pca_host(sources):
    """plugins/features_pca.py: FeaturesPca.__call__ on the stack (the SVD route)"""
    from elevation_mapping_cupy_amd.plugins.features_pca import _pca3
    src = np.asarray(sources, F32)
    shape = src.shape[1:]
    comp = _pca3(np.clip(src.reshape(len(src), -1).T, -1, 1).astype(np.float64)).reshape(shape + (3,))
    lo, hi = comp.min(axis=(0, 1)), comp.max(axis=(0, 1))
    span = np.where(hi > lo, hi - lo, 1.0)
    img = ((comp - lo) / span * 255).astype(np.uint8).astype(np.uint32)
    return ((img[:, :, 0] << np.uint32(16)) | (img[:, :, 1] << np.uint32(8)) | img[:, :, 2]).view(F32)


def ratios(stack):
    """sc.eigen_ratios, the third eigenvalue against the fourth included where the stack has one"""
    return sc.eigen_ratios(np.asarray(stack, F32))


def pca_visible(got, ref):
    """would sc.pca_condition refuse `got`: more than 1 level, or more than 0.1 % of the cells"""
    cells, lev, _ = sc.pca_disagreement(got, ref)
    return lev > sc.PCA_MAX_LEVEL or cells > sc.PCA_MAX_CELLS * np.asarray(ref).size


# ---- the inpainting's state -----------------------------------------------------------------------------------------------------------------
INP_LO, INP_HI = F32(-2.0), F32(2.0)      # beyond ic.elevation_plane (about -1.1 .. 0.7)


def inpaint_extremes(C):
    """(flat PHYSICAL index of the lowest known height, of the highest): the lowest in the first cell of pass 1 at 257 and in the last cell
    of part 255 at 363 (a cell of pass 1 there), the highest in the last cell; at 256 cell 0 and the last cell"""
    L = C * C
    lo = 0 if L <= HEAD else (HEAD if C == 257 else last_part_cell(C))
    return lo, L - 1


def inpaint_planes(C):
    """(elevation, is_valid) written on twins WITHOUT a move (gc.start(move=False)): the circular origin is zero, so the physical index
    the range strides over is the logical one of these planes.  Three cells of five known, at random; the two planted heights known
    (is_valid 1.0 and 0.5: the plugin's own >= 0.5); the last eight cells alternate between unknown and known, so that the ragged block
    and the last passes hold a share of both counts.  Heights finite everywhere."""
    L = C * C
    h = ic.elevation_plane(C).reshape(-1).copy()
    v = (np.random.default_rng(41 + C).uniform(0.0, 1.0, L) < 0.6).astype(F32)
    v[L - 8:] = np.tile(np.array([0.0, 1.0], F32), 4)
    lo, hi = inpaint_extremes(C)
    h[lo], h[hi] = INP_LO, INP_HI
    v[lo], v[hi] = 0.5, 1.0
    return h.reshape(C, C), v.reshape(C, C)


def inpaint_known_restated(h, valid, lose=None):
    """the plane the op leaves in the KNOWN cells (the fill does not touch them; tests/_inpaint_chain_cases.py: inpaint_quantise /
    inpaint_dequantise) with the cells `lose` left out of the range and the counts; None for the flat rule"""
    hf, vf = np.asarray(h, F32).reshape(-1), np.asarray(valid, F32).reshape(-1)
    keep = np.ones(hf.size, bool) if lose is None else ~lose
    r = ic.inpaint_range(hf[keep], vf[keep])
    if r is None:
        return None
    return ic.inpaint_dequantise(ic.inpaint_quantise(hf, *r), *r)[ic.known_of(vf)]


# ---- the configuration and the twins -----------------------------------------------------------------------------------------------------------
def config(C):
    """the filter and smooth ops, telea_fronts, the robot-centric elevation, a plane that is a copy of the semantic layer ero_src (a layer
    maximum of one layer, no step), four erosions -- of the traversability layer and of that plane, reverse both ways --, the semantic
    filter, the votes, a layer maximum, and the PCA at three widths"""
    e = [
        _entry("min_filter", "min_filter", height=True, dilation_size=1, iteration_n=30),
        _entry("smooth_filter", "smooth", height=True, input_layer_name="min_filter"),
        _entry("inpainting", "inpaint", height=True, method="telea_fronts"),
        _entry("robot_centric_elevation", "robot_centric_elevation", height=True, resolution=pc.resolution(C), use_threshold=False),
        _entry("max_layer_filter", "ero_plane_src", layers=["ero_src"], reverse=[False], thresholds=[False], scales=[1], default_value=0),
    ]
    for name, which, rev in EROSIONS:
        e.append(_entry("erosion", name, input_layer_name="traversability" if which == "map" else "ero_plane_src", kernel_size=ERO_K, iterations=ERO_IT, reverse=rev))
    e += [
        _entry("semantic_filter", "max_categories", classes=["^sem_.*$"]),
        _entry("semantic_traversability", "votes", layers=["traversability", "robot_centric_elevation"], thresholds=[0.3, 0.5], type=["traversability", "elevation"]),
        _entry("max_layer_filter", "max_layer", layers=["traversability", "sem_0", "votes"], reverse=[True, False, False], thresholds=[False, 0.5, False],
               scales=[1.0, 1.0, 1.0], default_value=0.0),
    ]
    return e + [_entry("features_pca", n, process_layer_names=pat) for n, pat in PCA_PATTERNS.items()]


INPUTS = ["min_filter", "smooth", "robot_centric_elevation", "ero_plane_src"]      # the planes other ops of the configuration read
PCA_NAMES = list(PCA_PATTERNS)
SEM_LAYERS = ["s0", "s1", "c0", "rgb"] + sc.SEM_NAMES + sc.FEAT_NAMES + ["ero_src"]


def dress(m, C):
    """the class and feature layers, the erosion's two sources: written AFTER the move, so that the band a move clears does not eat them
    (the circular origin is off zero; writing a layer writes the pending shift out)"""
    for n in sc.SEM_NAMES + sc.FEAT_NAMES + ["ero_src"]:
        m.semantic_map.add_layer(n)
    m.move_to(gc.MOVE + sc.EXTRA_MOVE, np.eye(3, dtype=F32))
    m.base_rotation = pc.TILT.copy()
    cls, feat = sc.class_layers(C), features(C)
    for k, n in enumerate(sc.SEM_NAMES):
        m.semantic_map.set_layer(n, cls[k])
    for k, n in enumerate(sc.FEAT_NAMES):
        m.semantic_map.set_layer(n, feat[k])
    m.semantic_map.set_layer("ero_src", erosion_layer(C, "plane"))
    m.set_layer_raw("traversability", erosion_layer(C, "map"))
    return m


def twins(C, path):
    return [dress(m, C) for m in pc.twins(C, config(C), path)]


def inpaint_twins(C, path):
    """twins without a move, elevation and is_valid written whole: physical = logical"""
    pair = pc.twins(C, [e for e in config(C) if e[0] in ("min_filter", "smooth", "inpaint")], path, move=False)
    h, v = inpaint_planes(C)
    for m in pair:
        m.set_layer_raw("elevation", h)
        m.set_layer_raw("is_valid", v)
    return pair


# ---- k_pca_eig: source tables built to reach its branches (cell_n 34 and 67) -----------------------------------------------------------------
EIG_SIZES = (34, 67)
EIG_LAYERS = sc.FEAT_NAMES + ["flat", "dis_0", "dis_1", "dis_2"]


def disjoint_layers(C):
    """(3, C, C): layer k is zero outside the k-th third of the first 3 * (C * C // 6) * 2 cells; inside, one half holds distinct multiples
    of 2^-20 below 2^-k and the other half their negatives, shuffled.  Every partial sum of such values is exact in double, so each mean
    is exactly 0 in any order of summation, every product of two layers is 0 in every cell, and the centred moments off the diagonal are
    exactly 0.0: the Jacobi sweeps have nothing to do.  The amplitudes 1, 1/2, 1/4 over equal areas put a factor 4 between the
    eigenvalues; each layer has one largest and one smallest cell, so no level sits on a tie."""
    half = C * C // 6
    rng = np.random.default_rng(51 + C)
    out = np.zeros((3, C * C), F32)
    for k in range(3):
        mag = (rng.permutation(1 << 16)[:half] + 1).astype(np.float64) * 2.0 ** (-16 - k)      # distinct, in (0, 2^-k]
        vals = np.concatenate([mag, -mag])
        out[k, 2 * half * k: 2 * half * (k + 1)] = rng.permutation(vals).astype(F32)
    assert (out.astype(np.float64) == out).all()
    return out.reshape(3, C, C)


def eig_layers(C):
    """name -> (C, C): sc.feature_layers, a constant layer and the three disjoint ones"""
    out = dict(zip(sc.FEAT_NAMES, sc.feature_layers(C)))
    out["flat"] = np.full((C, C), 0.375, F32)
    out.update(zip(["dis_0", "dis_1", "dis_2"], disjoint_layers(C)))
    return out


EIG_TABLES = {
    # feat_1 twice and feat_0 three times among five independent layers: exact zero eigenvalues below the top three, equal entries for the sign rule
    "repeated": ["feat_0", "feat_1", "feat_0", "feat_2", "feat_1", "feat_0", "feat_3", "feat_4"],
    # a zero row and column in the covariance, in the middle and not last
    "constant": ["feat_0", "flat", "feat_1", "feat_2", "feat_3"],
    # the leading eigenvalue arrives at the last diagonal entry
    "reversed": sc.FEAT_NAMES[::-1],
    "minimal": ["feat_2", "feat_0", "feat_1"],
    # off-diagonals exactly 0.0; the smallest variance first, so that the eigenvalue pick has to reorder
    "uncorrelated": ["dis_2", "dis_0", "dis_1"],
}


def eig_stack(C, table):
    lay = eig_layers(C)
    return np.stack([lay[n] for n in EIG_TABLES[table]])
