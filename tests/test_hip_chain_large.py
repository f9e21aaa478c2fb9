"""GPU: the plugin chain past the 256-workgroup clamp of its map-wide reductions -- the erosion's range (csrc/emap_plugchain.hip:
k_range_parts / k_range_final), the inpainting's known-height range and counts (csrc/emap_inpaint_chain.hip: k_inp_range_parts /
k_inp_range_final) and the PCA's means, moments and score range (csrc/emap_pca.hip) -- at cell_n 256 (all 256 parts, no second pass),
257 (a second pass of 513 cells) and 363 (a third, ragged pass), on start states dressed so that a lost pass, a lost ragged block or a
lost part record changes the result (tests/_chain_large_cases.py; tests/test_chain_large_cases.py shows on the CPU that it does).  The
yardstick of every value is the plugins' host route on a TWIN map: bit for bit -- uint32 views, NaN equal to NaN -- for everything but
FEATURES_PCA, which stays under the PCA condition (levels differ by at most 1, in at most 0.1 % of the cells).  Behind them the source
tables built to reach the branches of k_pca_eig, at cell_n 34 and 67, against sc.pca_restated of the same arrays."""
import numpy as np
import pytest

import _chain_large_cases as lc
import _grid_cases as gc
import _plug_cases as pc
import _semplug_cases as sc

pytestmark = pytest.mark.gpu
_pairs, _refs = {}, {}
BUILD = {
    "chain": lambda C, path: lc.twins(C, path),
    "inpaint": lambda C, path: lc.inpaint_twins(C, path),
    "core": lambda C, path: pc.twins(C, pc.CORE, path),
    "turtle": lambda C, path: sc.twins(C, sc.TURTLE, path),
}


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """pair(C, config) -> (map, twin): built once per module, for the tests that do not change the map"""
    def get(C, cfg):
        if (C, cfg) not in _pairs:
            _pairs[(C, cfg)] = tuple(BUILD[cfg](C, tmp_path_factory.mktemp("large") / ("%s_%d.yaml" % (cfg, C))))
        return _pairs[(C, cfg)]
    yield get
    for m, t in _pairs.values():
        m.close(); t.close()
    _pairs.clear(); _refs.clear()


def _ref(m, name):
    out = np.zeros((m.cell_n - 2, m.cell_n - 2), np.float32)
    m.get_map_with_name_ref(name, out)
    return out


def _yardstick(pair, C, cfg):
    """the twin's host route for every plugin layer of the configuration, in configuration order (inputs before their readers), once:
    name -> (published layer, raw plane)"""
    if (C, cfg) not in _refs:
        twin = pair(C, cfg)[1]
        refs = {"elevation": (_ref(twin, "elevation"), None)}
        for n in twin.plugin_manager.layer_names:
            pub = _ref(twin, n)
            refs[n] = (pub, twin.plugin_manager.host_layer(n).copy())
        for pub, raw in refs.values():
            pub.setflags(write=False)
            if raw is not None:
                raw.setflags(write=False)
        _refs[(C, cfg)] = refs
    return _refs[(C, cfg)]


def _is_pca(m, name):
    pm = m.plugin_manager
    return name in pm.layer_names and pm.plugin_names[pm.layer_names.index(name)] == "features_pca"


def _check(m, name, got, ref, order, what):
    want = ref if order == "rows" else gc.message_plane(ref)
    assert got.shape == want.shape and got.dtype == np.float32, what
    if _is_pca(m, name):
        sc.pca_condition(got, want, what)
        return
    ok = gc.same_bits(got, want)
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s (%s): %d of %d values differ bitwise, first at %s: %r vs %r" % (what, order, int((~ok).sum()), ok.size, i, got[i], want[i]))


def _plane(m, k):
    from elevation_mapping_cupy_amd import _lib
    out = np.empty((m.cell_n, m.cell_n), np.float32)
    assert m._lib.emap_plugin_plane_read(m._ctx, k, _lib.f32p(out)) == 0
    return out


def _check_plane(m, name, raw, what):
    """the RAW plane through emap_plugin_plane_read: border included, no flip, no NaN fill"""
    got = _plane(m, m.plugin_manager.layer_names.index(name))
    if _is_pca(m, name):
        sc.pca_condition(got, raw, "raw plane of " + what)
    else:
        _check(m, name, got, raw, "rows", "raw plane of " + what)


def _direct_pca(m, dst, sem_indices):
    """one FEATURES_PCA op through emap_plugin_chain_ex on the semantic layers `sem_indices`, in that order"""
    from elevation_mapping_cupy_amd import _lib
    ops = (_lib.EmapPluginOp * 1)()
    ops[0].type, ops[0].dst_plane, ops[0].src_index, ops[0].i0 = _lib.PLUGIN_OPS_EX["features_pca"], dst, 0, len(sem_indices)
    table = (_lib.EmapPluginSrc * len(sem_indices))()
    for t, i in zip(table, sem_indices):
        t.kind, t.index = _lib.PLUGIN_SRC_SEMANTIC, i
    rc = m._lib.emap_plugin_chain_ex(m._ctx, ops, 1, None, table, len(sem_indices))
    assert rc == 0, m._lib.emap_last_error(m._ctx)
    return _plane(m, dst)


# ---- 0. the twins and the dressing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", lc.LARGE)
def test_the_twins_hold_the_same_map_and_the_dressing_survived(pair, C):
    m, t = pair(C, "chain")
    assert m.semantic_map.layer_names == t.semantic_map.layer_names == lc.SEM_LAYERS
    for n in gc.BUILTINS + tuple(lc.SEM_LAYERS):
        assert gc.same_bits(_ref(m, n), _ref(t, n)).all(), n
    assert gc.same_bits(m.get_layer_raw("traversability"), lc.erosion_layer(C, "map")).all()
    assert gc.same_bits(m.semantic_map.get_layer("ero_src"), lc.erosion_layer(C, "plane")).all()
    feat = lc.features(C)
    for k, n in enumerate(sc.FEAT_NAMES):
        assert gc.same_bits(m.semantic_map.get_layer(n), feat[k]).all(), n
    assert np.isfinite(m.get_layer_raw("elevation")).all()


# ---- 1. every op alone and the whole list -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", lc.LARGE)
def test_each_op_alone_against_the_twin(pair, C):
    m = pair(C, "chain")[0]
    refs = _yardstick(pair, C, "chain")
    m.get_grid_map_layers(lc.INPUTS)                                  # the planes other ops read, as the yardstick computed them: configuration order
    assert m.last_plugin_route == {n: "device" for n in lc.INPUTS}
    for order in lc.ORDERS:
        for n in m.plugin_manager.layer_names:
            names, got = m.get_grid_map_layers([n], order=order)
            assert names == [n] and m.last_plugin_route == {n: "device"}, n
            _check(m, n, got[0], refs[n][0], order, "%s at %d" % (n, C))
            if order == "rows":
                _check_plane(m, n, refs[n][1], "%s at %d" % (n, C))


@pytest.mark.parametrize("order", lc.ORDERS)
@pytest.mark.parametrize("C", lc.LARGE)
def test_the_whole_list_in_one_call(pair, C, order):
    """four erosions, three PCAs and the inpainting in ONE chain: each op's scratch slot (chain_red, chain_pca, chain_inp) is written to
    its end while its neighbour's is live"""
    m = pair(C, "chain")[0]
    refs = _yardstick(pair, C, "chain")
    lst = m.plugin_manager.layer_names + ["elevation"]
    names, got = m.get_grid_map_layers(lst, order=order)
    assert names == lst and m.last_plugin_route == {n: "device" for n in m.plugin_manager.layer_names}
    for k, n in enumerate(names):
        _check(m, n, got[k], refs[n][0], order, "%s in the list at %d" % (n, C))
    for n in m.plugin_manager.layer_names:
        _check_plane(m, n, refs[n][1], "%s in the list at %d" % (n, C))


@pytest.mark.parametrize("C", lc.LARGE)
def test_the_yardstick_can_tell_the_ops_apart(pair, C):
    r = {n: raw for n, (pub, raw) in _yardstick(pair, C, "chain").items() if raw is not None}
    differs = lambda a, b: not gc.same_bits(a, b).all()      # noqa: E731
    assert gc.same_bits(r["ero_plane_src"], lc.erosion_layer(C, "plane")).all()          # the plane source is the dressed layer
    assert len({r[n].tobytes() for n, _, _ in lc.EROSIONS}) == 4
    for n, which, rev in lc.EROSIONS:                      # the window minimum keeps the planted end: -0.25, or 1 - 1.5 of the reversed layer given back as 1.5
        assert differs(r[n], lc.erosion_layer(C, which)) and (r[n].max() == lc.ERO_HI if rev else r[n].min() == lc.ERO_LO), n
    assert differs(r["inpaint"], pair(C, "chain")[1].get_layer_raw("elevation")) and differs(r["smooth"], r["min_filter"])
    assert len({r[n].tobytes() for n in lc.PCA_NAMES}) == 3
    for n in lc.PCA_NAMES:
        lv = sc.levels(r[n])                                                             # the raw plane holds the border: both ends of every score
        assert all(lv[..., ch].min() == 0 and lv[..., ch].max() == 255 for ch in range(3)), n


# ---- 2. the PCA: repeatable, and a table handed over directly -------------------------------------------------------------------------------------
def test_the_pca_is_repeatable_bit_for_bit(pair):
    C = 257
    m = pair(C, "chain")[0]
    _, a = m.get_grid_map_layers(lc.PCA_NAMES, order="message")
    planes_a = [_plane(m, m.plugin_manager.layer_names.index(n)) for n in lc.PCA_NAMES]
    _, b = m.get_grid_map_layers(lc.PCA_NAMES, order="message")
    planes_b = [_plane(m, m.plugin_manager.layer_names.index(n)) for n in lc.PCA_NAMES]
    assert a.tobytes() == b.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(planes_a, planes_b))
    assert m.last_plugin_route == {n: "device" for n in lc.PCA_NAMES}


@pytest.mark.parametrize("C", lc.LARGE)
def test_a_pca_table_of_seven_features_out_of_order(pair, C):
    m = pair(C, "chain")[0]
    dst = m.plugin_manager.layer_names.index("pca5")
    sem = [lc.SEM_LAYERS.index(sc.FEAT_NAMES[f]) for f in lc.DIRECT_ORDER]
    got = _direct_pca(m, dst, sem)
    src = np.stack([m.semantic_map.get_layer(i) for i in sem])
    assert gc.same_bits(src, lc.pca_stacks(C)["direct"]).all()
    sc.pca_condition(got, sc.pca_restated(src), "the direct table at %d" % C)


# ---- 3. the inpainting's range: twins without a move, physical = logical ----------------------------------------------------------------------------
@pytest.mark.parametrize("C", lc.LARGE)
def test_the_inpainting_range_past_the_clamp(pair, C):
    """k_inp_range_parts strides over the PHYSICAL cell index.  The library has no accessor for the circular origin, so this case is built
    on twins whose start state has no move (gc.start(move=False)): the origin is zero and the planted cells of lc.inpaint_planes lie at
    the physical indices lc.inpaint_extremes names.  The origin off zero of k_inp_quantise / k_inp_dequantise stays with the small sizes
    (tests/test_hip_inpaint_chain.py) and with the moved twins of the tests above."""
    m, t = pair(C, "inpaint")
    h, v = lc.inpaint_planes(C)
    for x in (m, t):
        assert gc.same_bits(x.get_layer_raw("elevation"), h).all() and gc.same_bits(x.get_layer_raw("is_valid"), v).all()
    refs = _yardstick(pair, C, "inpaint")
    for order in lc.ORDERS:
        names, got = m.get_grid_map_layers(["inpaint"], order=order)
        assert names == ["inpaint"] and m.last_plugin_route == {"inpaint": "device"}
        _check(m, "inpaint", got[0], refs["inpaint"][0], order, "inpaint at %d" % C)
        _check_plane(m, "inpaint", refs["inpaint"][1], "inpaint at %d" % C)
    lst = ["min_filter", "smooth", "inpaint", "elevation"]
    names, got = m.get_grid_map_layers(lst, order="message")
    assert names == lst and m.last_plugin_route == {n: "device" for n in lst[:3]}
    for k, n in enumerate(lst):
        _check(m, n, got[k], refs[n][0], "message", "%s in the list at %d" % (n, C))
    raw = refs["inpaint"][1].reshape(-1)
    known = v.reshape(-1) >= 0.5
    lo, hi = lc.inpaint_extremes(C)
    assert raw[lo] == lc.INP_LO and raw[hi] == lc.INP_HI                               # both ends of the range de-quantise to themselves: levels 0 and 255
    assert gc.same_bits(raw[known], lc.inpaint_known_restated(h, v)).all()             # the yardstick is the restatement the CPU cases lose pieces from
    assert not gc.same_bits(raw[~known], h.reshape(-1)[~known]).all()


# ---- 4. the shipped lists, at 257 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", lc.ORDERS)
def test_the_shipped_core_list_past_the_clamp(pair, order):
    C = 257
    m, t = pair(C, "core")
    lst = pc.FILTER_PUBLISHER + ["erosion"]
    refs = _yardstick(pair, C, "core")
    names, got = m.get_grid_map_layers(lst, order=order)
    assert names == lst and m.last_plugin_route == {"min_filter": "device", "smooth": "device", "inpaint": "host", "erosion": "device"}
    for k, n in enumerate(names):
        _check(m, n, got[k], refs[n][0], order, n)
    msg = m.get_grid_map_message(lst)                                                  # a host plugin (inpaint: telea) between device ops
    assert msg.layers == lst and m.last_plugin_route["inpaint"] == "host" and m.last_plugin_route["erosion"] == "device"
    for k, n in enumerate(msg.layers):
        _check(m, n, msg.data[k].data.reshape(C - 2, C - 2), refs[n][0], "message", n + " in the message")


@pytest.mark.parametrize("order", lc.ORDERS)
def test_the_turtle_bot_list_past_the_clamp(pair, order):
    C = 257
    m, t = pair(C, "turtle")
    refs = _yardstick(pair, C, "turtle")
    m.get_grid_map_layers(sc.TURTLE_INPUTS)
    names, got = m.get_grid_map_layers(sc.TURTLE_LIST, order=order)
    assert names == sc.TURTLE_LIST and m.last_plugin_route == {n: "device" for n in sc.TURTLE_SEMANTIC}
    for k, n in enumerate(names):
        _check(m, n, got[k], refs[n][0], order, n)
    msg = m.get_grid_map_message(sc.TURTLE_FULL)                                       # a host plugin (inpaint) between semantic ops
    assert msg.layers == sc.TURTLE_FULL and m.last_plugin_route["inpaint"] == "host"
    assert all(m.last_plugin_route[n] == "device" for n in sc.TURTLE_SEMANTIC + ["min_filter", "smooth"])
    for k, n in enumerate(msg.layers):
        _check(m, n, msg.data[k].data.reshape(C - 2, C - 2), refs[n][0] if n in refs else _ref(t, n), "message", n + " in the full list")


# ---- 5. a move between two ticks ------------------------------------------------------------------------------------------------------------------------
def test_the_ops_see_a_move_between_two_ticks(tmp_path):
    """after the move the logical tail behind pass 0 lies on other physical cells, and the band the move cleared lies inside the map"""
    C = 257
    m, t = lc.twins(C, tmp_path / "p.yaml")
    try:
        lst = [n for n in m.plugin_manager.layer_names] + ["elevation"]
        seen = []
        for step in range(2):
            if step == 1:
                for x in (m, t):
                    x.move_to(x.center + np.array([-0.12, 0.08, 0.0]), np.eye(3, dtype=np.float32))
                    x.base_rotation = pc.TILT.copy()
            names, got = m.get_grid_map_layers(lst, order="message")
            assert names == lst and m.last_plugin_route == {n: "device" for n in m.plugin_manager.layer_names}
            for k, n in enumerate(names):
                _check(m, n, got[k], _ref(t, n), "message", "%s at step %d" % (n, step))
            seen.append(got.copy())
        for k, n in enumerate(lst):
            assert not gc.same_bits(seen[0][k], seen[1][k]).all(), n
    finally:
        m.close(); t.close()


# ---- 6. k_pca_eig: tables built to reach its branches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", lc.EIG_SIZES)
def test_the_eigen_solver_on_tables_built_for_its_branches(C):
    """repeated sources (exact zero eigenvalues, equal entries for the sign rule), a constant layer (a zero row and column), sixteen
    features in reversed order (the leading eigenvalue last), three layers, and three uncorrelated layers whose off-diagonal moments are
    exactly 0.0 (the sweep loop ends at once).  tests/test_chain_large_cases.py shows every table has three determined components, so
    none is left out."""
    m = gc.start(C)
    try:
        base = len(m.semantic_map.layer_names)
        lay = lc.eig_layers(C)
        for n in lc.EIG_LAYERS:
            m.semantic_map.add_layer(n)
        for n in lc.EIG_LAYERS:
            m.semantic_map.set_layer(n, lay[n])
        assert m._lib.emap_plugin_planes(m._ctx, 2) == 0
        for table, names in lc.EIG_TABLES.items():
            sem = [base + lc.EIG_LAYERS.index(n) for n in names]
            got = _direct_pca(m, 1, sem)
            src = np.stack([m.semantic_map.get_layer(i) for i in sem])
            assert gc.same_bits(src, lc.eig_stack(C, table)).all(), table
            sc.pca_condition(got, sc.pca_restated(src), "%s at %d" % (table, C))
            again = _direct_pca(m, 0, sem)
            assert again.tobytes() == got.tobytes(), table
    finally:
        m.close()
