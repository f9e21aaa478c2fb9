"""What the tests of the publish-time plugins on resident planes share (tests/test_plug_cases.py and tests/test_plugin_chain_abi.py on the
CPU, tests/test_hip_plugin_chain.py on the GPU): the plugin configurations, the layer lists, the twin start state and the NumPy
restatement of the erosion's quantise / de-quantise arithmetic.

The yardstick of every value is the host route of the plugins (one get_map_with_name_ref per layer).  That call changes PluginManager
state, so it is made on a TWIN: a second map brought into the same state by the same calls (_grid_cases.start)."""
import numpy as np
import yaml

import _grid_cases as gc
from _util import make_parameter

SIZES = gc.SIZES
ORDERS = gc.ORDERS
TILT = np.array([[0.9396926, 0.0, 0.34202015], [0.05939117, 0.9848077, -0.16317591], [-0.33682409, 0.17364818, 0.9254166]], np.float32)      # pitch 20 deg, roll 10 deg


def resolution(C):
    return float(make_parameter(gc.config(), C).resolution)


def _entry(type_, layer, fill_nan=False, height=False, **extra):
    return layer, dict(enable=True, type=type_, fill_nan=bool(fill_nan), is_height_layer=bool(height), layer_name=layer, extra_params=extra)


def yaml_of(entries):
    return yaml.safe_dump(dict(entries), sort_keys=False)


# ---- the shipped configurations (the reference's config/core/plugin_config.yaml and config/setups/anymal/anymal_plugin_config.yaml) ----
CORE = [
    _entry("min_filter", "min_filter", height=True, dilation_size=1, iteration_n=30),
    _entry("smooth_filter", "smooth", height=True, input_layer_name="min_filter"),
    _entry("inpainting", "inpaint", height=True, method="telea"),
    _entry("erosion", "erosion", input_layer_name="traversability", dilation_size=3, iteration_n=20, reverse=True),
]
ANYMAL = [
    _entry("min_filter", "min_filter", height=True, dilation_size=1, iteration_n=30),
    _entry("max_filter", "max_filter", height=True, dilation_size=5, iteration_n=10),
    _entry("smooth_filter", "smooth", height=True, input_layer_name="min_filter"),
    _entry("inpainting", "inpaint", height=True, method="telea"),
]
FILTER_PUBLISHER = ["min_filter", "smooth", "inpaint", "elevation"]          # elevation_map_filter of the reference's example_setup.yaml
ANYMAL_LIST = ["min_filter", "max_filter", "smooth", "inpaint", "elevation"]
SEMANTIC_EROSION = [_entry("erosion", "erosion_sem", input_layer_name="s0", kernel_size=3, iterations=1)]


# ---- every device op, one layer each --------------------------------------------------------------------------------------------------
def ops_config(C):
    """min / max filters at d = 1 / 30 sweeps and d = 5 / 10 sweeps and one that stops early enough to leave NaN (min_few), smooth of a map
    layer and of plugin layers, the erosion of a layer that holds NaN (flat rule), the robot-centric elevation with and without its
    threshold, and fill_nan x is_height_layer in all four combinations"""
    res = resolution(C)
    return [
        _entry("min_filter", "min_filter", height=True, dilation_size=1, iteration_n=30),
        _entry("min_filter", "min5", height=True, dilation_size=5, iteration_n=10),
        _entry("min_filter", "min_few", height=True, dilation_size=1, iteration_n=1),
        _entry("max_filter", "max_filter", height=True, dilation_size=1, iteration_n=30),
        _entry("max_filter", "max5", height=True, dilation_size=5, iteration_n=10),
        _entry("smooth_filter", "smooth_elev", height=True, input_layer_name="elevation"),
        _entry("smooth_filter", "smooth", height=True, input_layer_name="min_filter"),
        _entry("smooth_filter", "smooth_few", height=True, input_layer_name="min_few"),
        _entry("erosion", "ero_nan", input_layer_name="min_few", kernel_size=3, iterations=1),
        _entry("robot_centric_elevation", "rce", resolution=res, use_threshold=False),
        _entry("robot_centric_elevation", "rce_thr", resolution=res, use_threshold=True, threshold=0.1),
        _entry("smooth_filter", "pub_00", fill_nan=False, height=False, input_layer_name="elevation"),
        _entry("smooth_filter", "pub_01", fill_nan=False, height=True, input_layer_name="elevation"),
        _entry("smooth_filter", "pub_10", fill_nan=True, height=False, input_layer_name="elevation"),
        _entry("smooth_filter", "pub_11", fill_nan=True, height=True, input_layer_name="elevation"),
    ]


EROSION_CASES = [(rev, k, it) for rev in (False, True) for k in (1, 3, 4) for it in (0, 1, 3)]


def erosion_name(rev, k, it):
    return "ero_%s_k%d_i%d" % ("r" if rev else "f", k, it)


def erosion_config():
    """the erosion of traversability for reverse both ways x kernel_size 1, 3, 4 (even: the anchor is off centre) x iterations 0, 1, 3, and
    of a constant layer (time, which the test overwrites with zeros): flat"""
    e = [_entry("erosion", erosion_name(rev, k, it), input_layer_name="traversability", kernel_size=k, iterations=it, reverse=rev)
         for rev, k, it in EROSION_CASES]
    return e + [_entry("erosion", "ero_const", input_layer_name="time", kernel_size=3, iterations=1)]


def erosion_traversability(C):
    """the raw traversability layer the erosion cases run on: the start state's is close to binary, this one gives the quantiser every
    value of 0 .. 1"""
    return np.random.default_rng(11).uniform(0.0, 1.0, (C, C)).astype(np.float32)


def oracle_start(C):
    """the start state of _grid_cases.start on the CPU oracle (heights only: the semantic cloud's points fuse as points): a terrain frame
    with visibility clean-up, update_time calls, a second frame, a move that shifts both axes"""
    import _fixtures as fx
    from oracle import emap_oracle as eo
    orc = eo.OracleMap(eo.make_params(gc.config(), cell_n=C))
    R, t = fx.POSES["identity"]
    N = max(40, C * C // 2)
    terrain = fx.cloud(C, N, 0)
    terrain[:, 2] = gc.relief(terrain)
    orc.update_map_with_kernel(terrain, R, t, 0.0, 0.0)
    for _ in range(3):
        orc.update_time()
    orc.update_map_with_kernel(np.ascontiguousarray(gc.semantic_frame(C, 2 * N, 1)[:, :3]), R, t, 0.0, 0.0)
    orc.update_time()
    orc.move_to(gc.MOVE)
    return orc


def box3_twice(plane):
    """SmoothFilter as the library computes it (k_box3 twice): per pass the 3-tap mean along axis 0 with double sums and a float32
    intermediate, then along axis 1; 'reflect' borders.  scipy's uniform_filter keeps a running sum along each line, which a NaN poisons
    to the line's end, so it cannot supply the smooth of a layer that holds NaN; on NaN-free planes the two agree (checked on the CPU)."""
    h = np.asarray(plane, np.float32)
    for _ in range(2):
        p = np.pad(h, 1, mode="edge").astype(np.float64)
        v = ((p[:-2] + p[1:-1] + p[2:]) / 3.0).astype(np.float32).astype(np.float64)
        h = ((v[:, :-2] + v[:, 1:-1] + v[:, 2:]) / 3.0).astype(np.float32)
    return h


def names_of(entries):
    return [v["layer_name"] for _, v in entries]


def manager(entries, cell_n, emap=None):
    """a PluginManager of the configuration, without a context"""
    from elevation_mapping_cupy_amd.plugins.plugin_manager import PluginManager, PluginParams
    pm = PluginManager(cell_n=cell_n, emap=emap)
    pm.init([PluginParams(name=v["type"], layer_name=v["layer_name"], fill_nan=v["fill_nan"], is_height_layer=v["is_height_layer"]) for _, v in entries],
            [v["extra_params"] for _, v in entries])
    return pm


def twins(C, entries, path, move=True):
    """two maps in the same state with the same plugins; the robot's base is tilted (the robot-centric elevation is not the elevation)"""
    path.write_text(yaml_of(entries))
    pair = []
    for _ in range(2):
        m = gc.start(C, plugin_file=path, move=move)
        m.base_rotation = TILT.copy()
        pair.append(m)
    return pair


# ---- the erosion's arithmetic around cv2.erode (reference EM/plugins/erosion.py:96-112), restated for float32 arrays ---------------------
def erosion_quantise(layer, reverse):
    """-> (q as float32 holding 0 .. 255, lo, hi) or None for the flat rule (no spread, or a NaN: np.min returns NaN and `not hi > lo` holds)"""
    x = np.asarray(layer, np.float32)
    if reverse:
        x = np.float32(1) - x
    lo, hi = x.min(), x.max()
    if not hi > lo:
        return None
    span = np.float32(np.float64(hi) - np.float64(lo))
    q = np.trunc((x - lo) * np.float32(255) / span).astype(np.uint8).astype(np.float32)
    return q, lo, hi


def erosion_dequantise(q, lo, hi, reverse):
    span = np.float32(np.float64(hi) - np.float64(lo))
    out = np.asarray(q, np.float32) * span / np.float32(255) + lo
    return (np.float32(1) - out) if reverse else out


def erode_loop(img, k, iterations):
    """k x k window minimum, anchor k // 2, pixels outside the image ignored (cv2.erode with a rectangle and the default border)"""
    a = k // 2
    x = np.asarray(img, np.float32)
    for _ in range(iterations):
        pad = np.pad(x, ((a, k - 1 - a), (a, k - 1 - a)), constant_values=np.inf)
        x = np.min([pad[dr:dr + x.shape[0], dc:dc + x.shape[1]] for dr in range(k) for dc in range(k)], axis=0)
    return x


def case_layers(C=34, seed=3):
    """layers the restatement is checked on: positive with a spread, negative values, both zeros, a constant one, one with a NaN"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 1.0, (C, C)).astype(np.float32)
    b = rng.uniform(-3.0, -1.0, (C, C)).astype(np.float32)
    z = np.zeros((C, C), np.float32); z[::2] = -0.0; z[1, 1] = 0.5
    c = np.full((C, C), 0.25, np.float32)
    n = a.copy(); n[2, 3] = np.nan
    return {"unit": a, "negative": b, "zeros": z, "constant": c, "nan": n}
