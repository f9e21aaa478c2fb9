"""CPU: the C ABI of the publish-time plugins on resident planes (emap_plugin_planes, emap_plugin_plane_write / _read, emap_plugin_chain,
emap_publish_grid_map_ex; include/emap_hip.h) as far as a machine without a device goes: declared, exported and bound; the structs of
the binding have the header's fields, sizes and offsets and the constants its values (the header compiled as C is the witness); calls
without a context or a table are refused before any device is touched; the ABI version stays 3."""
import ctypes as ct
import os
import re
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "emap_hip.h")
NEW = ("emap_plugin_planes", "emap_plugin_plane_write", "emap_plugin_plane_read", "emap_plugin_chain", "emap_publish_grid_map_ex")


def _header_fields(name):
    h = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            out += [f.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    return out


def test_the_entry_points_are_declared_exported_and_bound():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n, n_args in zip(NEW, (2, 3, 3, 4, 8)):
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
        assert len(getattr(lib, n).argtypes) == n_args, n
        assert re.search(r"\bint %s\(emap_ctx\* ctx," % n, h), n
    assert lib.emap_abi_version() == 3 and _lib.ABI_VERSION == 3          # additive: the version stays
    assert "#define EMAP_ABI_VERSION 3" in h


def test_the_structs_and_the_constants_have_the_headers_values():
    from elevation_mapping_cupy_amd import _lib
    lines = []
    for cname, cls in (("emap_plugin_op", _lib.EmapPluginOp), ("emap_grid_layer_ex", _lib.EmapGridLayerEx)):
        names = [f[0] for f in cls._fields_]
        assert names == _header_fields(cname)
        lines += ['printf("%%zu", sizeof(%s));' % cname] + ['printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names] + ['printf("\\n");']
    consts = ["EMAP_GRID_PLUGIN", "EMAP_GRID_FILL_NAN", "EMAP_GRID_ADD_Z", "EMAP_PLUGIN_MAX_PLANES", "EMAP_PLUGIN_MAX_OPS", "EMAP_PLUGIN_MIN_FILTER",
              "EMAP_PLUGIN_MAX_FILTER", "EMAP_PLUGIN_SMOOTH", "EMAP_PLUGIN_EROSION", "EMAP_PLUGIN_ROBOT_CENTRIC", "EMAP_PLUGIN_SRC_LAYER", "EMAP_PLUGIN_SRC_PLANE",
              "EMAP_PLUGIN_REVERSE", "EMAP_PLUGIN_THRESHOLD"]
    lines.append('printf("%s\\n", %s);' % (" ".join(["%d"] * len(consts)), ", ".join(consts)))
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write('#include "emap_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    op, ex = _lib.EmapPluginOp, _lib.EmapGridLayerEx
    assert [int(x) for x in out[0].split()] == [ct.sizeof(op)] + [getattr(op, f[0]).offset for f in op._fields_] == [32, 0, 4, 8, 12, 16, 20, 24, 28]
    assert [int(x) for x in out[1].split()] == [ct.sizeof(ex)] + [getattr(ex, f[0]).offset for f in ex._fields_] == [16, 0, 4, 8, 12]
    assert op._fields_[-1] == ("f0", ct.c_float)
    P = _lib.PLUGIN_OPS
    assert [int(x) for x in out[2].split()] == [_lib.GRID_PLUGIN, _lib.GRID_FILL_NAN, _lib.GRID_ADD_Z, _lib.PLUGIN_MAX_PLANES, _lib.PLUGIN_MAX_OPS, P["min_filter"],
                                                P["max_filter"], P["smooth"], P["erosion"], P["robot_centric"], _lib.PLUGIN_SRC_LAYER, _lib.PLUGIN_SRC_PLANE,
                                                _lib.PLUGIN_REVERSE, _lib.PLUGIN_THRESHOLD] == [3, 1, 2, 32, 32, 0, 1, 2, 3, 4, 0, 1, 1, 2]


def test_null_arguments_are_refused_without_touching_a_device():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    out = np.zeros(64, np.float32)
    fp = out.ctypes.data_as(ct.POINTER(ct.c_float))
    ops = (_lib.EmapPluginOp * 1)()
    table = (_lib.EmapGridLayerEx * 1)()
    assert lib.emap_plugin_planes(None, 1) == -1
    assert lib.emap_plugin_plane_write(None, 0, fp) == -1 and lib.emap_plugin_plane_read(None, 0, fp) == -1
    assert lib.emap_plugin_chain(None, ops, 1, fp) == -1 and lib.emap_plugin_chain(None, None, 0, None) == -1
    assert lib.emap_publish_grid_map_ex(None, table, 1, 0, 0.0, 0, fp, 1) == -1
    assert lib.emap_publish_grid_map_ex(None, None, 0, 0, 0.0, 0, None, 0) == -1
    assert not out.any()
