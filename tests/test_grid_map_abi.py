"""CPU: the C ABI of the GridMap message output (emap_publish_grid_map, include/emap_hip.h) as far as a machine without a device goes:
the entry point is declared, exported and bound, the struct of the binding has the header's fields, size and offsets (the header
compiled as C is the witness), and a call without a context or a table is refused before any device is touched."""
import ctypes as ct
import os
import re
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "emap_hip.h")


def _header_fields(name):
    h = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*\]", "", f.strip()) for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]


def test_the_entry_point_is_declared_exported_and_bound():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    assert "emap_publish_grid_map" in _lib.SYMBOLS and hasattr(lib, "emap_publish_grid_map")
    assert len(lib.emap_publish_grid_map.argtypes) == 8
    assert re.search(r"\bint emap_publish_grid_map\(emap_ctx\* ctx, const emap_grid_layer\* layers, int32_t n_layers, int32_t order,", open(HEADER).read())
    assert lib.emap_abi_version() == 3 and _lib.ABI_VERSION == 3          # additive: the version stays


def test_the_struct_and_the_constants_have_the_headers_values():
    from elevation_mapping_cupy_amd import _lib
    cname, cls = "emap_grid_layer", _lib.EmapGridLayer
    names = [f[0] for f in cls._fields_]
    assert names == _header_fields(cname)
    lines = ['printf("%%zu", sizeof(%s));' % cname] + ['printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names]
    lines.append('printf("\\n%d %d %d %d %d %d\\n", EMAP_GRID_ROWS, EMAP_GRID_MESSAGE, EMAP_GRID_BUILTIN, EMAP_GRID_SEMANTIC, EMAP_GRID_NORMAL_COLOR, EMAP_GRID_MAX_LAYERS);')
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write('#include "emap_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert [int(x) for x in out[0].split()] == [ct.sizeof(cls)] + [getattr(cls, n).offset for n in names] == [12, 0, 4, 8]
    assert [int(x) for x in out[1].split()] == [_lib.GRID_ORDERS["rows"], _lib.GRID_ORDERS["message"], _lib.GRID_BUILTIN, _lib.GRID_SEMANTIC,
                                                _lib.GRID_NORMAL_COLOR, _lib.GRID_MAX_LAYERS] == [0, 1, 0, 1, 2, 32]


def test_null_arguments_are_refused_without_touching_a_device():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    table = (_lib.EmapGridLayer * 1)()
    out = np.zeros(64, np.float32)
    fp = out.ctypes.data_as(ct.POINTER(ct.c_float))
    assert lib.emap_publish_grid_map(None, table, 1, 0, 0.0, 0, fp, 1) == -1
    assert lib.emap_publish_grid_map(None, None, 0, 0, 0.0, 0, None, 0) == -1
    assert not out.any()
