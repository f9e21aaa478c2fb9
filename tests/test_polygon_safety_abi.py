"""CPU: the C ABI of the safety-polygon service on the device (emap_polygon_safety, include/emap_hip.h) as far as a machine without a
device goes: declared, exported and bound; the verdict struct of the binding has the header's fields, size and offsets (the header
compiled as C is the witness); and every refusal that needs no context's state is refused before any device is touched -- with a context
the GPU tests (test_hip_polygon_safety.py) read the reason of each refusal."""
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
    return [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]


def test_the_entry_point_is_declared_exported_and_bound():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    assert "emap_polygon_safety" in _lib.SYMBOLS and hasattr(lib, "emap_polygon_safety")
    assert len(lib.emap_polygon_safety.argtypes) == 12
    assert re.search(r"\bint emap_polygon_safety\(emap_ctx\* ctx, const float\* polygons_xy, const int32_t\* vertex_begin", open(HEADER).read())
    assert "emap_polygon_mask" in _lib.SYMBOLS                            # the mask service stays
    assert lib.emap_abi_version() == 3 and _lib.ABI_VERSION == 3          # additive: the version stays


def test_the_header_still_compiles_as_c():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", HEADER])


def test_the_verdict_struct_and_the_constants_have_the_headers_values():
    from elevation_mapping_cupy_amd import _lib
    cname, cls = "emap_polygon_verdict", _lib.EmapPolygonVerdict
    names = [f[0] for f in cls._fields_]
    assert names == _header_fields(cname)
    lines = ['printf("%%zu", sizeof(%s));' % cname] + ['printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names]
    lines.append('printf("\\n%d %d %d %d %d %d %d %d\\n", EMAP_POLY_MAX_BATCH, EMAP_POLY_MAX_VERTS, EMAP_POLY_MAX_TILES, EMAP_POLY_MAP_LAYER, EMAP_POLY_SEMANTIC, '
                 'EMAP_POLY_PLUGIN, EMAP_POLY_HAS_NAN, EMAP_POLY_POISON);')
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write('#include "emap_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert [int(x) for x in out[0].split()] == [ct.sizeof(cls)] + [getattr(cls, n).offset for n in names] == [48, 0, 8, 16, 20, 24, 28, 32, 36, 40, 44]
    assert [int(x) for x in out[1].split()] == [_lib.POLY_MAX_BATCH, _lib.POLY_MAX_VERTS, _lib.POLY_MAX_TILES, _lib.POLY_MAP_LAYER, _lib.POLY_SEMANTIC,
                                                _lib.POLY_PLUGIN, _lib.POLY_HAS_NAN, _lib.POLY_POISON] == [4096, 256, 262144, 0, 1, 3, 1, 2]


def _call(lib, ctx=None, xy=True, begin=(0, 4), n=1, kind=0, index=3, verdicts=True, ext=True, ext_begin=(0, 64)):
    from elevation_mapping_cupy_amd import _lib
    pts = np.zeros((max(1, begin[-1] if begin else 1), 2), np.float32)
    b = np.asarray(begin if begin else (0,), np.int32)
    v = (_lib.EmapPolygonVerdict * max(1, n))()
    e = np.full(2 * 64 * max(1, n), 7, np.int32)
    eb = np.asarray(ext_begin if ext_begin else (0,), np.int64)
    rc = lib.emap_polygon_safety(ctx, pts.ctypes.data_as(ct.POINTER(ct.c_float)) if xy else None,
                                 b.ctypes.data_as(ct.POINTER(ct.c_int32)) if begin else None, n, 0.0, 0.0, kind, index, 0.5,
                                 v if verdicts else None, e.ctypes.data_as(ct.POINTER(ct.c_int32)) if ext else None,
                                 eb.ctypes.data_as(ct.POINTER(ct.c_int64)) if ext_begin else None)
    assert rc == 0 or ((e == 7).all() and not any(x.n_inside or x.flags for x in v))      # a refused call writes nothing
    return rc


def test_every_refusal_returns_an_error_without_a_device():
    """no context exists without a device, so each of these is refused at the latest by the null context: the point is that none of them
    reaches a HIP call (which would fail differently, or crash, on a machine without a device) and none writes to the outputs"""
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    bad = -1      # EMAP_ERR_INVALID
    assert _call(lib) == bad                                              # null context
    assert _call(lib, xy=False) == bad and _call(lib, begin=None) == bad and _call(lib, verdicts=False) == bad      # null pointers
    assert _call(lib, ext=False) == bad and _call(lib, ext_begin=None) == bad
    assert _call(lib, n=0) == bad and _call(lib, n=-3) == bad and _call(lib, n=_lib.POLY_MAX_BATCH + 1, begin=tuple(range(_lib.POLY_MAX_BATCH + 2)),
                                                                         ext_begin=(0,) * (_lib.POLY_MAX_BATCH + 2)) == bad
    assert _call(lib, begin=(0, 0)) == bad                                # a polygon without a vertex
    assert _call(lib, begin=(0, _lib.POLY_MAX_VERTS + 1)) == bad          # too many vertices
    assert _call(lib, n=2, begin=(0, 4, 2), ext_begin=(0, 64, 128)) == bad      # vertex_begin not increasing
    assert _call(lib, kind=2) == bad and _call(lib, kind=4) == bad and _call(lib, kind=-1) == bad      # unknown layer kinds
    assert _call(lib, kind=0, index=7) == bad and _call(lib, kind=0, index=-1) == bad and _call(lib, kind=1, index=0) == bad and _call(lib, kind=3, index=0) == bad


def test_the_entry_point_settles_and_is_documented():
    src = open(os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc", "emap_api_polysafe.hip")).read()
    body = src[src.index("int emap_polygon_safety("):]
    assert "SF_CHECK()" in body and body.index("single-strip contexts only") < body.index("SF_CHECK()") < body.index("hipSetDevice")
    assert "hipMalloc" not in src                                         # the context owns the scratch
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert doc.count("`emap_polygon_safety`") >= 2                        # both tables
