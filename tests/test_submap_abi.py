"""CPU: the C ABI of the submap service on the device (emap_publish_grid_windows, include/emap_hip.h) as far as a machine without a device
goes: declared, exported and bound; the window struct of the binding has the header's fields, size and offsets (the header compiled as
C is the witness); null arguments are refused before any device is touched; the version stays 3.  With a context the GPU tests
(tests/test_hip_submap.py) read the reason of each refusal."""
import ctypes as ct
import os
import re
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "emap_hip.h")
POISON = 0xA5A5A5A5


def test_the_entry_point_is_declared_exported_and_bound():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    assert "emap_publish_grid_windows" in _lib.SYMBOLS and hasattr(lib, "emap_publish_grid_windows")
    assert len(lib.emap_publish_grid_windows.argtypes) == 10
    hdr = open(HEADER).read()
    assert len(re.findall(r"\bint emap_publish_grid_windows\(", hdr)) == 1                          # declared once
    assert re.search(r"\bint emap_publish_grid_windows\(emap_ctx\* ctx, const emap_grid_layer_ex\* layers, int32_t n_layers, int32_t order,\s*"
                     r"float center_z, int32_t use_only_above_for_upper_bound, const emap_grid_window\* windows, int32_t n_windows,\s*"
                     r"float\* host_out, int64_t host_floats\);", hdr)
    assert "elevation_mapping_ros.cpp:507-553" in hdr                                                # the reference site
    assert "emap_publish_grid_map_ex" in _lib.SYMBOLS                                                # the whole-map door stays
    assert lib.emap_abi_version() == 3 and _lib.ABI_VERSION == 3                                     # additive: the version stays


def test_the_header_still_compiles_as_c():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", HEADER])


def test_the_window_struct_and_the_cap_have_the_headers_values():
    from elevation_mapping_cupy_amd import _lib
    cname, cls = "emap_grid_window", _lib.EmapGridWindow
    names = [f[0] for f in cls._fields_]
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), open(HEADER).read(), flags=re.S).group(1)
    assert names == [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    lines = ['printf("%%zu", sizeof(%s));' % cname] + ['printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names]
    lines.append('printf("\\n%d %d\\n", EMAP_GRID_MAX_WINDOWS, EMAP_ABI_VERSION);')
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write('#include "emap_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert [int(x) for x in out[0].split()] == [ct.sizeof(cls)] + [getattr(cls, n).offset for n in names] == [16, 0, 4, 8, 12]
    assert [int(x) for x in out[1].split()] == [_lib.GRID_MAX_WINDOWS, _lib.ABI_VERSION] == [64, 3]


def _call(lib, layers=True, windows=True, out=True, n_layers=1, n_windows=1):
    from elevation_mapping_cupy_amd import _lib
    table = (_lib.EmapGridLayerEx * 1)()
    wins = (_lib.EmapGridWindow * 1)()
    wins[0].ni = wins[0].nj = 2
    buf = np.full(4, POISON, np.uint32).view(np.float32)
    rc = lib.emap_publish_grid_windows(None, table if layers else None, n_layers, 0, 0.0, 0, wins if windows else None, n_windows,
                                       _lib.f32p(buf) if out else None, 4)
    assert (buf.view(np.uint32) == POISON).all()                               # a refused call writes nothing
    return rc


def test_null_arguments_are_refused_without_a_device():
    """no context exists without a device, so each of these is refused at the latest by the null context: the point is that none of them
    reaches a HIP call (which would fail differently, or crash, on a machine without a device) and none writes to host_out"""
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    bad = -1      # EMAP_ERR_INVALID
    assert _call(lib) == bad                                                   # null context
    assert _call(lib, layers=False) == bad and _call(lib, windows=False) == bad and _call(lib, out=False) == bad
    assert _call(lib, n_layers=0) == bad and _call(lib, n_windows=0) == bad and _call(lib, n_windows=_lib.GRID_MAX_WINDOWS + 1) == bad


def test_the_entry_point_refuses_first_settles_and_owns_its_buffers():
    src = open(os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc", "emap_api_submap.hip")).read()
    body = src[src.index("int emap_publish_grid_windows("):]
    assert "SF_CHECK()" in body and "FLUSH()" in body
    last_refusal = max(m.start() for m in re.finditer(r"\bCKARG\(", body))
    assert last_refusal < body.index("SF_CHECK()") < body.index("hipSetDevice") < body.index("FLUSH()") < body.index("hipMemcpyAsync")
    assert "hipMalloc" not in src                                              # the context owns the buffers (grow)
    assert body.count("hipMemcpyAsync(") == 2 and body.count("hipStreamSynchronize(") == 1 and body.count("launch_grid_windows(") == 1
    destroy = open(os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc", "emap_api.hip")).read()
    assert "hipFree(ctx->sub_tab)" in destroy and "hipFree(ctx->sub_out)" in destroy and "hipHostFree(ctx->sub_pin)" in destroy
    from elevation_mapping_cupy_amd.csrc import build
    assert "emap_submap.hip" in build.SOURCES and "emap_api_submap.hip" in build.SOURCES
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert doc.count("`emap_publish_grid_windows`") >= 2                       # both tables


def test_one_definition_of_the_values_for_both_kernels():
    csrc = os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc")
    dev = open(os.path.join(csrc, "emap_device.h")).read()
    assert dev.count("float normal_color(") == 1 and dev.count("float publish_value(") == 1
    walk = open(os.path.join(csrc, "emap_publish_tile.h")).read()             # the one walk of the layer table: both kernels run its grid_tile
    assert walk.count("normal_color(q.nrm[0][k]") == 1 and walk.count("publish_value(index, m, q.rr[k], q.c, C") == 1 and "float normal_color(" not in walk
    for f in ("emap_gridmsg.hip", "emap_submap.hip"):
        s = open(os.path.join(csrc, f)).read()
        assert "normal_color(" not in s and "publish_value(" not in s and s.count("publish_tile::grid_tile<ORDER>(") == 1, f
