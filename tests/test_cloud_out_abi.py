"""CPU: the C ABI of the point-cloud output on the device (emap_publish_point_cloud, include/emap_hip.h) as far as a machine without a
device goes: declared, exported and bound; the field struct of the binding has the header's fields, size and offsets (the header
compiled as C is the witness); null arguments are refused before any device is touched; every refusal comes before the settle door;
the version stays 3.  With a context the GPU tests (tests/test_hip_cloud_out.py) read the reason of each refusal."""
import ctypes as ct
import os
import re
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "emap_hip.h")
CSRC = os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc")
POISON = 0xA5


def test_the_entry_point_is_declared_exported_and_bound():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    assert "emap_publish_point_cloud" in _lib.SYMBOLS and hasattr(lib, "emap_publish_point_cloud")
    assert len(lib.emap_publish_point_cloud.argtypes) == 13
    hdr = open(HEADER).read()
    assert len(re.findall(r"\bint emap_publish_point_cloud\(", hdr)) == 1                           # declared once
    assert re.search(r"\bint emap_publish_point_cloud\(emap_ctx\* ctx, const emap_cloud_field\* fields, int32_t n_fields, float center_z,\s*"
                     r"int32_t use_only_above_for_upper_bound, const float\* x_of_i, const float\* y_of_j, double normal_min,\s*"
                     r"int32_t call_flags, uint8_t\* host_out, int64_t capacity_points, int64_t\* n_points, int32_t\* point_step\);", hdr)
    assert "elevation_mapping_ros.cpp:501-505" in hdr and ":751-809" in hdr                          # the reference sites
    assert "emap_publish_grid_windows" in _lib.SYMBOLS and "emap_publish_grid_map_ex" in _lib.SYMBOLS      # the other doors stay
    assert lib.emap_abi_version() == 3 and _lib.ABI_VERSION == 3                                     # additive: the version stays


def test_the_header_still_compiles_as_c():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", HEADER])


def test_the_field_struct_and_the_flags_have_the_headers_values():
    from elevation_mapping_cupy_amd import _lib
    cname, cls = "emap_cloud_field", _lib.EmapCloudField
    names = [f[0] for f in cls._fields_]
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), open(HEADER).read(), flags=re.S).group(1)
    assert names == [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    lines = ['printf("%%zu", sizeof(%s));' % cname] + ['printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names]
    lines.append('printf("\\n%d %d %d %d %d %d %d\\n", EMAP_CLOUD_POINT, EMAP_CLOUD_TEST, EMAP_CLOUD_HIDDEN, EMAP_CLOUD_NORMAL_MIN, EMAP_CLOUD_INDEX, EMAP_GRID_MAX_LAYERS, EMAP_ABI_VERSION);')
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write('#include "emap_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert [int(x) for x in out[0].split()] == [ct.sizeof(cls)] + [getattr(cls, n).offset for n in names] == [16, 0, 4, 8, 12]
    assert [int(x) for x in out[1].split()] == [_lib.CLOUD_POINT, _lib.CLOUD_TEST, _lib.CLOUD_HIDDEN, _lib.CLOUD_NORMAL_MIN, _lib.CLOUD_INDEX,
                                                _lib.GRID_MAX_LAYERS, _lib.ABI_VERSION] == [1, 2, 4, 8, 16, 32, 3]


def _call(lib, fields=True, xs=True, ys=True, out=True, n_out=True, step_out=True, n_fields=1, capacity=4):
    from elevation_mapping_cupy_amd import _lib
    table = (_lib.EmapCloudField * 1)()
    table[0].cloud_flags = _lib.CLOUD_POINT
    pos = np.zeros(8, np.float32)
    buf = np.full(64, POISON, np.uint8)
    n, step = ct.c_int64(-7), ct.c_int32(-7)
    rc = lib.emap_publish_point_cloud(None, table if fields else None, n_fields, 0.0, 0, _lib.f32p(pos) if xs else None, _lib.f32p(pos) if ys else None, 0.1, 0,
                                      buf.ctypes.data_as(ct.POINTER(ct.c_uint8)) if out else None, capacity, ct.byref(n) if n_out else None,
                                      ct.byref(step) if step_out else None)
    assert (buf == POISON).all() and n.value == -7 and step.value == -7           # a refused call writes nothing
    return rc


def test_null_arguments_are_refused_without_a_device():
    """no context exists without a device, so each of these is refused at the latest by the null context: the point is that none of them
    reaches a HIP call (which would fail differently, or crash, on a machine without a device) and none writes through a pointer"""
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    bad = -1      # EMAP_ERR_INVALID
    assert _call(lib) == bad                                                   # null context
    for k in ("fields", "xs", "ys", "out", "n_out", "step_out"):
        assert _call(lib, **{k: False}) == bad, k
    assert _call(lib, n_fields=0) == bad and _call(lib, n_fields=_lib.GRID_MAX_LAYERS + 1) == bad and _call(lib, capacity=-1) == bad


def test_the_entry_point_refuses_first_settles_and_owns_its_buffers():
    src = open(os.path.join(CSRC, "emap_api_cloudout.hip")).read()
    body = src[src.index("int emap_publish_point_cloud("):]
    assert "SF_CHECK()" in body and "FLUSH()" in body
    last_refusal = max(m.start() for m in re.finditer(r"\bCKARG\(", body))
    assert last_refusal < body.index("SF_CHECK()") < body.index("hipSetDevice") < body.index("FLUSH()") < body.index("hipMemcpyAsync")
    assert "hipMalloc" not in src                                              # the context owns the buffers (grow)
    # one upload, three launches, the count's copy and a wait, the records' copy and a second wait
    assert body.count("hipMemcpyAsync(") == 3 and body.count("hipStreamSynchronize(") == 2
    assert body.count("launch_cloud_count(") == 1 and body.count("launch_cloud_scan(") == 1 and body.count("launch_cloud_write(") == 1
    destroy = open(os.path.join(CSRC, "emap_api.hip")).read()
    assert "hipFree(ctx->cloud_tab)" in destroy and "hipFree(ctx->cloud_out)" in destroy and "hipHostFree(ctx->cloud_pin)" in destroy
    from elevation_mapping_cupy_amd.csrc import build
    assert "emap_cloudout.hip" in build.SOURCES and "emap_api_cloudout.hip" in build.SOURCES
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert doc.count("`emap_publish_point_cloud`") >= 2                        # both tables


def test_one_definition_of_the_values_and_no_atomic():
    dev = open(os.path.join(CSRC, "emap_device.h")).read()
    assert dev.count("float normal_color(") == 1 and dev.count("float publish_value(") == 1
    s = open(os.path.join(CSRC, "emap_cloudout.hip")).read()
    assert "float normal_color(" not in s and "float publish_value(" not in s
    walk = open(os.path.join(CSRC, "emap_publish_tile.h")).read()
    assert walk.count("normal_color(q.nrm[0][k], q.nrm[1][k], q.nrm[2][k])") == 1 and walk.count("publish_value(index, m, q.rr[k], q.c, C") == 1      # one walk ...
    for door in (s, open(os.path.join(CSRC, "emap_gridmsg.hip")).read(), open(os.path.join(CSRC, "emap_submap.hip")).read()):
        assert "normal_color(" not in door and "publish_value(" not in door      # ... that no door restates
    assert s.count("tile_value(A.tab, l, q, C, v)") == 2                       # and both kernels call
    code = "\n".join(line.split("//")[0] for line in s.splitlines())
    assert "atomic" not in code                                                # no atomic decides a position
    launch = open(os.path.join(CSRC, "emap_launch.h")).read()
    for name in ("launch_cloud_count", "launch_cloud_scan", "launch_cloud_write"):
        assert launch.count("void %s(" % name) == 1 and s.count("void %s(" % name) == 1      # declared once, defined once
