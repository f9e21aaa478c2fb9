"""CPU: the C ABI of the planar regions on the device (emap_planar_regions, include/emap_hip.h) as far as a machine without a device
goes: declared once, exported and bound; the two structs of the binding have the header's fields, sizes and offsets (the header compiled
as C is the witness); null and out-of-range arguments are refused before any device is touched and nothing is written; every refusal
comes before the settle door; the context owns the buffers; the version stays 3.  With a context the GPU tests
(tests/test_hip_planar_regions.py) read the reason of each refusal."""
import ctypes as ct
import os
import re
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "emap_hip.h")
CSRC = os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc")
LAUNCHERS = ("launch_rg_images", "launch_rg_cracks", "launch_rg_trace")


def test_the_entry_point_is_declared_exported_and_bound():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    assert "emap_planar_regions" in _lib.SYMBOLS and hasattr(lib, "emap_planar_regions") and len(lib.emap_planar_regions.argtypes) == 11
    hdr = open(HEADER).read()
    assert len(re.findall(r"\bint emap_planar_regions\(", hdr)) == 1
    assert re.search(r"\bint emap_planar_regions\(emap_ctx\* ctx, const int32_t\* host_labels, int32_t side, int32_t n_labels, const emap_region_params\* params,\s*"
                     r"emap_region_ring\* host_rings, int64_t capacity_rings, int32_t\* host_vertices, int64_t capacity_vertices,\s*int64_t\* n_rings, int64_t\* n_vertices\);", hdr)
    for site in ("ContourExtraction.cpp:28-128", "Upsampling.cpp:12-68", "DESIGN.md section 23"):
        assert site in hdr, site
    assert lib.emap_abi_version() == 3 and _lib.ABI_VERSION == 3      # additive: the version stays
    assert "emap_plane_segmentation" in _lib.SYMBOLS and "emap_planar_terrain" in _lib.SYMBOLS      # the other doors of the pipeline stay


def test_the_structs_have_the_headers_layout():
    from elevation_mapping_cupy_amd import _lib
    from elevation_mapping_cupy_amd import planar_regions as pr
    hdr = open(HEADER).read()
    lines = []
    pairs = (("emap_region_params", _lib.EmapRegionParams, 16), ("emap_region_ring", _lib.EmapRegionRing, 32))
    for cname, cls, _ in pairs:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        declared = [re.sub(r"\[\d+\]", "", f.strip()) for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
        names = [f[0] for f in cls._fields_]
        assert declared == names, cname
        lines.append('printf("%%zu", sizeof(%s));' % cname)
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names]
        lines.append('printf("\\n");')
    lines.append('printf("%d %d %d %d\\n", EMAP_REGION_MARGIN_MAX, EMAP_REGION_SIDE_MAX, EMAP_REGION_RAW_SIDE_MAX, EMAP_ABI_VERSION);')
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write('#include "emap_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    for row, (_, cls, size) in zip(out, pairs):
        assert [int(x) for x in row.split()] == [ct.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_] and ct.sizeof(cls) == size
    assert [int(x) for x in out[2].split()] == [_lib.REGION_MARGIN_MAX, _lib.REGION_SIDE_MAX, _lib.REGION_RAW_SIDE_MAX, _lib.ABI_VERSION] == [pr.MARGIN_MAX, pr.SIDE_MAX, pr.RAW_SIDE_MAX, 3]
    dt = pr.RING_DTYPE                                                         # the NumPy view of a ring is the struct
    assert dt.itemsize == 32 and [dt.fields[n][1] for n in dt.names] == [getattr(_lib.EmapRegionRing, n).offset for n in dt.names]
    launch = open(os.path.join(CSRC, "emap_launch.h")).read()
    assert re.search(r"#define EM_REGION_MARGIN_MAX %d\b" % pr.MARGIN_MAX, launch)


def _call(lib, null=(), labels=True, side=4, n_labels=1, mode=0, margin_size=1, cap_r=4, cap_v=16):
    from elevation_mapping_cupy_amd import _lib
    P = _lib.EmapRegionParams(mode, margin_size)
    lab = np.zeros(side * side if side > 0 else 1, np.int32)
    rings, verts = np.full(8 * 5, 0xA5A5A5A5, np.uint32), np.full(2 * 17, 0xA5A5A5A5, np.uint32)
    n_r, n_v = ct.c_int64(-7), ct.c_int64(-7)
    rc = lib.emap_planar_regions(None, lab.ctypes.data_as(ct.POINTER(ct.c_int32)) if labels else None, side, n_labels, None if "params" in null else ct.byref(P),
                                 None if "rings" in null else rings.ctypes.data_as(ct.POINTER(_lib.EmapRegionRing)), cap_r,
                                 None if "vertices" in null else verts.ctypes.data_as(ct.POINTER(ct.c_int32)), cap_v,
                                 None if "n_rings" in null else ct.byref(n_r), None if "n_vertices" in null else ct.byref(n_v))
    assert (rings == 0xA5A5A5A5).all() and (verts == 0xA5A5A5A5).all() and n_r.value == -7 and n_v.value == -7      # a refused call writes nothing
    return rc


def test_null_and_out_of_range_arguments_are_refused_without_a_device():
    """no context exists without a device, so each of these is refused at the latest by the null context: none reaches a HIP call and
    none writes through a pointer"""
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    bad = -1      # EMAP_ERR_INVALID
    assert _call(lib) == bad
    for k in ("params", "rings", "vertices", "n_rings", "n_vertices"):
        assert _call(lib, null=(k,)) == bad, k
    for over in (dict(mode=2), dict(mode=-1), dict(margin_size=15), dict(margin_size=-1), dict(side=1), dict(side=0), dict(labels=False), dict(n_labels=-1),
                 dict(cap_r=-1), dict(cap_v=-1), dict(labels=False, mode=1)):
        assert _call(lib, **over) == bad, over


def test_the_entry_point_refuses_first_settles_and_owns_its_buffers():
    src = open(os.path.join(CSRC, "emap_api_regions.hip")).read()
    body = src[src.index("int emap_planar_regions("):]
    refusals = [m.start() for m in re.finditer(r"\bCKARG\(", body)]
    assert len(refusals) >= 12 and max(refusals) < body.index("SF_CHECK()") < body.index("hipSetDevice") < body.index("hipMemcpyAsync") < body.index("launch_rg_images(")
    for what in ("mode must be", "margin_size", "single-strip", "no valid resident labels", "at least 2 x 2", "too large", "capacity", "only 0 and 1"):
        assert what in body[:body.index("SF_CHECK()")], what
    assert "hipMalloc" not in src and "DevBuf" not in src                      # the context owns the buffers (grow)
    assert body.count("hipStreamSynchronize(") == 3                            # three waits: the cracks, the counts, the answer
    assert body.count("launch_ps_components(") == 2 and "launch_cloud_scan(" in body      # the segmentation's union-find and the cloud's scan, not copies
    destroy = open(os.path.join(CSRC, "emap_api.hip")).read()
    assert "hipFree(ctx->reg_buf)" in destroy and "hipFree(ctx->reg_cracks)" in destroy and "hipHostFree(ctx->reg_pin)" in destroy
    assert destroy.count("ctx->pseg_labels = nullptr") == 2                    # emap_clear and emap_shift take the mark off the resident labels
    seg = open(os.path.join(CSRC, "emap_api_planeseg.hip")).read()
    assert seg.index("ctx->pseg_labels = nullptr") < seg.index("grow(ctx, &ctx->pseg_buf") and "ctx->pseg_labels = B.parent" in seg
    from elevation_mapping_cupy_amd.csrc import build
    assert "emap_regions.hip" in build.SOURCES and "emap_api_regions.hip" in build.SOURCES
    assert "emap_regions.hip" in open(os.path.join(ROOT, "tools", "kernel_resources.py")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert doc.count("`emap_planar_regions`") >= 2                             # both tables


def test_the_launchers_are_declared_once_and_the_kernels_keep_their_rules():
    launch = open(os.path.join(CSRC, "emap_launch.h")).read()
    s = open(os.path.join(CSRC, "emap_regions.hip")).read()
    for name in LAUNCHERS:
        assert launch.count("void %s(" % name) == 1 and s.count("void %s(" % name) == 1, name
    code = "\n".join(line.split("//")[0] for line in s.splitlines())
    for name in ("k_ps_local", "k_ps_merge", "k_ps_flatten", "ps_union", "ps_find", "atomicAdd", "atomicMin", "atomicMax", "asm"):
        assert name not in code, name                          # the union-find is reused through its launchers; no atomic decides a position
    assert code.count("atomicOr(") == 1 and "launch_ps_link(" in code and "launch_cloud_scan(" in code      # the fallback flag: idempotent
    walk = code[code.index("void k_rg_vertex("):code.index("void k_rg_flatten(")]
    assert "for (int e = 0; e < 3; ++e)" in walk and "while" not in walk      # a crack looks at most 3 cracks back: no lane walks a border
    assert "__syncthreads" not in code[:code.index("void k_rg_scan(")]
