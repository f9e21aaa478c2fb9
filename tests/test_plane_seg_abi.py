"""CPU: the C ABI of the plane segmentation on the device (emap_plane_segmentation, include/emap_hip.h) as far as a machine without a
device goes: declared once, exported and bound; the two structs of the binding have the header's fields, sizes and offsets (the
header compiled as C is the witness); null and out-of-range arguments are refused before any device is touched and nothing is
written; every refusal comes before the settle door; the context owns the buffers; the launchers are declared once and defined
once; the version stays 3.  With a context the GPU tests (tests/test_hip_plane_seg.py) read the reason of each refusal."""
import ctypes as ct
import os
import re
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "emap_hip.h")
CSRC = os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc")
LAUNCHERS = ("launch_ps_source", "launch_ps_window", "launch_ps_morph", "launch_ps_labels", "launch_ps_moments", "launch_ps_planes")


def test_the_entry_point_is_declared_exported_and_bound():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    assert "emap_plane_segmentation" in _lib.SYMBOLS and hasattr(lib, "emap_plane_segmentation")
    assert len(lib.emap_plane_segmentation.argtypes) == 9
    hdr = open(HEADER).read()
    assert len(re.findall(r"\bint emap_plane_segmentation\(", hdr)) == 1
    assert re.search(r"\bint emap_plane_segmentation\(emap_ctx\* ctx, const emap_grid_layer_ex\* source, const emap_plane_params\* params, int32_t\* host_labels,\s*"
                     r"float\* host_normals, emap_plane_record\* host_planes, int64_t capacity_planes, int32_t\* n_labels,\s*int64_t\* n_planes\);", hdr)
    for site in ("SlidingWindowPlaneExtractor.cpp:49-77", ":115-144", ":147-150", ":165-199", ":277-300"):      # the reference sites
        assert site in hdr, site
    assert "emap_publish_point_cloud" in _lib.SYMBOLS and "emap_publish_grid_map_ex" in _lib.SYMBOLS      # the other doors stay
    assert lib.emap_abi_version() == 3 and _lib.ABI_VERSION == 3                                          # additive: the version stays


def test_the_header_still_compiles_as_c():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", HEADER])


def _flat_names(cls):
    return [f[0] for f in cls._fields_]


def test_the_structs_have_the_headers_layout():
    from elevation_mapping_cupy_amd import _lib
    hdr = open(HEADER).read()
    lines = []
    for cname, cls in (("emap_plane_params", _lib.EmapPlaneParams), ("emap_plane_record", _lib.EmapPlaneRecord)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        declared = [re.sub(r"\[\d+\]", "", f.strip()) for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
        assert declared == _flat_names(cls), cname
        lines.append('printf("%%zu", sizeof(%s));' % cname)
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in _flat_names(cls)]
        lines.append('printf("\\n");')
    lines.append('printf("%d %d\\n", EMAP_PLANE_OPEN_MAX, EMAP_ABI_VERSION);')
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write('#include "emap_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    for row, cls, size in ((out[0], _lib.EmapPlaneParams, 96), (out[1], _lib.EmapPlaneRecord, 64)):
        assert [int(x) for x in row.split()] == [ct.sizeof(cls)] + [getattr(cls, n).offset for n in _flat_names(cls)] and ct.sizeof(cls) == size
    assert [int(x) for x in out[2].split()] == [_lib.PLANE_OPEN_MAX, _lib.ABI_VERSION] == [8, 3]
    dt = _lib.PLANE_RECORD_DTYPE                                               # the NumPy view of a record is the struct
    assert dt.itemsize == 64 and [dt.fields[n][1] for n in dt.names] == [getattr(_lib.EmapPlaneRecord, n).offset for n in dt.names]
    from elevation_mapping_cupy_amd import plane_segmentation as ps
    assert ps.PLANE_DTYPE == dt


def _call(lib, null=(), capacity=4, **over):
    from elevation_mapping_cupy_amd import _lib
    src = _lib.EmapGridLayerEx(0, 0, 0, 0)
    vals = dict(kernel_size=3, planarity_opening_filter=0, min_number_points_per_label=4, connectivity=4, use_only_above_for_upper_bound=0, reserved=0,
                center_z=0.0, reserved_f=0.0, resolution=0.04, origin_x=0.0, origin_y=0.0, plane_patch_error_threshold=0.02, cos_local_plane_inclination=0.8,
                cos_plane_inclination=0.85, global_plane_fit_distance_error_threshold=0.025, cos_global_plane_fit_angle=0.9)
    vals.update(over)
    P = _lib.EmapPlaneParams(**vals)
    labels, normals, rec = np.full(64, -7, np.int32), np.full(192, -7.0, np.float32), np.full(64 * 5, 0xA5, np.uint8)
    n_labels, n_planes = ct.c_int32(-7), ct.c_int64(-7)
    rc = lib.emap_plane_segmentation(None, None if "source" in null else ct.byref(src), None if "params" in null else ct.byref(P),
                                     None if "labels" in null else labels.ctypes.data_as(ct.POINTER(ct.c_int32)), normals.ctypes.data_as(ct.POINTER(ct.c_float)),
                                     None if "planes" in null else rec.ctypes.data_as(ct.POINTER(_lib.EmapPlaneRecord)), capacity,
                                     None if "n_labels" in null else ct.byref(n_labels), None if "n_planes" in null else ct.byref(n_planes))
    assert (labels == -7).all() and (normals == -7.0).all() and (rec == 0xA5).all() and n_labels.value == -7 and n_planes.value == -7      # a refused call writes nothing
    return rc


def test_null_and_out_of_range_arguments_are_refused_without_a_device():
    """no context exists without a device, so each of these is refused at the latest by the null context: the point is that none of them
    reaches a HIP call (which would fail differently, or crash, on a machine without a device) and none writes through a pointer"""
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    bad = -1      # EMAP_ERR_INVALID
    assert _call(lib) == bad                                                   # null context
    for k in ("source", "params", "labels", "planes", "n_labels", "n_planes"):
        assert _call(lib, null=(k,)) == bad, k
    for over in (dict(kernel_size=4), dict(kernel_size=9), dict(connectivity=6), dict(planarity_opening_filter=9), dict(plane_patch_error_threshold=0.0),
                 dict(global_plane_fit_distance_error_threshold=-1.0), dict(resolution=float("nan")), dict(cos_plane_inclination=2.0), dict(capacity=-1)):
        assert _call(lib, **over) == bad, over


def test_the_entry_point_refuses_first_settles_and_owns_its_buffers():
    src = open(os.path.join(CSRC, "emap_api_planeseg.hip")).read()
    body = src[src.index("int emap_plane_segmentation("):]
    assert "SF_CHECK()" in body and "FLUSH()" in body
    refusals = [m.start() for m in re.finditer(r"\bCKARG\(|check_layer_entry\(", body)]
    assert len(refusals) >= 12
    assert max(refusals) < body.index("SF_CHECK()") < body.index("hipSetDevice") < body.index("FLUSH()") < body.index("launch_ps_source(") < body.index("hipMemcpyAsync")
    for what in ("kernel_size", "connectivity", "planarity_opening_filter", "capacity_planes", "null argument", "single-strip"):
        assert what in body[:body.index("SF_CHECK()")], what
    assert "hipMalloc" not in src and "DevBuf" not in src                      # the context owns the buffers (grow)
    assert body.count("hipStreamSynchronize(") == 2                            # two waits: the counts, the results
    assert body.index("launch_cloud_scan(") < body.index("hipStreamSynchronize(") < body.index("launch_ps_moments(") < body.index("launch_ps_planes(")
    assert body.count("launch_cloud_scan(") == 2                               # the numbering and the slots: an order-fixed scan each
    destroy = open(os.path.join(CSRC, "emap_api.hip")).read()
    assert "hipFree(ctx->pseg_buf)" in destroy and "hipFree(ctx->pseg_slots)" in destroy and "hipHostFree(ctx->pseg_pin)" in destroy
    from elevation_mapping_cupy_amd.csrc import build
    assert "emap_planeseg.hip" in build.SOURCES and "emap_api_planeseg.hip" in build.SOURCES
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert doc.count("`emap_plane_segmentation`") >= 2                         # both tables


def test_the_launchers_are_declared_once_and_the_kernels_keep_their_rules():
    launch = open(os.path.join(CSRC, "emap_launch.h")).read()
    s = open(os.path.join(CSRC, "emap_planeseg.hip")).read()
    for name in LAUNCHERS:
        assert launch.count("void %s(" % name) == 1 and s.count("void %s(" % name) == 1, name      # declared once, defined once
    code = "\n".join(line.split("//")[0] for line in s.splitlines())
    assert code.count("tile_load(") == 1 and code.count("tile_value(") == 1    # the source plane comes through the shared walk, once
    assert "phys_row" not in code and "phys_col" not in code and "publish_value(" not in code      # and nothing here restates it
    merge = code[code.index("void k_ps_merge("):code.index("void k_ps_flatten(")]
    assert "parent[" not in merge and merge.count("ps_union_agent(parent") == 4      # the border merge touches parent[] through the atomics alone
    agent = code[code.index("int ps_find_agent("):code.index("ps_rank(")]
    assert "__HIP_MEMORY_SCOPE_AGENT" in agent and "atomicMin(&parent[a], b)" in agent and agent.count("parent[") == 2
    flatten = code[code.index("void k_ps_flatten("):code.index("void k_ps_count(")]
    assert "root[idx] = r" in flatten and "parent[idx] =" not in flatten      # the roots go to a plane of their own
    assert "__syncthreads" not in code[code.index("void k_ps_merge("):] and "while (" not in code      # no barrier past the tile pass, no spin
    assert "atomic" not in code[code.index("ps_rank("):code.index("ps_next_group(")]      # no atomic decides a number
