"""CPU: the C ABI of the image message input (emap_input_image_message, include/emap_hip.h) as far as a machine without a device goes:
the entry point is exported and bound, a call without a context is refused before any device is touched, and the two structs of the
binding have the header's fields, sizes and offsets (the header compiled as C is the witness)."""
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
    assert "emap_input_image_message" in _lib.SYMBOLS and hasattr(lib, "emap_input_image_message")
    assert len(lib.emap_input_image_message.argtypes) == 12
    assert re.search(r"\bint emap_input_image_message\(emap_ctx\* ctx, const emap_image_msg_desc\* desc, const uint8_t\* data,", open(HEADER).read())
    assert lib.emap_abi_version() == 3                      # additive: the version stays


def test_the_structs_have_the_headers_layout():
    from elevation_mapping_cupy_amd import _lib
    pairs = (("emap_image_msg_desc", _lib.EmapImageMsgDesc), ("emap_image_spec", _lib.EmapImageSpec))
    lines = []
    for cname, cls in pairs:
        names = [f[0] for f in cls._fields_]
        assert names == _header_fields(cname), cname
        lines.append('printf("%%zu", sizeof(%s));' % cname)
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (cname, n) for n in names]
        lines.append('printf("\\n");')
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write('#include "emap_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    for (cname, cls), line in zip(pairs, out):
        want = [ct.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_]
        assert [int(x) for x in line.split()] == want, (cname, line, want)
    assert ct.sizeof(_lib.EmapImageMsgDesc) == 28 and ct.sizeof(_lib.EmapImageSpec) == 24 and _lib.EmapImageSpec.alpha.offset == 16


def test_null_arguments_are_refused_without_touching_a_device():
    from elevation_mapping_cupy_amd import _lib
    lib = _lib.load()
    d = _lib.EmapImageMsgDesc(height=2, width=2, step=2, elem=0, n_chan=1, is_bigendian=0, swap_rb=0)
    spec = (_lib.EmapImageSpec * 1)()
    data = np.zeros(16, np.uint8)
    f = np.zeros(12, np.float32)
    fp = f.ctypes.data_as(ct.POINTER(ct.c_float))
    args = (ct.byref(d), ct.c_void_p(data.ctypes.data), 1.0, 1.0, 1.0, fp, fp, fp, fp, spec, 1)
    assert lib.emap_input_image_message(None, *args) == -1
    assert lib.emap_input_image_message(None, None, None, 0.0, 0.0, 0.0, None, None, None, None, None, 0) == -1
    assert not data.any() and not f.any()
