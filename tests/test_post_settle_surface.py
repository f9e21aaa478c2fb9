"""CPU: the settle surface of the pending stencil pass.

emap_update may leave the last frame's stencil pass pending (emap_api.hip: frame_impl), to be launched together with the next frame's
histogram.  Every entry point of the C ABI therefore launches a pending pass before it reads, changes or waits for anything -- through
SF_CHECK() (emap_host.h: small frames in flight, then the pending pass) or a direct call of post_settle -- except the calls written
out below.  This test scans every `emap_*` definition in csrc/*.hip, so an entry point added later cannot silently skip the door."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc")

# The calls a frame is made of, and the calls that touch neither the map nor the stream: they leave a pending pass pending.
NEXT_FRAME_OR_UNTOUCHED = {
    "emap_set_points_device": "binds the next frame's cloud",
    "emap_set_points_device_split": "binds the next frame's cloud",
    "emap_frame_semantics": "declares the next frame's semantic fusion",
    "emap_update": "the frame itself: takes the pending pass into its histogram launch or launches it first (frame_impl)",
    "emap_last_error": "reads the context's message",
    "emap_last_update_path": "reads a host-side word",
    "emap_get_stage_times": "reads host-side floats",
    "emap_enable_stage_timing": "sets a host-side flag",
    "emap_timer_begin": "records the start of an interval: the pending pass belongs inside it",
}
# No context of this kind in their arguments: there is nothing to settle.
NO_MAP_CONTEXT = {
    "emap_abi_version": "no arguments",
    "emap_create": "creates the context",
    "emap_comm_unique_id": "no context",
    "emap_normal_lag_plan": "pure host arithmetic on its arguments, no context",
}

ALLOWED = dict(NEXT_FRAME_OR_UNTOUCHED, **NO_MAP_CONTEXT)
SETTLES = re.compile(r"\bSF_CHECK\(\)|\bpost_settle\(")
DEFINITION = re.compile(r"^(?:int|void|const char\*|int64_t|uint32_t) (emap_\w+)\(([^;{]*?)\)\s*\{", re.M | re.S)


def _definitions():
    """(file, name, parameter list, body) of every emap_* function defined at file scope"""
    out = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        src = open(path).read()
        for m in DEFINITION.finditer(src):
            depth, j = 0, m.end() - 1
            while True:
                depth += {"{": 1, "}": -1}.get(src[j], 0)
                if depth == 0:
                    break
                j += 1
            out.append((os.path.basename(path), m.group(1), m.group(2), src[m.end() - 1:j + 1]))
    return out


def test_every_entry_point_settles_or_is_written_out():
    defs = _definitions()
    names = [d[1] for d in defs]
    assert len(names) == len(set(names)) and len(names) >= 96, len(names)      # the 95 of the parent + emap_post_fused_launches
    missing = [(f, n) for f, n, _, body in defs if n not in ALLOWED and not SETTLES.search(body)]
    assert not missing, "entry points that neither settle the pending stencil pass nor are written out as exceptions: %r" % missing


def test_the_exceptions_exist_and_do_not_settle():
    """a stale name in the list would hide nothing but shows the list is not maintained; an exception that settles is no exception"""
    defs = {n: (args, body) for _, n, args, body in _definitions()}
    for n in ALLOWED:
        assert n in defs, n
    for n in NEXT_FRAME_OR_UNTOUCHED:
        assert not SETTLES.search(defs[n][1]), n
    for n in NO_MAP_CONTEXT:
        assert "emap_ctx* ctx" not in defs[n][0] or n == "emap_create", n


def test_the_frame_decides_about_the_pending_pass_itself():
    src = open(os.path.join(CSRC, "emap_api.hip")).read()
    body = src[src.index("static int frame_impl(emap_ctx* ctx, const float R[9], const float t[3], double position_noise, double orientation_noise, emap_stats* stats, bool sharded) {"):]
    head = body[:body.index("Frame fr;")]
    assert "SF_SETTLE_FRAMES()" in head and "SF_CHECK()" not in head
    assert "post_pending" in head and "post_settle(ctx)" in head      # frames that cannot take the pass launch it first
    assert body.index("CKARG(ctx && R && t") < body.index("post_settle(ctx)")      # arguments are checked before the pass is consumed


def test_the_new_entry_point_is_declared_and_bound():
    from elevation_mapping_cupy_amd import _lib
    assert "emap_post_fused_launches" in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "emap_hip.h")).read()
    assert re.search(r"int emap_post_fused_launches\(emap_ctx\* ctx, uint32_t\* launches\);", hdr)
