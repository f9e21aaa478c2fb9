"""What the kernel-variant tests share (tests/test_hip_post_variants.py, test_hip_ray_variants.py, test_hip_bin_variants.py and their child
programs _post_variants.py, _ray_variants.py, _bin_variants.py): a launcher's hooks are read once per process, so one process is one
variant, and this module is the one place that starts such a process, judges how it ended and decides whether another may follow.

A child that ran into its time limit, was ended by a signal, exited with an error or named a HIP error on stderr (BadExit) may have
left the device in a state in which the next one does the same: after it NO further child is started by any user of this module in
this pytest process (HALT), whichever test file asks.  A child that merely computed wrong values stops nothing.

Imports nothing of the project at module level: the child programs import it too (child_setup)."""
import os
import re
import shutil
import signal
import subprocess
import sys
import time

import numpy as np

HIP_ERROR = re.compile(r"hipError|HIP error|HSA_STATUS_ERROR|illegal memory access|Memory access fault|GPU core dump", re.I)
FLAG = {"true": "true", "false": "false", "(bool)1": "true", "(bool)0": "false", "1": "true", "0": "false"}


class BadExit(Exception):
    """a child that ran into its time limit, was ended by a signal, exited with an error or reported a HIP error"""


class Halt:
    """the stop rule's state: the message of the first child that ended badly, None as long as none did"""
    message = None


HALT = Halt()                      # of this pytest process, shared by every test file


def run_child(script, variant, env, drop, tmp, limit_s, tracer="rocprofv3"):
    """`python <script> <tmp>/out.npz` as one child process: the inherited environment without the hook variables `drop` names (a
    collection of names or a predicate) plus `env`, under `rocprofv3 --kernel-trace -d <tmp>/trace --` (tracer=None: bare; a list: that
    prefix), in a session of its own, killed as a group at the time limit.  Returns (the arrays of out.npz, the trace directory)."""
    dropped = drop if callable(drop) else (lambda k: k in drop)
    full = {k: v for k, v in os.environ.items() if not dropped(k)}
    full.update(env)
    out, trace = os.path.join(tmp, "out.npz"), os.path.join(tmp, "trace")
    if tracer == "rocprofv3":
        prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        assert os.path.exists(prof), "rocprofv3 not found: the kernel selection cannot be verified"
        tracer = [prof, "--kernel-trace", "-d", trace, "--"]
    cmd = list(tracer or []) + [sys.executable, script, out]
    t0 = time.time()
    p = subprocess.Popen(cmd, env=full, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, start_new_session=True)
    try:
        _, err = p.communicate(timeout=limit_s)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        _, err = p.communicate()
        raise BadExit("variant %s: the child ran into its time limit of %d s; stderr ends:\n%s" % (variant, limit_s, err.decode(errors="replace")[-3000:]))
    print("variant %s: child took %.1f s" % (variant, time.time() - t0))
    err = err.decode(errors="replace")
    if p.returncode != 0:
        raise BadExit("variant %s: the child exited with %d; stderr ends:\n%s" % (variant, p.returncode, err[-3000:]))
    if HIP_ERROR.search(err):
        raise BadExit("variant %s: the child's stderr names a HIP error:\n%s" % (variant, err[-3000:]))
    with np.load(out) as z:
        return {k: z[k] for k in z.files}, trace


def lazy_children(run, halt=HALT):
    """variant -> run(variant): one child per variant, started the first time a test needs it, never twice; a child that failed fails
    every test of its variant with the same message.  After a BadExit no further child is started through `halt`: every test that
    still needs one fails with that first message."""
    import pytest
    done = {}

    def get(variant):
        if variant not in done:
            if halt.message is not None:
                pytest.fail("not started: an earlier child ended badly -- %s" % halt.message, pytrace=False)
            try:
                done[variant] = run(variant)
            except BadExit as e:
                halt.message = str(e)
                done[variant] = e
            except Exception as e:          # remembered, not retried
                done[variant] = e
        if isinstance(done[variant], Exception):
            pytest.fail("%s" % done[variant], pytrace=False)
        return done[variant]

    return get


def cached_oracle(compute):
    """key -> compute(key), computed once with eight oracle threads and left unchanged"""
    done = {}

    def get(key):
        if key not in done:
            from oracle import emap_oracle as eo
            eo.set_threads(8)
            try:
                done[key] = compute(key)
            finally:
                eo.set_threads(1)
        return done[key]

    return get


def canonical_kernel_name(name, types):
    """a traced dispatch name with its template arguments in one spelling (booleans as false / true), None for a kernel `types` does
    not name.  `types`: kernel -> one letter per template argument, i = integer, b = boolean ("" = no template: the bare name)."""
    for k in types:
        if not types[k] and re.search(r"\b%s\b" % k, name):
            return k
    m = re.search(r"\b(%s)<([^<>]*)>" % "|".join(k for k in types if types[k]), name)
    if not m:
        return None
    a = [x.strip() for x in m.group(2).split(",")]
    if len(a) != len(types[m.group(1)]):
        return "%s<%s>" % (m.group(1), m.group(2))
    return "%s<%s>" % (m.group(1), ", ".join(FLAG[x] if ty == "b" else str(int(x)) for x, ty in zip(a, types[m.group(1)])))


def assert_case_planes(got, key, want_map, want_normal, want_trav_in, what):
    """the three planes every child records per case, bit for bit against the oracle's"""
    from _util import assert_planes_equal
    assert_planes_equal(got[key + "_map"], want_map, what=what)
    assert_planes_equal(got[key + "_normal"], want_normal, names=["nx", "ny", "nz"], what=what)
    assert_planes_equal(got[key + "_trav_in"][None], want_trav_in[None], names=["traversability_input"], what=what)


def child_setup():
    """the start of every child's main: the repository root onto sys.path; returns the weights of tests/golden/weights.npz"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    w = np.load(os.path.join(root, "tests", "golden", "weights.npz"))
    return {k: w[k] for k in ("w1", "w2", "w3", "w_out")}
