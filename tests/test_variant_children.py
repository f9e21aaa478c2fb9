"""CPU: the child runner, the stop rule and the small parts of tests/_variant_children.py, on tiny Python children written into tmp_path
(no GPU, no tracer, nothing of the project imported by a child).  Every case has a halt object of its own."""
import os
import time

import numpy as np
import pytest

import _variant_children as vc

GOOD = "import sys, numpy as np\nnp.savez(sys.argv[1], a=np.arange(5), b=np.float32([1.5]))\n"
BAD = {          # name -> (program, time limit in s, what its message must hold)
    "status3": ("import sys\nsys.stderr.write('tail of the log\\n')\nsys.exit(3)\n", 60, ["exited with 3", "tail of the log"]),
    "hip_error": ("import sys\nsys.stderr.write('x: hipErrorIllegalAddress y\\n')\n", 60, ["names a HIP error", "hipErrorIllegalAddress"]),
    "sleeper": ("import os, sys, time\nopen(os.environ['PID_FILE'], 'w').write(str(os.getpid()))\ntime.sleep(30)\n", 1, ["time limit of 1 s"]),
}


def _script(tmp_path, name, text):
    p = tmp_path / (name + ".py")
    p.write_text(text)
    return str(p)


def _run(tmp_path, name, text, limit_s=60, env=None):
    d = tmp_path / ("run_" + name)
    d.mkdir()
    return vc.run_child(_script(tmp_path, name, text), name, env or {}, ("DROPPED_HOOK",), str(d), limit_s, tracer=None)


def test_a_good_child_returns_its_arrays(tmp_path, monkeypatch):
    monkeypatch.setenv("DROPPED_HOOK", "1")
    monkeypatch.setenv("KEPT", "2")
    text = GOOD + "import os\nassert 'DROPPED_HOOK' not in os.environ and os.environ['KEPT'] == '2' and os.environ['ADDED'] == '3'\n"
    arrays, trace = _run(tmp_path, "good", text, env={"ADDED": "3"})
    assert sorted(arrays) == ["a", "b"] and list(arrays["a"]) == [0, 1, 2, 3, 4] and arrays["b"][0] == np.float32(1.5)
    assert trace == str(tmp_path / "run_good" / "trace")


def test_the_hooks_to_drop_may_be_a_predicate(tmp_path, monkeypatch):
    monkeypatch.setenv("HOOK_A", "1")
    d = tmp_path / "d"
    d.mkdir()
    script = _script(tmp_path, "pred", GOOD + "import os\nassert 'HOOK_A' not in os.environ\n")
    vc.run_child(script, "pred", {}, lambda k: k.startswith("HOOK_"), str(d), 60, tracer=None)


@pytest.mark.parametrize("name", list(BAD))
def test_a_bad_exit_is_told_apart(name, tmp_path):
    text, limit_s, holds = BAD[name]
    pid_file = tmp_path / "pid"
    t0 = time.time()
    with pytest.raises(vc.BadExit) as e:
        _run(tmp_path, name, text, limit_s, env={"PID_FILE": str(pid_file)})
    assert time.time() - t0 < 10
    assert all(h in str(e.value) for h in holds + ["variant " + name]), str(e.value)
    if name == "sleeper":
        with pytest.raises(ProcessLookupError):             # killed and reaped before the call returned
            os.kill(int(pid_file.read_text()), 0)


def _table(tmp_path, programs, halt):
    """a lazy table over `programs` (variant -> program text); every child also leaves the marker file started_<variant>"""
    def run(variant):
        mark = "import os\nopen(os.environ['MARK'], 'w').close()\n"
        text, limit_s = programs[variant]
        return _run(tmp_path, variant, mark + text, limit_s, env={"MARK": str(tmp_path / ("started_" + variant)), "PID_FILE": str(tmp_path / "pid")})
    return vc.lazy_children(run, halt)


@pytest.mark.parametrize("name", list(BAD))
def test_after_a_bad_exit_no_child_is_started(name, tmp_path):
    halt = vc.Halt()
    get = _table(tmp_path, {"bad": BAD[name][:2], "next": (GOOD, 60)}, halt)
    with pytest.raises(pytest.fail.Exception) as first:
        get("bad")
    assert (tmp_path / "started_bad").exists() and halt.message == first.value.msg and BAD[name][2][0] in halt.message
    with pytest.raises(pytest.fail.Exception) as second:
        get("next")
    assert second.value.msg == "not started: an earlier child ended badly -- " + halt.message
    assert not (tmp_path / "started_next").exists()
    (tmp_path / "started_bad").unlink()
    with pytest.raises(pytest.fail.Exception) as again:
        get("bad")
    assert again.value.msg == first.value.msg and not (tmp_path / "started_bad").exists()
    other = _table(tmp_path, {"other": (GOOD, 60)}, halt)           # another test file's table on the same halt object
    with pytest.raises(pytest.fail.Exception):
        other("other")
    assert not (tmp_path / "started_other").exists() and vc.HALT.message is None


def test_a_child_without_output_is_an_ordinary_error(tmp_path):
    halt = vc.Halt()
    get = _table(tmp_path, {"silent": ("", 60), "next": (GOOD, 60)}, halt)
    with pytest.raises(pytest.fail.Exception) as first:
        get("silent")
    assert "out.npz" in first.value.msg and halt.message is None
    (tmp_path / "started_silent").unlink()
    with pytest.raises(pytest.fail.Exception) as again:                            # remembered, not retried
        get("silent")
    assert again.value.msg == first.value.msg and not (tmp_path / "started_silent").exists()
    arrays, _ = get("next")
    assert (tmp_path / "started_next").exists() and list(arrays["a"]) == [0, 1, 2, 3, 4]
    (tmp_path / "started_next").unlink()
    assert get("next")[0] is arrays and not (tmp_path / "started_next").exists()


RAYS = {"k_rays": "ibibibi"}
BINS = {"k_bin_hist": "iib", "k_bin_scan": "", "k_tile_fuse": "bbbib"}


@pytest.mark.parametrize("t, f", [("true", "false"), ("(bool)1", "(bool)0"), ("1", "0")])
def test_canonical_kernel_name_has_one_spelling(t, f):
    name = "void k_rays<0, %s, 2, %s, 512, %s, 1>(KP) [clone .kd]" % (f, f, t)
    assert vc.canonical_kernel_name(name, RAYS) == "k_rays<0, false, 2, false, 512, true, 1>"
    name = "void k_tile_fuse<%s, %s, %s, 2, %s>(KP)" % (t, f, t, f)
    assert vc.canonical_kernel_name(name, BINS) == "k_tile_fuse<true, false, true, 2, false>"


def test_canonical_kernel_name_other_kernels_and_wrong_counts():
    assert vc.canonical_kernel_name("void k_post<4, 1>(KP)", RAYS) is None
    assert vc.canonical_kernel_name("void k_rays<0, true, 2>(KP)", BINS) is None
    assert vc.canonical_kernel_name("k_bin_scan(KP)", BINS) == "k_bin_scan"
    assert vc.canonical_kernel_name("void k_rays<0, true, 2>(KP)", RAYS) == "k_rays<0, true, 2>"
    assert vc.canonical_kernel_name("void k_bin_hist<0, 1024>(KP)", BINS) == "k_bin_hist<0, 1024>"
