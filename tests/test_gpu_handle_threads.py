"""Handles of one context on several threads: tests/handles_threads_check.py runs ONCE as a child process under a time
limit -- a deadlock ends there, and nothing else of this module is started after a child that did not finish -- and the tests below
read the lines it printed: three threads at the C ABI, each with its own handle, stream and error text; three threads of the drop-in
module keeping frames from the process-wide pool of page-locked buffers; the borrow guard of one object under a poll from a second
thread."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

LIMIT_S = 240
_RUN = {}                                              # the child's outcome: it runs once, whatever becomes of it


def _child():
    if not _RUN:
        _RUN["rc"], _RUN["out"] = None, ""
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "handles_threads_check.py")], capture_output=True, text=True, timeout=LIMIT_S)
            _RUN["rc"], _RUN["out"] = r.returncode, r.stdout + r.stderr
        except subprocess.TimeoutExpired as e:
            out = e.stdout or b""
            _RUN["rc"], _RUN["out"] = "timeout", out.decode(errors="replace") if isinstance(out, bytes) else str(out)
        print(_RUN["out"])
    # 0: all checks passed, 1: some check failed (the tests below say which); anything else: the child did not finish
    assert _RUN["rc"] in (0, 1), f"handles_threads_check.py did not finish (exit {_RUN['rc']}); nothing else of this module is started:\n{_RUN['out'][-3000:]}"
    return _RUN["out"]


@pytest.fixture
def checks(_built):
    out = _child()
    found = {}
    for line in out.splitlines():
        f = line.split(None, 3)
        if len(f) >= 3 and f[0] == "CHECK":
            found[f[1]] = (f[2], f[3] if len(f) > 3 else "")
    return found


def _passed(checks, name):
    assert name in checks, f"the child printed no line for {name}: {sorted(checks)}"
    verdict, text = checks[name]
    print(name, verdict, text)
    assert verdict == "OK", f"{name}: {text}"
    return text


def test_three_threads_at_the_c_abi_draw_their_own_frames(checks):
    _passed(checks, "abi_frames")


def test_three_threads_at_the_c_abi_read_their_own_error_text(checks):
    _passed(checks, "abi_error_text")


def test_three_threads_of_the_module_keep_frames_from_the_pinned_pool(checks):
    _passed(checks, "pool_frames")


def test_a_method_entered_while_another_thread_renders_raises_already_borrowed(checks):
    text = _passed(checks, "borrow_guard")
    assert "vacuous" not in text


def test_the_polled_batch_drew_the_right_frames(checks):
    _passed(checks, "borrow_frames")
