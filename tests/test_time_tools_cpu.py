"""No GPU: what the effect nodes' timing tools share (tools/nodetime.py).  The driver against a stub script that records its step and then exits,
sleeps or dies as told; the two timing loops against a context that records every call and answers nae_event_elapsed_ms from a script; every
tool's --help without a device or a library; and every tool's step list against the labels its docstring names."""
import importlib.util
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
NODES = "fir conv eq dyn dynkey denoise loud echo mod sat gate mb hpss lim".split()

STUB = '''import os, resource, signal, sys, time
label, do, log = sys.argv[1:4]
with open(log, "a") as f:
    f.write(f"{label} {os.getpid()}\\n")
if do == "sleep":
    time.sleep(60)
if do == "segv":
    resource.setrlimit(resource.RLIMIT_CORE, (0, 0))
    os.kill(os.getpid(), signal.SIGSEGV)
sys.exit(int(do) if do.isdigit() else 0)
'''


def load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


nodetime = load("nodetime")


def drive(tmp_path, second, limit=30):
    """three steps a, b, c of the stub, b doing what second says: drive's status and the (label, pid) pairs the stub logged"""
    stub, log = tmp_path / "stub.py", tmp_path / "log"
    stub.write_text(STUB)
    steps = [(label, [label, do]) for label, do in (("a", "0"), ("b", second), ("c", "0"))]
    rc = nodetime.drive(str(stub), steps, limit, [str(log)])
    return rc, [(line.split()[0], int(line.split()[1])) for line in log.read_text().splitlines()]


def test_drive_runs_every_step_in_order(tmp_path, capsys):
    rc, ran = drive(tmp_path, "0")
    assert rc == 0 and [label for label, _ in ran] == ["a", "b", "c"]
    assert len({pid for _, pid in ran}) == 3 and os.getpid() not in {pid for _, pid in ran}    # a fresh process each
    assert capsys.readouterr().out == ""


def test_drive_stops_at_the_first_failing_status(tmp_path, capsys):
    rc, ran = drive(tmp_path, "3")
    assert rc == 3 and [label for label, _ in ran] == ["a", "b"]
    assert capsys.readouterr().out == "b: exit status 3; stopping\n"


def test_drive_kills_and_stops_at_the_time_limit(tmp_path, capsys):
    rc, ran = drive(tmp_path, "sleep", limit=1)
    assert rc == 124 and [label for label, _ in ran] == ["a", "b"]
    with pytest.raises(ProcessLookupError):     # killed and reaped: nothing of the step is left
        os.kill(ran[1][1], 0)
    assert capsys.readouterr().out == "b: no result within 1 s; stopping\n"


def test_drive_reports_a_signal_as_the_shell_does(tmp_path, capsys):
    rc, ran = drive(tmp_path, "segv")
    assert rc == 139 and [label for label, _ in ran] == ["a", "b"]
    assert capsys.readouterr().out == "b: exit status 139; stopping\n"


def test_driver_process_does_not_import_the_binding(tmp_path):
    """a process that imports every tool and drives a step has neither naeload nor the package among its modules"""
    stub, log = tmp_path / "stub.py", tmp_path / "log"
    stub.write_text(STUB)
    code = (f"import sys, json, importlib; sys.path.insert(0, {TOOLS!r}); import nodetime\n"
            f"for n in {NODES!r}: importlib.import_module(n + '_time')\n"
            f"rc = nodetime.drive({str(stub)!r}, [('a', ['a', '0'])], 30, [{str(log)!r}])\n"
            "print(json.dumps([rc, sorted(m for m in sys.modules if 'nae' in m or 'nodey' in m)]))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.splitlines()[-1]) == [0, []]
    assert log.read_text().split()[0] == "a"


class FakeCtx:
    """records every call; nae_event_elapsed_ms answers from script, the clock probe from 2.0 upwards"""

    def __init__(self, script):
        self.calls, self.script, self.events, self.clocks = [], iter(script), 0, 0

    def event(self):
        self.events += 1
        self.calls.append("event")
        return f"e{self.events}"

    def sync(self):
        self.calls.append("sync")

    def clock_ghz(self):
        self.clocks += 1
        self.calls.append("clock")
        return 1.0 + self.clocks

    def record(self, ev):
        self.calls.append(("record", ev))

    def elapsed_ms(self, a, b):
        self.calls.append(("elapsed", a, b))
        return next(self.script)

    def destroy_event(self, ev):
        self.calls.append(("destroy", ev))


def one(tag):
    return [("record", "e1"), tag, ("record", "e2"), ("elapsed", "e1", "e2")]


@pytest.mark.parametrize("clock", (True, False))
def test_rounds_call_sequence_and_medians(clock):
    import statistics
    ctx = FakeCtx([3.0, 10.0, 1.0, 30.0, 2.0, 20.0])
    cases = [("x", "case x", lambda: ctx.calls.append("x")), ("y", "case y", lambda: ctx.calls.append("y"), "a fourth field")]
    ms, before, after = nodetime.rounds(ctx, cases, 3, 2, **({} if clock else {"clock": False}))
    probe = ["clock"] if clock else []
    assert ctx.calls == (["event", "event"] + ["x", "y"] * 2 + ["sync"] + probe + (one("x") + one("y")) * 3 + probe
                         + [("destroy", "e1"), ("destroy", "e2")])
    assert ms == {"x": [3.0, 1.0, 2.0], "y": [10.0, 30.0, 20.0]} and list(ms) == ["x", "y"]
    assert (before, after) == ((2.0, 3.0) if clock else (None, None))
    assert [statistics.median(ms[t]) for t in ms] == [2.0, 20.0]


def test_timed_call_sequence_and_median():
    ctx = FakeCtx([5.0, 1.0, 9.0, 4.0, 2.0])
    assert nodetime.timed(ctx, lambda: ctx.calls.append("f"), 5, 2) == (4.0, 1.0, 9.0)
    assert ctx.calls == ["event", "event", "f", "f", "sync"] + one("f") * 5 + [("destroy", "e1"), ("destroy", "e2")]


def test_timed_behind_call_sequence_and_median():
    ctx = FakeCtx([100.0, 200.0, 5.0, 1.0, 9.0])
    got = nodetime.timed_behind(ctx, lambda: ctx.calls.append("before"), lambda: ctx.calls.append("f"), 3, 2)
    assert got == (5.0, 1.0, 9.0)       # the warm-up rounds are timed like the rest and dropped
    assert ctx.calls == ["event", "event"] + (["before"] + one("f")) * 5 + [("destroy", "e1"), ("destroy", "e2")]


def test_setup_and_release():
    class Arr:
        def __init__(self, log, n):
            self.log, self.ptr = log, f"p{len(log)}"
            log.append(("empty", n))

        def free(self):
            self.log.append(("free", self.ptr))

    class Ctx:
        def __init__(self):
            self.log = []

        def empty(self, n):
            return Arr(self.log, n)

        def fill_uniform(self, *a):
            self.log.append(("fill",) + a)

    class Nae:
        class Sig:
            interleaved = staticmethod(lambda ptr, T, ch: ("sig", ptr, T, ch))

    ctx = Ctx()
    d_in, d_out, src, dst = nodetime.setup(Nae, ctx, 3, 100)
    assert ctx.log == [("empty", 600), ("empty", 600), ("fill", "p0", 200, 200, 3, 0, 0)]
    assert (src, dst) == (("sig", "p0", 100, 2), ("sig", "p1", 100, 2))
    nodetime.release(d_in, d_out)
    assert ctx.log[3:] == [("free", "p0"), ("free", "p1")]


@pytest.mark.parametrize("node", NODES)
def test_help_needs_no_device(node):
    env = dict(os.environ, NAE_GPU_LIB="/nonexistent/libnae_gpu.so", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(TOOLS, node + "_time.py"), "--help"], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stderr
    assert all(flag in r.stdout for flag in ("--runs", "--warmup", "--quick", "--limit"))


@pytest.mark.parametrize("node", NODES)
def test_steps_are_the_labels_of_the_docstring(node):
    """'Steps: A, B (--quick: C, D).' in the tool's docstring is what its driver runs, and every step starts the tool in its child mode"""
    tool = load(node + "_time")
    full, quick = re.search(r"^Steps: (.+) \(--quick: (.+)\)\.", tool.__doc__, re.M).groups()
    for text, steps in ((full, tool.steps(False)), (quick, tool.steps(True))):
        assert [label for label, _ in steps] == text.split(", ")
        for label, tail in steps:
            assert tail[0] == ("--n-fft" if node == "hpss" else "--shape") and tail[1] == label.split()[-1]
            if node != "hpss":
                assert label in getattr(tool, "SHAPES", nodetime.SHAPES)
    assert ("--quick" in tool.steps(True)[0][1]) == (node == "hpss")    # where the step is no shape, the child is told the size as well
