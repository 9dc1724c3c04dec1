"""tools/_rate.py, the harness of the tools/*_rate.py scripts: its statistics, its alternation, its environment arm, its report
and its one-process-per-scene runner, held with fake children that never open a device (CPU only)."""
import os
import statistics
import subprocess
import sys
import threading
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)
import _rate  # noqa: E402

RATE_TOOLS = ["camera_rate", "denoise_rate", "direct_light_rate", "direct_pick_rate", "hemisphere_rate", "lightmap_rate", "occlusion_rate",
              "probe_light_rate", "probe_rate", "probe_visibility_rate", "query_rate", "radiance_rate", "reproject_rate"]


def child(code):
    return [sys.executable, "-c", code]


def lines_of(path):
    with open(path) as f:
        return f.read().splitlines()


def test_med_and_its_text_are_what_the_tools_computed():
    xs = [3.25, 1.0, 10.5, 2.0]
    assert _rate.med(xs) == (statistics.median(xs), max(xs) - min(xs)) == (2.625, 9.5)
    assert _rate.med_text(xs) == f"{statistics.median(xs):9.3f} ({max(xs) - min(xs):6.3f})" == "    2.625 ( 9.500)"


def test_alternating_reverses_odd_rounds_and_drops_the_warm_up():
    calls = []

    def measure(arm):
        calls.append(arm)
        return len(calls)
    got = _rate.alternating(("a", "b", "c"), 2, measure)
    assert calls == ["a", "b", "c", "c", "b", "a", "a", "b", "c"]
    assert got == {"a": [6, 7], "b": [5, 8], "c": [4, 9]}


@pytest.mark.parametrize("before", ["old", None])
@pytest.mark.parametrize("raises", [False, True])
def test_env_restores_what_was_there(monkeypatch, before, raises):
    name = "RB_RATE_HARNESS_TEST"
    if before is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, before)
    try:
        with _rate.env(name, "new"):
            assert os.environ[name] == "new"
            if raises:
                raise KeyError("from the body")
    except KeyError:
        assert raises
    assert os.environ.get(name) == before


def test_report_has_a_line_on_disk_before_it_is_closed(tmp_path, capsys):
    path = tmp_path / "made" / "by" / "report.txt"
    with _rate.Report(str(path)) as r:
        r.say("x")
        assert path.read_text().endswith("x\n")
        r.say()
    assert path.read_text() == "x\n\n"
    assert capsys.readouterr().out == "x\n\n"
    _rate.Report(None).say("only printed")   # no file asked for: none made


def run(tmp_path, codes, limit_s=30):
    """run_children over the fake children `codes`; the report's lines, the verdict, and which child was called first"""
    out, firsts = tmp_path / "report.txt", []

    def argv_of(name, first):
        firsts.append((name, first))
        return child(codes[name])
    with _rate.Report(str(out)) as r:
        verdict = _rate.run_children(r, argv_of, list(codes), limit_s)
    return lines_of(out), verdict, firsts


def test_children_that_all_hold(tmp_path):
    codes = {n: f"print('{n} 1'); print('{n} 2')" for n in ("p", "q", "r")}
    lines, verdict, firsts = run(tmp_path, codes)
    assert lines == ["p 1", "p 2", "q 1", "q 2", "r 1", "r 2"]
    assert verdict == (True, True)
    assert firsts == [("p", True), ("q", False), ("r", False)]


def test_a_missed_requirement_does_not_stop_the_run(tmp_path):
    codes = {"p": "print('p')", "q": "import sys; print('q'); sys.exit(3)", "r": "print('r')"}
    lines, verdict, _ = run(tmp_path, codes)
    assert lines == ["p", "q", "r"]
    assert verdict == (False, True)


def test_a_failed_child_is_the_last_one_started(tmp_path):
    marker = tmp_path / "third_ran"
    codes = {"p": "print('p')", "q": "import sys; print('q'); sys.exit(1)", "r": f"open({str(marker)!r}, 'w').close(); print('r')"}
    lines, verdict, firsts = run(tmp_path, codes)
    assert not marker.exists() and [n for n, _ in firsts] == ["p", "q"]
    assert lines[:2] == ["p", "q"] and len(lines) == 3
    assert lines[2].startswith("# q:") and "status 1" in lines[2] and "nothing more is started" in lines[2]
    assert verdict == (False, False)


def test_a_signal_ends_the_run_too(tmp_path):
    codes = {"p": "import os, signal; os.kill(os.getpid(), signal.SIGTERM)", "q": "print('q')"}
    lines, verdict, firsts = run(tmp_path, codes)
    assert len(lines) == 1 and "status -15" in lines[0] and verdict == (False, False) and len(firsts) == 1


def test_the_time_limit_kills_the_child_and_ends_the_run(tmp_path):
    marker, pid_file = tmp_path / "second_ran", tmp_path / "pid"
    codes = {"p": f"import os, time; open({str(pid_file)!r}, 'w').write(str(os.getpid())); print('measured', flush=True); time.sleep(60)",
             "q": f"open({str(marker)!r}, 'w').close()"}
    t0 = time.monotonic()
    lines, verdict, _ = run(tmp_path, codes, limit_s=1)
    assert time.monotonic() - t0 < 10
    assert lines[0] == "measured" and len(lines) == 2
    assert lines[1].startswith("# p:") and "did not end within 1 s" in lines[1] and "nothing more is started" in lines[1]
    assert verdict == (False, False) and not marker.exists()
    with pytest.raises(ProcessLookupError):   # killed and reaped: no such process, not even a zombie
        os.kill(int(pid_file.read_text()), 0)


def test_a_line_reaches_the_report_while_its_child_still_runs(tmp_path):
    out, go = tmp_path / "report.txt", tmp_path / "go"
    code = (f"import os, time\nprint('early', flush=True)\nt0 = time.monotonic()\n"
            f"while not os.path.exists({str(go)!r}) and time.monotonic() - t0 < 20: time.sleep(0.01)\n"
            f"print('released' if os.path.exists({str(go)!r}) else 'gave up')")
    result = []

    def parent():
        with _rate.Report(str(out)) as r:
            result.append(_rate.run_children(r, lambda name, first: child(code), ["p"], 30))
    t = threading.Thread(target=parent)
    t.start()
    deadline = time.monotonic() + 15
    while time.monotonic() < deadline and not (out.exists() and lines_of(out)[:1] == ["early"]):
        time.sleep(0.01)
    seen_early = out.exists() and lines_of(out) == ["early"]   # the child is still waiting: nothing else can be there yet
    go.write_text("")
    t.join(30)
    assert seen_early
    assert lines_of(out) == ["early", "released"] and result == [(True, True)]


@pytest.mark.parametrize("tool", RATE_TOOLS)
def test_help_opens_neither_torch_nor_the_library(tool):
    code = ("import os, runpy, sys\nsys.argv = [sys.argv[1], '--help']\nsys.path.insert(0, os.path.dirname(sys.argv[0]))\n"
            "try:\n    runpy.run_path(sys.argv[0], run_name='__main__')\nexcept SystemExit as e:\n    status = e.code or 0\n"
            "heavy = [m for m in ('torch', 'renderbaby_amd') if m in sys.modules]\n"
            "print('STATUS', status, 'HEAVY', heavy)")
    p = subprocess.run(child(code) + [os.path.join(TOOLS, tool + ".py")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert p.stdout.splitlines()[-1] == "STATUS 0 HEAVY []", p.stdout[-400:] + p.stderr[-400:]
    assert "usage:" in p.stdout
