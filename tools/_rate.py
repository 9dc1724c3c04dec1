"""What every tools/*_rate.py shares: the median and its text, the scenes by their short names, the report that is written line
by line, arms measured in alternating order, an environment variable set for the length of a call, and one process per scene.

A child process says whether its requirement held by its exit status alone: 0 -- it ran, and every judged requirement held (or
nothing is judged); 3 -- it ran, and a judged requirement was missed.  Anything else, a signal or the time limit is a failure,
and after a failure nothing more is started on the device.  Nothing heavy is imported here: a parent that starts children
through this module never opens the device.
"""
import contextlib, os, statistics, subprocess, sys, threading

MISSED = 3   # a child's exit status: it ran to its end, a judged requirement was missed


def med(xs):
    return statistics.median(xs), max(xs) - min(xs)


def med_text(xs):
    m, s = med(xs)
    return f"{m:9.3f} ({s:6.3f})"


def scene_of(name, own=None):
    """the scene of a short name; `own`: a tool's entries that differ from the table's"""
    from renderbaby_amd import refscenes, scenes
    table = {"c2": scenes.cornell_c2, "c3": scenes.mesh_c3, "c4": scenes.spheres_scene, "c5": scenes.mesh_c5, "lamp": refscenes.ref_lamp,
             "cornell": scenes.cornell_c1, "feature": scenes.feature_scene, **(own or {})}
    if name not in table:
        raise SystemExit(f"unknown configuration {name}")
    return table[name]()


class Report:
    """say(line) prints and, with an --out path, appends to that file, flushed line by line: a run that is cut short keeps
    what it measured"""

    def __init__(self, out_path=None):
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        self.file = open(out_path, "w") if out_path else None

    def say(self, line=""):
        print(line, flush=True)
        if self.file:
            self.file.write(line + "\n")
            self.file.flush()

    def close(self):
        if self.file:
            self.file.close()
            self.file = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def alternating(arms, runs, measure):
    """one warm-up round, then `runs` rounds of measure(arm) for every arm, odd rounds in reverse order: {arm: [value per
    measured round]}"""
    arms = list(arms)
    got = {arm: [] for arm in arms}
    for run in range(runs + 1):
        for arm in (arms if run % 2 == 0 else arms[::-1]):
            value = measure(arm)
            if run:
                got[arm].append(value)
    return got


@contextlib.contextmanager
def env(name, value):
    """the environment variable set for the length of the block, then what was there before"""
    before = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if before is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = before


def child_argv(script, name, a, options, first=False):
    """the command of one child: the script again with --child NAME, the parent's values of `options` (argparse names), and
    --header for the first"""
    passed = [x for o in options for x in ("--" + o.replace("_", "-"), str(getattr(a, o)))]
    return [sys.executable, os.path.abspath(script), "--child", name] + passed + (["--header"] if first else [])


def run_children(report, argv_of, names, limit_s, merge_stderr=False):
    """One fresh process per name, one after another: argv_of(name, first) is started, its stdout goes to the report line by
    line as it arrives, and it has limit_s seconds.  Exit status 0: held; MISSED: the requirement was missed, the next is
    started all the same.  Any other status, a signal or the time limit: said in a # line, and nothing more is started --
    whatever ended that process may have left the device in a bad state.  Returns (held, completed): every child returned 0;
    every child ran to its end."""
    held = True
    for i, name in enumerate(names):
        p = subprocess.Popen(argv_of(name, i == 0), stdout=subprocess.PIPE, stderr=subprocess.STDOUT if merge_stderr else None, text=True)
        late = []

        def expire():
            late.append(True)
            p.kill()
        timer = threading.Timer(limit_s, expire)
        timer.start()
        try:
            for line in p.stdout:
                report.say(line.rstrip("\n"))
            status = p.wait()
        finally:
            timer.cancel()
            if p.poll() is None:   # (an exception in this process: the child does not outlive it)
                p.kill()
                p.wait()
        if late and status < 0:
            report.say(f"# {name}: the measuring process did not end within {limit_s} s and was killed; nothing more is started")
            return False, False
        if status not in (0, MISSED):
            report.say(f"# {name}: the measuring process ended with status {status}; nothing more is started")
            return False, False
        held = held and status == 0
    return held, True


def child_header():
    """the first child's first line: the device's name"""
    from renderbaby_amd import engine
    print(f"# {engine.device_name(0)}", flush=True)


def child_exit(held=True):
    sys.exit(0 if held else MISSED)
