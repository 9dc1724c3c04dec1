"""bench.py's plain run and --dump-outputs: the plain line times the steps it is asked for and nothing else, and the
files it dumps are what the timed path returned (the frame of the last step, as float32), equal to the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from renderbaby_amd import scenes
from tests import _oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, capture_output=True,
                         text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_dumps_the_timed_frame(tmp_path):
    d = tmp_path / "out"
    j = _bench(["--workload", "c1", "--spp", "4", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d),
                "--dump-frame", str(tmp_path / "frame.npy")])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["full"] is False
    assert j["unit"] == "Msamples/s" and j["value"] > 0 and j["ms_per_step"] > 0 and j["higher_is_better"] is True
    assert j["dtype"] == "f32" and j["metric"].startswith("Msamples/s")
    # the --full legs did not run
    assert j["cpu_baseline"] is None and j["end_to_end"] is None and j["verify"] is None
    assert set(j["roofline"]) == {"kernel", "kernel_ms", "launches_per_step", "accumulate_ms_per_step"}
    assert j["roofline"]["kernel_ms"] > 0
    assert sorted(os.listdir(d)) == ["frame.npy"]
    f = np.load(d / "frame.npy")
    assert f.dtype == np.float32 and f.shape == (512, 512, 4)
    assert np.array_equal(f, np.load(tmp_path / "frame.npy").astype(np.float32))
    _, _, o_rgba, o_st = _oracle.render(scenes.cornell_c1().with_params(spp=4))
    assert np.array_equal(f, o_rgba.astype(np.float32))
    assert j["config"]["segments_per_step"] == o_st["segments"]


def test_large_frame_is_dumped_as_a_fixed_sample(tmp_path):
    # C4's 4096 x 4096 frame would be 256 MiB as float32: a seeded sample of its pixels and their indices instead
    a, b = tmp_path / "a", tmp_path / "b"
    common = ["--workload", "c4", "--spp", "1", "--steps", "1", "--warmup", "0"]
    _bench(common + ["--dump-outputs", str(a), "--dump-frame", str(tmp_path / "frame.npy")])
    assert sorted(os.listdir(a)) == ["frame_sample.npy", "frame_sample_index.npy"]
    s, i = np.load(a / "frame_sample.npy"), np.load(a / "frame_sample_index.npy")
    assert s.dtype == np.float32 and i.dtype == np.float64 and s.shape == (len(i), 4)
    assert s.nbytes + i.nbytes <= 64 << 20
    assert np.all(np.diff(i) > 0) and i[0] >= 0 and i[-1] < 4096 * 4096
    frame = np.load(tmp_path / "frame.npy").reshape(-1, 4)
    assert np.array_equal(s, frame[i.astype(np.int64)].astype(np.float32))
    _bench(common + ["--dump-outputs", str(b)])
    assert np.array_equal(np.load(b / "frame_sample_index.npy"), i) and np.array_equal(np.load(b / "frame_sample.npy"), s)
