"""A plain bench.py run on the GPU: the result line's timed steps, the null
`--full` records, and `--dump-outputs` (the last timed step's fmx_block_out
as float .npy files that agree with the line's own `check` figures).  One
small run (64 channels, 3 timed steps) shared by the tests."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
C = 64


def _bench(d, *args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--channels", str(C), "--dump-outputs", str(d)]
                       + list(args), capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return line, {os.path.splitext(f)[0]: np.load(d / f) for f in os.listdir(d)}


@pytest.fixture(scope="module")
def plain_run(torch_cuda, tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("dump"), "--steps", "3", "--warmup", "2")


def test_more_steps_than_resident_blocks(torch_cuda, tmp_path):
    """Room for 4 blocks of IQ, 1 + 9 blocks run: the steps go round the
    resident blocks, all 9 are timed, and the last one's outputs are whole."""
    d, a = _bench(tmp_path, "--steps", "9", "--warmup", "1", "--iq-bytes", str(4 * C * 2 * 40960 + 100))
    assert d["steps"] == 9 and d["config"]["iq_blocks_resident"] == 4
    iq = C * 9 * 4096 * 10
    assert d["value"] == pytest.approx(iq / (d["ms_per_step"] * 9 * 1e-3) / 1e6, rel=1e-3)
    assert set(a["pcm_count"].tolist()) <= {546.0, 547.0}
    assert all(np.isfinite(x).all() for x in a.values())
    assert a["pcm_l"].std() > 1e-3 and np.all(np.abs(a["pcm_l"]) <= 1.0)


def test_plain_line_times_the_steps_asked_for(plain_run):
    d, _ = plain_run
    assert d["steps"] == 3 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["config"]["iq_blocks_resident"] == 5  # fresh IQ for every block
    assert d["unit"] == "MS/s" and d["higher_is_better"] is True and d["ms_per_step"] > 0
    iq = C * d["steps"] * 4096 * 10
    assert d["value"] == pytest.approx(iq / (d["ms_per_step"] * d["steps"] * 1e-3) / 1e6, rel=1e-3)
    # the per-kernel figures come from the timed steps themselves
    assert d["kernels"] and d["roofline"]["kernel"]
    # what only --full measures is absent, not stale
    assert d["cpu_baseline"] is None and d["scan"] is None


def test_dumped_outputs_are_the_last_steps(plain_run):
    d, a = plain_run
    assert set(a) == {"pcm_channels", "pcm_l", "pcm_r", "pcm_count", "stereo", "pilot_tenths", "stereo_indicator",
                      "clip_ratio", "groups", "group_count", "signal"}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 * 1000 * 1000
    assert all(np.isfinite(x).all() for x in a.values())
    # 4096 samples at 240 kHz are 546 or 547 frames at 32 kHz
    assert a["pcm_count"].shape == (C,) and set(a["pcm_count"].tolist()) <= {546.0, 547.0}
    assert a["pcm_l"].shape == (C, int(a["pcm_count"].max())) and a["pcm_r"].shape == a["pcm_l"].shape
    assert np.array_equal(a["pcm_channels"], np.arange(C))
    assert np.all(np.abs(a["pcm_l"]) <= 1.0) and np.all(np.abs(a["pcm_r"]) <= 1.0)
    assert a["pcm_l"].std() > 1e-3 and a["pcm_r"].std() > 1e-3  # a programme, not silence
    # the line's own figures of the same step
    assert int(a["group_count"].sum()) == d["check"]["rds_groups_last_step"]
    assert float(a["stereo"].mean()) == pytest.approx(d["check"]["stereo_fraction"], abs=1e-6)
    assert a["groups"].shape == (C, 8, 6) and a["signal"].shape == (C, 6)
    assert np.all((a["signal"][:, 0] >= 0) & (a["signal"][:, 0] <= 120))  # the 120-point level scale
