"""bench.py's multi-rank plumbing on the CPU (no GPU): `--gpus N` without a
launcher spawns N ranks under torch.distributed.run before any GPU call,
shards the channels with fmx_dist.shard, and carries the collectives
(gather of the scan levels, summed channel count) over gloo (--dry-run)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=240, env=env)
    return r


@pytest.mark.parametrize("workload,n,total,rank0", [("cfg3", 2, 8192, 4096), ("cfg4", 2, 16384, 8192),
                                                     ("cfg4", 3, 16384, 5462)])
def test_spawned_ranks_shard_and_gather(workload, n, total, rank0):
    r = _run(["--gpus", str(n), "--workload", workload, "--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == n and d["world_reported"] == n
    assert d["total_channels"] == total and d["channels_summed"] == total
    assert d["channels_rank0"] == rank0
    assert d["gathered"] == total
    assert d["scaling"] == ("weak" if workload == "cfg3" else "strong")


def test_single_rank_dry_run():
    r = _run(["--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 1 and d["channels_summed"] == 4096 and d["scaling"] == "weak"


def test_driver_scaling_invocation_defaults_to_cfg4():
    """The driver's N>1 command names no workload: it gets BASELINE's Cfg4
    curve (16384 channels sharded, 2048 per GPU at N=8)."""
    r = _run(["--gpus", "2", "--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["total_channels"] == 16384 and d["channels_rank0"] == 8192 and d["scaling"] == "strong"


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_the_default():
    """--full and --dump-outputs are off unless asked for; --steps is the
    number of timed steps as given."""
    b = _bench_module()
    a = b.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = b.parse(["--full", "--dump-outputs", "x"])
    assert a.full is True and a.dump_outputs == "x"


def test_resident_iq_is_bounded_for_any_number_of_steps():
    """All blocks stay resident while they fit in the budget (the default
    run: fresh IQ at every step); past it the count stops growing, so
    --steps in the thousands allocates no more than the budget."""
    b = _bench_module()
    n_iq, budget = 40960, b.parse([]).iq_bytes
    assert b.iq_blocks(105, 4096, n_iq, budget) == 105
    assert b.iq_blocks(25, 4096, n_iq, budget) == 25
    assert b.iq_blocks(105, 16384, n_iq, budget) == 105  # Cfg4 on one GPU, as it runs today
    for steps in (512, 513, 2443, 100_000):
        n = b.iq_blocks(steps, 4096, n_iq, budget)
        assert n == 512 and n * 4096 * 2 * n_iq <= budget
    assert b.iq_blocks(1000, 4096, n_iq, 1) == 3        # never below the pipeline's depth
    assert b.iq_blocks(2, 4096, n_iq, 1) == 2


def test_dump_outputs_writes_what_the_block_defines(tmp_path):
    """dump_outputs on host tensors laid out as fmx_block_out's fields: float
    arrays only, PCM past pcm_count and group slots past group_count zeroed,
    fmx_rds_group and fmx_signal_level unpacked field by field."""
    import numpy as np
    import torch
    b = _bench_module()
    C, B, GS = 5, 16, 3
    rng = np.random.default_rng(3)
    pl = rng.standard_normal((C, B)).astype(np.float32)
    pr = rng.standard_normal((C, B)).astype(np.float32)
    cnt = np.array([7, 6, 7, 0, 5], np.int32)
    gcnt = np.array([0, 1, 3, 2, 1], np.int32)
    raw = np.zeros((C, GS), dtype=[("a", "<u2"), ("b", "<u2"), ("c", "<u2"), ("d", "<u2"), ("errors", "u1"),
                                   ("pad", "u1"), ("pad2", "<u2"), ("block_index", "<u4")])
    for f in raw.dtype.names:
        raw[f] = rng.integers(0, np.iinfo(raw.dtype[f]).max, (C, GS), endpoint=True)
    raw["block_index"][2, 1] = 0xFFFFFFF0  # the sign bit of the 32-bit word it travels in
    sig = np.zeros(C, dtype=[("level120", "<f4"), ("smoothed", "<f4"), ("dbfs", "<f8"), ("comp", "<f8"),
                             ("hard", "<f8"), ("near", "<f8")])
    for f in sig.dtype.names:
        sig[f] = rng.standard_normal(C)
    out = {"pcm_l": torch.from_numpy(pl), "pcm_r": torch.from_numpy(pr), "pcm_count": torch.from_numpy(cnt),
           "stereo": torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32),
           "pilot_tenths": torch.tensor([90, 0, 88, 91, 3], dtype=torch.int32),
           "stereo_indicator": torch.tensor([1, 0, 1, 1, 1], dtype=torch.int32),
           "clip_ratio": torch.linspace(0.0, 0.5, C),
           "groups": torch.from_numpy(raw.view(np.int32).reshape(C, GS, 4).copy()),
           "group_count": torch.from_numpy(gcnt),
           "signal": torch.from_numpy(sig.view(np.float32).reshape(C, 10).copy())}
    b.dump_outputs(str(tmp_path), 0, out)
    got = {os.path.splitext(f)[0]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"pcm_channels", "pcm_l", "pcm_r", "pcm_count", "stereo", "pilot_tenths", "stereo_indicator",
                        "clip_ratio", "groups", "group_count", "signal"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["pcm_channels"], np.arange(C))
    live = np.arange(7)[None, :] < cnt[:, None]
    assert got["pcm_l"].shape == (C, 7)
    assert np.array_equal(got["pcm_l"], np.where(live, pl[:, :7], 0)) and got["pcm_l"].dtype == np.float32
    assert np.array_equal(got["pcm_r"], np.where(live, pr[:, :7], 0))
    assert np.array_equal(got["pcm_count"], cnt) and np.array_equal(got["group_count"], gcnt)
    assert np.array_equal(got["pilot_tenths"], [90, 0, 88, 91, 3])
    assert np.array_equal(got["clip_ratio"], out["clip_ratio"].numpy())
    want = np.stack([raw[f].astype(np.float64) for f in ("a", "b", "c", "d", "errors", "block_index")], axis=-1)
    want[np.arange(GS)[None, :] >= gcnt[:, None]] = 0.0
    assert np.array_equal(got["groups"], want)
    assert got["groups"][2, 1, 5] == float(0xFFFFFFF0)
    assert np.array_equal(got["signal"], np.stack([sig[f].astype(np.float64) for f in sig.dtype.names], axis=1))


def test_dump_outputs_samples_channels_over_the_size_limit(tmp_path, monkeypatch):
    """Over the PCM budget a fixed, seeded set of channels is written, the
    same one every time, named by pcm_channels."""
    import numpy as np
    import torch
    b = _bench_module()
    C, B = 40, 8
    monkeypatch.setattr(b, "DUMP_PCM_BYTES", 10 * 2 * 4 * B)  # room for 10 channels
    pl = torch.arange(C * B, dtype=torch.float32).reshape(C, B)
    z = torch.zeros(C, dtype=torch.int32)
    out = {"pcm_l": pl, "pcm_r": -pl, "pcm_count": torch.full((C,), B, dtype=torch.int32), "stereo": z,
           "pilot_tenths": z, "stereo_indicator": z, "clip_ratio": torch.zeros(C),
           "groups": torch.zeros((C, 2, 4), dtype=torch.int32), "group_count": z}
    picks = []
    for name in ("a", "b"):
        b.dump_outputs(str(tmp_path / name), 0, out)
        ch = np.load(tmp_path / name / "pcm_channels.npy").astype(int)
        assert ch.size == 10 and np.all(np.diff(ch) > 0) and ch.min() >= 0 and ch.max() < C
        assert np.array_equal(np.load(tmp_path / name / "pcm_l.npy"), pl.numpy()[ch])
        assert np.array_equal(np.load(tmp_path / name / "pcm_r.npy"), -pl.numpy()[ch])
        assert np.load(tmp_path / name / "pcm_count.npy").shape == (C,)
        picks.append(ch)
    assert np.array_equal(picks[0], picks[1])


def test_launcher_world_mismatch_fails():
    r = _run(["--gpus", "4", "--dry-run"], env_extra={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr
