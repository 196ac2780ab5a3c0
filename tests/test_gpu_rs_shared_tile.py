"""k_rs with several channel groups per workgroup: a
workgroup takes FMX_RS_G adjacent 16-channel groups, builds each output
tile's band matrix once and walks the (tile, group) sequence with it.  The
shapes here are the smallest at which that loop can go wrong: channel counts
that are no multiple of 16 G (a last workgroup with fewer groups, a partial
last group), tile counts the parts do not divide, and a ragged last tile
(n = 1024: 729 or 730 RDS samples, n = 3000: 2137 or 2138, n = 4096: 2918 or
2919 -- none a multiple of 16).  Bars: those of tests/test_gpu_parity.py."""
import os
import re

import numpy as np
import pytest

import gpu_harness as H
from test_gpu_parity import check, make_iq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shipped_g():
    with open(os.path.join(ROOT, "fmtuner-sdr_amd", "csrc", "fmx_internal.h")) as f:
        m = re.search(r"^#define FMX_RS_G (\d+)", f.read(), re.M)
    return int(m.group(1))


G = _shipped_g()
NBLK = 4
_one = {}  # n -> (one channel's IQ [1][row], its oracle blocks): computed once, never changed


def _one_signal(fmx, oracle, n):
    if n not in _one:
        iq, _ = make_iq(fmx, 2, 1, NBLK, n=n)
        _one[n] = (iq, H.run_oracle_pipeline(oracle, oracle.make_cfg(), iq[0], NBLK, n=n))
    return _one[n]


def _run_pipelined(fmx, torch, iq, n, nblk):
    """nblk fmx_process_block calls of n samples with no host synchronisation
    in between, every output to per-block buffers.  -> (per-block dicts as
    gpu_harness.run_gpu_pipeline's, kernel_times)."""
    cfg = fmx.make_config()
    C, B, M, GS = iq.shape[0], cfg.block, cfg.iq_rate // cfg.dsp_rate, 8
    dev = torch.device("cuda")
    h = fmx.Handle(cfg, C)
    d_iq = torch.from_numpy(np.ascontiguousarray(iq)).to(dev)
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    T = dict(mpx=f(nblk, C, B), pcm_l=f(nblk, C, B), pcm_r=f(nblk, C, B), clip=f(nblk, C), count=z(nblk, C),
             stereo=z(nblk, C), pilot=z(nblk, C), indicator=z(nblk, C), gcount=z(nblk, C), grp=z(nblk, C, GS, 4))
    torch.cuda.synchronize()
    h.timing_enable(True)
    for b in range(nblk):
        p = {k: v[b].data_ptr() for k, v in T.items()}
        out = fmx.BlockOut(p["mpx"], B, p["pcm_l"], p["pcm_r"], B, p["count"], p["stereo"], p["pilot"], p["clip"],
                           p["grp"], GS, p["gcount"], None, p["indicator"])
        h.process_block(d_iq.data_ptr() + b * 2 * n * M, iq.shape[1], n, out)
    h.sync()
    torch.cuda.synchronize()
    kt = h.kernel_times()
    R = {k: v.cpu().numpy() for k, v in T.items()}
    h.close()
    res = []
    for b in range(nblk):
        d = {k: (R[k][b][:, :n] if k == "mpx" else R[k][b]) for k in R}
        d["groups"] = H._groups_of(R["grp"][b], R["gcount"][b], GS)
        res.append(d)
    return res, kt


def _assert_k_rs_ran(kt, nblk):
    assert kt["rs"][1] == nblk and kt["frontend"][1] == nblk and kt["frontend_generic"][1] == 0, kt


@pytest.mark.parametrize("n", [1024, 3000, 4096])
@pytest.mark.parametrize("C", [19, 16 * G - 1, 16 * G + 1, 2 * 16 * G + 3])
def test_one_signal_on_every_row(fmx, oracle, torch_cuda, C, n):
    """The same IQ on every row: every output field of every channel equals
    channel 0's bit for bit (a group that read another group's window slot, or
    a skipped or doubled group, differs), and channel 0 meets the oracle."""
    iq1, o0 = _one_signal(fmx, oracle, n)
    g, kt = _run_pipelined(fmx, torch_cuda, np.repeat(iq1, C, axis=0), n, NBLK)
    _assert_k_rs_ran(kt, NBLK)
    for b in range(NBLK):
        for k in ("mpx", "pcm_l", "pcm_r", "clip", "count", "stereo", "pilot", "indicator", "gcount", "grp"):
            a = g[b][k].view(np.uint32) if g[b][k].dtype == np.float32 else g[b][k]
            diff = np.nonzero((a != a[0]).reshape(C, -1).any(axis=1))[0]
            assert diff.size == 0, (b, k, "channels that differ from channel 0", diff[:16].tolist())
    check(g, o0, 0, NBLK, f"rs_shared C={C} n={n}")


def test_distinct_channels(fmx, oracle, torch_cuda):
    """16 G + 5 different channels: the first and last channel of the first
    two groups, of the last full group, and of the partial group that the
    second workgroup takes alone, against the oracle; RDS groups bit-exact."""
    C, nblk = 16 * G + 5, 20
    iq, _ = make_iq(fmx, 2, C, nblk, ch0=300)
    kt = {}
    g = H.run_gpu_pipeline(fmx, torch_cuda, fmx.make_config(), iq, nblk, ktimes=kt)
    _assert_k_rs_ran(kt, nblk)
    ngroups = 0
    for c in (0, 15, 16, 16 * G - 1, 16 * G, C - 1):
        o = H.run_oracle_pipeline(oracle, oracle.make_cfg(), iq[c], nblk)
        ngroups += len(check(g, o, c, nblk, "rs_shared_distinct")["groups_oracle"])
    assert ngroups >= 6
