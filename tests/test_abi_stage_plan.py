"""The input of the 19-channel stage entry point test
(tests/test_gpu_abi_geometry.py::test_stage_chain_19_channels_ragged) is one
the oracle decides the same way under ten times the GPU's error: the stereo
flag, the pilot level and the RDS groups of every call are exact comparisons
there, so the chosen synthetic channels (gpu_harness.STAGE_CH0 ..), call
sizes, resets and setters must not sit on a decision the oracle itself makes
differently when its MPX moves by 1e-5 (tests/rds_wave.perturbed: ten times
the logged GPU-to-oracle MPX RMS).  No GPU."""
import numpy as np

import gpu_harness as H
import rds_wave as W


def _run(oracle, iq_row, c, seed):
    """Channel c's stereo flags, pilot tenths and groups per call; seed: the
    perturbation of the MPX the stereo and RDS stages are given (None: none)."""
    ch = H.OracleChannel(oracle)
    pos, M = 0, 10
    flags, groups = [], []
    for i, n in enumerate(H.STAGE_SIZES):
        H.stage_events(ch, i, c)
        bb = ch.decimate(iq_row[2 * M * pos:2 * M * (pos + n)], n)
        mpx, _ = ch.demod(bb, n)
        if seed is not None:
            mpx = W.perturbed(mpx, 1000 * seed + i)
        _, _, st, pil = ch.stereo(mpx, n)
        flags.append((st, pil))
        groups.append(ch.rds_groups(mpx, n))
        pos += n
    ch.close()
    return flags, groups


def test_stage_schedule_is_stable_under_mpx_perturbation(oracle):
    import fmx
    iq = H.stage_iq(fmx)
    jobs = [(c, s) for c in range(H.STAGE_C) for s in (None, 1, 2)]
    res = dict(zip(jobs, W.pmap(lambda j: _run(oracle, iq[j[0]], j[0], j[1]), jobs)))
    ngroups = 0
    for c in range(H.STAGE_C):
        f0, g0 = res[(c, None)]
        for s in (1, 2):
            f1, g1 = res[(c, s)]
            assert f1 == f0, (c, s, [(i, a, b) for i, (a, b) in enumerate(zip(f0, f1)) if a != b])
            assert g1 == g0, (c, s)
        ngroups += sum(len(x) for x in g0)
    # the resets (before call 6) show: the pilot level of channels 5 and 18
    # starts over, the others' keeps rising; every channel ends in stereo
    for c in range(H.STAGE_C):
        f = res[(c, None)][0]
        assert (f[6][1] < f[5][1]) == (c in (5, 18)), (c, f[5], f[6])
        assert f[-1][0] == 1, (c, f[-1])
    assert ngroups >= H.STAGE_C
