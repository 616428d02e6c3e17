"""Every sampler of the output iterations at once (sample_outputs, csrc/lbm_launch.inc.hpp): force log, per-body forces, statistics, frames
and probes on a group of two strips, driven by one host thread per strip and by the calling thread alone. 128x32 in 16 + 16 rows,
output_frequency 5, 11 steps (samples at t = 0, 5, 10), every ring two slots deep: the third sample goes into the slot a partial drain
freed, and the last drain copies the ring in two pieces. Each drained quantity is np.array_equal to that of a run with its sampler alone:
the samplers read P_t and write memory of their own, so none may change what another reports."""

import numpy as np
import pytest

from tests.helpers import PLANS, lbm_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

NX, NY, OF = 128, 32, 5
BOUNDS = [(0, 16), (16, 16)]
FRAME_K = 4
XY = np.array([(5.0, 15.5), (127.0, 15.5), (0.0, 15.75), (40.0, 16.0), (100.25, 3.5), (70.5, 30.125), (33.0, 0.0), (33.0, 31.0)])
SAMPLERS = ("bodies", "stats", "frames", "probes")


def body_labels():
    """two discs: body 1 across the face between the strips, body 2 in the upper strip alone"""
    y, x = np.mgrid[0:NY, 0:NX]
    lab = np.zeros((NY, NX), np.uint8)
    lab[(x - 30) ** 2 + (y - 15) ** 2 <= 16] = 1
    lab[(x - 70) ** 2 + (y - 24) ** 2 <= 9] = 2
    return lab


def run(lbm, on, threads=1):
    """what every strip drains, sampler by sampler; the samplers not in `on` are off (without "bodies" the labels are a plain mask)"""
    lab = body_labels()
    geometry = dict(bodies=lab) if "bodies" in on else dict(solid=lab != 0)
    out = {}
    with lbm.Group(NX, NY, BOUNDS, options=dict(PLANS["rowil-fuse3-12-nt-xcd"], group_threads=threads), tau=0.6, force_log_capacity=2, **geometry) as g:
        g.initialise()
        if "stats" in on:
            g.stats_begin(0)
        if "frames" in on:
            g.frames_begin(FRAME_K, 2)
        if "probes" in on:
            g.probes_begin(XY, 2)
        g.step(10, OF)                                   # t = 0, 5: every ring is full
        first = [(c.drain_force_log(), c.drain_body_force_log(2), c.drain_frames(1), c.drain_probes(1)) for c in g.ctxs]      # the oldest sample of each ring
        g.step(1, OF)                                    # t = 10: into the slot that was freed
        rest = [(c.drain_force_log(), c.drain_body_force_log(), c.drain_frames(), c.drain_probes()) for c in g.ctxs]
        assert g.first_unstable_step() == -1 and g.steps_done == 11
        out["forces"] = [np.array(a[0] + b[0]) for a, b in zip(first, rest)]
        if "bodies" in on:
            out["bodies"] = [np.array(a[1] + b[1]) for a, b in zip(first, rest)]
            assert all(len(a[1]) == 2 and v.shape == (6, 4) and v[:, 0].tolist() == [0, 0, 5, 5, 10, 10] for a, v in zip(first, out["bodies"]))
        if "stats" in on:
            assert g.stats_samples() == 3
            out["stats"] = [c.stats_sums() for c in g.ctxs]
        if "frames" in on:
            fr = [a[2] + b[2] for a, b in zip(first, rest)]
            assert all(len(a[2]) == 1 and [t for t, _ in f] == [0, 5, 10] for a, f in zip(first, fr))
            out["frames"] = [np.stack([v for _, v in f]) for f in fr]
        if "probes" in on:
            assert all(a[3][0].tolist() == [0] and b[3][0].tolist() == [5, 10] for a, b in zip(first, rest))
            out["probes"] = [np.concatenate([a[3][1], b[3][1]]) for a, b in zip(first, rest)]
        assert all(v.shape == (3, 3) and v[:, 0].tolist() == [0, 5, 10] for v in out["forces"])
    return out


_alone = {}


def alone(lbm, name):
    if name not in _alone:
        _alone[name] = run(lbm, {name})
    return _alone[name]


@pytest.mark.parametrize("threads", [1, 0], ids=["threaded", "eager"])
def test_all_samplers_together_report_what_each_reports_alone(lbm, threads):
    got = run(lbm, set(SAMPLERS), threads)
    for name in SAMPLERS:
        ref = alone(lbm, name)
        for key in ("forces", name):
            for strip, (a, b) in enumerate(zip(got[key], ref[key])):
                assert a.shape == b.shape and np.array_equal(a, b), (name, key, strip)
    assert np.any(got["bodies"][1][:, 2:] != 0.0) and np.any(got["probes"][0][-1] != got["probes"][0][0])      # a flow, not a state at rest
    assert not np.array_equal(got["frames"][0][0], got["frames"][0][2]) and np.any(got["stats"][1][2] != 0.0)
