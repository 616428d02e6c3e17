"""The gathers of a group of strips live in the library (lbm_group_get_* / lbm_group_drain_*, csrc/lbm_group.inc.hpp): what lbm.Group
returns for the whole lattice against the same quantities read member by member through g.ctxs from an identical second group and put
together here in numpy by the stated rules — rows by y_start (frames: y_start / k), ghost rows of the populations from the end strips,
sums as strip 0's value plus the others in strip order, counts that agree, min / max. fp64, pinned plan, 64 columns; 32 rows as
12 + 20 and 36 rows as 12 + 12 + 12 (sums of three addends); two bodies, frames of stride 4, five probes, statistics from step 0,
step(9, 3): samples at t = 0, 3, 6. Everything np.array_equal, iterations included. Then the drains' all-or-nothing rule."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import PLANS, lbm_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

NX, K = 64, 4
CASES = {"12+20": [(0, 12), (12, 20)], "12+12+12": [(0, 12), (12, 12), (24, 12)]}
# one probe per strip of the three-strip case, one half-way between the rows either side of the first face, one on a node
XY = np.array([(10.25, 5.5), (20.5, 17.25), (40.75, 30.5), (30.5, 11.5), (33.0, 20.0)])


def make(lbm, bounds):
    ny = bounds[-1][0] + bounds[-1][1]
    lab = np.zeros((ny, NX), np.uint8)
    lab[10:27, 20:25] = 1                                # body 1: rows 10..26, across every face
    lab[3:7, 40:44] = 2                                  # body 2: inside strip 0
    g = lbm.Group(NX, ny, bounds, options=dict(PLANS["rowil-fuse3-12-nt-xcd"]), tau=0.6, bodies=lab, frames=K, probes=XY)
    g.initialise()
    g.stats_begin(0)
    g.step(9, 3)
    return g


def in_strip_order(parts):
    """strip 0's value, then += the others, left to right"""
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    return total


def by_members(g):
    """every quantity of the whole lattice from the members' parts, by the rules of include/lbm_hip.h"""
    cs = g.ctxs
    out = {}
    bad = [t for t in (c.first_unstable_step() for c in cs) if t >= 0]
    out["first_unstable_step"] = min(bad) if bad else -1
    out["max_velocity_sq"] = max(c.max_velocity_sq() for c in cs)
    out["forces"] = np.array(in_strip_order([np.array(c.forces()) for c in cs]))
    out["body_forces"] = in_strip_order([c.body_forces() for c in cs])
    for j, name in enumerate(("rho", "ux", "uy")):
        out[name] = np.concatenate([c.macros()[j] for c in cs], axis=0)
    for which in ("f_current", "f_next"):
        parts = [c.populations(which) for c in cs]
        out[which] = np.concatenate([parts[0][:1]] + [p[1:-1] for p in parts] + [parts[-1][-1:]], axis=0)
    samples = {c.stats_samples() for c in cs}
    assert len(samples) == 1
    out["stats_samples"] = samples.pop()
    out["stats_sums"] = np.concatenate([c.stats_sums() for c in cs], axis=1)
    assert len({c.frames_pending() for c in cs}) == 1 and len({c.probes_pending() for c in cs}) == 1
    out["frames_pending"], out["probes_pending"] = cs[0].frames_pending(), cs[0].probes_pending()
    logs = [np.array(c.drain_force_log()) for c in cs]
    assert all(np.array_equal(l[:, 0], logs[0][:, 0]) for l in logs)
    out["force_log"] = np.column_stack([logs[0][:, 0], in_strip_order([l[:, 1:] for l in logs])])
    logs = [np.array(c.drain_body_force_log()) for c in cs]
    assert all(np.array_equal(l[:, :2], logs[0][:, :2]) for l in logs)
    out["body_force_log"] = np.column_stack([logs[0][:, :2], in_strip_order([l[:, 2:] for l in logs])])
    frames = [c.drain_frames() for c in cs]
    assert all([t for t, _ in f] == [t for t, _ in frames[0]] for f in frames)
    out["frame_steps"] = np.array([t for t, _ in frames[0]])
    out["frames"] = np.stack([np.concatenate([f[j][1] for f in frames], axis=1) for j in range(len(frames[0]))])
    probes = [c.drain_probes() for c in cs]
    assert all(np.array_equal(t, probes[0][0]) for t, _ in probes)
    out["probe_steps"], out["probes"] = probes[0][0], in_strip_order([v for _, v in probes])
    return out


def by_group(g):
    out = {"first_unstable_step": g.first_unstable_step(), "max_velocity_sq": g.max_velocity_sq(), "forces": np.array(g.forces()),
           "body_forces": g.body_forces()}
    out["rho"], out["ux"], out["uy"] = g.macros()
    out["f_current"], out["f_next"] = g.populations("f_current"), g.populations("f_next")
    out["stats_samples"], out["stats_sums"] = g.stats_samples(), g.stats_sums()
    out["frames_pending"], out["probes_pending"] = g.frames_pending(), g.probes_pending()
    out["force_log"], out["body_force_log"] = np.array(g.drain_force_log()), np.array(g.drain_body_force_log())
    frames = g.drain_frames()
    out["frame_steps"], out["frames"] = np.array([t for t, _ in frames]), np.stack([v for _, v in frames])
    out["probe_steps"], out["probes"] = g.drain_probes()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_the_group_returns_what_its_members_parts_add_up_to(lbm, case):
    bounds = CASES[case]
    ny = bounds[-1][0] + bounds[-1][1]
    with make(lbm, bounds) as a, make(lbm, bounds) as b:
        got, want = by_group(a), by_members(b)
        assert got.keys() == want.keys()
        for key in want:
            assert np.shape(got[key]) == np.shape(want[key]) and np.array_equal(got[key], want[key]), key
        # ... of a flow with something in every quantity: three samples at t = 0, 3, 6 on every ring, both bodies loaded, every probe owned once
        assert got["first_unstable_step"] == -1 and got["stats_samples"] == got["frames_pending"] == got["probes_pending"] == 3
        assert got["force_log"][:, 0].tolist() == [0, 3, 6] and got["body_force_log"][:, :2].tolist() == [[t, k] for t in (0, 3, 6) for k in (1, 2)]
        assert got["frame_steps"].tolist() == got["probe_steps"].tolist() == [0, 3, 6]
        assert got["frames"].shape == (3, 4, ny // K, NX // K) and got["probes"].shape == (3, len(XY), 3) and got["f_next"].shape == (ny + 2, NX + 2, 9)
        assert np.any(got["body_forces"] != 0.0) and np.all(got["probes"][:, :, 0] > 0.5) and np.any(got["frames"][2, 3] != 0.0)
        assert a.drain_frames() == [] and a.drain_probes()[1].shape == (0, len(XY), 3) and a.drain_force_log() == [] and a.drain_body_force_log() == []
        # the inverse of the statistics gather: every member is given its rows
        sums = np.arange(6 * ny * NX, dtype=np.float64).reshape(6, ny, NX)
        a.stats_restore(sums, 7)
        for c in a.ctxs:
            assert c.stats_samples() == 7 and np.array_equal(c.stats_sums(), sums[:, c.y_start:c.y_start + c.local_ny])
        with pytest.raises(ValueError):
            a.stats_restore(sums[:, 1:], 7)


@pytest.mark.parametrize("case", list(CASES))
def test_a_drain_takes_from_every_member_or_from_none(lbm, case):
    """One frame / probe sample drained from member 0 alone: the group's drain must refuse BEFORE it takes anything from any member."""
    with make(lbm, CASES[case]) as g:
        L, n = lbm.lib(), len(g.ctxs)
        assert len(g.ctxs[0].drain_frames(1)) == 1 and len(g.ctxs[0].drain_probes(1)[0]) == 1
        pending = [2] + [3] * (n - 1)
        with pytest.raises(lbm.LbmError, match="disagree"):
            g.drain_frames()
        assert [c.frames_pending() for c in g.ctxs] == pending
        with pytest.raises(lbm.LbmError, match="disagree"):
            g.drain_probes()
        assert [c.probes_pending() for c in g.ctxs] == pending
        # the library's drains themselves (Group asks for the pending count first), asked for ONE sample, which every member has
        ts, frames, vals = (C.c_int * 3)(), np.empty((3, 4, g.ny // K, NX // K), np.float32), np.empty((3, len(XY), 3))
        assert L.lbm_group_drain_frames(g._arr, n, ts, frames.ctypes.data_as(C.POINTER(C.c_float)), 1) == -1 and b"disagree" in L.lbm_last_error()
        assert L.lbm_group_drain_probes(g._arr, n, ts, vals.ctypes.data_as(C.POINTER(C.c_double)), 1) == -1 and b"disagree" in L.lbm_last_error()
        assert [c.frames_pending() for c in g.ctxs] == pending and [c.probes_pending() for c in g.ctxs] == pending
        # what is left is intact: member 0 still hands out t = 3, 6 and the others t = 0, 3, 6
        assert [[t for t, _ in c.drain_frames()] for c in g.ctxs] == [[3, 6]] + [[0, 3, 6]] * (n - 1)
        assert [c.drain_probes()[0].tolist() for c in g.ctxs] == [[3, 6]] + [[0, 3, 6]] * (n - 1)
