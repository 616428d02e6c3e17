"""Option "split" on the GPU: a whole-domain deep launch of the register family issued as 3 / 4 row-range kernels on two streams
(csrc/lbm_strips.inc.hpp, issue_split) computes, bit for bit, what the single launch computes.

The ranges are cut at multiples of the launch's output height, so the tile grid is the single launch's and equality is exact, not a
tolerance: every comparison between `split` 3 / 4 and `split` 0 on the same plan below is np.array_equal. The ordering of the kernels
(events between the two streams) is what tests/test_choreography_split_cpu.py proves on the CPU; a missing dependency would show here
as a mismatch that comes and goes. "split_min" 1 makes every deep launch a split one, however few lie ahead (by default a sequence of
range launches starts only with eight launches ahead in its segment); the headline run at the end keeps the default."""
import numpy as np
import pytest

from tests.helpers import lbm_gpu, linf_rel, load_golden, golden_params, macro_errors  # noqa: F401

pytestmark = pytest.mark.gpu
TOL = 1e-10


COL6 = dict(tune=0, layout=1, pair_ty=12, xcd=1, deep=7)
# (precision, plan): fp64 contracted (the bench's mode), fp64 strict (64 x 24 regions), fp32 on 64 x 32 and on the tall 64 x 48 regions
VARIANTS = {
    "f64-contracted": ("f64", dict(COL6, nt=1, alternate=0, arith=1)),
    "f64-strict": ("f64", dict(COL6, nt=0, alternate=1, arith=0)),
    "f64-strict-col5": ("f64", dict(COL6, nt=1, alternate=0, arith=0, deep=6)),
    "f32": ("f32", dict(COL6, nt=0, ntl=1, alternate=1, arith=1)),
    "f32-tall": ("f32", dict(COL6, nt=0, alternate=0, arith=0, deep=8)),
}
NX, NY = 512, 300          # 300 rows: 14 bands of 22 rows, the last one partial; ranges of 4 / 5 / 5 bands


def mixed_calls(lbm, precision, plan, split, nx=NX, ny=NY, **kw):
    """step(5); step(20); step(97, of=10): full launches, remainders of every depth and force outputs inside a call."""
    with lbm.Context(nx, ny, precision=precision, options=dict(plan, split=split, split_min=1, timing=1), **kw) as c:
        solid = c.initialise()
        assert c.plan_options().get("split", 0) == split
        dispatches = launches = 0
        for n, of in ((5, 0), (20, 0), (97, 10)):
            c.step(n, of)
            launches += c.last_step_stats()[1]
            dispatches += c.last_step_dispatches()
        # the accessors right after a call whose deep launches were split
        out = dict(f_current=c.populations("f_current"), f_next=c.populations("f_next"), macros=c.macros(), umax=c.max_velocity_sq(),
                   log=c.drain_force_log(), forces=c.forces(), bad=c.first_unstable_step(), solid=solid, steps=c.steps_done)
        assert (dispatches > launches) if split else (dispatches == launches), (dispatches, launches)
        return out


def same(a, b):
    assert a["bad"] == b["bad"] and a["solid"] == b["solid"] and a["steps"] == b["steps"] == 122
    assert np.array_equal(a["f_next"], b["f_next"]) and np.array_equal(a["f_current"], b["f_current"])
    for u, v in zip(a["macros"], b["macros"]):
        assert np.array_equal(u, v)
    assert a["umax"] == b["umax"] and a["log"] == b["log"] and len(a["log"]) == 10 and a["forces"] == b["forces"]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_split_launches_equal_the_single_launch(lbm, variant):
    precision, plan = VARIANTS[variant]
    kw = dict(inlet_velocity=0.08)
    whole = mixed_calls(lbm, precision, plan, 0, **kw)
    assert whole["bad"] == -1
    for split in (3, 4):
        same(mixed_calls(lbm, precision, plan, split, **kw), whole)


def test_split_les_context(lbm):
    precision, plan = VARIANTS["f64-contracted"]
    kw = dict(inlet_velocity=0.08, smagorinsky=0.17)
    whole = mixed_calls(lbm, precision, plan, 0, **kw)
    for split in (3, 4):
        same(mixed_calls(lbm, precision, plan, split, **kw), whole)


def test_split_with_a_solid_mask_and_an_inlet_profile(lbm):
    precision, plan = VARIANTS["f64-strict"]
    solid = np.zeros((NY, NX), dtype=np.uint8)
    solid[80:100, 90:130] = 1          # a block across the first cut (row 88)
    solid[190:205, 300:310] = 1        # ... and one across the second (row 198)
    y = (np.arange(NY) + 0.5) / NY
    kw = dict(solid=solid, inlet_profile=0.09 * 4.0 * y * (1.0 - y))
    whole = mixed_calls(lbm, precision, plan, 0, **kw)
    assert whole["bad"] == -1 and whole["solid"] == int(solid.sum())
    for split in (3, 4):
        same(mixed_calls(lbm, precision, plan, split, **kw), whole)


@pytest.mark.parametrize("name", ["g8a_unstable_128x32", "g8b_unstable_128x32"])
def test_first_unstable_iteration(lbm, name):
    """The golden unstable cases (32 rows: too few for the ranges, the launches stay whole) and a lattice that does split."""
    g = load_golden(name)
    kw = golden_params(g)
    got = []
    for split in (0, 3, 4):
        with lbm.Context(options=dict(VARIANTS["f64-strict"][1], split=split, split_min=1), **kw) as c:
            c.initialise()
            c.step(int(g["p_steps"]), int(g["p_output_frequency"]))
            got.append(c.first_unstable_step())
    assert got == [int(g["unstable_t"])] * 3, got
    tall = dict(kw, ny=320)
    got = []
    for split in (0, 3, 4):
        with lbm.Context(options=dict(VARIANTS["f64-strict"][1], split=split, split_min=1), **tall) as c:
            c.initialise()
            assert c.plan_options().get("split", 0) == split
            c.step(int(g["p_steps"]), int(g["p_output_frequency"]))
            got.append(c.first_unstable_step())
    print(f"{name} at 320 rows: first unstable iteration {got}")
    assert got == [got[0]] * 3, got


def test_checkpoint_round_trip_of_a_split_context(lbm, tmp_path):
    precision, plan = VARIANTS["f64-contracted"]
    path = tmp_path / "split.ckpt"
    with lbm.Context(NX, NY, inlet_velocity=0.08, options=dict(plan, split=3, split_min=1)) as c:
        c.initialise()
        c.step(50, 0)          # ends on a single iteration behind split launches
        c.save_state(path)
        c.step(41, 0)
        want = c.populations("f_next")
    for split in (3, 0):
        with lbm.Context(NX, NY, inlet_velocity=0.08, options=dict(plan, split=split, split_min=1)) as c:
            c.initialise()
            c.load_state(path)
            c.step(41, 0)
            assert c.steps_done == 91 and np.array_equal(c.populations("f_next"), want)


def test_headline_grid_against_the_oracle(lbm):
    """4096x1024 x 300 iterations: strict populations bit-identical to the oracle, contracted macros and populations within 1e-10."""
    from oracle.oracle import Oracle, make_params
    nx, ny, steps = 4096, 1024, 300
    kw = dict(inlet_velocity=0.06510417)
    o = Oracle(make_params(nx, ny, **kw))
    assert o.run(steps) == -1
    for split in (3, 4):
        with lbm.Context(nx, ny, options=dict(COL6, nt=1, alternate=0, arith=0, split=split), **kw) as c:
            c.initialise()
            assert c.plan_options()["split"] == split
            c.step(steps, 0)
            assert c.first_unstable_step() == -1
            assert np.array_equal(c.populations("f_next"), o.f_next)
        with lbm.Context(nx, ny, options=dict(COL6, nt=1, alternate=0, arith=1, split=split), **kw) as c:
            c.initialise()
            c.step(steps, 0)
            assert c.first_unstable_step() == -1
            er, eu = macro_errors(*c.macros(), o.rho, o.ux, o.uy)
            ef = linf_rel(c.populations("f_next"), o.f_next)
            print(f"4096x1024 x {steps} contracted split {split}: rho {er:.2e} u {eu:.2e} f {ef:.2e}")
            assert er < TOL and eu < TOL and ef < TOL, (er, eu, ef)
    o.close()
