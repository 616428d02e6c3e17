"""The LDS tile kernels of three to eight iterations (k_step3_tile, k_step4_tile, k_stepd_tile: one body, step_tile in
csrc/lbm_kernels.hpp) on two lattices that between them reach every kind of block and every class of region cell.

200x100: three tile columns and at least three tile rows of every shape up to 32x32 at eight iterations, so LEAN tiles, general
tiles, a partial last column (8 cells) and a partial last band occur in one launch. 70x20: narrower than two tiles and lower than
one 32-row tile, so every block is general and region cells lie outside the domain on both sides at once. Each lattice carries the
default disc and one solid cell on a tile edge.

Two calls of 17 and 5 iterations, in two series. With a force output every 4 iterations no launch is deeper than four (a launch
ends where an output needs the state in memory): remainder depths and segment ends occur, and the deep plans run entirely on the
two- to four-iteration kernels. With an output every 16 the first call holds one segment of 16 iterations, which a deep plan
runs at its own depth (6 + 6 + 4, 7 + 7 + 2, 8 + 8); that k_stepd_tile ran is asserted by the launch count, since kernel_name()
names the plan, not the launches: no kernel but the plan's own fuses more than four iterations, so fewer than 16 / 4 launches for
that segment contain one.

fp64 against the stepwise oracle at the bars of tests/helpers.py assert_matches_reference (strict: f_next bit for bit, rho within
1e-14; contracted: 1e-10); fp32 (held to a float32 reference in tests/test_gpu_f32_oracle.py) bit for bit against the same context stepped one iteration per launch."""
import functools

import numpy as np
import pytest

from oracle.oracle import Oracle, make_params
from tests.helpers import assert_matches_reference, lbm_gpu, u_bar_rel, where  # noqa: F401
from tests.reference import oracle_run

pytestmark = pytest.mark.gpu

CALLS = (17, 5)
SERIES = [4, 16]                # output_frequency: segments of at most four iterations / one segment of 16 in the first call
KW = dict(inlet_velocity=0.05)
LATTICES = {(200, 100): (128, 48), (70, 20): (64, 8)}      # lattice -> the solid cell: first column of a tile, first row of a band
BASE = dict(tune=0, layout=1, nt=1, alternate=0, xcd=1, timing=1)
TILE_PLANS = {       # plan -> (options, the kernel family its name must show)
    "fuse3-8": (dict(fuse=3, pair_ty=8), "k_step3_tile<%s,8,512,"),
    "fuse3-12": (dict(fuse=3, pair_ty=12), "k_step3_tile<%s,12,1024,"),
    "fuse4": (dict(fuse=4, pair_ty=8), "k_step4_tile<%s,8,"),
    "deep6": (dict(pair_ty=12, deep=1), "k_stepd_tile<%s,64,16,6,"),
    "deep7": (dict(pair_ty=12, deep=2), "k_stepd_tile<%s,64,16,7,"),
    "deep8": (dict(pair_ty=12, deep=3), "k_stepd_tile<%s,32,32,8,"),
}
cases = pytest.mark.parametrize("lattice,of,plan,arith", [(l, of, p, a) for l in LATTICES for of in SERIES for p in TILE_PLANS for a in (0, 1)],
                                ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))


@functools.lru_cache(maxsize=None)
def mask_of(nx, ny):
    o = Oracle(make_params(nx, ny, **KW))
    m = np.array(o.solid, dtype=np.uint8).reshape(ny, nx).copy()
    o.close()
    assert m.any()                                            # the default disc
    x, y = LATTICES[(nx, ny)]
    assert m[y, x] == 0
    m[y, x] = 1
    m.flags.writeable = False
    return m


@functools.lru_cache(maxsize=None)
def reference(nx, ny, of):
    """The oracle after sum(CALLS) iterations: once per lattice and series, shared, read-only."""
    ref = oracle_run(nx, ny, sum(CALLS), of, mask=mask_of(nx, ny), **KW)
    assert ref.first_unstable == -1 and np.all(np.isfinite(ref.f_next))
    for a in (ref.f_next, ref.rho, ref.ux, ref.uy):
        a.flags.writeable = False
    return ref


def run(lbm, nx, ny, of, opts, **kw):
    """Both calls; returns (solid count, first unstable step, f_next, macros, force log, kernel name, launches per call)."""
    with lbm.Context(nx, ny, options=opts, solid=np.array(mask_of(nx, ny)), **KW, **kw) as ctx:
        count = ctx.initialise()
        launches = []
        for n in CALLS:
            ctx.step(n, of)
            _, nl, ni = ctx.last_step_stats()
            assert ni == n
            launches.append(nl)
        return (count, ctx.first_unstable_step(), ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log(),
                ctx.kernel_name().replace(" ", ""), launches)


def assert_family_ran(plan, of, launches):
    """The launches of the first call: a segment of min(of, 16) iterations from t = 0, then what is left of the 17."""
    if of == 4:
        assert launches[0] >= 5, launches                     # no launch crosses an output iteration
    elif plan.startswith("deep"):
        assert launches[0] < 16 // 4 + 1, launches            # the segment of 16 in fewer than four launches, + the seventeenth
    else:
        assert launches[0] <= 16 // 3 + 1 + 1, launches       # five launches of three (or four of four) and the remainders


_site_f32 = {}


def site_f32(lbm, nx, ny, of, arith):
    key = (nx, ny, of, arith)
    if key not in _site_f32:
        _site_f32[key] = run(lbm, nx, ny, of, dict(BASE, fuse=1, arith=arith), precision="f32")
        assert _site_f32[key][5].startswith("k_step_site<float,") and _site_f32[key][6] == list(CALLS)
    return _site_f32[key]


@cases
def test_fp64_against_the_oracle(lbm, lattice, of, plan, arith):
    nx, ny = lattice
    opts, name = TILE_PLANS[plan]
    ref = reference(nx, ny, of)
    count, bad, fn, macros, log, kernel, launches = run(lbm, nx, ny, of, dict(BASE, arith=arith, **opts))
    assert kernel.startswith(name % "double") and kernel.endswith(",%d>" % arith), kernel
    assert_family_ran(plan, of, launches)
    assert count == ref.solid_count and bad == -1
    assert_matches_reference(arith, fn, macros, log, ref, u_bar_rel(ref))


@cases
def test_fp32_against_one_iteration_per_launch(lbm, lattice, of, plan, arith):
    nx, ny = lattice
    opts, name = TILE_PLANS[plan]
    count, bad, fn, macros, log, kernel, launches = run(lbm, nx, ny, of, dict(BASE, arith=arith, **opts), precision="f32")
    rcount, rbad, rfn, rmacros, rlog, _, _ = site_f32(lbm, nx, ny, of, arith)
    assert kernel.startswith(name % "float") and kernel.endswith(",%d>" % arith), kernel
    assert_family_ran(plan, of, launches)
    assert count == rcount == int(mask_of(nx, ny).sum()) and bad == rbad == -1
    assert np.all(np.isfinite(rfn)) and np.array_equal(fn, rfn), where(fn, rfn)
    for u, v in zip(macros, rmacros):
        assert np.array_equal(u, v)
    assert log == rlog and [r[0] for r in log] == [t for t in range(sum(CALLS)) if t % of == 0]
