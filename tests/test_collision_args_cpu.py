"""The launch-uniform values of the collision models (csrc/lbm_collision.hpp: the values of each model, formed on the host, and the one
map of their names to the slots of the kernels' argument block), without a GPU: lbm_debug_collision_args fills the argument block of a
context no device knows as a launch would and reads the model's values back with the code the kernels read them with. Every value
must be the float64 evaluation of its formula, cast once to the element type: the library's host code is built without contraction,
so both sides are the same IEEE operations and equality is exact."""
import ctypes

import numpy as np
import pytest

from tests.helpers import lbm_cpu  # noqa: F401
from tests.test_mrt_cpu import setters

BGK, LES, TRT, FORCING, MRT, SPONGE = -1, 0, 1, 2, 3, 6      # lbm_debug_collision_setters' numbering; -1: no setter
BASE = {BGK: 0, LES: 2, TRT: 4, FORCING: 8, MRT: 16, SPONGE: 32}
GX, GY, HX, HY, U0, U1, U2 = range(7)                        # the seven shared slots, in the hook's order
OWNED = {BGK: (), LES: (U0, U1, U2), TRT: (U0, U1, U2), FORCING: (GX, GY, HX, HY), MRT: (GX, GY, U0, U1, U2), SPONGE: ()}
TAUS = (0.51, 0.6, 1.0)
PARAMS = {BGK: [(0.0, 0.0)], LES: [(0.1, 0.0), (0.17, 0.0)], TRT: [(3.0 / 16.0, 0.0), (0.25, 0.0)],
          FORCING: [(2e-5, -1e-5), (1e-6, 3e-6)], MRT: [(1.0, 3.0 / 16.0), (1.7, 0.25)], SPONGE: [(16, 1.5), (48, 2.0)]}
CASES = [(m, tau, p) for m in PARAMS for tau in TAUS for p in PARAMS[m]]


def expected(model, tau, v1, v2):
    """The model's named values in float64, in its struct's order: the issue's formulas in their order of operations."""
    tau, v1, v2 = np.float64(tau), np.float64(v1), np.float64(v2)
    half, one = np.float64(0.5), np.float64(1.0)
    wp = one / tau
    if model == BGK:
        return [wp]
    if model == LES:
        return [tau, tau * tau, np.float64(18.0) * np.sqrt(np.float64(2.0)) * (v1 * v1)]
    if model == FORCING:
        k = one - half * wp
        return [wp, k * v1, k * v2, half * v1, half * v2]
    if model == SPONGE:
        return []
    magic = v2 if model == MRT else v1
    wm = one / (half + magic / (tau - half))
    trt = [wp, wm, half * (wp + wm), half * (wp - wm)]
    return trt if model == TRT else trt + [v1, np.float64(0.25) * (v1 * tau - one)]


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model, tau, params", CASES)
def test_named_values_are_the_formulas_and_sit_in_the_models_own_slots(lbm, precision, model, tau, params):
    T = np.float64 if precision == "f64" else np.float32
    named, slots = lbm.debug_collision_args(tau, precision, model, *params)
    want = [np.float64(T(x)) for x in expected(model, tau, *params)]
    assert len(named) == len(want) and len(slots) == 7
    assert all(g == w for g, w in zip(named, want)), (named.tolist(), want)
    assert all(np.isfinite(named))
    # every shared slot the model does not own reads zero
    assert all(slots[i] == 0.0 for i in range(7) if i not in OWNED[model]), slots.tolist()
    # ... and its own slots are its values, name by name
    if model == LES:
        assert slots[[U0, U1, U2]].tolist() == named.tolist()                  # tau, tau^2, C
    if model in (TRT, MRT):
        assert slots[[U0, U1, U2]].tolist() == named[1:4].tolist()             # wm, wa, wb
    if model == MRT:
        assert slots[[GX, GY]].tolist() == named[4:6].tolist()                 # sb, kb
        assert slots[HX] == 0.0 and slots[HY] == 0.0
    if model == FORCING:
        assert slots[[GX, GY, HX, HY]].tolist() == named[1:5].tolist()         # gx, gy, hx, hy


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("model, tau, params", [c for c in CASES if c[0] in (LES, TRT, MRT)])
def test_values_are_those_of_the_context_the_setters_leave(lbm, precision, model, tau, params):
    """The same inputs through lbm_debug_collision_setters: the context holds the model, and (MRT) what lbm_get_mrt reports is what
    the argument block's sb, kb and the three rates were formed from."""
    T = np.float32 if precision else np.float64
    out, state = setters(lbm, [(model, params[0], params[1])], tau=tau, precision=precision)
    assert out == [(0, "")] and state[0] == BASE[model]
    named, _ = lbm.debug_collision_args(tau, precision, model, *params)
    assert len(named) == {LES: 3, TRT: 4, MRT: 6}[model]
    if model == MRT:
        assert state[1:] == params
        assert named.tolist() == [np.float64(T(x)) for x in expected(MRT, tau, state[1], state[2])]


def test_refusals(lbm):
    with pytest.raises(lbm.LbmError, match="lbm_debug_collision_args: setter -1, 0, 1, 2, 3 or 6 only"):
        lbm.debug_collision_args(0.6, "f64", 4)
    with pytest.raises(lbm.LbmError, match=r"lbm_set_mrt: tau = 0.5 \(the MRT rates need tau > 0.5\)"):
        lbm.debug_collision_args(0.5, "f64", MRT, 1.0, 0.25)
    fn = lbm.lib().lbm_debug_collision_args
    out = (ctypes.c_double * 16)()
    assert fn(0.6, 0, MRT, 1.0, 0.25, out, 12) == -1 and b"13 values, room for 12" in lbm.lib().lbm_last_error()
    assert fn(0.6, 0, MRT, 1.0, 0.25, out, 13) == 6
    assert fn(0.6, 0, BGK, 0.0, 0.0, None, 16) == -1
