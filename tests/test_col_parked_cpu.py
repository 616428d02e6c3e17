"""The 64x40 fp64 regions of the register kernel (plans `deep` 10 / 11) on the host side, no GPU: which contexts get the candidates, what
their kernel is called, and the choreography of `split` over their output heights (30 rows at six iterations, 28 at seven)."""
import itertools

from tests.test_bench_cpu import load_bench, plan_candidates
from tests.test_choreography_split_cpu import CALLS, HEIGHTS, dry, kernels  # noqa: F401

TALL = "64x40 in registers"


def names(nx, ny, precision, arith):
    return [c for c in plan_candidates(nx, ny, precision, arith) if TALL in c["name"]]


def test_candidates_for_fp64_contracted_whole_domains_only():
    """(A strip never reaches them: plan_candidates returns its strip lists first, and lbm_initialise refuses the pinned ids on anything but a
    whole domain — tests/test_gpu_col_parked.py.)"""
    for nx, ny in ((4096, 1024), (8192, 2048)):
        got = names(nx, ny, 0, 1)
        assert {(c["name"].split("/", 1)[1], c["options"].split("deep=")[1]) for c in got} == {
            ("6-step 64x40 in registers/nt-load/alternate/xcd", "10 ntl=1"), ("6-step 64x40 in registers/nt-load/xcd", "10 ntl=1"),
            ("6-step 64x40 in registers/alternate/xcd", "10"), ("6-step 64x40 in registers/nt-store/xcd", "10"),
            ("7-step 64x40 in registers/alternate/xcd", "11"), ("7-step 64x40 in registers/nt-load/xcd", "11 ntl=1"),
            ("7-step 64x40 in registers/nt-load/alternate/xcd", "11 ntl=1")}, got
        assert len(names(nx, ny, 0, 5)) == len(names(nx, ny, 0, 3)) == 7      # TRT and Smagorinsky have the shape
        for precision, arith in ((1, 1), (1, 0), (0, 0), (0, 2), (0, 4)):    # not fp32, not strict
            assert not names(nx, ny, precision, arith), (nx, ny, precision, arith)
    assert not names(1024, 256, 0, 1)                                    # fewer than six rounds of blocks


def test_kernel_names_parse():
    b = load_bench()
    for c in names(4096, 1024, 0, 1):
        depth = 6 if "deep=10" in c["options"] else 7
        assert b.kernel_family(c["kernel"]) == ("k_stepc_col", "double", depth, 5, 8), c
        assert b.plan_depth_of(c["kernel"]) == depth == int(c["depth"])
        assert c["kernel"] == "k_stepc_col<double,5,8,%d,%s,1>" % (depth, "true" if "nt=1" in c["options"] else "false")


def test_split_launches_over_the_new_output_heights(dry):
    """No race and no stale read, as tests/test_choreography_split_cpu.py holds it for the other plans."""
    runs = 0
    for deep, sp, alt, tp, smin in itertools.product((10, 11), (3, 4), (0, 1), (0, 1), (1, 8)):
        opts = dict(tune=0, nt=0, xcd=1, alternate=alt, trailing_pair=tp, split=sp, split_min=smin, deep=deep, arith=1)
        for ny in HEIGHTS:
            for calls in CALLS:
                rc, text = dry(ny, opts, calls, 0)
                runs += 1
                assert rc == 0, f"{opts} ny {ny} calls {calls}: rc {rc}\n{text[:3000]}"
    assert runs > 10000
    for deep, depth, oh in ((10, 6, 30), (11, 7, 28)):      # four launches of the plan's depth: twelve range kernels cut at multiples of its height
        rc, text = dry(1024, dict(tune=0, nt=0, xcd=1, alternate=0, trailing_pair=1, split=3, split_min=1, deep=deep, arith=1), [(4 * depth, 0)], dump=1)
        assert rc == 0, text
        ks = kernels(text)
        assert len(ks) == 12 and [k[0] for k in ks] == ["main", "side"] * 6, ks
        assert all(k[1] % oh == 0 for k in ks), ks
