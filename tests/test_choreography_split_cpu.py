"""The choreography of a SPLIT whole-domain launch (option "split": a deep launch of the register family issued as 3 / 4 row-range kernels
round-robin on two streams, csrc/lbm_strips.inc.hpp issue_split), checked on the CPU with the detector of test_choreography_cpu.py.

The rule under test: kernel i of the issue order runs on stream i mod 2, records event i mod 3 and waits for the event of kernel i-3 —
one record and one wait per kernel. Claimed sufficient because a range kernel depends only on the three ranges around its own of the
previous launch (K_{i-n-1} .. K_{i-n+1}), never on K_{i-1}. `lbm_debug_choreography` runs the very functions that issue the launches on a
context without a device and replays the record with vector clocks: RACE = two conflicting accesses to a row that no event orders,
STALE = a launch reads a row that does not hold the iteration it starts from.
The enumeration: split 3 / 4 x plan depths 5 / 6 / 7 (and the tall fp32 shape) x both arithmetic modes (their regions differ) x walk
direction alternating or not x calls that may end on a fused launch or not x the call patterns of the strip test (remainders of every
depth, force outputs inside and between calls, two calls in a row) x heights from too short for the ranges (the launch then stays whole)
to 2048 rows."""
import ctypes as C
import importlib
import itertools
import re

import pytest

from tests.helpers import PKG


@pytest.fixture(scope="module")
def dry():
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    L = C.CDLL(pkg.lib_path())
    L.lbm_debug_choreography.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_int,
                                         C.c_int, C.c_char_p, C.c_int]
    L.lbm_last_error.restype = C.c_char_p
    out = C.create_string_buffer(1 << 20)

    def run(ny, options, calls, precision=0, dump=0, nx=256):
        b = (C.c_int * 2)(0, ny)           # one strip = the whole lattice: no internal face, no transport
        cl = (C.c_int * (2 * len(calls)))(*[v for p in calls for v in p])
        rc = L.lbm_debug_choreography(nx, ny, b, 1, precision, 0, " ".join(f"{k}={v}" for k, v in options.items()).encode(), cl,
                                      len(calls), dump, out, len(out))
        return rc, (out.value.decode() if rc >= 0 else L.lbm_last_error().decode())
    return run


PLANS = [(dict(deep=d, arith=a), 0) for d in (6, 7, 9) for a in (0, 1)] + [(dict(deep=8, arith=a), 1) for a in (0, 1)]
CALLS = [[(1, 0)], [(2, 0)], [(6, 0)], [(7, 0)], [(12, 0)], [(19, 0)], [(20, 0)], [(24, 0)], [(13, 0), (6, 0)], [(31, 7)], [(50, 13)], [(64, 8)], [(97, 0)],
         [(97, 31), (5, 0)], [(5, 0), (20, 0), (97, 10)], [(120, 0), (120, 0)]]
HEIGHTS = list(range(24, 132, 4)) + [133, 150, 177, 200, 256, 300, 401, 512, 777, 1024, 1500, 2048]


def kernels(text):
    """(stream, first row, end row) of every kernel of a dumped record"""
    return [(m.group(1), int(m.group(2)), int(m.group(3))) for m in re.finditer(r"(main|side) stream: kernel t=\d+ depth=\d+ writes buf \d rows \[(-?\d+),(-?\d+)\)", text)]


def test_split_launches_order_their_accesses_and_read_fresh_rows(dry):
    """No race and no stale read in the whole enumeration."""
    runs = 0
    for (plan, prec), sp, alt, tp, smin in itertools.product(PLANS, (3, 4), (0, 1), (0, 1), (1, 8)):
        # split_min 1: every deep launch is split, however short its segment; 8 (the default): sequences start only with eight launches ahead
        opts = dict(tune=0, nt=0, xcd=1, alternate=alt, trailing_pair=tp, split=sp, split_min=smin, **plan)
        for ny in HEIGHTS:
            for calls in CALLS:
                rc, text = dry(ny, opts, calls, prec)
                runs += 1
                assert rc == 0, f"{opts} ny {ny} calls {calls}: rc {rc}\n{text[:3000]}"
    assert runs > 40000


def test_the_ranges_are_really_issued_on_two_streams(dry):
    """What the test above checked was a split schedule: at 1024 rows every deep launch is n kernels over disjoint ranges that cover the
    lattice, alternating between the two streams, cut at multiples of the output height."""
    for sp in (3, 4):
        rc, text = dry(1024, dict(tune=0, nt=0, xcd=1, alternate=0, trailing_pair=1, split=sp, split_min=1, deep=7, arith=1), [(24, 0)], dump=1)
        assert rc == 0, text
        ks = kernels(text)
        assert len(ks) == 4 * sp, ks
        assert [k[0] for k in ks] == ["main", "side"] * (2 * sp)
        for g in range(4):
            grp = ks[g * sp:(g + 1) * sp]
            assert grp[0][1] == 0 and grp[-1][2] == 1024 and all(grp[j][2] == grp[j + 1][1] for j in range(sp - 1)), grp
            assert all(k[1] % 22 == 0 for k in grp), grp            # six iterations on 64 x 32 regions store 22 rows per band
            assert len({k[2] - k[1] for k in grp}) > 1              # unequal ranges
            assert grp[0][2] == ((7 if sp == 3 else 5) if g == 0 else (14 if sp == 3 else 10)) * 22, grp      # a short first range after a join
            assert all(k[2] - k[1] > 12 for k in grp)


def test_dropping_the_cross_stream_wait_is_flagged(dry):
    """Negative control (option "debug_skip_split_wait": kernel i does not wait for the event of kernel i-3): a race the detector names."""
    for sp, deep in itertools.product((3, 4), (6, 7, 9)):
        base = dict(tune=0, nt=0, xcd=1, alternate=0, trailing_pair=1, split=sp, split_min=1, deep=deep, arith=1)
        rc, text = dry(1024, base, [(60, 0)])
        assert rc == 0, text
        rc, text = dry(1024, dict(base, debug_skip_split_wait=1), [(60, 0)])
        assert rc > 0 and "RACE strip 0 buffer" in text and "side stream: kernel" in text and "main stream: kernel" in text, text


def test_a_lattice_too_short_for_the_ranges_keeps_the_single_launch(dry):
    """n ranges of more than 2 x depth rows each do not fit: the launch is issued whole, on the main stream, and nothing fails."""
    for sp, ny in ((3, 24), (4, 24), (3, 40), (4, 44)):
        rc, text = dry(ny, dict(tune=0, nt=0, xcd=1, alternate=0, trailing_pair=1, split=sp, split_min=1, deep=7, arith=1), [(24, 0)], dump=1)
        assert rc == 0, text
        ks = kernels(text)
        assert len(ks) == 4 and all(k == ("main", 0, ny) for k in ks), ks
    # ... and contexts that may not split at all: an LDS shape, a strip with a face
    rc, text = dry(1024, dict(tune=0, nt=1, xcd=1, split=3, split_min=1, deep=1), [(24, 0)], dump=1)
    assert rc == 0 and all(k == ("main", 0, 1024) for k in kernels(text)), text


def test_a_sequence_starts_only_with_enough_launches_ahead(dry):
    """The default "split_min" (8): a 20-iteration call (6 + 7 + 7) runs as three single launches; a 120-iteration call is split from its
    first launch to its last; with force outputs every 30 iterations (five launches a segment) nothing is split."""
    opts = dict(tune=0, nt=0, xcd=1, alternate=0, trailing_pair=1, split=3, deep=7, arith=1)
    rc, text = dry(1024, opts, [(20, 0)], dump=1)
    assert rc == 0 and kernels(text) == [("main", 0, 1024)] * 3, text
    rc, text = dry(1024, opts, [(120, 0)], dump=1)
    ks = kernels(text)
    assert rc == 0 and len(ks) == 60 and [k[0] for k in ks] == ["main", "side"] * 30, text
    rc, text = dry(1024, opts, [(120, 30)], dump=1)
    assert rc == 0 and all(k == ("main", 0, 1024) for k in kernels(text)), text
