"""The table behind option "deep" (csrc/lbm_plan.hpp: region_kinds, deep_shapes), without a GPU. Everything that launches, names or
refuses a deep shape reads that table, so three things are held against literals here: the table itself as lbm_debug_deep_shapes prints
it; the launch depths plan_launch derives from it, as the dry run (lbm_debug_choreography) recorded them on the commit before the table
existed; and which (id, precision, arithmetic, extent) the library refuses, with the words of the refusal."""
import ctypes as C
import importlib
import re

import pytest

from tests.helpers import PKG, deep_shapes

IDS = (1, 2, 3, 6, 7, 9, 8, 10, 11)
STD = ((5, "nt+plain", False), (6, "nt+plain", False), (7, "plain", True))           # (depth, store policies built, barred with a strip face)
TALL = ((6, "plain", False), (7, "plain", False), (8, "plain", True))
PARK = ((5, "nt+plain", False), (6, "nt+plain", False), (7, "plain", False))
ALL4 = (("f64", 0), ("f64", 1), ("f32", 0), ("f32", 1))
# id: (family, iterations per launch, {(precision, contracted): (width, height, rows per thread, waves)}, offered depths, restrictions)
TABLE = {
    1: ("lds", 6, {k: (64, 16, 1, 16) for k in ALL4}, ((6, "", False),), ""),
    2: ("lds", 7, {k: (64, 16, 1, 16) for k in ALL4}, ((7, "", False),), ""),
    3: ("lds", 8, {k: (32, 32, 1, 16) for k in ALL4}, ((8, "", False),), ""),
    6: ("registers", 5, {("f64", 0): (64, 24, 2, 12), ("f64", 1): (64, 32, 4, 8), ("f32", 0): (64, 32, 4, 8), ("f32", 1): (64, 32, 4, 8)}, STD, ""),
    7: ("registers", 6, {("f64", 0): (64, 24, 2, 12), ("f64", 1): (64, 32, 4, 8), ("f32", 0): (64, 32, 4, 8), ("f32", 1): (64, 32, 4, 8)}, STD, ""),
    9: ("registers", 7, {("f64", 0): (64, 24, 2, 12), ("f64", 1): (64, 32, 4, 8), ("f32", 0): (64, 32, 4, 8), ("f32", 1): (64, 32, 4, 8)}, STD, ""),
    8: ("registers", 7, {("f32", 0): (64, 48, 6, 8), ("f32", 1): (64, 48, 4, 12)}, TALL, "fp32 only, model flag tall"),
    10: ("registers", 6, {("f64", 1): (64, 40, 5, 8)}, PARK, "fp64 only, contracted arithmetic on whole domains, model flag park"),
    11: ("registers", 7, {("f64", 1): (64, 40, 5, 8)}, PARK, "fp64 only, contracted arithmetic on whole domains, model flag park"),
}

CALLS = ((5, 0), (6, 0), (7, 0), (8, 0), (13, 0), (20, 0), (31, 7))
# (id, extent, trailing_pair): the depths of the launches of each call of CALLS, recorded from the dry run of the commit before the
# table (256 columns; "whole": 200 rows on their own; "middle": rows 200..399 of 600, one rank of a multi-process run with both faces;
# fp64, id 8 fp32; contracted arithmetic). 20 = 7 + 7 + 6 in registers on a whole domain; a strip's ghost rows bar the seventh iteration
# of the 64x32 regions' remainders and the eighth of the 64x48 ones. Ids 10 / 11 exist on whole domains only.
LAUNCHES = {
    (1, "whole", 0): [[4, 1], [2, 3, 1], [6, 1], [3, 4, 1], [6, 6, 1], [6, 6, 3, 4, 1], [3, 4, 3, 4, 3, 4, 3, 4, 2, 1]],
    (1, "whole", 1): [[2, 3], [6], [3, 4], [4, 4], [6, 3, 4], [6, 6, 4, 4], [3, 4, 3, 4, 3, 4, 3, 4, 3]],
    (1, "middle", 0): [[1, 3, 1], [2, 3, 1], [6, 1], [6, 1, 1], [6, 6, 1], [6, 6, 6, 1, 1], [6, 1, 6, 1, 6, 1, 6, 1, 2, 1]],
    (1, "middle", 1): [[2, 3], [6], [6, 1], [6, 2], [6, 6, 1], [6, 6, 6, 2], [6, 1, 6, 1, 6, 1, 6, 1, 3]],
    (2, "whole", 0): [[4, 1], [2, 3, 1], [3, 3, 1], [7, 1], [4, 4, 4, 1], [7, 4, 4, 4, 1], [7, 7, 7, 7, 2, 1]],
    (2, "whole", 1): [[2, 3], [3, 3], [7], [4, 4], [7, 3, 3], [7, 7, 3, 3], [7, 7, 7, 7, 3]],
    (2, "middle", 0): [[1, 3, 1], [2, 3, 1], [3, 3, 1], [7, 1], [7, 2, 3, 1], [7, 7, 2, 3, 1], [7, 7, 7, 7, 2, 1]],
    (2, "middle", 1): [[2, 3], [3, 3], [7], [7, 1], [7, 3, 3], [7, 7, 3, 3], [7, 7, 7, 7, 3]],
    (3, "whole", 0): [[4, 1], [2, 3, 1], [3, 3, 1], [3, 4, 1], [8, 4, 1], [8, 8, 3, 1], [3, 4, 3, 4, 3, 4, 3, 4, 2, 1]],
    (3, "whole", 1): [[2, 3], [3, 3], [3, 4], [8], [8, 2, 3], [8, 8, 4], [3, 4, 3, 4, 3, 4, 3, 4, 3]],
    (3, "middle", 0): [[1, 3, 1], [2, 3, 1], [3, 3, 1], [1, 3, 3, 1], [3, 3, 3, 3, 1], [8, 8, 3, 1], [1, 3, 3, 1, 3, 3, 1, 3, 3, 1, 3, 3, 2, 1]],
    (3, "middle", 1): [[2, 3], [3, 3], [1, 3, 3], [8], [8, 2, 3], [8, 3, 3, 3, 3], [1, 3, 3, 1, 3, 3, 1, 3, 3, 1, 3, 3, 3]],
    (6, "whole", 0): [[4, 1], [5, 1], [6, 1], [7, 1], [5, 7, 1], [5, 7, 7, 1], [7, 7, 7, 7, 2, 1]],
    (6, "whole", 1): [[5], [6], [7], [5, 3], [6, 7], [5, 5, 5, 5], [7, 7, 7, 7, 3]],
    (6, "middle", 0): [[1, 3, 1], [5, 1], [6, 1], [5, 2, 1], [6, 6, 1], [5, 5, 3, 6, 1], [5, 2, 5, 2, 5, 2, 5, 2, 2, 1]],
    (6, "middle", 1): [[5], [6], [5, 2], [5, 3], [5, 5, 3], [5, 5, 5, 5], [5, 2, 5, 2, 5, 2, 5, 2, 3]],
    (7, "whole", 0): [[4, 1], [5, 1], [6, 1], [7, 1], [6, 6, 1], [6, 6, 7, 1], [7, 7, 7, 7, 2, 1]],
    (7, "whole", 1): [[5], [6], [7], [3, 5], [6, 7], [6, 7, 7], [7, 7, 7, 7, 3]],
    (7, "middle", 0): [[1, 3, 1], [5, 1], [6, 1], [2, 5, 1], [6, 6, 1], [6, 3, 5, 5, 1], [2, 5, 2, 5, 2, 5, 2, 5, 2, 1]],
    (7, "middle", 1): [[5], [6], [2, 5], [3, 5], [3, 5, 5], [5, 5, 5, 5], [2, 5, 2, 5, 2, 5, 2, 5, 3]],
    (9, "whole", 0): [[4, 1], [5, 1], [6, 1], [7, 1], [7, 5, 1], [7, 7, 5, 1], [7, 7, 7, 7, 2, 1]],
    (9, "whole", 1): [[5], [6], [7], [3, 5], [7, 6], [7, 7, 6], [7, 7, 7, 7, 3]],
    (9, "middle", 0): [[1, 3, 1], [5, 1], [6, 1], [7, 1], [7, 5, 1], [7, 7, 5, 1], [7, 7, 7, 7, 2, 1]],
    (9, "middle", 1): [[5], [6], [7], [3, 5], [7, 6], [7, 7, 6], [7, 7, 7, 7, 3]],
    (8, "whole", 0): [[4, 1], [2, 3, 1], [6, 1], [7, 1], [6, 6, 1], [7, 6, 6, 1], [7, 7, 7, 7, 2, 1]],
    (8, "whole", 1): [[2, 3], [6], [7], [8], [7, 6], [7, 7, 6], [7, 7, 7, 7, 3]],
    (8, "middle", 0): [[1, 3, 1], [2, 3, 1], [6, 1], [7, 1], [6, 6, 1], [7, 6, 6, 1], [7, 7, 7, 7, 2, 1]],
    (8, "middle", 1): [[2, 3], [6], [7], [2, 6], [7, 6], [7, 7, 6], [7, 7, 7, 7, 3]],
    (10, "whole", 0): [[4, 1], [5, 1], [6, 1], [7, 1], [6, 6, 1], [6, 6, 7, 1], [7, 7, 7, 7, 2, 1]],
    (10, "whole", 1): [[5], [6], [7], [3, 5], [6, 7], [6, 7, 7], [7, 7, 7, 7, 3]],
    (11, "whole", 0): [[4, 1], [5, 1], [6, 1], [7, 1], [7, 5, 1], [7, 7, 5, 1], [7, 7, 7, 7, 2, 1]],
    (11, "whole", 1): [[5], [6], [7], [3, 5], [7, 6], [7, 7, 6], [7, 7, 7, 7, 3]],
}
EXTENTS = {"whole": ([(0, 200)], 200, 0), "middle": ([(200, 200)], 600, 2)}      # bounds, rows of the lattice, transport


@pytest.fixture(scope="module")
def dry():
    """(return code, the record's dump or the refusal) of a dry run of one strip; lbm_set_option and the check of lbm_initialise refuse in it
    as they do on a device."""
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    L = C.CDLL(pkg.lib_path())
    L.lbm_debug_choreography.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_int,
                                         C.c_int, C.c_char_p, C.c_int]
    L.lbm_last_error.restype = C.c_char_p
    out = C.create_string_buffer(1 << 16)

    def run(extent, precision, options, call=(1, 0), bounds=None):
        b, ny, transport = EXTENTS[extent]
        b = bounds or b
        ba = (C.c_int * (2 * len(b)))(*[v for p in b for v in p])
        rc = L.lbm_debug_choreography(256, ny, ba, len(b), int(precision == "f32"), transport, " ".join(f"{k}={v}" for k, v in options.items()).encode(),
                                      (C.c_int * 2)(*call), 1, 1, out, len(out))
        return rc, (out.value.decode() if rc >= 0 else L.lbm_last_error().decode())
    return run


def test_the_table_is_the_one_written_here():
    rows = deep_shapes()
    assert sorted({k[0] for k in rows}) == sorted(IDS)
    assert sorted(rows) == sorted((i, p, a) for i, (_, _, shapes, _, _) in TABLE.items() for p, a in shapes)
    for (i, p, a), row in rows.items():
        family, depth, shapes, offered, only = TABLE[i]
        assert (row.family, row.depth, (row.w, row.h, row.rows, row.waves), row.offered, row.only) == (family, depth, shapes[p, a], offered, only), row
        assert row.arith == ("contracted" if a else "strict") and depth in [d for d, _, _ in offered], row


@pytest.mark.parametrize("deep", IDS)
def test_launch_depths_are_the_recorded_ones(dry, deep):
    precision = "f32" if deep == 8 else "f64"
    for extent in EXTENTS:
        for tp in (0, 1):
            if (deep, extent, tp) not in LAUNCHES:
                assert deep in (10, 11) and extent == "middle"
                continue
            got = []
            for call in CALLS:
                rc, text = dry(extent, precision, dict(tune=0, nt=1, xcd=1, trailing_pair=tp, deep=deep, arith=1), call)
                assert rc == 0, text
                depth_at = {int(t): int(d) for t, d in re.findall(r"kernel t=(\d+) depth=(\d+)", text)}        # (a strip's edge bands: a second kernel)
                got.append([depth_at[t] for t in sorted(depth_at)])
                assert sum(got[-1]) == call[0]
            assert got == LAUNCHES[deep, extent, tp], (deep, extent, tp)


def test_refused_exactly_where_the_table_says(dry):
    accepted = 0
    for deep in IDS:
        for precision, arith, extent in ((p, a, e) for p in ("f64", "f32") for a in (0, 1) for e in EXTENTS):
            rc, text = dry(extent, precision, dict(tune=0, deep=deep, arith=arith))
            shapes, only = TABLE[deep][2], TABLE[deep][4]
            if not any(p == precision for p, _ in shapes):          # lbm_set_option: the precision is the context's
                assert rc < 0 and ("fp32 only" if "fp32 only" in only else "fp64 only") in text and "deep %d (64x4" % deep in text, (deep, precision, text)
            elif (precision, arith) not in shapes or ("whole domains" in only and extent != "whole"):       # the check of lbm_initialise
                assert rc < 0 and "deep %d (64x40 regions in registers) exists for contracted arithmetic on whole domains only" % deep in text, (deep, text)
            else:
                assert rc == 0, (deep, precision, arith, extent, text)
                accepted += 1
    assert accepted == 6 * 8 + 4 + 2
    for deep in (10, 11):       # the other extents that are no whole domain: a strip exchanging with itself, a strip of an in-process group
        for b, transport in (([(0, 200)], "loopback"), ([(0, 100), (100, 100)], "whole")):
            rc, text = dry("whole", "f64", dict(tune=0, deep=deep, arith=1, **({"loopback": 1} if transport == "loopback" else {})), bounds=b)
            assert rc < 0 and "contracted arithmetic on whole domains only" in text, (deep, b, text)
    for deep in (-1, 4, 5, 12):
        rc, text = dry("whole", "f64", dict(tune=0, deep=deep))
        assert rc < 0 and "deep must be 0..3 or 6..11 (4 / 5, round 2's 32x16 LDS tiles, are retired)" in text, (deep, text)
    assert dry("whole", "f64", dict(tune=0, deep=0))[0] == 0
