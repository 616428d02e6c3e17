"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, exports every symbol that
include/lbm_hip.h declares, and refuses to run without a GPU (no CPU fallback). No compute calls here."""
import ctypes
import importlib
import os
import re

import pytest

from tests.helpers import PKG, ROOT


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG)
    p.build_all()
    return p


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lbm_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_expected_surface():
    syms = declared_symbols()
    for s in ("lbm_create", "lbm_destroy", "lbm_initialise", "lbm_step", "lbm_get_macros", "lbm_get_forces",
              "lbm_get_populations", "lbm_first_unstable_step", "lbm_max_velocity_sq", "lbm_comm_init",
              "lbm_halo_export", "lbm_halo_import"):
        assert s in syms


def test_library_exports_every_declared_symbol(pkg):
    lib = ctypes.CDLL(pkg.lib_path())
    for s in declared_symbols():
        assert hasattr(lib, s), f"liblbm_hip.so does not export {s}"


def test_library_carries_the_hash_of_its_sources(pkg):
    """build() ties the binary to the tree: the id embedded in the .so (readable without dlopen) == SHA-256 of csrc/* and
    include/lbm_hip.h == what lbm_build_id() returns; a stale .so is rebuilt (build.py)."""
    assert re.fullmatch(r"[0-9a-f]{16}", pkg.source_id())
    assert pkg.embedded_id() == pkg.source_id() == pkg.build_id()


def test_no_cpu_fallback(pkg):
    """Without a HIP device lbm_create must fail with LBM_ERR_HIP; with one this test is vacuous."""
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.LbmError, match="no HIP device"):
        pkg.Context(64, 32)


def test_product_sources_never_touch_the_oracle():
    """The oracle is test infrastructure: nothing under the package or include/ may reference it."""
    bad = []
    for base in (os.path.join(ROOT, PKG), os.path.join(ROOT, "include")):
        for d, _, files in os.walk(base):
            for f in files:
                if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp", "Makefile")):
                    txt = open(os.path.join(d, f), errors="ignore").read()
                    if re.search(r"lbm_oracle|oracle\.oracle|liblbm_oracle|lbmo_", txt):
                        bad.append(os.path.join(d, f))
    assert not bad, bad


def test_argument_errors_are_reported_without_a_device(pkg):
    """Error behaviour of the boundary (no exceptions across the C-ABI: negative codes + lbm_last_error text)."""
    import ctypes as C
    L = pkg.lib()
    h = C.c_void_p()
    assert L.lbm_create(None, 0, C.byref(h)) == -1 and b"null" in L.lbm_last_error()
    p = pkg.Params(0.6, 0.01, 0, 32, 0.2, 0.5, 0.05, 0, 0, 0, 0)           # nx = 0
    assert L.lbm_create(C.byref(p), 0, C.byref(h)) == -1 and b"bad nx/ny/tau" in L.lbm_last_error()
    p = pkg.Params(0.6, 0.01, 64, 32, 0.2, 0.5, 0.05, 0, 0, 7, 0)          # unknown precision
    assert L.lbm_create(C.byref(p), 0, C.byref(h)) == -1 and b"precision" in L.lbm_last_error()
    assert L.lbm_step(None, 1, 0) == -1
    assert L.lbm_steps_done(None) == -1
    assert L.lbm_set_option(None, b"tune", 0) == -1
    L.lbm_destroy(None)                                                     # destroying nothing is a no-op


def test_group_gathers_refuse_an_empty_group_without_a_device(pkg):
    """Every lbm_group_* gather starts with the group check: a null group or n < 1 is LBM_ERR_ARG, whatever else is passed."""
    import ctypes as C
    L = pkg.lib()
    one = (C.c_void_p * 1)(None)
    t, v, rows, brows = C.c_int(), C.c_double(), (pkg.binding.ForceRow * 1)(), (pkg.binding.BodyForceRow * 1)()
    f = (C.c_float * 1)()
    dv = C.byref(v)
    calls = {"first_unstable_step": (C.byref(t),), "max_velocity_sq": (dv,), "get_forces": (dv, dv), "drain_force_log": (rows, 1),
             "get_body_forces": (dv,), "drain_body_force_log": (brows, 1), "get_macros": (dv, dv, dv), "get_populations": (0, dv),
             "stats_samples": (), "get_stat_sums": (dv,), "stats_restore": (dv, 0), "frames_pending": (), "probes_pending": (),
             "drain_frames": (C.byref(t), f, 1), "drain_probes": (C.byref(t), dv, 1)}
    for name, rest in calls.items():
        fn = getattr(L, "lbm_group_" + name)
        assert fn(None, 1, *rest) == -1 and b"empty group" in L.lbm_last_error(), name
        assert fn(one, 0, *rest) == -1 and b"empty group" in L.lbm_last_error(), name
        assert fn(one, 1, *rest) == -1 and b"null context in group" in L.lbm_last_error(), name
    assert L.lbm_debug_gather(0, 0, None, 8, 8, 1, 1, None, None) == -1 and b"bad argument" in L.lbm_last_error()


def test_strip_schedule_pins_are_agreed_over_the_ranks(pkg):
    """the schedule trials of lbm_initialise are collective, so ranks with different overlap / deep_halo pins must get
    an error on every rank, not a different number of trials (a hang in RCCL). lbm_debug_strip_pins runs the very decision
    functions of tune_strip_schedule (strip_pins_pack -> MIN over the ranks -> strip_pins_agree) without a device."""
    lib = ctypes.CDLL(pkg.lib_path())
    lib.lbm_debug_strip_pins.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]

    def agree(ranks):
        ranks = [tuple(r) + (0, 0) if len(r) == 5 else tuple(r) for r in ranks]        # (halo_trim unpinned unless given)
        flat = (ctypes.c_int * (7 * len(ranks)))(*[v for r in ranks for v in r])
        out = (ctypes.c_int * 7)()
        rc = lib.lbm_debug_strip_pins(flat, len(ranks), out)
        return rc, list(out)[:5], list(out)[5:]

    # nobody pins anything: tune, nothing pinned
    assert agree([(1, 0, 1, 0, 1)] * 4)[:2] == (0, [1, 0, -1, 0, -1])
    # everybody pins overlap=2: agreed, the deep-halo half is still measured
    assert agree([(1, 1, 2, 0, 1)] * 3)[:2] == (0, [1, 1, 2, 0, -1])
    # one strip too short to tune: nobody tunes
    rc, out, _ = agree([(1, 0, 1, 0, 1), (0, 0, 1, 0, 1)])
    assert rc == 0 and out[0] == 0
    # one rank pins overlap, the other does not / pins another value: error on every rank
    assert agree([(1, 1, 1, 0, 1), (1, 0, 1, 0, 1)])[0] < 0
    assert agree([(1, 1, 1, 0, 1), (1, 1, 0, 0, 1)])[0] < 0
    assert agree([(1, 0, 1, 1, 0), (1, 0, 1, 1, 1)])[0] < 0
    # the message trimming (round 5) is a third pin of the same kind
    assert agree([(1, 0, 1, 0, 1, 1, 1)] * 2) == (0, [1, 0, -1, 0, -1], [1, 1])
    assert agree([(1, 0, 1, 0, 1, 1, 1), (1, 0, 1, 0, 1, 0, 0)])[0] < 0 and agree([(1, 0, 1, 0, 1, 1, 1), (1, 0, 1, 0, 1, 1, 0)])[0] < 0
    # both halves pinned alike everywhere
    assert agree([(1, 1, 0, 1, 1)] * 8)[:2] == (0, [1, 1, 0, 1, 1])


def test_the_trimmed_halo_message_is_exactly_what_the_receiver_reads(pkg):
    """Option "halo_trim" (round 5, VERDICT r04 #7a): of the hr rows of a face an exchange need carry only what can still reach the
    strip in the hr iterations until the next exchange. Derived here independently of the library from the dependency cone — ghost
    row g (1 = next to the strip) is read for level 1 of rows g-1, g, g+1, and level 1 is computed on rows 1 .. hr-1 only: population
    i of row g travels iff some row in 1 .. hr-1 pulls it, i.e. iff g - cy_toward(i) is such a row — and compared with the runs the
    transports walk (lbm_debug_face_runs), for every frame depth the schedules use (six, seven, eight and twelve rows)."""
    lib = ctypes.CDLL(pkg.lib_path())
    lib.lbm_debug_face_runs.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)]
    cy = [0, 0, 1, 0, -1, 1, 1, -1, -1]
    for hr in (6, 7, 8, 12):
        for south_block in (1, 0):
            out = (ctypes.c_int * 10)()
            n = lib.lbm_debug_face_runs(hr, 1, south_block, out)
            assert n == 5
            got = set()
            for k in range(n):
                assert out[2 * k + 1] > 0
                got |= set(range(out[2 * k], out[2 * k] + out[2 * k + 1]))
            assert len(got) == sum(out[2 * k + 1] for k in range(n)) == 9 * hr - 9        # disjoint runs, 45 of 54 at six rows
            want = set()
            for g in range(1, hr + 1):
                # memory row of ghost row g inside the block: a block below its strip stores the outermost row first
                mem = hr - g if south_block else g - 1
                for i in range(9):
                    toward = cy[i] if south_block else -cy[i]        # +1: the population moves towards the strip, -1: away from it
                    puller = g - toward                               # the ghost row (0 = the strip's own edge row) whose level 1 pulls it
                    if 0 <= puller <= hr - 1:
                        want.add(9 * mem + i)
            assert got == want, (hr, south_block, sorted(want - got), sorted(got - want))
            assert lib.lbm_debug_face_runs(hr, 0, south_block, out) == 1 and (out[0], out[1]) == (0, 9 * hr)


def test_group_threads_rendezvous_is_bounded_and_names_the_straggler(pkg):
    """VERDICT r04 #1, on the CPU: the host threads of an in-process group (GroupPool: one per strip, three rendezvous per launch) on a
    dummy job, through lbm_debug_group_pool. (a) a clean job passes every rendezvous, again and again on the same pool; (b) a strip that
    reports an error between two rendezvous makes every thread leave at the SAME rendezvous (none is left waiting) and the caller gets the
    strip's error; (c) a strip that stalls turns into LBM_ERR_TIMEOUT within the bound, naming it and where it was last seen — rounds 3-4
    waited on a std::barrier without a time-out; (d) tearing the pool down after a time-out waits for the straggler instead of hanging."""
    import time
    lib = ctypes.CDLL(pkg.lib_path())
    lib.lbm_debug_group_pool.argtypes = [ctypes.c_int] * 7 + [ctypes.c_long, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.lbm_last_error.restype = ctypes.c_char_p
    passed = ctypes.c_int()

    def pool(n, rounds, fail=(-1, -1), stall=(-1, -1, 0), timeout_ms=0, repeat=1):
        rc = lib.lbm_debug_group_pool(n, rounds, fail[0], fail[1], stall[0], stall[1], stall[2], timeout_ms, repeat, ctypes.byref(passed))
        return rc, passed.value, (lib.lbm_last_error().decode() if rc else "")

    assert pool(8, 300, repeat=5) == (0, 300, "")
    assert pool(2, 50) == (0, 50, "") and pool(5, 7, repeat=3) == (0, 7, "")
    rc, done, msg = pool(6, 40, fail=(3, 17), repeat=2)          # the first run of the pool is clean, the second fails in round 17
    assert rc == -2 and done == 17 and "injected fault: strip 3, round 17" in msg
    t0 = time.time()
    rc, done, msg = pool(4, 20, stall=(2, 9, 1500), timeout_ms=200)
    assert rc == -5 and done == 9, (rc, done, msg)
    assert "waited 200 ms at rendezvous 1 of launch 9 of this call for: strip 2 (last seen at rendezvous 1 of launch 8)" in msg, msg
    assert 0.2 <= time.time() - t0 < 6.0          # the bound, then the teardown waits for the straggler's 1.5 s sleep: no hang, no crash
    rc, done, msg = pool(3, 5, stall=(0, 2, 600), timeout_ms=150)      # the CALLER's own strip is the slow one: the others time out on it
    assert rc == -5 and "for: strip 0 (last seen at rendezvous 1 of launch 1)" in msg, msg

