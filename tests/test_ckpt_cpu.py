"""The head of a checkpoint file (csrc/lbm_ckpt.hpp) without a device, through the two hooks that run the very functions lbm_save_state and
lbm_load_state call: lbm_debug_ckpt_save (a described context -> the bytes of its head) and lbm_debug_ckpt_load (bytes + a described
loading context -> the bytes consumed, or lbm_load_state's refusal).

The expectations are stated here, independently of the library: `pack` writes a head from the documented format with struct.pack, and
`first_difference` is the order in which lbm_load_state has always named what differs — the collision models forcing, TRT, Smagorinsky,
then the walls, the inlet profile, the inlet schedule, the obstacle mask, and last the fixed header. The space of described runs is taken
whole: mask x profile x collision in {none, LES, TRT, forced} x walls x schedule = 64 descriptions on one fixed header (the grid does not
matter to the head: 128 x 32)."""
import collections
import ctypes
import importlib
import itertools
import struct

import numpy as np
import pytest

from tests.helpers import PKG

FIXED = collections.OrderedDict(nx=128, ny=32, y_start=0, local_ny=32, precision=0, steps_done=11, tau=0.6, inlet_velocity=0.05,
                                cylinder_x=0.2, cylinder_y=0.5, cylinder_radius=0.125)
# the collision models: name -> (what lbm_ckpt_head.collision holds, LBMCKPT3 flag bit, parameters, noun of the refusals)
MODELS = collections.OrderedDict([("LES", (2, 4, (0.17,), "Smagorinsky constant")), ("TRT", (4, 8, (0.1875,), "TRT magic parameter")),
                                  ("forced", (8, 64, (1e-5, -2.5e-6), "forcing"))])
MODEL_ORDER = ("forced", "TRT", "LES")                      # the order in which a collision mismatch is named
WALLS = (2.0, 0.05, 1.0, 0.0)                               # south kind, south velocity, north kind, north velocity
MASK_D, PROFILE_D, SCHED_D = 0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x0F1E2D3C4B5A6978

Desc = collections.namedtuple("Desc", "fixed mask profile collision params walls sched")      # None: the run has no such field


def describe(mask=False, profile=False, collision=None, walls=False, sched=False):
    return Desc(dict(FIXED), MASK_D if mask else None, PROFILE_D if profile else None, collision,
                MODELS[collision][2] if collision else None, WALLS if walls else None, SCHED_D if sched else None)


ALL = [describe(m, p, c, w, s) for m, p, c, w, s in itertools.product((False, True), (False, True), (None,) + tuple(MODELS), (False, True), (False, True))]


def pack(d):
    """The head of the file as documented: magic, six ints, five doubles; LBMCKPT3: the flags and the fields in the order of their bits;
    LBMCKPT2: the mask's digest; LBMCKPT1: nothing more."""
    f = d.fixed
    fixed = struct.pack("<6i5d", f["nx"], f["ny"], f["y_start"], f["local_ny"], f["precision"], f["steps_done"], f["tau"],
                        f["inlet_velocity"], f["cylinder_x"], f["cylinder_y"], f["cylinder_radius"])
    if d.profile is None and d.collision is None and d.walls is None and d.sched is None:
        return (b"LBMCKPT2" + fixed + struct.pack("<Q", d.mask)) if d.mask is not None else b"LBMCKPT1" + fixed
    fields = {1: struct.pack("<Q", d.mask) if d.mask is not None else None, 2: struct.pack("<Q", d.profile) if d.profile is not None else None,
              16: struct.pack("<4d", *d.walls) if d.walls is not None else None, 32: struct.pack("<Q", d.sched) if d.sched is not None else None}
    if d.collision:
        fields[MODELS[d.collision][1]] = struct.pack("<%dd" % len(d.params), *d.params)
    present = sorted(bit for bit, v in fields.items() if v is not None)
    return b"LBMCKPT3" + fixed + struct.pack("<Q", sum(present)) + b"".join(fields[bit] for bit in present)


def first_difference(file, here):
    """(field, how) of the first thing lbm_load_state names, or None where the context loads the file. how: "file lacks", "context
    lacks", "differs"."""
    def one(field, a, b):
        if (a is None) != (b is None):
            return field, "file lacks" if a is None else "context lacks"
        return (field, "differs") if a is not None and a != b else None
    checks = [(m, file.params if file.collision == m else None, here.params if here.collision == m else None) for m in MODEL_ORDER]
    checks += [("walls", file.walls, here.walls), ("profile", file.profile, here.profile), ("schedule", file.sched, here.sched),
               ("mask", file.mask, here.mask)]
    for field, a, b in checks:
        r = one(field, a, b)
        if r:
            return r
    if any(file.fixed[k] != here.fixed[k] for k in FIXED if k != "steps_done"):
        return "header", "differs"
    return None


DIGEST_NOUNS = {"profile": "inlet profile", "schedule": "inlet schedule", "mask": "obstacle mask"}


def check_refusal(msg, field, how):
    """The message names the field and says which side lacks it, in the words lbm_load_state has always used."""
    assert msg.startswith("checkpoint x.ckpt was written "), msg
    if field == "header":
        assert msg.endswith("for different parameters"), msg
    elif field == "walls":
        assert "wall" in msg
        want = {"file lacks": "with two no-slip walls; this context has a ", "context lacks": "; this context has two no-slip walls",
                "differs": "for different walls: south kind "}[how]
        assert want in msg, msg
    elif field in DIGEST_NOUNS:
        noun = DIGEST_NOUNS[field]
        want = {"file lacks": "without an %s; this context has one", "context lacks": "with an %s; this context has none",
                "differs": "for a different %s"}[how] % noun
        assert msg.endswith("was written " + want), msg
    else:
        noun = MODELS[field][3]
        if how == "file lacks":
            assert "written without a %s" % noun in msg and "; this context has " in msg and "none" not in msg, msg
        elif how == "context lacks":
            assert "written with %s " % noun in msg and "; this context has none" in msg and "without" not in msg, msg
        else:
            assert "written with %s " % noun in msg and "; this context has " in msg and "none" not in msg and "without" not in msg, msg


@pytest.fixture(scope="module")
def lbm():
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    return pkg


@pytest.fixture(scope="module")
def head(lbm):
    def make(d):
        h = lbm.CkptHead(**d.fixed)
        h.has_mask, h.mask_digest = d.mask is not None, d.mask or 0
        h.has_profile, h.profile_digest = d.profile is not None, d.profile or 0
        h.has_sched, h.sched_digest = d.sched is not None, d.sched or 0
        if d.collision:
            h.collision = MODELS[d.collision][0]
            h.collision_param = (ctypes.c_double * 2)(*d.params)
        if d.walls is not None:
            h.has_walls, h.walls = 1, (ctypes.c_double * 4)(*d.walls)
        return h
    return make


@pytest.fixture(scope="module")
def refusal(lbm, head):
    """The text with which a context described by `here` refuses the bytes (of a Desc, or as given); None where it loads them."""
    def run(file, here):
        data = file if isinstance(file, bytes) else pack(file)
        try:
            used = lbm.debug_ckpt_load(data, head(here))
        except lbm.LbmError as e:
            return str(e)
        assert used == len(data) if not isinstance(file, bytes) else used <= len(data)
        return None
    return run


def test_the_bytes_of_every_head_are_the_documented_ones(lbm, head):
    assert len(ALL) == 64 and len({pack(d) for d in ALL}) == 64
    for d in ALL:
        assert lbm.debug_ckpt_save(head(d)) == pack(d), d
    assert max(len(pack(d)) for d in ALL) <= lbm.binding.CKPT_HEAD_MAX
    # the spots the GPU tests look at
    data = lbm.debug_ckpt_save(head(describe(walls=True)))
    assert data[:8] == b"LBMCKPT3" and struct.unpack("<Q4d", data[72:112]) == (16,) + WALLS and len(data) == 112
    data = lbm.debug_ckpt_save(head(describe(collision="forced")))
    assert data[:8] == b"LBMCKPT3" and struct.unpack("<Qdd", data[72:96]) == (64,) + MODELS["forced"][2] and len(data) == 96
    data = lbm.debug_ckpt_save(head(describe(mask=True, profile=True, collision="TRT", walls=True)))
    assert struct.unpack("<Q", data[72:80]) == (1 | 2 | 8 | 16,) and struct.unpack("<d4d", data[96:136]) == (0.1875,) + WALLS
    data = lbm.debug_ckpt_save(head(describe(sched=True, collision="forced")))      # the force stands behind the schedule, as its bit says
    assert struct.unpack("<QQdd", data[72:104]) == (32 | 64, SCHED_D) + MODELS["forced"][2]
    assert lbm.debug_ckpt_save(head(describe(mask=True)))[:8] == b"LBMCKPT2" and lbm.debug_ckpt_save(head(describe()))[:8] == b"LBMCKPT1"


def test_every_head_loads_into_its_own_description(lbm, head):
    for d in ALL:
        assert lbm.debug_ckpt_load(pack(d), head(d)) == len(pack(d)), d
        assert lbm.debug_ckpt_load(pack(d) + bytes(300), head(d)) == len(pack(d)), d      # the populations stand behind it
        later = d._replace(fixed=dict(d.fixed, steps_done=12345))                          # the iteration counter is the file's to say
        assert lbm.debug_ckpt_load(pack(later), head(d)) == len(pack(later)), d
    # an LBMCKPT3 file may announce the mask alone, or nothing
    m = describe(mask=True)
    v3 = b"LBMCKPT3" + pack(m)[8:72] + struct.pack("<QQ", 1, MASK_D)
    assert lbm.debug_ckpt_load(v3, head(m)) == 88
    assert lbm.debug_ckpt_load(b"LBMCKPT3" + pack(m)[8:72] + struct.pack("<Q", 0), head(describe())) == 80


def test_presence_mismatches_are_refused_in_the_order_they_always_were(refusal):
    for file in ALL:
        for here in ALL:
            msg, want = refusal(file, here), first_difference(file, here)
            assert (msg is None) == (file == here) == (want is None), (file, here, msg)
            if want:
                assert want[1] != "differs"
                check_refusal(msg, *want)


def test_value_mismatches_are_refused_field_by_field_and_the_header_last(refusal):
    def changed(d, **kw):
        return d._replace(**kw)
    for model, (_, _, params, _) in MODELS.items():
        full = describe(True, True, model, True, True)
        cases = [("mask", changed(full, mask=MASK_D ^ 1)), ("profile", changed(full, profile=PROFILE_D ^ (1 << 63))),
                 ("schedule", changed(full, sched=SCHED_D ^ (1 << 31))),
                 ("walls", changed(full, walls=(2.0, 0.0625, 1.0, 0.0))), ("walls", changed(full, walls=(2.0, 0.05, 0.0, 0.0))),
                 (model, changed(full, params=params[:-1] + (params[-1] * 0.5,)))]      # Cs, the magic parameter, fy alone
        for field, other in cases:
            for file, here in ((full, other), (other, full)):
                assert first_difference(file, here) == (field, "differs")
                check_refusal(refusal(file, here), field, "differs")
        for key, v in FIXED.items():
            other = changed(full, fixed=dict(full.fixed, **{key: v + 1}))
            if key == "steps_done":
                assert refusal(other, full) is None
                continue
            check_refusal(refusal(other, full), "header", "differs")
            check_refusal(refusal(full, other), "header", "differs")
            # every field is named before the header
            for field, worse in cases:
                both = worse._replace(fixed=other.fixed)
                check_refusal(refusal(both, full), field, "differs")
    # doubles are compared as numbers: a force (-0.0, fy) loads into a context with (0.0, fy)
    f = describe(collision="forced")
    assert refusal(f._replace(params=(-0.0, 0.5)), f._replace(params=(0.0, 0.5))) is None


def test_the_texts_are_those_lbm_load_state_has_always_written(refusal):
    none, W, P, S, M = describe(), describe(walls=True), describe(profile=True), describe(sched=True), describe(mask=True)
    les, trt, forced = describe(collision="LES"), describe(collision="TRT"), describe(collision="forced")
    pre = "checkpoint x.ckpt was written "
    texts = [
        (W, none, "with wall kinds 2 (south) and 1 (north); this context has two no-slip walls"),
        (none, W, "with two no-slip walls; this context has a moving south wall and a free-slip north wall"),
        (W, W._replace(walls=(2.0, 0.0625, 1.0, 0.0)), "for different walls: south kind 2 u = 0.050000000000000003, north kind 1 u = 0; "
                                                       "this context has south kind 2 u = 0.0625, north kind 1 u = 0"),
        (none, P, "without an inlet profile; this context has one"),
        (P, none, "with an inlet profile; this context has none"),
        (P, P._replace(profile=1), "for a different inlet profile"),
        (none, S, "without an inlet schedule; this context has one"),
        (S, none, "with an inlet schedule; this context has none"),
        (S, S._replace(sched=1), "for a different inlet schedule"),
        (none, M, "without an obstacle mask; this context has one"),
        (M, none, "with an obstacle mask; this context has none"),
        (M, M._replace(mask=1), "for a different obstacle mask"),
        (none, none._replace(fixed=dict(FIXED, tau=0.7)), "for different parameters"),
        (none, les, "without a Smagorinsky constant (BGK); this context has Cs = 0.17"),
        (les, none, "with Smagorinsky constant Cs = 0.17; this context has none (BGK)"),
        (les, les._replace(params=(0.125,)), "with Smagorinsky constant Cs = 0.17000000000000001; this context has Cs = 0.125"),
        (none, trt, "without a TRT magic parameter; this context has 0.1875"),
        (trt, none, "with TRT magic parameter 0.1875; this context has none"),
        (trt, trt._replace(params=(0.25,)), "with TRT magic parameter 0.1875; this context has 0.25"),
        (none, forced, "without a forcing; this context has F = (1e-05, -2.5e-06)"),
        (forced, none, "with forcing F = (1e-05, -2.5e-06); this context has none"),
        (forced, forced._replace(params=(1e-5, 0.0)), "with forcing F = (1.0000000000000001e-05, -2.5000000000000002e-06); "
                                                      "this context has F = (1.0000000000000001e-05, 0)"),
        # one model against another: the later row of the table speaks first
        (les, trt, "without a TRT magic parameter; this context has 0.1875"),
        (forced, les, "with forcing F = (1e-05, -2.5e-06); this context has none"),
    ]
    for file, here, text in texts:
        assert refusal(file, here) == pre + text
    assert refusal(b"LBMCKPT1" + bytes(10), none) == "x.ckpt is not a checkpoint"


def test_malformed_heads_are_not_checkpoints(refusal):
    for d in ALL:
        data = pack(d)
        for n in range(len(data)):
            assert refusal(data[:n], d) == "x.ckpt is not a checkpoint", (d, n)
        assert refusal(b"LBMCKPT4" + data[8:], d) == "x.ckpt is not a checkpoint"
        assert refusal(b"lbmckpt" + data[7:], d) == "x.ckpt is not a checkpoint"
        assert refusal(b"LBMCKPT0" + data[8:], d) == "x.ckpt is not a checkpoint"
        if data[:8] == b"LBMCKPT3":
            flags, = struct.unpack("<Q", data[72:80])
            for unknown in (128, 1 << 63):
                assert refusal(data[:72] + struct.pack("<Q", flags | unknown) + data[80:] + bytes(64), d) == "x.ckpt is not a checkpoint"
    # a context has one collision model, and so has a head
    two = b"LBMCKPT3" + pack(describe())[8:72] + struct.pack("<Qdd", 4 | 8, 0.17, 0.1875)
    for d in (describe(), describe(collision="LES"), describe(collision="TRT")):
        assert refusal(two, d) == "x.ckpt is not a checkpoint"


def fnv1a(words):
    """64-bit FNV-1a over 32-bit words."""
    d = 1469598103934665603
    for w in words:
        d = ((d ^ (w & 0xFFFFFFFF)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return d


def halves(values):
    """the low and the high half of each double's bit pattern"""
    out = []
    for v in values:
        b, = struct.unpack("<Q", struct.pack("<d", v))
        out += [b & 0xFFFFFFFF, b >> 32]
    return out


def test_the_three_digests_come_from_one_accumulator_and_keep_their_values(lbm):
    """mask: {nx, ny, a 0 / 1 word per cell, row 0 first}; profile: {ny, the halves of each velocity}; schedule: {mode, n, the halves of
    each factor} — formed by the functions the setters call."""
    def small(**kw):
        return lbm.CkptHead(**dict(FIXED, nx=7, ny=5, local_ny=5, **kw))
    mask = (np.random.default_rng(7).random((5, 7)) < 0.4).astype(np.uint8)
    mask[0, 0], mask[4, 6] = 1, 0
    h = small()
    data = lbm.debug_ckpt_save(h, mask=mask * 255)                                    # any nonzero byte is a solid cell
    want = fnv1a([7, 5] + [int(v) for v in mask.ravel()])
    assert h.has_mask == 1 and h.mask_digest == want and data == b"LBMCKPT2" + data[8:72] + struct.pack("<Q", want)
    u = [0.0, 0.03, -0.0, 0.0625, 1e-300]
    h = small()
    data = lbm.debug_ckpt_save(h, profile=u)
    want = fnv1a([5] + halves(u))
    assert h.has_profile == 1 and h.profile_digest == want and data[72:] == struct.pack("<QQ", 2, want)
    s = [0.0, 0.5, 1.0]
    seen = set()
    for name, mode in (("hold", 0), ("repeat", 1)):
        h = small()
        data = lbm.debug_ckpt_save(h, schedule=(s, name))
        want = fnv1a([mode, 3] + halves(s))
        assert h.has_sched == 1 and h.sched_digest == want and data[72:] == struct.pack("<QQ", 32, want)
        seen.add(want)
    assert len(seen) == 2
