"""The collision models' build units, the parts that need no GPU: every launcher the host translation unit references is defined in
some object of the library (ctypes binds lazily, so a forgotten unit would otherwise show only at the first launch), and the unit
list holds the same kinds of object for every model."""
import importlib
import re
import subprocess

import pytest

from tests.helpers import PKG


@pytest.fixture(scope="module")
def build():
    return importlib.import_module(PKG + ".build")


def test_library_leaves_no_launcher_unresolved(build):
    lib = build.build_all()
    out = subprocess.run(["nm", "-D", "--undefined-only", "--demangle", lib], stdout=subprocess.PIPE, text=True, check=True, timeout=60).stdout
    assert "hipLaunchKernel" in out             # (the listing is the library's: it does import the HIP runtime)
    assert [line for line in out.splitlines() if "lbmk::" in line] == []


def test_every_collision_base_has_the_same_units(build):
    units = build.units("0123456789abcdef")
    assert len({obj for _, _, obj in units}) == len(units)
    kinds = {}
    for src, flags, obj in units:
        base = [f for f in flags if f.startswith("-DLBM_AR_BASE=")]
        if base:
            rest = tuple(f for f in flags if f not in base)
            kinds.setdefault(int(base[0].split("=")[1]), set()).add((src, rest, re.sub(r"_ar\d+", "", obj)))
    assert sorted(kinds) == sorted(build.COLLISION_BASES) == [0, 2, 4, 8]
    assert kinds[0] == kinds[2] == kinds[4] == kinds[8] and len(kinds[0]) == 3
    assert {src for src, _, _ in kinds[0]} == {"lbm_step_k.hip", "lbm_col.hip"}
