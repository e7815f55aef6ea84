"""Which variant of the register-resident soft kernels the host selects, for every case of tests/variant_cases.py, without a GPU: the cases run
against the stand-in HIP runtime of tests/hostcheck (kernels never run; the variant census -- s2amd_get_variant_entry -- counts the launchers'
selections all the same), in a child process (tests/hostcheck/drive_variant_cases.py).

  * every case selects exactly the (family, key) set the table says;
  * the union over the table IS the enumeration of the six variant tables: no entry of the library is unreached, and the table names no entry
    the library does not have.  A table entry exists if and only if a case runs it; tests/test_gpu_variant_census.py runs the same cases on
    the GPU, bit for bit against the oracle.

The sanitizers the hostcheck library is built with are along for the ride (it cannot be loaded without their runtime); a report fails the run."""
import glob
import json
import os
import subprocess
import sys

import pytest

from tests import variant_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "tests", "hostcheck")


def _asan_runtime():
    hits = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    return hits[-1] if hits else None


@pytest.fixture(scope="module")
def run():
    if not os.path.exists("/opt/rocm/bin/hipcc") or _asan_runtime() is None:
        pytest.skip("needs hipcc and clang's ASan runtime")
    subprocess.check_call(["make", "-s", "-j8", "-C", HOSTCHECK])
    env = dict(os.environ)
    env["LD_PRELOAD"] = _asan_runtime()
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0:exitcode=23"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1:exitcode=24"
    env["S2AMD_LIB"] = os.path.join(HOSTCHECK, "_build", "libs2amd_hostcheck.so")
    p = subprocess.run([sys.executable, os.path.join(HOSTCHECK, "drive_variant_cases.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "VARIANT CASES DRIVER OK" in out and "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    cases, enumeration = {}, None
    for line in out.splitlines():
        if line.startswith("CASE "):
            row = json.loads(line[5:])
            cases[row["name"]] = row
        elif line.startswith("ENUMERATION "):
            enumeration = json.loads(line[12:])
    assert enumeration is not None and sorted(cases) == sorted(c.name for c in variant_cases.CASES), out[-4000:]
    return cases, enumeration


def _pairs(rows):
    return {(family, tuple(key)) for family, key in rows}


@pytest.mark.parametrize("case", variant_cases.CASES, ids=[c.name for c in variant_cases.CASES])
def test_case_selects_exactly_its_variants(run, case):
    row = run[0][case.name]
    assert row["error"] is None, row["error"]
    got = _pairs(row["selected"])
    assert got == set(case.expect), "%s: selected but not expected %s; expected but not selected %s" % (
        case.name, sorted(got - set(case.expect)), sorted(set(case.expect) - got))


def test_the_tables_have_six_families_with_named_keys(run):
    families = run[1]["families"]
    assert sorted(families) == ["islandStepKernel", "pairStepKernel", "stripSoftKernel", "stripStepKernel", "wideIslandKernel", "wideStepKernel"]
    assert families["wideStepKernel"] == ["POINTS", "RPH", "SR", "SL", "IL", "MODE", "KIND"] and families["stripSoftKernel"] == ["KIND", "WARM"]
    for family, key in _pairs(run[1]["entries"]):
        assert len(key) == len(families[family]), (family, key)


def test_every_layout_and_island_form_is_reached_without_a_forcing_bit():
    """persist_debug bits 16 / 64 / 128 make the host pick a roomier layout than the partition needs; each of the five wideStepKernel layouts and
    the six- and eight-round island forms must also be selected by a case that sets none of them."""
    unforced = set().union(*[c.expect for c in variant_cases.CASES if not c.forced])
    layouts = {key[1:5] for family, key in unforced if family == "wideStepKernel"}
    assert layouts == {variant_cases.L32, variant_cases.L33, variant_cases.L42, variant_cases.L322, variant_cases.L3222}, layouts
    assert {key[1] for family, key in unforced if family == "wideIslandKernel"} == {6, 8}
    assert {key[2] for family, key in unforced if family == "islandStepKernel"} == {6, 8}


def test_the_union_of_the_cases_is_the_whole_enumeration(run):
    """No table entry without a case, no case for an entry that does not exist."""
    cases, enumeration = run
    entries = _pairs(enumeration["entries"])
    selected = set().union(*[_pairs(row["selected"]) for row in cases.values()])
    expected = set().union(*[c.expect for c in variant_cases.CASES])
    print("reached %d of %d entries: %s" % (len(selected & entries), len(entries), sorted(selected & entries)))
    assert not entries - selected, "table entries no case selects (delete them or give them a case): %s" % sorted(entries - selected)
    assert not selected - entries and not expected - entries, "cases name entries the tables do not have: %s" % sorted((selected | expected) - entries)
    assert expected == entries
