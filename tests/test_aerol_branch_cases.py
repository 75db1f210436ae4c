"""CPU: the cases of tests/aerol_branch_cases.py.
(a) every case takes the oracle branches it names (jo_aerol_coverage) and its predicates hold;
(b) over a family's cases plus the survey of what the existing Aero-L GPU tests feed (profiles/aerol_branches.json), every counter of the
    family's chain is reached or stands in UNREACHABLE with its derivation -- and nothing on that list is ever counted;
(c) the oracle's rows do not depend on how the stream is cut into writes (R/T: cut at group ends only);
(d) every case through the device code compiled for the host (tests/host_emul: k_aerol_bits<false> / k_aerolb_bits<both> / k_aerolc_bits with their
    post, tick and end-of-write kernels) equals the oracle exactly: rows, events, packets, voice and every tick's return."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import aerol_branch_cases as ABC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ABC.all_cases()
IDS = [c.name for c in ALL]


@pytest.fixture(scope="module")
def runs(oracle_mod):
    """every case through the oracle, once"""
    return {c.name: ABC.run_oracle(oracle_mod, c) for c in ALL}


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_case_takes_its_branches(runs, case):
    r = runs[case.name]
    missed = [h for h in case.hits if not r["coverage"][h]]
    assert not missed, missed
    assert case.hits or case.predicate
    if case.predicate:
        case.predicate(case, r)


@pytest.mark.parametrize("fam", list(ABC.FAMILIES))
def test_family_chain_is_covered(oracle_mod, runs, fam):
    with open(os.path.join(ROOT, "profiles", "aerol_branches.json")) as f:
        prof = json.load(f)
    names = ABC.chain_counters(oracle_mod, fam)
    assert set(prof["survey"][fam]) == set(oracle_mod.AeroL.coverage_names()), "profiles/aerol_branches.json is not of this oracle: scripts/aerol_branch_survey.py"
    total = {n: int(prof["survey"][fam][n]) for n in names}
    for c in ABC.cases(fam):
        for n in names:
            total[n] += runs[c.name]["coverage"][n]
    unreachable = ABC.UNREACHABLE[fam]
    assert set(unreachable) <= set(names)
    assert [n for n in names if not total[n] and n not in unreachable] == []
    assert [n for n in unreachable if total[n]] == [], "a counter an input reached stands in UNREACHABLE"
    # a work-list counter (zero in the survey) has a case that NAMES it
    named = {h for c in ABC.cases(fam) for h in c.hits}
    assert [n for n in names if not prof["survey"][fam][n] and n not in unreachable and n not in named] == []


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_oracle_rows_do_not_depend_on_the_cut(oracle_mod, runs, case):
    want = runs[case.name]
    for plan in ABC.cut_plans(case):
        got = ABC.run_oracle(oracle_mod, case, plan)
        for k in ("sus", "events", "packets", "dcd") + (("voice", "voice_frames") if case.fb == 8400 else ()):
            assert np.array_equal(got[k], want[k]), (k, plan[:4])


# ------------------------------------------------------------------------------------------------------------ (d) host emulators
def build_emul(kind, root=ROOT, outdir=None):
    """tests/host_emul/aerol{p,b,c}_emul.cpp of the tree at `root` as a shared library (the oracle's Viterbi decoder linked in)"""
    outdir = outdir or tempfile.mkdtemp(prefix=f"aerol{kind}_cases_")
    so = os.path.join(outdir, f"libaerol{kind}_emul.so")
    cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(root, "tests", "host_emul", "stub"), "-o", so,
           os.path.join(root, "tests", "host_emul", f"aerol{kind}_emul.cpp"), "-L" + os.path.join(ROOT, "oracle"), "-l:liboracle.so",
           "-Wl,-rpath," + os.path.join(ROOT, "oracle")]
    subprocess.check_call(cmd)
    L = C.CDLL(so)
    pre = {"p": "emulp", "b": "emulb", "c": "emul"}[kind]
    create = getattr(L, pre + "_create")
    create.restype = C.c_void_p
    create.argtypes = [C.c_int, C.c_int] if kind == "c" else [C.c_int, C.c_int, C.c_int]
    getattr(L, pre + "_destroy").argtypes = [C.c_void_p]
    getattr(L, pre + "_write").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + ([C.c_int] if kind == "b" else [])
    getattr(L, pre + "_read").argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    getattr(L, pre + ("_tick_out" if kind == "c" else "_tick")).argtypes = [C.c_void_p, C.c_void_p]
    return L


def run_emul(L, case, plan, wide=-1):
    """one case through its family's emulator as channel 0 of a one-channel bank: the same writes and ticks as run_oracle"""
    kind = "c" if case.fb == 8400 else "b" if case.burst else "p"
    pre = {"p": "emulp", "b": "emulb", "c": "emul"}[kind]
    h = getattr(L, pre + "_create")(*((1, 4000) if kind == "c" else (1, case.fb, 4000)))
    write, tick = getattr(L, pre + "_write"), getattr(L, pre + ("_tick_out" if kind == "c" else "_tick"))
    dcd, flags = [], np.zeros(64, np.int32)
    for s, e, t in plan:
        stride = max(8, (e - s + 7) // 8 * 8)
        buf = np.zeros((1, stride), np.int16)
        buf[0, :e - s] = case.stream[s:e]
        cnt = np.array([e - s], np.int32)
        args = (h, buf.ctypes.data, cnt.ctypes.data, stride, e - s)
        assert (write(*args, wide) if kind == "b" else write(*args)) in (0, None)
        for _ in range(t):
            tick(h, flags.ctypes.data)
            dcd.append(int(flags[0]))
    read = getattr(L, pre + "_read")
    rows = np.zeros((4000, 16), np.int32)
    n = read(h, 0, 0, rows.ctypes.data, 4000)
    ev = np.zeros((256, 3), np.int64)
    out = {("packets" if case.burst else "sus"): rows[:n].copy(), "dcd": np.array(dcd, np.int32)}
    if kind == "c":
        v = np.zeros((1400, 304), np.uint8)
        nv = read(h, 0, 1, v.ctypes.data, 1400)
        out["voice_frames"], out["voice"] = v[:nv, :4].copy().view(np.uint32).reshape(-1), v[:nv, 4:].copy()
        m = read(h, 0, 2, ev.ctypes.data, 256)
    else:
        m = read(h, 0, 1, ev.ctypes.data, 256)
    out["events"] = ev[:m].copy()
    getattr(L, pre + "_destroy")(h)
    return out


def compare_emul(L, case, want):
    """asserts that the emulator's rows, events, packets, voice and tick returns are the oracle's"""
    for wide in ((0, 1) if case.burst else (-1,)):
        got = run_emul(L, case, want["plan"], wide)
        for k in got:
            assert np.array_equal(got[k], want[k]), (case.name, k, wide, got[k][:3].tolist() if len(got[k]) else [], want[k][:3].tolist() if len(want[k]) else [])


@pytest.fixture(scope="module")
def emul(oracle_mod):
    oracle_mod.lib()
    return {k: build_emul(k) for k in "pbc"}


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_case_through_the_host_emulator(emul, runs, case):
    kind = "c" if case.fb == 8400 else "b" if case.burst else "p"
    compare_emul(emul[kind], case, runs[case.name])
