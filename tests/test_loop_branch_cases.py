"""CPU: the cases of tests/loop_branch_cases.py against the oracle alone -- every case takes the branch it exists for (a crossing case also
leaves it, a meter case takes it inside a one-sample write), the cases of a family together take every counter of Demod.COVERAGE that its
chain has, the verdicts survive noise at 1e-9 of the stream, and jo_demod_loop_state reads back what it set.  tests/test_gpu_loop_branches.py
runs the same cases on the kernels: it cannot pass vacuously while this passes."""
import os
import re

import numpy as np
import pytest

import loop_branch_cases as LC

NDRAWS = 10
# Conditioning of the 8400 bps cases.  The loops amplify a change of the input: noise at 1e-9 moves the oracle's soft symbols by up to 3e-3
# on this module's 8400 bps streams (1.4e-3 on its ordinary data streams).  That chain's prefilter is an FFT filter whose rounding is not the
# reference's (k_pre8400.h), the one place where a sample loop's input differs from the oracle's at all; under this amplification the bank
# meets SYM_TOL.  An unmodulated tone in the channel amplifies the same noise to 1e-1 and showed the prefilter's rounding as 5e-5 on the
# device: such a stream says nothing about a branch, and no 8400 bps case may be that sensitive.  (The other chains run the oracle's
# operations one for one; their figures are printed.)
E_N_MAX_8400 = 1e-2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_write_plans():
    w = LC.plan_writes(48000)
    assert w[:6] == LC.WRITES and w[-3:] == [1, 1, 1] and sum(w) == 48000
    w = LC.plan_writes(48000, cuts=(LC.MID, LC.LATE))
    b = np.cumsum(w).tolist()
    assert LC.MID in b and LC.LATE in b and w[:6] == LC.WRITES  # the mid-stream pokes fall on boundaries of the plain cycle
    w = LC.plan_writes(30000, singles=(0, 20000, 20001))
    b = [0] + np.cumsum(w).tolist()
    assert w[0] == 1 and w[b.index(20000)] == 1 and w[b.index(20001)] == 1 and max(w) <= LC.MAX_WRITE
    assert {g.family for g in LC.GROUPS.values()} == set(LC.FAMILIES)
    for g in LC.GROUPS.values():
        assert g.n <= LC.N_LOOP or g.name == "meter", g.id  # only the meter groups are longer (the module says why)
        assert len({c.name for c in g.cases}) == len(g.cases)


@pytest.mark.parametrize("gid", LC.GROUP_IDS)
def test_every_case_takes_the_branch_it_exists_for(oracle_mod, gid):
    O = oracle_mod
    g = LC.GROUPS[gid]
    writes, p0 = LC.group_plan(O, gid)
    thr = LC.THRESH[LC.fam(g.family)["kind"]]
    for ci, c in enumerate(g.cases):
        e = LC.expected(O, gid, ci)
        v = LC.verdicts(g, c, e, p0)
        print(f"loop_branches {gid} {c.name}: mse {e.ref['mse']:.3f} soft {len(e.ref['soft'])} status rows {len(e.ref['status'])} "
              f"st_freq - stref {e.states[-1]['st_freq'] - LC.stref(g.family):+.3e} taken { {k: n for k, n in e.cov.items() if n} }")
        assert all(v.values()), (gid, c.name, {k: x for k, x in v.items() if not x}, e.cov)
        if c.pokes and (c.on_clamp or c.crossing):
            assert e.ref["mse"] < thr, (gid, c.name, "the loop does not end in lock", e.ref["mse"])
            assert len(e.ref["soft"]) > 1000
        if c.pokes:  # the poke changes what the stream gives: the neighbour is another run
            nb = LC.expected(O, gid, ci, poked=False)
            assert nb.states[-1] != e.states[-1], (gid, c.name)


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_the_cases_of_a_family_take_every_branch_its_chain_has(oracle_mod, family):
    O = oracle_mod
    total = dict.fromkeys(O.Demod.COVERAGE, 0)
    for gid, g in LC.GROUPS.items():
        if g.family == family:
            for ci in range(len(g.cases)):
                for k, n in LC.expected(O, gid, ci).cov.items():
                    total[k] += n
    print(f"loop_branches {family}: union {total}")
    assert set(LC.NOT_IN_CHAIN[family]) <= set(total) and not set(LC.NOT_IN_CHAIN[family]) & set(LC.AFC_COUNTERS)
    for k, n in total.items():
        if k in LC.NOT_IN_CHAIN[family]:
            assert n == 0, (family, k, "listed as not in the chain, yet taken", n)
        elif k in LC.AFC_COUNTERS:
            path, test, param = LC.AFC_CREDIT[family]
            src = open(os.path.join(ROOT, path)).read()
            m = re.search(r"@pytest\.mark\.parametrize\(\"name\", (\[[^\]]*\])\)\ndef " + test + r"\(", src)
            assert m and f'"{param}"' in m.group(1), (family, k, "credited to a test that does not exist", LC.AFC_CREDIT[family])
        else:
            assert n > 0, (family, k, "no case of this module takes it")


@pytest.mark.parametrize("gid", LC.GROUP_IDS)
def test_verdicts_and_decisions_survive_noise(oracle_mod, gid):
    """Ten draws of additive noise at 1e-9 of the stream's rms (exact zeros stay zeros): no hard decision, soft length, status-row count or
    taken / not-taken verdict of the oracle changes, and no soft symbol of an 8400 bps case moves by E_N_MAX_8400.  What the kernels differ from the oracle by is
    smaller still."""
    O = oracle_mod
    g = LC.GROUPS[gid]
    writes, p0 = LC.group_plan(O, gid)
    for ci, c in enumerate(g.cases):
        e = LC.expected(O, gid, ci)
        want = LC.verdicts(g, c, e, p0)
        x = LC.stream(c.stream)
        worst = 0.0
        for draw in range(NDRAWS):
            r = LC.run(O, g.family, LC.noisy(x, draw, ci), writes, LC.poke_dict(c))
            tag = (gid, c.name, draw)
            assert len(r.ref["soft"]) == len(e.ref["soft"]) and r.ref["pending"] == e.ref["pending"], (tag, "soft length")
            assert np.array_equal(r.ref["soft"] >= 128, e.ref["soft"] >= 128), (tag, "a hard decision")
            assert len(r.ref["status"]) == len(e.ref["status"]) and np.array_equal(r.ref["status"][:, 5], e.ref["status"][:, 5]), (tag, "status rows")
            assert LC.verdicts(g, c, r, p0) == want, (tag, LC.verdicts(g, c, r, p0), want)
            assert r.ref["symbols"].shape == e.ref["symbols"].shape, tag
            worst = max(worst, float(np.max(np.abs(r.ref["symbols"] - e.ref["symbols"]), initial=0.0)))
        print(f"loop_branches {gid} {c.name}: largest symbol change under the noise draws {worst:.2e}")
        assert g.family != "oqpsk_8400" or worst < E_N_MAX_8400, (gid, c.name, worst)


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_loop_state_reads_back_what_it_set(oracle_mod, family):
    """jo_demod_loop_state: a set is read back as set wherever px / py stand; the frequencies go through SetFreq (the step follows); a set to
    the current values changes no later output bit."""
    O = oracle_mod
    gid = [k for k, g in LC.GROUPS.items() if g.family == family][0]
    x = LC.stream(LC.GROUPS[gid].cases[-1].stream)
    sett = LC.oracle_settings(O, family)
    a, b = O.Demod(sett, capture_symbols=True), O.Demod(sett, capture_symbols=True)
    s = 0
    for k, m in enumerate([4096, 3000, 1, 777, 13, 14, 15, 4095, 4096]):  # odd numbers of symbols in between: px and py in every position
        a.write(x[s:s + m]); b.write(x[s:s + m])
        s += m
        b.set_loop_state(**b.loop_state)  # to the current values
        assert a.loop_state == b.loop_state, (family, k)
    for d in (a, b):
        d.write(x[s:s + 8000])
    assert a.loop_state == b.loop_state and a.mse == b.mse and a.freq_est == b.freq_est and a.ebno == b.ebno
    assert np.array_equal(a.take_soft(), b.take_soft()) and np.array_equal(a.take_symbols().view(np.uint64), b.take_symbols().view(np.uint64))
    want = dict(st_freq=LC.stref(family) + 0.03125, m2_freq=1234.5, lf_x1=1.0, lf_x2=-2.0, lf_y1=3.0, lf_y2=-4.0)
    for k in range(7):
        a.write(x[s:s + 9 + k])  # moves px / py
        s += 9 + k
        a.set_loop_state(**want)
        assert a.loop_state == want, (family, k, a.loop_state)
    if LC.fam(family)["kind"] == "oqpsk" and family == "oqpsk_10500":
        # the history is what IIR::update reads: y = b0 x + b1 x1 + b2 x2 - a1 y1 - a2 y2 behind a set, whatever x is, moves with y1 and y2
        a.set_loop_state(lf_x1=0.0, lf_x2=0.0, lf_y1=3.0, lf_y2=3.0)
        before = a.coverage()["lf_pi2_pos"]
        a.write(x[s:s + 40])
        assert a.coverage()["lf_pi2_pos"] > before
    a.set_loop_state(st_freq=-1.0)
    assert a.loop_state["st_freq"] == 0.0  # WaveTable::SetFreq's floor
