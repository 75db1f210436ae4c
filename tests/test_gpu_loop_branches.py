"""GPU (-m gpu): the continuous sample loops in the states of tests/loop_branch_cases.py -- st_osc on and across its 0.1 Hz clamp, the +-pi/2
clamp behind the carrier loop filter, mixer2 off by a part of the locking band, and the lines of both EbNo meters on one-sample writes --
against the oracle.  tests/test_loop_branch_cases.py shows on the CPU that every case takes the branch it exists for.

A group of cases is one bank of 70 channels (two channel groups, the second with six live lanes), max_write_samples 4096, EbNo, status log and
symbol capture on.  Channels 0, 1, 63, 64 and 69 carry the five cases, every other channel the ordinary neighbour of one of them: the same
stream, never poked.  A twin bank takes the same writes and no poke.  Pokes (jaero_debug_loop_poke) go in where the oracle's went in, between
two writes.  Compared: the case channels against the oracle's poked run with the project's contract (length and hard decisions exact, no soft
byte off, symbols within SYM_TOL, status rows and final values to 1e-6 -- test_gpu_parity.compare); the EbNo meter's value behind every one-sample write (1e-6); what jaero_debug_loop_peek returns behind
every sixth write and the last: st_freq bit for bit wherever the case sits on the clamp (T1: every peek; T2: the last, if the oracle's is the
clamp's value -- one SetFreq of a constant), st_freq and m2_freq to 1e-6 elsewhere, the filter history to 1e-6; the twin's case channels
against the oracle's unpoked run; every other channel of the poked bank bit for bit against the twin."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import kernel_variants as KV
import loop_branch_cases as LC
from test_gpu_parity import SYM_TOL, compare

pytestmark = pytest.mark.gpu

RUNS = [pytest.param(gid, layout, id=f"{gid}-L{layout}") for gid in LC.GROUP_IDS for layout in LC.layouts(LC.GROUPS[gid].family)]
PEEK_EVERY = 6
_LEDGER = {}  # per case: oracle branch counts, largest symbol deviation, soft bytes compared (profiles/loop_branches.json is a copy of a run)


@pytest.fixture
def sample_loop_layout():
    """Forces the sample-loop layout of the banks created next (jaero_debug_sample_loop_layout); back to "by size" afterwards."""
    from jaero_amd import capi

    L = capi.lib()
    try:
        yield lambda mode: capi.check(L.jaero_debug_sample_loop_layout(mode))
    finally:
        L.jaero_debug_sample_loop_layout(0)


def case_of(c, ncases):
    """(case index, poked) of channel c"""
    if c in LC.SPECIAL and LC.SPECIAL.index(c) < ncases:
        return LC.SPECIAL.index(c), True
    return c % ncases, False


def peek(bank, ch):
    from jaero_amd import capi

    st = capi.LoopState()
    capi.check(bank.L.jaero_debug_loop_peek(bank.h, ch, C.byref(st)))
    return {k: getattr(st, k) for k, _ in capi.LoopState._fields_}


def poke(bank, ch, **fields):
    """the named fields replaced, the others written back as read: what Demod.set_loop_state does to the oracle"""
    from jaero_amd import capi

    st = capi.LoopState(**dict(peek(bank, ch), **fields))
    capi.check(bank.L.jaero_debug_loop_poke(bank.h, ch, C.byref(st)))


@functools.lru_cache(maxsize=2)
def device_pcm(gid):
    """Frame-major [n, NCH] on cuda:0"""
    import torch

    g = LC.GROUPS[gid]
    rows = [LC.stream(g.cases[case_of(c, len(g.cases))[0]].stream) for c in range(LC.NCH)]
    return torch.from_numpy(np.ascontiguousarray(np.stack(rows).T)).to(torch.device("cuda", 0))


def outputs(bank, ch):
    st = bank.read_status(ch)
    return dict(soft=bank.read_softbits(ch), sym=bank.read_symbols(ch), log=bank.read_status_log(ch),
                status=(st.mse, st.ebno, st.freq_est, st.freq_center, st.signal, st.n_estimates), loop=tuple(peek(bank, ch).values()))


def same_bits(a, b):
    return (np.array_equal(a["soft"], b["soft"]) and np.array_equal(a["sym"].view(np.uint64), b["sym"].view(np.uint64)) and
            np.array_equal(a["log"].view(np.uint64), b["log"].view(np.uint64)) and
            np.array_equal(np.array(a["status"]).view(np.uint64), np.array(b["status"]).view(np.uint64)) and
            np.array_equal(np.array(a["loop"]).view(np.uint64), np.array(b["loop"]).view(np.uint64)))


def check_against_oracle(family, got, e, peeks, tag, clamp_bits, last_on_clamp):
    ref = e.ref
    compare(got["soft"], got["sym"], got["log"], ref, check_ebno=True)
    mse, ebno, freq_est, freq_center, signal, nest = got["status"]
    assert nest == len(ref["status"]), (tag, nest, len(ref["status"]))
    assert abs(mse - ref["mse"]) < 1e-6 and abs(freq_est - ref["freq_est"]) < 1e-6 and abs(freq_center - ref["freq_center"]) < 1e-6, tag
    assert abs(ebno - ref["ebno"]) < 1e-6, (tag, ebno, ref["ebno"])
    assert signal == (0 if ref["mse"] > LC.THRESH[LC.fam(family)["kind"]] else 1), tag
    for w, st in peeks:
        want = e.states[w]
        last = w == len(e.writes) - 1
        if clamp_bits or (last and last_on_clamp):
            assert st["st_freq"] == want["st_freq"], (tag, "st_freq, bit for bit, behind write", w, st["st_freq"].hex(), want["st_freq"].hex())
        for k in st:
            assert abs(st[k] - want[k]) < 1e-6, (tag, k, "behind write", w, st[k], want[k])
    d = float(np.max(np.abs(got["sym"] - ref["symbols"]), initial=0.0))
    return d, int(len(ref["soft"])), int((got["soft"][:len(ref["soft"])].astype(int) != ref["soft"].astype(int)).sum())


@pytest.mark.parametrize("gid,layout", RUNS)
def test_group_against_the_oracle(oracle_mod, sample_loop_layout, gid, layout):
    from jaero_amd import capi
    from jaero_amd import demodulator as D

    O = oracle_mod
    g = LC.GROUPS[gid]
    f = LC.fam(g.family)
    writes, p0 = LC.group_plan(O, gid)
    ncases = len(g.cases)
    pokes = {}  # sample -> [(channel, fields)]
    for ci, c in enumerate(g.cases):
        for s, fields in c.pokes:
            pokes.setdefault(s, []).append((LC.SPECIAL[ci], dict(fields)))
    sample_loop_layout(layout)
    cap = int(g.n * f["fb"] / f["Fs"]) + 256
    kw = dict(ebno=True, status_log=True, capture_symbols=True, max_write_samples=LC.MAX_WRITE, softbit_capacity=cap)
    sets = [LC.bank_settings(g.family)] * LC.NCH
    bank, twin = D.DemodulatorBank(sets, **kw), D.DemodulatorBank(sets, **kw)
    try:
        want_kernel = KV.find(g.family, True, True, layout).kernel0
        assert bank.kernel_variant(0) == want_kernel and twin.kernel_variant(0) == want_kernel
        pcm = device_pcm(gid)
        peeks = {ch: [] for ch in LC.SPECIAL}
        exp = [LC.expected(O, gid, ci) for ci in range(ncases)]
        s = 0
        for w, m in enumerate(writes):
            for ch, fields in pokes.get(s, ()):
                poke(bank, ch, **fields)
            bank.write(pcm[s:s + m], layout=capi.PCM_FRAME_MAJOR)
            twin.write(pcm[s:s + m], layout=capi.PCM_FRAME_MAJOR)
            s += m
            if m == 1:
                # the meter behind every one-sample write: its value forgets a sample as 0.8^k, so a line taken in that sample (a tebno of
                # 52 held to 50, a NaN made 50, a floored mvr made 0) shows here and nowhere later
                for ci in range(ncases):
                    ebno = bank.read_status(LC.SPECIAL[ci]).ebno
                    assert abs(ebno - exp[ci].meter[w][0]) < 1e-6, (gid, layout, g.cases[ci].name, "EbNo behind the one-sample write", w, "at sample", s - 1,
                                                                    ebno, exp[ci].meter[w][0])
            if w % PEEK_EVERY == PEEK_EVERY - 1 or w == len(writes) - 1:
                for ch in LC.SPECIAL:
                    peeks[ch].append((w, peek(bank, ch)))
        got = {ch: outputs(bank, ch) for ch in range(LC.NCH)}
        got_twin = {ch: outputs(twin, ch) for ch in range(LC.NCH)}
        for ci, c in enumerate(g.cases):
            ch = LC.SPECIAL[ci]
            e = LC.expected(O, gid, ci)
            tag = f"{gid} L{layout} {c.name} (channel {ch})"
            clamp = LC.stref(g.family) + (0.1 if "st_high" in c.branch else -0.1)
            try:
                dev, nsoft, ndiff = check_against_oracle(g.family, got[ch], e, peeks[ch], tag, c.on_clamp,
                                                         c.crossing and e.states[-1]["st_freq"] == clamp)
                nb = LC.expected(O, gid, ci, poked=False)
                check_against_oracle(g.family, got_twin[ch], nb, [(len(writes) - 1, dict(zip(peeks[ch][-1][1], got_twin[ch]["loop"])))], tag + " twin", False, False)
            except AssertionError as err:
                raise AssertionError(f"{tag}: {err}") from err
            if c.pokes:  # the poke reached its channel: the twin's went another way
                assert not same_bits(got[ch], got_twin[ch]), (tag, "the poked channel equals its twin")
            else:
                assert same_bits(got[ch], got_twin[ch]), (tag, "a channel without a poke differs from its twin")
            _LEDGER[f"{gid}-L{layout}/{c.name}"] = dict(branches={k: n for k, n in e.cov.items() if n}, max_symbol_deviation=dev,
                                                        soft_compared=nsoft, soft_differing=ndiff)
        for ch in range(LC.NCH):
            if ch not in LC.SPECIAL:
                assert same_bits(got[ch], got_twin[ch]), (gid, layout, "neighbour channel", ch, "differs from the bank that was never poked")
                ci = case_of(ch, ncases)[0]
                mate = next(c2 for c2 in range(LC.NCH) if c2 not in LC.SPECIAL and c2 != ch and case_of(c2, ncases)[0] == ci)
                assert same_bits(got[ch], got[mate]), (gid, layout, "channels", ch, mate, "carry the same stream and differ")
    finally:
        bank.close()
        twin.close()
    # the figures of profiles/loop_branches.json: written where LOOP_BRANCHES_LEDGER says, if it says
    out = os.environ.get("LOOP_BRANCHES_LEDGER")
    if out:
        with open(out, "w") as fh:
            json.dump(_LEDGER, fh, indent=1, sort_keys=True)


def test_hook_refusals_and_a_write_behind_a_poke(oracle_mod):
    """JAERO_EINVAL for a burst bank, a channel out of range, a negative frequency, a value that is not finite, a null state (the null context
    is a CPU case of tests/test_capi_host.py); a refused poke changes nothing; a write behind a poke works and continues from the poked values
    as the oracle does."""
    from jaero_amd import capi
    from jaero_amd import demodulator as D

    O = oracle_mod
    L = capi.lib()
    bb = D.DemodulatorBank([D.BurstOqpskSettings()] * 2, max_write_samples=LC.MAX_WRITE, softbit_capacity=4096)
    try:
        st = capi.LoopState(10500.0, 8000.0, 0.0, 0.0, 0.0, 0.0)
        assert L.jaero_debug_loop_poke(bb.h, 0, C.byref(st)) == capi.E_INVAL and b"burst" in L.jaero_last_error()
        assert L.jaero_debug_loop_peek(bb.h, 0, C.byref(st)) == capi.E_INVAL and b"burst" in L.jaero_last_error()
    finally:
        bb.close()
    family = "oqpsk_10500"
    bank = D.DemodulatorBank([LC.bank_settings(family)] * 3, ebno=True, status_log=True, capture_symbols=True, max_write_samples=LC.MAX_WRITE,
                             softbit_capacity=8192)
    try:
        x = LC.stream(LC.GROUPS["oqpsk_10500-c1"].cases[0].stream)[:20000]
        pcm = np.stack([x, x, x])
        bank.write(pcm[:, :4096])
        before = [peek(bank, ch) for ch in range(3)]
        good = dict(before[1])
        for ch in (-1, 3):
            assert L.jaero_debug_loop_poke(bank.h, ch, C.byref(capi.LoopState(**good))) == capi.E_INVAL, ch
            assert L.jaero_debug_loop_peek(bank.h, ch, C.byref(capi.LoopState())) == capi.E_INVAL, ch
        assert L.jaero_debug_loop_poke(bank.h, 1, None) == capi.E_INVAL and L.jaero_debug_loop_peek(bank.h, 1, None) == capi.E_INVAL
        for k, v in (("st_freq", -1.0), ("m2_freq", -0.5), ("st_freq", float("nan")), ("m2_freq", float("inf")), ("lf_x1", float("nan")),
                     ("lf_x2", float("-inf")), ("lf_y1", float("inf")), ("lf_y2", float("nan"))):
            assert L.jaero_debug_loop_poke(bank.h, 1, C.byref(capi.LoopState(**dict(good, **{k: v})))) == capi.E_INVAL, (k, v)
            assert b"jaero_debug_loop_poke" in L.jaero_last_error()
        assert [peek(bank, ch) for ch in range(3)] == before  # a refused poke wrote nothing
        poke(bank, 1, lf_y1=3.0, lf_y2=3.0)
        assert peek(bank, 1) == dict(good, lf_y1=3.0, lf_y2=3.0) and peek(bank, 0) == before[0] and peek(bank, 2) == before[2]
        for s in range(4096, 20000, 4096):  # the bank takes writes behind a poke
            bank.write(pcm[:, s:s + 4096])
        d = O.Demod(LC.oracle_settings(O, family), capture_symbols=True)
        d.write(x[:4096])
        d.set_loop_state(lf_y1=3.0, lf_y2=3.0)
        for s in range(4096, 20000, 4096):
            d.write(x[s:s + 4096])
        assert d.coverage()["lf_pi2_pos"] > 0
        ref = {"soft": d.take_soft(), "status": d.take_status(), "pending": d.pending, "symbols": d.take_symbols()}
        compare(bank.read_softbits(1), bank.read_symbols(1), bank.read_status_log(1), ref)
        assert np.array_equal(bank.read_softbits(0), bank.read_softbits(2)) and not np.array_equal(bank.read_symbols(0), bank.read_symbols(1))
    finally:
        bank.close()
