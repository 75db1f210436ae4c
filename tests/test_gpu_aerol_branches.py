"""GPU (-m gpu): the cases of tests/aerol_branch_cases.py -- the decisions of the three Aero-L bit pipelines that no generated frame stream takes
(tests/test_aerol_branch_cases.py shows on the CPU that each case takes its branch) -- in 70-channel banks against oracle/aerol_oracle.c.
The cases sit on scattered channels (0, 1, 31, 63, 64, 69, ..) with ordinary generated channels between them, so the lanes of a wavefront
diverge; every channel has its own oracle object, fed the same writes and ticks; signal units, events, packets, voice rows and every
tick_dcd return have to be equal, on every channel.  Both Viterbi layouts: the lane layout also selects k_aerol_post_packed and the
lane-layout R/T and C decoders."""
import ctypes as C

import numpy as np
import pytest

import aerol_branch_cases as ABC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    from jaero_amd import capi
    from jaero_amd import demodulator as D

    capi.lib()
    return D


def raw_packets(bank, ch, cap=4096):
    from jaero_amd import capi

    buf = np.empty((cap, 16), dtype=np.int32)
    n = C.c_int(0)
    capi.check(bank.L.jaero_aerol_read_packets(bank.h, ch, buf.ctypes.data, cap, C.byref(n)))
    return buf[: n.value].copy()


def run_bank(D, O, fam, which, width=None):
    per, plans, ticks, last, stride = ABC.bank(fam, which, width)
    fb, burst = ABC.FAMILIES[fam]
    bank = D.AeroLBank(ABC.NCH, fb, max_softbits_per_write=stride, su_capacity=1500, burst=burst)
    orc = [O.AeroL(fb, burst=burst) for _ in per]
    nticks = 0
    for buf, cnt, segs, t in ABC.bank_writes(per, plans, ticks, last, stride):
        bank.write(buf, cnt)
        for c, a in enumerate(orc):
            ABC.oracle_write(O, a, per[c], segs[c])
        for _ in range(t):
            got = np.asarray(bank.tick_dcd()).astype(np.int64)[: ABC.NCH]
            want = np.array([a.tick_dcd() for a in orc], dtype=np.int64)
            assert np.array_equal(got, want), (fam, which, "tick", nticks, np.flatnonzero(got != want).tolist())
            nticks += 1
    nrows = 0
    for c, a in enumerate(orc):
        who = (fam, which, c, per[c].name)
        assert np.array_equal(bank.read_events(c), a.take_events()), who
        if burst:
            want = a.take_packets()
            assert np.array_equal(raw_packets(bank, c), want), who
        else:
            want = a.take_sus()
            assert np.array_equal(bank.read_sus(c, 4096), want), who
        nrows += len(want)
        if fb == 8400:
            fn, voice = bank.read_voice(c)
            ofn, ovoice = a.take_voice()
            assert np.array_equal(fn, ofn) and np.array_equal(voice, ovoice), who
    bank.close()
    assert nrows > ABC.NCH  # the banks decode: the fillers alone give more rows than that
    return nticks


BANKS = [(fam, which, None) for fam in ABC.FAMILIES for which in ("quiet", "ticked")] + [("P10500", "quiet", 40000), ("P10500", "ticked", 40000)]


@pytest.mark.parametrize("layout", ["wave", "lanes"])
@pytest.mark.parametrize("fam,which,width", BANKS, ids=[f"{f}-{w}-{n or ABC.WIDTH}" for f, w, n in BANKS])
def test_branch_cases_bank_vs_oracle(D, oracle_mod, force_viterbi_layout, fam, which, width, layout):
    """The "quiet" bank holds the cases whose ticks come behind the stream, the "ticked" bank the case that ticks inside its stream (every channel of
    that bank is ticked with it).  P 10 500 also with writes of 40 000: k_aerol_bits<true> past its first frame."""
    force_viterbi_layout(layout)
    run_bank(D, oracle_mod, fam, which, width)


@pytest.mark.parametrize("layout", ["wave", "lanes"])
def test_wide_writes(D, oracle_mod, force_viterbi_layout, layout):
    """10 500 bps, max_softbits_per_write = 65 536, three writes: what a user who decodes a file in 64 Ki writes runs.  Locked channels holding twelve
    frames per write; noise channels with six planted one-arm words per write (more than the scan's AEROL_NMATCH); a word across position 32 768 (the
    scan's end); a marker only the scan's loop behind it sees; a channel that acquires lock behind it; a false sync ending five positions behind it;
    cases of 40 000 per write between them."""
    force_viterbi_layout(layout)
    per, plans, ticks, last, stride = ABC.bank("P10500", "wide")
    assert stride == 65536 and len(ticks) == 3 and sum(ticks) + last == 0
    assert {c.name.split(".")[-1] for c in per if "wide." in c.name} >= {"locked_seven_frames", "noise_six_words", "marker_behind_32768",
                                                                       "acquires_behind_32768", "false_sync_at_32768", "noise_six_words_40000"}
    run_bank(D, oracle_mod, "P10500", "wide")
