"""CPU: the rate lines read on the device, without a device.  The definition (tests/rate_lines_oracle.py, literal loops) followed by
decide_rates equals classify_rates -- np.array_equal, audio with equal_nan -- on the oracle's sums of the case rows, on the made rows and
on the blind chain's sums, at 48 and 12 kHz and for kmin 8, 7 and 1 (both parities of the median's count); the tie rule is under test
because most maxima of the case rows are ties; the two new exports exist and refuse what needs no handle."""
import ctypes as C

import numpy as np
import pytest

import rate_cases as RC
import rate_lines_cases as LC
import rate_lines_oracle as LO
import rate_oracle as RO
from jaero_amd import capi, ratemeter as RM
from jaero_amd.ratemeter import decide_rates  # the import this file fails on without the feature

L, BINS = RO.L, RO.BINS


@pytest.fixture(scope="module")
def case_R():
    """the oracle's sums of the 11 case rows over three segments and a tail"""
    o = RO.RateOracle(11)
    o.write(RC.case_rows(11, RC.N_PARITY))
    assert o.n == 3
    o.R.flags.writeable = False
    return o.R


@pytest.fixture(scope="module")
def chain_R():
    import chan_oracle as CO

    _, _, ystar = RC.chain()
    o = RO.RateOracle(5)
    assert o.write(CO.to_int16(ystar)) == RC.CHAIN_SEGS
    o.R.flags.writeable = False
    return o.R


def test_distances_are_classify_rates_own():
    assert RM.rate_distances(48000.0) == [51, 102, 717, 896]
    assert RM.rate_distances(12000.0) == [205, 410, 2867, 3584]
    assert RM.rate_distances(48000.0, (1200,)) == [102]


@pytest.mark.parametrize("kmin", LC.KMIN)
@pytest.mark.parametrize("fs", LC.FS)
def test_definition_and_decide_rates_equal_classify_rates(case_R, chain_R, fs, kmin):
    for name, R in (("case rows", case_R), ("made rows", LC.made_rows()), ("chain", chain_R)):
        got = LC.decide_from_oracle(R, fs, kmin)
        want = LC.classify_reference(R, fs, kmin)
        LC.assert_decisions_equal(got, want, f"{name}, fs={fs}, kmin={kmin}")
        if fs == 12000.0:
            assert np.isneginf(got[2][:, 2:]).all()  # 8400 and 10 500 bps: skipped


def test_skipped_distances_and_the_chain(chain_R):
    d = RM.rate_distances(12000.0)
    floor, score, where = LO.lines(chain_R, 8, d)
    assert (where[:, 2:] == -1).all() and (score[:, 2:] == 0.0).all() and (where[:, :2] >= 8).all()
    rate, audio, _ = LC.decide_from_oracle(chain_R, RC.CHAIN_FS_OUT, 8)
    assert rate.tolist() == RC.CHAIN_RATES and np.isnan(audio[4])


def test_most_maxima_of_the_case_rows_are_ties(case_R):
    """The three-bin maximum makes plateaus: of the 44 (row, rate) maxima more than half are attained at more than one a, so a search that
    did not take the smallest a would be caught by the comparisons above."""
    t = LO.ties(case_R, 8, LC.D48)
    print(f"{int(t.sum())} of {t.size} (row, rate) maxima of the case rows are ties")
    assert t.size == 44 and t.sum() > 22


def test_made_rows_do_what_they_were_made_for():
    R = LC.made_rows()
    floor, score, where = LO.lines(R, 8, LC.D48)
    assert where[1, 1] == 99 and score[1, 1] == 50.0            # pairs (100, 202) and (300, 402): the first, and its plateau's first bin
    assert floor[5] in (1.0, 2.0, 3.0) and floor[6] == 5e-324
    assert score[4, 3] == 1e300 and where[4, 3] == 599
    assert where[7, 0] == 1996 and score[7, 0] == 100.0          # 1997 and 2048 are 51 apart; P carries the line to 2047
    assert where[8, 0] == LC.AT_KMIN and score[8, 0] == 80.0
    assert (score[9] == 0.0).all() and (where[9] == 8).all() and floor[9] == 0.0
    assert (where[0] == 8).all() and (score[0] == 1.0).all()     # all ones: everything ties, kmin wins
    for kmin in LC.KMIN:  # the median is numpy's, for both parities
        f = LO.lines(R, kmin, LC.D48)[0]
        with np.errstate(over="ignore"):
            assert np.array_equal(f, np.median(R[:, kmin:], axis=1))
    rate, audio, score_db = LC.decide_from_oracle(R, 48000.0, 8)
    assert np.isposinf(score_db[4, 3]) and rate[4] == 10500
    assert rate[9] == 0 and np.isneginf(score_db[9]).all()


def test_decide_rates_takes_one_row():
    R = LC.made_rows()[1]
    d = RM.rate_distances(48000.0)
    f, s, w = LO.lines_row(R, 8, d)
    rate, audio, score_db = decide_rates(f, s, w, d, 48000.0)
    want = RM.classify_rates(R, 48000.0)
    assert rate == want[0] == 1200 and audio == want[1] and np.array_equal(score_db, want[2])
    with pytest.raises(ValueError):
        decide_rates(f, s[:3], w[:3], d, 48000.0)


# ---------------------------------------------------------------------------------------------- the C ABI without a device
def test_library_exports_the_two_new_symbols():
    Lb = capi.lib()
    for name in ("jaero_lines_classify", "jaero_debug_rate_poke"):
        assert name in capi.EXPORTS and hasattr(Lb, name), name
    assert Lb.jaero_abi_version() == 1


def test_refusals_that_need_no_handle():
    Lb = capi.lib()
    d = np.array([51, 102], dtype=np.int32)
    floor, score, where = np.zeros(1), np.zeros(2), np.zeros(2, np.int32)
    n, ms = C.c_longlong(0), C.c_double(0.0)
    fake = C.c_void_p(1)  # never dereferenced: a null pointer is refused first
    args = lambda **kw: [kw.get(k, v) for k, v in (("r", fake), ("kmin", 8), ("nd", 2), ("d", d.ctypes.data), ("floor", floor.ctypes.data),
                                                   ("score", score.ctypes.data), ("where", where.ctypes.data), ("nseg", C.byref(n)),
                                                   ("ms", C.byref(ms)))]
    for kw, word in (({"r": None}, b"null handle"), ({"d": None}, b"d is null"), ({"floor": None}, b"floor is null"),
                     ({"score": None}, b"score is null"), ({"where": None}, b"where is null"), ({"nseg": None}, b"nseg is null")):
        assert Lb.jaero_lines_classify(*args(**kw)) == capi.E_INVAL, kw
        assert b"jaero_lines_classify" in Lb.jaero_last_error() and word in Lb.jaero_last_error(), Lb.jaero_last_error()
    sums = np.zeros(BINS)
    assert Lb.jaero_debug_rate_poke(None, sums.ctypes.data, 0) == capi.E_INVAL
    assert b"jaero_debug_rate_poke" in Lb.jaero_last_error()
    assert Lb.jaero_debug_rate_poke(fake, None, 0) == capi.E_INVAL
