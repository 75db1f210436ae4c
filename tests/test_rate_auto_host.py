"""CPU: the one-pass gates without a device -- the jaero_gate2_* exports and refusals, energy_bin / bin_edge / hist_extremes in exact
integers, the oracle (tests/rate_auto_oracle.py) against the tables of energy sequences, against RateOracle and against itself, and the
rates, counts, starts and margins of the GPU burst tests (tests/test_gpu_rate_auto.py) met by the oracles alone."""
import ctypes as C

import numpy as np
import pytest

import rate_auto_cases as AC
import rate_auto_oracle as AO
import rate_cases as RC
import rate_gate_cases as GC
import rate_oracle as RO
from jaero_amd import capi, ratemeter as RM

L, BINS = RO.L, RO.BINS
NONE = AC.NONE


# ---------------------------------------------------------------------------------------------- the C ABI without a device
def test_library_exports_the_gate2_symbols():
    names = [s for s in capi.EXPORTS if s.startswith("jaero_gate2_")]
    assert sorted(names) == ["jaero_gate2_enable", "jaero_gate2_read", "jaero_gate2_read_hist"]
    Lb = capi.lib()
    for name in names:
        assert hasattr(Lb, name), name
    assert (capi.GATE_MANUAL, capi.GATE_AUTO, capi.GATE_HIST, capi.GATE_HBINS) == (1, 2, 4, 321)
    assert Lb.jaero_abi_version() == 1


def test_null_handles_and_modes_are_refused():
    Lb = capi.lib()
    st, g, h, n = np.zeros(6, np.uint64), np.zeros(1, np.uint64), np.zeros(321, np.uint32), C.c_longlong(0)
    for mode in (0, 1, 2, 3, 4, 5, 7, -1):
        assert Lb.jaero_gate2_enable(None, mode) == capi.E_INVAL
        assert b"jaero_gate2_enable" in Lb.jaero_last_error()
    assert Lb.jaero_gate2_read(None, st.ctypes.data, g.ctypes.data, C.byref(n)) == capi.E_INVAL
    assert b"jaero_gate2_read" in Lb.jaero_last_error() and b"jaero_gate2_read_hist" not in Lb.jaero_last_error()
    assert Lb.jaero_gate2_read_hist(None, h.ctypes.data, C.byref(n)) == capi.E_INVAL
    assert b"jaero_gate2_read_hist" in Lb.jaero_last_error()


# ---------------------------------------------------------------------------------------------- the histogram's bins
def test_energy_bin_and_bin_edge():
    for E, b in zip([0, 1, 7, 8, 15, 16, 17, 18, 2 ** 42 - 1, 2 ** 42], [0, 1, 7, 8, 15, 16, 16, 17, 319, 320]):
        assert RM.energy_bin(E) == b == AO.energy_bin(E), (E, b)
    edges = [RM.bin_edge(b) for b in range(RM.HBINS)]
    assert RM.HBINS == 321 and edges[:9] == list(range(9)) and edges[320] == 2 ** 42
    assert all(a < b for a, b in zip(edges, edges[1:]))
    for b, e in enumerate(edges):
        assert RM.energy_bin(e) == b and (b == 320 or RM.energy_bin(edges[b + 1] - 1) == b)
    rng = np.random.default_rng(3)
    for E in [int(v) for v in rng.integers(0, 2 ** 42, 2000)] + [int(v) for v in rng.integers(0, 5000, 500)]:
        b = RM.energy_bin(E)
        assert b == AO.energy_bin(E) and RM.bin_edge(b) <= E and (b == 320 or E < RM.bin_edge(b + 1))
    width = [10 * np.log10(edges[b + 1] / edges[b]) for b in range(8, 320)]
    assert 0.27 < min(width) and max(width) < 0.52  # from 8 upward a bin is 0.28 to 0.51 dB wide
    for bad in (lambda: RM.energy_bin(-1), lambda: RM.bin_edge(321), lambda: RM.bin_edge(-1)):
        with pytest.raises(ValueError):
            bad()


def test_hist_extremes_and_suggest_gate_on_them():
    h = np.zeros((4, RM.HBINS), dtype=np.uint32)
    h[0, [40, 100, 200]] = [5, 2, 1]   # the single segment in bin 200 is a click: it falls out
    h[1, [7, 9]] = [1, 1]              # no bin with two segments
    h[2, 50] = 9                       # one level
    #    row 3: empty
    hi, lo = RM.hist_extremes(h)
    assert hi.dtype == lo.dtype == np.uint64
    assert hi.tolist() == [RM.bin_edge(100), 0, RM.bin_edge(50), 0] and lo.tolist() == [RM.bin_edge(40), NONE, RM.bin_edge(50), NONE]
    assert RM.suggest_gate(hi, lo) == [(RM.bin_edge(100) + RM.bin_edge(40)) // 2, 0, 0, 0]
    hi1, lo1 = RM.hist_extremes(h, min_count=1)
    assert hi1.tolist() == [RM.bin_edge(200), RM.bin_edge(9), RM.bin_edge(50), 0] and lo1[1] == 7
    assert RM.hist_extremes(h[0])[0].tolist() == [RM.bin_edge(100)]  # one row
    with pytest.raises(ValueError):
        RM.hist_extremes(np.zeros((2, 320)))


# ---------------------------------------------------------------------------------------------- the rule on chosen energies
def auto_of(pcm, cuts=None, mode=AO.AUTO):
    o = AO.AutoRateOracle(pcm.shape[0], mode)
    pos = 0
    for n in (cuts or [pcm.shape[1]]):
        o.write(pcm[:, pos:pos + n])
        pos += n
        assert o.n == pos // L
    assert pos == pcm.shape[1]
    return o


def from_start(pcm, c, o):
    """RateOracle fed channel c's joined segments from `start` on, in order: what the definition says its R equals bit for bit"""
    alone = RO.RateOracle(1)
    if o.joined[c]:
        alone.write(AC.joined_only(pcm, c, o.joined[c]))
    assert alone.n == len(o.joined[c]) == o.njoin[c]
    assert o.start[c] == NONE or o.joined[c][0] == o.start[c]
    return alone.R[0]


def test_empty_state():
    o = AO.AutoRateOracle(3)
    assert [v.tolist() for v in o.stats()] == [[0] * 3, [NONE] * 3, [0] * 3, [0] * 3, [0] * 3, [NONE] * 3]
    assert all(v.dtype == np.uint64 for v in o.stats()) and o.gate == [0] * 3 and o.n == 0 and not o.R.any() and not o.hist_array().any()


def test_ones_rows_give_the_table():
    for idx, pcm in AC.ones_groups():
        o = auto_of(pcm)
        for c, i in enumerate(idx):
            energies, gates, joined, start = AC.ONES[i]
            assert o.n == len(energies)
            assert gates is None or o.gates[c] == gates, (i, o.gates[c])
            assert o.joined[c] == joined and o.start[c] == start and o.njoin[c] == len(joined), (i, o.joined[c], o.start[c])
            assert o.ejoin[c] == sum(energies[j] for j in joined)
            assert o.emax[c] == max(energies) and o.emin[c] == min(energies) and o.e2[c] == sorted(energies)[-2]
            assert np.array_equal(o.R[c], from_start(pcm, c, o)), i
            # the histogram is what energy_bin says, and the row's total is the segment count
            want = np.bincount([RM.energy_bin(e) for e in energies], minlength=RM.HBINS)
            assert np.array_equal(o.hist_array()[c], want) and o.hist_array()[c].sum() == len(energies)


def test_level_rows_are_the_ungated_oracle():
    """the case rows over three segments and a tail never leave gate 0: R is RateOracle's bit for bit, start stays 2^64 - 1, and a row of
    zeros joins everything with R == 0"""
    pcm = RC.case_rows(11, RC.N_PARITY)
    want = RO.RateOracle(11)
    want.write(pcm)
    o = auto_of(pcm)
    assert o.n == want.n == 3 and np.array_equal(o.R, want.R)
    assert o.gate == [0] * 11 and o.start == [NONE] * 11 and o.njoin == [3] * 11
    for c in RC.exact_rows(11):
        assert not o.R[c].any()
    assert o.emax[RC.ZERO] == o.e2[RC.ZERO] == 0


def test_mixed_rows_join_and_restart_as_built():
    pcm = AC.auto_mixed()
    o = auto_of(pcm)
    assert o.n == AC.AMIX_NSEG and o.joined == AC.AMIX_JOINS and o.start == AC.AMIX_START
    whole = RO.RateOracle(AC.AMIX_NCH)
    whole.write(pcm)
    for c in range(AC.AMIX_NCH):
        assert np.array_equal(o.R[c], from_start(pcm, c, o)), c
        if o.gate[c] == 0:  # whoever never leaves gate 0 is the ungated channel
            assert np.array_equal(o.R[c], whole.R[c]) and o.start[c] == NONE
    assert not o.R[2].any() and o.njoin[2] == AC.AMIX_NSEG
    assert o.hist_array().sum(axis=1).tolist() == [AC.AMIX_NSEG] * AC.AMIX_NCH


def test_auto_oracle_is_cut_independent():
    pcm = AC.auto_mixed()
    assert sum(AC.AMIX_CUTS) == pcm.shape[1] and AC.AMIX_CUTS[:5] == RC.CUTS[:5]
    whole, cut = auto_of(pcm), auto_of(pcm, AC.AMIX_CUTS)
    assert np.array_equal(whole.R, cut.R) and whole.n == cut.n and whole.gate == cut.gate
    assert all(np.array_equal(a, b) for a, b in zip(whole.stats(), cut.stats())) and whole.hist == cut.hist


def test_manual_with_histogram_is_the_gated_oracle():
    import rate_gate_oracle as GO

    pcm, gates = GC.mixed()
    o = AO.AutoRateOracle(GC.MIX_NCH, AO.MANUAL | AO.HIST)
    o.set_gate(gates)
    o.write(pcm)
    want = GO.GatedRateOracle(GC.MIX_NCH)
    want.set_gate(gates)
    want.write(pcm)
    assert np.array_equal(o.R, want.R) and o.joined == want.joined == GC.MIX_JOINS and o.gate == gates and o.start == [NONE] * GC.MIX_NCH
    assert all(np.array_equal(a, b) for a, b in zip(o.stats()[:4], want.stats()))


def test_reset_under_auto_zeroes_the_gates_and_keeps_the_grid():
    pcm = AC.auto_mixed()
    o = AO.AutoRateOracle(AC.AMIX_NCH)
    o.write(pcm[:, :4 * L + 50])
    assert o.gate[0] > 0 and o.start[0] == 3
    o.reset()
    assert o.gate == [0] * AC.AMIX_NCH and o.n == 0 and not o.R.any() and o.start == [NONE] * AC.AMIX_NCH and o.e2 == [0] * AC.AMIX_NCH
    o.write(pcm[:, 4 * L + 50:])
    want = auto_of(pcm[:, 4 * L:])
    assert o.n == want.n == 4 and np.array_equal(o.R, want.R) and o.joined == want.joined and o.gate == want.gate


# ---------------------------------------------------------------------------------------------- the burst rows in one pass
@pytest.mark.parametrize("arrangement", AC.ARRANGEMENTS)
def test_burst_rows_in_one_pass_on_the_oracle(arrangement):
    """Rates, joined counts and starts as on record for the three arrangements; every winner >= 13.0 dB, the noise row <= 7 dB (the
    margins of tests/test_rate_gate_host.py); every channel's R is RateOracle's on its joined segments from start on."""
    pcm = AC.burst_rows(arrangement)
    o = AC.burst_auto(arrangement)
    rate, audio, score = RM.classify_rates(o.R, GC.BURST_FS)
    best = score.max(axis=1)
    print(arrangement, "best scores, dB:", np.round(best, 1), "joined:", o.njoin, "start:", o.start, "gates:", o.gate)
    assert o.n == 256
    assert rate.tolist() == AC.AUTO_RATES
    assert o.njoin == AC.AUTO_JOINED[arrangement] and o.start == AC.AUTO_START[arrangement]
    assert (best[:4] >= 13.0).all() and best[4] <= 7.0, best
    assert all(g > 0 for g in o.gate[:3]) and o.gate[3:] == [0, 0]
    for c in range(5):
        assert np.array_equal(o.R[c], from_start(pcm, c, o)), c
    assert o.hist_array().sum(axis=1).tolist() == [256] * 5



def test_click_rows_two_passes_on_the_oracle():
    """Today's flow on the click rows fails on the 10 500 bps row and nearly on the noise row; the gates from the histogram's extremes
    read every rate."""
    f = AC.click_two_pass()
    gates, R, st = f["today"]
    rate, _, score = RM.classify_rates(R, GC.BURST_FS)
    print("today:", gates, rate.tolist(), np.round(score.max(axis=1), 1), "joined:", st[2])
    assert rate.tolist() == AC.CLICK_RATES_TODAY  # the failure
    gates, R, st = f["hist"]
    rate, _, score = RM.classify_rates(R, GC.BURST_FS)
    best = score.max(axis=1)
    print("histogram:", gates, rate.tolist(), np.round(best, 1), "joined:", st[2])
    assert gates == AC.CLICK_HIST_GATES
    assert rate.tolist() == AC.AUTO_RATES and (best[:4] >= 13.0).all() and best[4] <= 7.0, best
