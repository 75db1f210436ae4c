"""CPU: the gated rate lines without a device -- the jaero_gate_* exports and refusals, the oracle (tests/rate_gate_oracle.py) against
RateOracle and against itself, suggest_gate literally, and the margins of the GPU classification test (tests/test_gpu_rate_gate.py) met by
the oracles alone."""
import ctypes as C

import numpy as np

import rate_cases as RC
import rate_gate_cases as GC
import rate_gate_oracle as GO
import rate_oracle as RO
from jaero_amd import capi, ratemeter as RM

L, BINS = RO.L, RO.BINS


# ---------------------------------------------------------------------------------------------- the C ABI without a device
def test_library_exports_the_gate_symbols():
    names = [s for s in capi.EXPORTS if s.startswith("jaero_gate_")]
    assert sorted(names) == ["jaero_gate_enable", "jaero_gate_read", "jaero_gate_set"]
    Lb = capi.lib()
    for name in names:
        assert hasattr(Lb, name), name
    assert sorted(s for s in capi.EXPORTS if s.startswith("jaero_rate_")) == sorted(
        "jaero_rate_" + n for n in ("create", "destroy", "write", "reset", "read", "profile_enable", "profile_read"))
    assert Lb.jaero_abi_version() == 1


def test_null_handles_and_arguments_are_refused():
    Lb = capi.lib()
    st, g, n = np.zeros(4, np.uint64), np.zeros(1, np.uint64), C.c_longlong(0)
    assert Lb.jaero_gate_enable(None, 1) == capi.E_INVAL
    assert b"jaero_gate_enable" in Lb.jaero_last_error()
    assert Lb.jaero_gate_set(None, g.ctypes.data) == capi.E_INVAL
    assert b"jaero_gate_set" in Lb.jaero_last_error()
    assert Lb.jaero_gate_read(None, st.ctypes.data, g.ctypes.data, C.byref(n)) == capi.E_INVAL
    assert b"jaero_gate_read" in Lb.jaero_last_error()


# ---------------------------------------------------------------------------------------------- the oracle against itself
def gated_of(pcm, gates=None, cuts=None):
    o = GO.GatedRateOracle(pcm.shape[0])
    if gates is not None:
        o.set_gate(gates)
    pos = 0
    for n in (cuts or [pcm.shape[1]]):
        o.write(pcm[:, pos:pos + n])
        pos += n
        assert o.n == pos // L
    assert pos == pcm.shape[1]
    return o


def test_empty_state():
    o = GO.GatedRateOracle(3)
    emax, emin, njoin, ejoin = o.stats()
    assert emax.tolist() == [0] * 3 and emin.tolist() == [2 ** 64 - 1] * 3 and njoin.tolist() == ejoin.tolist() == [0] * 3
    assert emin.dtype == np.uint64 and o.n == 0 and not o.R.any() and o.gate == [0] * 3
    o.write(RC.case_rows(3, L - 1))  # no segment yet
    assert o.stats()[1].tolist() == [2 ** 64 - 1] * 3 and o.n == 0


def test_gate_zero_is_the_ungated_oracle():
    pcm = RC.case_rows(11, RC.N_PARITY)
    want = RO.RateOracle(11)
    want.write(pcm)
    o = gated_of(pcm)
    assert o.n == want.n == 3 and np.array_equal(o.R, want.R)
    assert o.njoin == [3] * 11 and all(o.joined[c] == [0, 1, 2] for c in range(11))
    E = np.array([GO.segment_energy(pcm[:, j * L:(j + 1) * L]) for j in range(3)])
    assert o.emax == E.max(axis=0).tolist() and o.emin == E.min(axis=0).tolist() and o.ejoin == E.sum(axis=0).tolist()
    assert max(o.emax) < 2 ** 43
    for c in RC.exact_rows(11):  # a zero row joins under gate 0, with R == 0 exactly; so does a constant one
        assert not o.R[c].any() and o.njoin[c] == 3
    assert o.emax[RC.ZERO] == 0 and o.emin[RC.CONST] == L * 12345 ** 2


def test_a_channels_R_is_the_ungated_R_of_its_joined_segments():
    pcm, gates = GC.mixed()
    o = gated_of(pcm, gates)
    assert o.n == GC.MIX_NSEG and o.joined == GC.MIX_JOINS
    for c, joins in enumerate(GC.MIX_JOINS):
        assert o.njoin[c] == len(joins)
        if not joins:
            assert not o.R[c].any() and o.ejoin[c] == 0  # a zero row never joins under a gate > 0 (channel 2); nor does channel 5
            continue
        alone = RO.RateOracle(1)
        alone.write(GC.joined_only(pcm, c, joins))
        assert alone.n == len(joins) and np.array_equal(o.R[c], alone.R[0]), c
    whole = RO.RateOracle(GC.MIX_NCH)
    whole.write(pcm)
    assert np.array_equal(o.R[3], whole.R[3]) and np.array_equal(o.R[4], whole.R[4])  # whoever joins everything is the ungated channel


def test_gated_oracle_is_cut_independent():
    pcm, gates = GC.mixed()
    assert sum(GC.MIX_CUTS) == pcm.shape[1] and GC.MIX_CUTS[:5] == RC.CUTS[:5]
    whole, cut = gated_of(pcm, gates), gated_of(pcm, gates, GC.MIX_CUTS)
    assert np.array_equal(whole.R, cut.R) and whole.n == cut.n == GC.MIX_NSEG
    assert all(np.array_equal(a, b) for a, b in zip(whole.stats(), cut.stats()))


def test_reset_keeps_the_gates_and_the_grid():
    pcm, gates = GC.mixed()
    o = GO.GatedRateOracle(GC.MIX_NCH)
    o.set_gate(gates)
    o.write(pcm[:, :2 * L + 50])
    o.reset()
    assert o.gate == gates and o.n == 0 and not o.R.any() and o.stats()[1].tolist() == [2 ** 64 - 1] * GC.MIX_NCH
    o.write(pcm[:, 2 * L + 50:])
    want = gated_of(pcm[:, 2 * L:], gates)
    assert o.n == want.n == 4 and np.array_equal(o.R, want.R) and o.joined == want.joined
    assert o.joined[0] == [0, 3] and o.joined[6] == [1]  # segments 2, 5 and 3 of the grid, counted from the reset


def test_a_gate_holds_from_the_next_completed_segment():
    pcm, gates = GC.mixed()
    o = GO.GatedRateOracle(GC.MIX_NCH)
    o.write(pcm[:, :2 * L + 50])  # segments 0 and 1 under gate 0; 50 samples of segment 2 pending
    o.set_gate(gates)
    o.write(pcm[:, 2 * L + 50:])  # segment 2 is completed by this write: the new gates decide
    assert o.joined[1] == [0, 1] and o.joined[2] == [0, 1] and o.joined[0] == [0, 1, 2, 5] and o.joined[6] == [0, 1, 3]


# ---------------------------------------------------------------------------------------------- suggest_gate
def test_suggest_gate_literally():
    big = 2 ** 43 - 1
    emax = [0, 10, 10, 3, 2, 299, 300, 7, big, 2 ** 63]
    emin = [2 ** 64 - 1, 10, 0, 2, 2, 200, 200, 5, big - 1, 1]
    #       empty        equal  emin 0  3:2  equal 299:200  3:2   7:5   close    wide
    want = [0, 0, 5, 2, 0, 0, 250, 0, 0, (2 ** 63 + 1) // 2]
    assert RM.suggest_gate(emax, emin) == want
    assert RM.suggest_gate(np.array(emax[:8], dtype=np.uint64), np.array(emin[:8], dtype=np.uint64)) == want[:8]
    for hi, lo, w in zip(emax, emin, want):  # the definition, per channel
        assert w == ((hi + lo) // 2 if hi > 0 and 2 * hi >= 3 * lo else 0)
    assert RM.suggest_gate([0], [0]) == [0]                    # a zero row
    assert RM.suggest_gate([7], [5], min_ratio=1.4) == [6]     # 7 : 5 is 1.4 exactly
    assert RM.suggest_gate([6999], [5000], min_ratio=1.4) == [0]
    assert all(isinstance(v, int) for v in RM.suggest_gate(np.array([4], dtype=np.uint64), np.array([1], dtype=np.uint64)))


# ---------------------------------------------------------------------------------------------- the classification test's margins
def test_burst_margins_on_the_oracle():
    """The conditions of the GPU burst test, met by the oracles alone.  Ungated, the three burst rows' best score is at most 9.0 dB and they
    read 0; gated by suggest_gate of their own statistics they read their rate with at least 13.0 dB, the audio offset within a bin of fc.
    The continuous row and the noise row get gate 0.  (If a row misses a margin after a signalgen change: lengthen it or raise Eb/N0.)"""
    f = GC.burst_flow()
    (R0, st0, n0), gates, (R1, st1, n1) = f["first"], f["gates"], f["second"]
    assert n0 == n1 == GC.BURST_NSEG
    ungated = RO.RateOracle(5)
    ungated.write(GC.burst_rows()[:, :8 * L])
    assert np.array_equal(ungated.R, gated_of(GC.burst_rows()[:, :8 * L]).R)
    rate0, _, score0 = RM.classify_rates(R0, GC.BURST_FS)
    rate1, audio1, score1 = RM.classify_rates(R1, GC.BURST_FS)
    print("ungated, dB:\n", np.round(score0, 1), "\ngated, dB:\n", np.round(score1, 1), "\naudio:", audio1, "\njoined:", st1[2], "gates:", gates)
    assert rate0.tolist() == GC.BURST_RATES_UNGATED and rate1.tolist() == GC.BURST_RATES
    assert (score0[:3].max(axis=1) <= 9.0).all(), score0[:3].max(axis=1)
    assert (score1[:3].max(axis=1) >= 13.0).all(), score1[:3].max(axis=1)
    assert (np.abs(audio1[:3] - np.array(GC.BURST_FC)) <= GC.BURST_FS / L).all(), audio1
    assert st1[2].tolist() == GC.BURST_JOINED and all(g > 0 for g in gates[:3]) and gates[3:] == [0, 0]
    assert np.array_equal(R1[3:], R0[3:])  # under gate 0 the continuous rows are what they were


def test_continuous_rows_get_gate_zero():
    """suggest_gate leaves the blind chain's five channels and the nine case rows over 16 segments ungated."""
    import chan_oracle as CO

    _, _, ystar = RC.chain()
    for pcm in (CO.to_int16(ystar), RC.base_rows(16 * L)):
        o = gated_of(pcm)
        ratio = [hi / lo if lo else float("nan") for hi, lo in zip(o.emax, o.emin)]
        print("strongest over weakest segment:", np.round(ratio, 3))
        assert RM.suggest_gate(o.emax, o.emin) == [0] * pcm.shape[0]
