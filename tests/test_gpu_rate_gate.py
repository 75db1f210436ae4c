"""GPU (-m gpu): the gated rate lines (jaero_gate_*; k_rate_lines_gated in jaero_amd/csrc/k_rate.h) against their definition
(tests/rate_gate_oracle.py) and against the ungated meter.

R against an oracle goes by tests/rate_cases.py's assert_rule (RTOL = 1e-12, the rate lines' bound); what include/jaero_hip.h calls
bit-identical is compared with np.array_equal; the four numbers per channel are integers and compared exactly."""
import numpy as np
import pytest

import rate_cases as RC
import rate_gate_cases as GC
import rate_gate_oracle as GO
import rate_oracle as RO

pytestmark = pytest.mark.gpu

L, BINS = RO.L, RO.BINS
EMPTY = ([0], [2 ** 64 - 1], [0], [0])


@pytest.fixture(scope="module")
def RM():
    from jaero_amd import capi, ratemeter

    capi.lib()
    return ratemeter


def feed(m, pcm, cuts=None, device=False):
    """writes pcm [nch, n] into the meter in writes of `cuts` samples, from host memory or from a device tensor"""
    pos = 0
    for k in cuts or [pcm.shape[1]]:
        part = np.array(pcm[:, pos:pos + k])  # a contiguous, writable copy (the shared rows are read-only)
        if device:
            import torch

            t = torch.from_numpy(part).cuda()
            m.write_device(t.data_ptr(), k)
            torch.cuda.synchronize()  # t is freed when it goes out of scope
        else:
            m.write(part)
        pos += k
    assert pos == pcm.shape[1]


def run(RM, pcm, gates=None, cuts=None, device=False):
    """(R, (emax, emin, njoin, ejoin), nseg) of a fresh meter: gated under `gates` (None: ungated, no statistics)"""
    m = RM.RateMeter(pcm.shape[0], 48000.0, max_write_samples=max(cuts or [pcm.shape[1]]))
    if gates is not None:
        m.gate_enable()
        m.set_gate(gates)
    feed(m, pcm, cuts, device)
    R, nseg = m.read()
    st = None
    if gates is not None:
        *st, g, n2 = m.read_gate()
        assert n2 == nseg and g.tolist() == list(gates)
    m.close()
    return R, st, nseg


def assert_stats(got, want, where=""):
    for name, a, b in zip(("emax", "emin", "njoin", "ejoin"), got, want):
        assert a.dtype == np.uint64 and np.array_equal(a, np.asarray(b, dtype=np.uint64)), (where, name, a, b)


@pytest.mark.parametrize("nch", [1, 5, 67])
def test_gate_zero_is_the_ungated_meter(RM, nch):
    """Three segments and a tail of the case rows, every gate 0: the gated kernel's R equals the ungated kernel's bit for bit, everything
    joins, and the energies are the oracle's integers."""
    pcm = RC.case_rows(nch, RC.N_PARITY)
    o = GO.GatedRateOracle(nch)
    o.write(pcm)
    R, st, nseg = run(RM, pcm, [0] * nch)
    R0, _, n0 = run(RM, pcm)
    assert nseg == n0 == o.n == 3
    assert np.array_equal(R, R0), "gate 0 is not the ungated meter"
    RC.assert_rule(R, o.R, f"gate 0, nch={nch}")
    assert_stats(st, o.stats(), f"nch={nch}")
    assert st[2].tolist() == [3] * nch
    for c in RC.exact_rows(nch):
        assert (R[c] == 0.0).all()


@pytest.fixture(scope="module")
def mixed_whole(RM):
    """the mixed rows and their tail in one write from host memory"""
    pcm, gates = GC.mixed()
    return run(RM, pcm, gates)


def test_mixed_joining_inside_a_workgroup(RM, mixed_whole):
    """7 channels x 6 segments: 0 joins {0, 2, 5} beside 1 joining {1}; 2 nothing beside 3 everything; 4 everything beside 5 nothing; 6,
    alone in the last workgroup, {3}.  Gates exactly at a segment's E_j (joins) and at E_j + 1 (does not)."""
    pcm, gates = GC.mixed()
    o = GO.GatedRateOracle(GC.MIX_NCH)
    o.set_gate(gates)
    o.write(pcm)
    assert o.joined == GC.MIX_JOINS
    R, st, nseg = mixed_whole
    assert nseg == o.n == GC.MIX_NSEG
    RC.assert_rule(R, o.R, "mixed")
    assert_stats(st, o.stats(), "mixed")
    for c, joins in enumerate(GC.MIX_JOINS):
        if not joins:
            assert (R[c] == 0.0).all() and st[2][c] == 0 and st[3][c] == 0
            continue
        alone, _, n = run(RM, GC.joined_only(pcm, c, joins))  # an ungated meter fed this channel's joined segments alone
        assert n == len(joins) and np.array_equal(R[c], alone[0]), (c, "R is not that of the joined segments alone")


def test_cuts_and_input_memory_change_nothing(RM, mixed_whole):
    """The mixed rows and a 100-sample tail in one write and cut as [1, 4095, 4097, 1, 8197, rest], from host memory and from a device
    tensor: four times the same bits and the same numbers."""
    pcm, gates = GC.mixed()
    R, st, nseg = mixed_whole
    for cuts, device in ((GC.MIX_CUTS, False), (None, True), (GC.MIX_CUTS, True)):
        R2, st2, n2 = run(RM, pcm, gates, cuts, device)
        assert n2 == nseg == GC.MIX_NSEG
        assert np.array_equal(R, R2), ("R depends on the cuts or on where the input lies", cuts, device)
        assert_stats(st2, st, f"cuts={cuts} device={device}")


def test_life_cycle(RM):
    """set_gate between two writes holds from the next completed segment; reset clears sums and numbers and keeps gates and the pending
    segment; gate_enable(False) gives the ungated meter on the rest of the same grid, refuses set and read, and keeps the gates."""
    from jaero_amd import capi

    pcm, gates = GC.mixed()
    nch = GC.MIX_NCH
    cut = [2 * L + 50, 3 * L + 50, 4 * L + 50]
    m = RM.RateMeter(nch, 48000.0, max_write_samples=2 * L + 50)
    o = GO.GatedRateOracle(nch)
    m.gate_enable()
    *st, g, n = m.read_gate()
    assert_stats(st, [v * nch for v in EMPTY], "at enable")
    assert n == 0 and g.tolist() == [0] * nch
    for x in (m, o):
        x.write(pcm[:, :cut[0]])          # segments 0 and 1 under gate 0; 50 samples pending
        x.set_gate(gates)
        x.write(pcm[:, cut[0]:cut[1]])    # segment 2: the new gates decide
    R, n = m.read()
    *st, g, n2 = m.read_gate()
    assert n == n2 == o.n == 3 and g.tolist() == gates and o.joined[1] == [0, 1] and o.joined[0] == [0, 1, 2]
    RC.assert_rule(R, o.R, "gates set between two writes")
    assert_stats(st, o.stats(), "gates set between two writes")
    m.reset()
    o.reset()
    R, n = m.read()
    *st, g, n2 = m.read_gate()
    assert n == n2 == 0 and not R.any() and g.tolist() == gates
    assert_stats(st, [v * nch for v in EMPTY], "after reset")
    for x in (m, o):
        x.write(pcm[:, cut[1]:cut[2]])    # segment 3, with the 50 samples that were pending
    R, n = m.read()
    *st, g, n2 = m.read_gate()
    assert n == n2 == o.n == 1 and o.joined[6] == [0] and o.joined[0] == []
    RC.assert_rule(R, o.R, "after reset")
    assert_stats(st, o.stats(), "after reset")
    # off: the parent's meter on what is left of the same grid
    m.gate_enable(False)
    R, n = m.read()
    assert n == 0 and not R.any()
    for call in (lambda: m.set_gate([7] * nch), m.read_gate):
        with pytest.raises(capi.JaeroError) as e:
            call()
        assert e.value.code == capi.E_INVAL and "jaero_gate_" in str(e.value)
    m.write(pcm[:, cut[2]:])              # segments 4 and 5 and the tail
    R, n = m.read()
    fresh, _, n3 = run(RM, pcm[:, 4 * L:])
    assert n == n3 == 2 and np.array_equal(R, fresh), "gate_enable(False) is not the ungated meter"
    m.gate_enable()
    *st, g, n2 = m.read_gate()
    assert n2 == 0 and g.tolist() == gates, "the refused set_gate, or a switch, changed the gates"
    assert_stats(st, [v * nch for v in EMPTY], "enabled again")
    m.close()


def test_burst_rows_read_their_rate(RM):
    """Three burst rows, one continuous 1200 bps MSK row and one noise row, 256 segments in 4-segment writes, by the flow of
    jaero_amd/ratemeter.py's docstring: gate 0 -> read_gate -> set_gate(suggest_gate) -> reset -> measure -> classify_rates.  The margins
    are asserted on the CPU oracles alone in tests/test_rate_gate_host.py."""
    pcm = GC.burst_rows()
    f = GC.burst_flow()
    cuts = [GC.BURST_WRITE] * (pcm.shape[1] // GC.BURST_WRITE)
    m = RM.RateMeter(5, GC.BURST_FS, max_write_samples=GC.BURST_WRITE)
    ungated = RM.RateMeter(5, GC.BURST_FS, max_write_samples=GC.BURST_WRITE)
    feed(ungated, pcm, cuts)
    Ru, nu = ungated.read()
    ungated.close()
    m.gate_enable()
    feed(m, pcm, cuts)
    R0, n0 = m.read()
    emax, emin, njoin, ejoin, g, _ = m.read_gate()
    assert n0 == nu == GC.BURST_NSEG and np.array_equal(R0, Ru) and g.tolist() == [0] * 5
    RC.assert_rule(R0, f["first"][0], "bursts, gate 0")
    assert_stats((emax, emin, njoin, ejoin), f["first"][1], "bursts, gate 0")
    gates = RM.suggest_gate(emax, emin)
    assert gates == f["gates"]
    m.set_gate(gates)
    m.reset()
    feed(m, pcm, cuts)
    R1, n1 = m.read()
    *st, g, n2 = m.read_gate()
    m.close()
    assert n1 == n2 == GC.BURST_NSEG and g.tolist() == gates
    RC.assert_rule(R1, f["second"][0], "bursts, gated")
    assert_stats(st, f["second"][1], "bursts, gated")
    rate, audio, score = RM.classify_rates(R1, m.fs)
    rate_u = RM.classify_rates(Ru, m.fs)[0]
    print("gated scores, dB:\n", np.round(score, 1), "\naudio:", audio, "\nduty:", st[2] / n1)
    assert rate.tolist() == GC.BURST_RATES
    assert rate_u.tolist() == GC.BURST_RATES_UNGATED
