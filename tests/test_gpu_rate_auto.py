"""GPU (-m gpu): the one-pass gates (jaero_gate2_*; k_rate_lines_auto in jaero_amd/csrc/k_rate.h) against their definition
(tests/rate_auto_oracle.py), against the ungated meter and against the gated one.

R against an oracle goes by tests/rate_cases.py's assert_rule (RTOL = 1e-12, the rate lines' bound); what include/jaero_hip.h calls
bit-identical is compared with np.array_equal; the numbers, the gates and the histogram are integers and compared exactly."""
import numpy as np
import pytest

import rate_auto_cases as AC
import rate_auto_oracle as AO
import rate_cases as RC
import rate_gate_cases as GC
import rate_gate_oracle as GO
import rate_oracle as RO

pytestmark = pytest.mark.gpu

L, BINS = RO.L, RO.BINS
NONE = AC.NONE
NAMES = ("emax", "emin", "njoin", "ejoin", "e2", "start")


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


def run_auto(RM, pcm, cuts=None, device=False, hist=True):
    """(R, (emax, emin, njoin, ejoin, e2, start), gate, hist, nseg) of a fresh meter under AUTO (| HIST)"""
    m = RM.RateMeter(pcm.shape[0], 48000.0, max_write_samples=max(cuts or [pcm.shape[1]]))
    m.gate_enable(auto=True, hist=hist)
    feed(m, pcm, cuts, device)
    R, nseg = m.read()
    *st, g, n2 = m.read_gate_auto()
    h = None
    if hist:
        h, n3 = m.read_gate_hist()
        assert n3 == nseg and h.dtype == np.uint32 and h.shape == (pcm.shape[0], 321)
    four = m.read_gate()
    assert n2 == nseg and all(np.array_equal(a, b) for a, b in zip(four[:4], st[:4])) and np.array_equal(four[4], g)
    m.close()
    return R, st, g, h, nseg


def run_ungated(RM, pcm):
    m = RM.RateMeter(pcm.shape[0], 48000.0, max_write_samples=pcm.shape[1])
    m.write(np.array(pcm))
    R, nseg = m.read()
    m.close()
    return R, nseg


def assert_stats(got, want, where=""):
    assert len(got) == len(want)
    for name, a, b in zip(NAMES, got, want):
        assert a.dtype == np.uint64 and np.array_equal(a, np.asarray(b, dtype=np.uint64)), (where, name, a, b)


def assert_is_oracle(got, o, where):
    """R by the rule; numbers, gates and histogram exactly"""
    R, st, g, h, nseg = got
    assert nseg == o.n
    RC.assert_rule(R, o.R, where)
    assert_stats(st, o.stats(), where)
    assert g.tolist() == o.gate, (where, g, o.gate)
    if h is not None:
        assert np.array_equal(h, o.hist_array()), where
        assert h.sum(axis=1).tolist() == [nseg] * len(g)


def assert_from_start(RM, pcm, got, o, where):
    """every channel's R is bit-identical to an ungated one-channel handle fed its joined segments from `start` on"""
    R = got[0]
    for c in range(pcm.shape[0]):
        assert o.joined[c], (where, c)
        alone, n = run_ungated(RM, AC.joined_only(pcm, c, o.joined[c]))
        assert n == len(o.joined[c]) and np.array_equal(R[c], alone[0]), (where, c, "R is not that of the joined segments from start on")


def test_ones_rows_follow_the_table(RM):
    """Rows of +-1 whose segment energies are chosen integers: 2 * 300 == 3 * 200 exactly, 598 < 600, loud first, a click, small numbers."""
    for idx, pcm in AC.ones_groups():
        o = AO.AutoRateOracle(len(idx), AO.AUTO | AO.HIST)
        o.write(pcm)
        got = run_auto(RM, pcm)
        assert_is_oracle(got, o, f"ones rows {idx}")
        assert_from_start(RM, pcm, got, o, f"ones rows {idx}")
        for c, i in enumerate(idx):
            energies, gates, joined, start = AC.ONES[i]
            assert o.joined[c] == joined and got[1][5][c] == start and got[1][2][c] == len(joined)
            assert gates is None or got[2][c] == gates[-1]
            assert np.array_equal(got[3][c], np.bincount([RM.energy_bin(e) for e in energies], minlength=321))


@pytest.fixture(scope="module")
def mixed_whole(RM):
    """the mixed rows and their tail in one write from host memory"""
    return run_auto(RM, AC.auto_mixed())


def test_mixed_joining_and_restarting_inside_a_workgroup(RM, mixed_whole):
    """7 channels x 8 segments: 0 (quiet first, restarts at 3) beside 1 (loud first, never restarts); 2 (zeros) beside 3 (level); 4 (a
    click: gate 0) beside 5 (restarts at 2); 6 alone in the last workgroup."""
    pcm = AC.auto_mixed()
    o = AO.AutoRateOracle(AC.AMIX_NCH, AO.AUTO | AO.HIST)
    o.write(pcm)
    assert o.joined == AC.AMIX_JOINS and o.start == AC.AMIX_START
    assert_is_oracle(mixed_whole, o, "auto_mixed")
    assert_from_start(RM, pcm, mixed_whole, o, "auto_mixed")
    R, st, g, h, nseg = mixed_whole
    whole, n = run_ungated(RM, pcm)
    assert n == nseg == AC.AMIX_NSEG
    for c in (2, 3, 4):  # never left gate 0: the ungated meter bit for bit, start never set
        assert np.array_equal(R[c], whole[c]) and g[c] == 0 and st[5][c] == NONE and st[2][c] == nseg, c
    assert (R[2] == 0.0).all()


@pytest.mark.parametrize("nch", [1, 5, 67])
def test_level_rows_are_the_ungated_meter(RM, nch):
    """Three segments and a tail of the case rows: no channel leaves gate 0, R equals the ungated kernel's bit for bit."""
    pcm = RC.case_rows(nch, RC.N_PARITY)
    o = AO.AutoRateOracle(nch, AO.AUTO | AO.HIST)
    o.write(pcm)
    got = run_auto(RM, pcm)
    R0, n0 = run_ungated(RM, pcm)
    assert got[4] == n0 == 3
    assert np.array_equal(got[0], R0), "a level row is not the ungated meter"
    assert_is_oracle(got, o, f"level rows, nch={nch}")
    assert got[2].tolist() == [0] * nch and got[1][5].tolist() == [NONE] * nch and got[1][2].tolist() == [3] * nch
    for c in RC.exact_rows(nch):
        assert (got[0][c] == 0.0).all()


def test_cuts_and_input_memory_change_nothing(RM, mixed_whole):
    """The mixed rows and a 100-sample tail in one write and cut as [1, 4095, 4097, 1, 8197, rest], from host memory and from a device
    tensor: four times the same bits, numbers, gates and histogram."""
    pcm = AC.auto_mixed()
    R, st, g, h, nseg = mixed_whole
    for cuts, device in ((AC.AMIX_CUTS, False), (None, True), (AC.AMIX_CUTS, True)):
        R2, st2, g2, h2, n2 = run_auto(RM, pcm, cuts, device)
        assert n2 == nseg == AC.AMIX_NSEG
        assert np.array_equal(R, R2), ("R depends on the cuts or on where the input lies", cuts, device)
        assert_stats(st2, st, f"cuts={cuts} device={device}")
        assert np.array_equal(g, g2) and np.array_equal(h, h2), (cuts, device)


def test_manual_with_histogram_is_the_gated_meter(RM):
    """MANUAL | HIST on the gated tests' mixed rows under their gates: R and the four numbers are bit-identical to today's MANUAL handle
    (k_rate_lines_auto and k_rate_lines_gated agree), the histogram is the oracle's."""
    from jaero_amd import capi

    pcm, gates = GC.mixed()
    res = []
    for hist in (False, True):
        m = RM.RateMeter(GC.MIX_NCH, 48000.0, max_write_samples=pcm.shape[1])
        m.gate_enable(hist=hist)
        m.set_gate(gates)
        feed(m, pcm)
        R, nseg = m.read()
        *st, g, n2 = m.read_gate()
        assert n2 == nseg == GC.MIX_NSEG and g.tolist() == gates
        if hist:
            h, n3 = m.read_gate_hist()
            with pytest.raises(capi.JaeroError) as e:
                m.read_gate_auto()
            assert e.value.code == capi.E_INVAL and "jaero_gate2_read" in str(e.value)
        else:
            with pytest.raises(capi.JaeroError) as e:
                m.read_gate_hist()
            assert e.value.code == capi.E_INVAL and "jaero_gate2_read_hist" in str(e.value)
        m.close()
        res.append((R, st))
    assert np.array_equal(res[0][0], res[1][0]), "the two kernels differ under the same gates"
    assert all(np.array_equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    o = AO.AutoRateOracle(GC.MIX_NCH, AO.MANUAL | AO.HIST)
    o.set_gate(gates)
    o.write(pcm)
    assert o.joined == GC.MIX_JOINS and n3 == GC.MIX_NSEG
    assert np.array_equal(h, o.hist_array())
    RC.assert_rule(res[1][0], o.R, "MANUAL | HIST")


def test_life_cycle(RM):
    """Bad modes and set_gate under AUTO are refused and change nothing; reset under AUTO zeroes the gates and keeps the pending samples;
    AUTO -> MANUAL keeps the device's gates for a pass under them; -> mode 0 is the ungated meter on the rest of the grid."""
    from jaero_amd import capi

    pcm = AC.auto_mixed()
    nch = AC.AMIX_NCH
    m = RM.RateMeter(nch, 48000.0, max_write_samples=4 * L + 50)
    o = AO.AutoRateOracle(nch)
    for call in (m.read_gate_auto, m.read_gate_hist):  # mode 0
        with pytest.raises(capi.JaeroError) as e:
            call()
        assert e.value.code == capi.E_INVAL and "jaero_gate2_read" in str(e.value)
    m.gate_enable(auto=True)
    for mode in (3, 4, 7, 8, -1):
        assert m.lib.jaero_gate2_enable(m.h, mode) == capi.E_INVAL and b"jaero_gate2_enable" in m.lib.jaero_last_error()
    *st, g, n = m.read_gate_auto()
    assert n == 0 and g.tolist() == [0] * nch
    assert_stats(st, AO.AutoRateOracle(nch).stats(), "at enable")
    with pytest.raises(capi.JaeroError) as e:
        m.read_gate_hist()  # AUTO without HIST
    assert e.value.code == capi.E_INVAL
    for x in (m, o):
        x.write(pcm[:, :4 * L + 50])      # segments 0 .. 3; 50 samples pending
    with pytest.raises(capi.JaeroError) as e:
        m.set_gate([7] * nch)
    assert e.value.code == capi.E_INVAL and "jaero_gate_set" in str(e.value)
    R, n = m.read()
    *st, g, n2 = m.read_gate_auto()
    assert n == n2 == o.n == 4 and g.tolist() == o.gate and o.start[0] == 3 and g[0] > 0, "the refused set_gate changed the gates"
    RC.assert_rule(R, o.R, "four segments")
    assert_stats(st, o.stats(), "four segments")
    m.reset()
    o.reset()
    R, n = m.read()
    *st, g, n2 = m.read_gate_auto()
    assert n == n2 == 0 and not R.any() and g.tolist() == [0] * nch
    assert_stats(st, o.stats(), "after reset")
    for x in (m, o):
        x.write(pcm[:, 4 * L + 50:6 * L + 50])  # segments 4 and 5, with the 50 samples that were pending: 0 and 1 since the reset
    R, n = m.read()
    *st, g, n2 = m.read_gate_auto()
    assert n == n2 == o.n == 2 and g.tolist() == o.gate
    RC.assert_rule(R, o.R, "after reset")
    assert_stats(st, o.stats(), "after reset")
    # AUTO -> MANUAL: the device's gates stay, and a pass under them is the gated meter's
    for x in (m, o):
        x.write(pcm[:, 6 * L + 50:7 * L + 50])  # segment 6: the gates the rest runs under
    frozen = o.gate
    assert frozen[0] > 0 and frozen[6] > 0 and frozen[3] == 0
    m.gate_enable()
    *st4, g, n2 = m.read_gate()
    assert n2 == 0 and g.tolist() == frozen and st4[2].tolist() == [0] * nch
    go = GO.GatedRateOracle(nch)
    go.set_gate(frozen)
    m.write(pcm[:, 7 * L + 50:8 * L + 50])      # segment 7 under the frozen gates
    go.write(pcm[:, 7 * L:8 * L])
    R, n = m.read()
    *st4, g, n2 = m.read_gate()
    assert n == n2 == go.n == 1 and g.tolist() == frozen
    RC.assert_rule(R, go.R, "frozen gates")
    assert all(np.array_equal(a, b) for a, b in zip(st4, go.stats()))
    assert 0 < sum(len(j) for j in go.joined) < nch  # some join and some do not
    m.close()
    # -> mode 0: the ungated meter on the rest of the grid
    m = RM.RateMeter(nch, 48000.0, max_write_samples=6 * L + 50)
    m.gate_enable(auto=True, hist=True)
    m.write(np.array(pcm[:, :2 * L + 50]))
    m.gate_enable(False)
    R, n = m.read()
    assert n == 0 and not R.any()
    m.write(np.array(pcm[:, 2 * L + 50:]))
    R, n = m.read()
    m.close()
    fresh, n3 = run_ungated(RM, pcm[:, 2 * L:])
    assert n == n3 == 6 and np.array_equal(R, fresh), "mode 0 is not the ungated meter"


@pytest.mark.parametrize("arrangement", AC.ARRANGEMENTS)
def test_burst_rows_read_their_rate_in_one_pass(RM, arrangement):
    """Three burst rows, one continuous 1200 bps MSK row and one noise row, 256 segments in 4-segment writes under AUTO | HIST, once:
    the rates, joined counts and starts on record.  The click rows then go through the click-proof two-pass flow on the device's own
    histogram.  The margins are asserted on the CPU oracles alone in tests/test_rate_auto_host.py."""
    pcm = AC.burst_rows(arrangement)
    o = AC.burst_auto(arrangement)
    cuts = [GC.BURST_WRITE] * (pcm.shape[1] // GC.BURST_WRITE)
    got = run_auto(RM, pcm, cuts)
    R, st, g, h, nseg = got
    assert nseg == GC.BURST_NSEG
    assert_is_oracle(got, o, f"bursts, {arrangement}")
    rate, audio, score = RM.classify_rates(R, GC.BURST_FS)
    print(arrangement, "scores, dB:\n", np.round(score, 1), "\naudio:", audio, "\njoined:", st[2], "start:", st[5], "gates:", g)
    assert rate.tolist() == AC.AUTO_RATES
    assert st[2].tolist() == AC.AUTO_JOINED[arrangement] and st[5].tolist() == AC.AUTO_START[arrangement]
    if arrangement != "click":
        return
    gates = RM.suggest_gate(*RM.hist_extremes(h))
    assert gates == AC.CLICK_HIST_GATES
    m = RM.RateMeter(5, GC.BURST_FS, max_write_samples=GC.BURST_WRITE)
    m.gate_enable()
    m.set_gate(gates)
    feed(m, pcm, cuts)
    R2, n2 = m.read()
    njoin = m.read_gate()[2]
    m.close()
    want_gates, want_R, want_st = AC.click_two_pass()["hist"]
    assert n2 == GC.BURST_NSEG and want_gates == gates and np.array_equal(njoin, want_st[2])
    RC.assert_rule(R2, want_R, "click rows, second pass under the histogram's gates")
    assert RM.classify_rates(R2, GC.BURST_FS)[0].tolist() == AC.AUTO_RATES


def test_scale_one_launch(RM):
    """33 091 channels x (4096 + 7) samples made on the device, one launch under AUTO | HIST (rows at odd addresses: every row's first
    and last 16-byte word is shared with its neighbours); 16 spread rows against the oracle, every row's numbers and histogram."""
    import torch

    nch, n = 33091, L + 7
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    t = torch.randint(-32768, 32768, (nch, n), device="cuda", dtype=torch.int32, generator=g).to(torch.int16)
    m = RM.RateMeter(nch, 48000.0, max_write_samples=n)
    m.gate_enable(auto=True, hist=True)
    assert m.write_device(t.data_ptr(), n) == 1
    R, nseg = m.read()
    emax, emin, njoin, ejoin, e2, start, gate, n2 = m.read_gate_auto()
    h, n3 = m.read_gate_hist()
    m.close()
    assert nseg == n2 == n3 == 1
    E = (t[:, :L].to(torch.int64) ** 2).sum(dim=1).cpu().numpy().astype(np.uint64)
    assert np.array_equal(emax, E) and np.array_equal(emin, E) and np.array_equal(ejoin, E)
    assert (njoin == 1).all() and not e2.any() and not gate.any() and (start == NONE).all()
    assert (h.sum(axis=1) == 1).all()
    bins = np.array([RM.energy_bin(int(e)) for e in E])
    assert (h[np.arange(nch), bins] == 1).all()
    rows = np.unique(np.concatenate([np.linspace(0, nch - 1, 14).astype(int), [1, nch - 2]]))
    assert len(rows) == 16
    pcm = t[torch.from_numpy(rows).cuda()].cpu().numpy()
    o = RO.RateOracle(len(rows))
    o.write(pcm)
    RC.assert_rule(R[rows], o.R, "scale")
    assert (R > 0.0).any(axis=1).all()
