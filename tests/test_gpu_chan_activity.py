"""GPU (-m gpu): the channeliser's activity (jaero_activity_*; k_chan_psd<SUM, PEAK> and k_chan_level<D, LEVEL, ACT> in
jaero_amd/csrc/k_chan.h) against its definition (tests/chan_activity_oracle.py), and the blind chains it exists for: a capture with a
carrier that is seldom on -> peak-hold spectrum -> centres -> block statistics -> duty and gains, and capture -> burst bank.

Tolerance against the oracle for P, emax and emin: the survey tests' (tests/test_gpu_chan_survey.py) -- |got - want| <= 1e-12 (want +
ref), ref = mean_k(P) or max_c(emax) -- because P[k] and e_{c,p} are single terms of the sums that bound was set for.  `when` and `hist`
are integers and must be equal; every case first asserts on the oracle that no block term lies within 1e-9 (relative) of a bin edge or of
its channel's next largest term, so that a difference in the last bits cannot move either.  Cut independence and the one-block
identities are exact: np.array_equal on the float64."""
import numpy as np
import pytest

import chan_activity_cases as AC
import chan_activity_oracle as AO
import chan_oracle as CO
from chan_cases import AUDIO, CH, FS_OUT

pytestmark = pytest.mark.gpu

N, HP = AO.N, AO.HP
RTOL = 1e-12


def assert_close(got, want, ref, where):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    assert ref > 0 and np.isfinite(got).all(), where
    err = float(np.max(np.abs(got - want) / (want + ref)))
    print(f"{where}: largest |got - want| / (want + ref) = {err:.2e} over {got.size} values")
    assert err <= RTOL, (where, err)


def assert_activity(ch, o, where):
    """every output of the handle against the oracle's"""
    P, nb = ch.read_peak_sums()
    a = ch.read_activity()
    assert nb == o.peak_blocks and np.array_equal(a.n, o.an), (where, nb, a.n, o.an)
    assert_close(P, o.P, float(o.P.mean()), f"peak, {where}")
    has = o.an > 0
    ref = float(o.emax.max())
    assert_close(a.emax[has], o.emax[has], ref, f"emax, {where}")
    assert_close(a.emin[has], o.emin[has], ref, f"emin, {where}")
    assert np.isnan(a.emax[~has]).all() and np.isnan(a.emin[~has]).all()
    assert np.array_equal(a.when, o.when), (where, a.when, o.when)
    assert a.hist.dtype == np.uint32 and np.array_equal(a.hist, o.hist), where
    assert (a.hist.sum(axis=1) == a.n).all()
    return P, a


def same_outputs(x, y):
    (Px, nx, ax), (Py, ny, ay) = x, y
    return (nx == ny and np.array_equal(Px, Py) and np.array_equal(ax.emax, ay.emax, equal_nan=True)
            and np.array_equal(ax.emin, ay.emin, equal_nan=True) and np.array_equal(ax.when, ay.when) and np.array_equal(ax.n, ay.n)
            and np.array_equal(ax.hist, ay.hist))


def outputs(ch):
    P, nb = ch.read_peak_sums()
    return P, nb, ch.read_activity()


# ---------------------------------------------------------------------------------------------- 1. definition
@pytest.mark.parametrize("decim", [16, 32, 64, 128, 256])
def test_activity_equals_definition(CH, decim):
    """19 channels x 7 blocks at every D (M = 1024 .. 64: every instantiation, the largest and the smallest reduction), in writes of 3 and
    4 hops with everything on (the fused launches), on a second handle with the activity alone (the statistics-only and peak-only
    launches).  Channel 0's run of bins wraps at the seam of the spectrum, channel 1 sits on bin 0, channels 2 and 3 share a tune word."""
    iq, chans, taps = AC.definition_case(decim)
    fs_out = FS_OUT[decim]
    x = CO.as_complex(iq)
    o = AO.ChanActivityOracle(decim, chans, taps)
    AC.assert_terms_comparable(o.block_terms(x))  # asserted, never skipped
    assert o.survey(x) == AC.DEF_HOPS
    assert (o.emax > o.emin).all() and o.when[4] in (2, 3, 4) and o.emax[4] > 4 * o.emin[4]  # the gated carrier stands out
    both = CH.Channeliser(decim, chans, taps=taps, max_write_iq=4 * HP, fs_out=fs_out)
    alone = CH.Channeliser(decim, chans, taps=taps, max_write_iq=4 * HP, fs_out=fs_out)
    both.survey_enable()
    for c in (both, alone):
        c.activity_enable()
        c.write(iq[:3 * HP])
        c.write(iq[3 * HP:])
    Pb, ab = assert_activity(both, o, f"D={decim}, survey + activity")
    Pa, aa = assert_activity(alone, o, f"D={decim}, activity alone")
    assert same_outputs((Pb, 7, ab), (Pa, 7, aa)), "the activity depends on whether the survey runs beside it"
    assert np.array_equal(ab.emax[2], ab.emax[3]) and np.array_equal(ab.hist[2], ab.hist[3])  # one tune word: one set of terms
    S, nb = both.read_psd_sums()
    E, n = both.read_level_sums()
    assert nb == 7 and (n == 7).all()
    assert_close(S, o.S, float(o.S.mean()), f"D={decim}, spectrum beside the peak")
    assert_close(E, o.E, float(o.E.max()), f"D={decim}, levels beside the statistics")
    assert (Pb <= S).all() and (Pb >= S / 7).all() and (ab.emin <= E / 7).all() and (E / 7 <= ab.emax).all()
    both.close(); alone.close()


# ---------------------------------------------------------------------------------------------- 2. exact invariants
@pytest.mark.parametrize("decim", [16, 256])
def test_one_block_identities(CH, decim):
    """After one block with everything on: P == S and emax == emin == E bit for bit (the same instructions form the terms), when == 0,
    one count per row of hist."""
    iq, chans, taps = AC.definition_case(decim)
    ch = CH.Channeliser(decim, chans, taps=taps, max_write_iq=HP, fs_out=FS_OUT[decim])
    ch.survey_enable()
    ch.activity_enable()
    assert ch.write(iq[:HP]) == ch.Mo
    P, nb = ch.read_peak_sums()
    S, nbs = ch.read_psd_sums()
    E, n = ch.read_level_sums()
    a = ch.read_activity()
    ch.close()
    assert nb == nbs == 1 and (n == 1).all() and (a.n == 1).all()
    assert np.array_equal(P, S) and P.min() > 0
    assert np.array_equal(a.emax, E) and np.array_equal(a.emin, E) and E.min() > 0
    assert (a.when == 0).all() and (a.hist.sum(axis=1) == 1).all()
    assert np.array_equal(np.argmax(a.hist, axis=1), [AO.act_bin(e) for e in E])


# ---------------------------------------------------------------------------------------------- 3. cut independence
def test_cut_independence_plain_handle(CH):
    """D = 32: the definition case's capture written at once and in the ragged pieces of the survey's tests: all five outputs equal bit
    for bit, and equal the definition."""
    decim = 32
    iq, chans, taps = AC.definition_case(decim)
    iq = np.concatenate([iq, iq[::-1]])[:12 * HP + 77]  # longer than the pieces' sum, with a tail that completes no block
    sizes = [1, 8191, 8193, 3 * 8192 + 5, 0, 8191 - 5, 4 * HP, 2 * HP, 3]
    whole = CH.Channeliser(decim, chans, taps=taps, max_write_iq=len(iq))
    pieces = CH.Channeliser(decim, chans, taps=taps, max_write_iq=4 * HP)
    for c in (whole, pieces):
        c.activity_enable()
    whole.write(iq)
    pos = 0
    for n in sizes + [len(iq) - sum(sizes)]:
        pieces.write(iq[pos:pos + n])
        pos += n
    assert pos == len(iq)
    a, b = outputs(whole), outputs(pieces)
    assert a[1] == 12 and (a[2].n == 12).all()
    assert same_outputs(a, b), "the activity depends on how the writes were cut"
    o = AO.ChanActivityOracle(decim, chans, taps, psd=False, levels=False)
    AC.assert_terms_comparable(o.block_terms(CO.as_complex(iq)))
    o.survey(CO.as_complex(iq))
    assert_activity(pieces, o, "D=32, ragged writes")
    whole.close(); pieces.close()


def test_cut_independence_capture_handle(CH):
    """cu8 at 1.2 MS/s into D = 16 (resampled by 16 / 25): the same capture written at once and in pieces gives all five outputs bit
    for bit -- the activity hangs off the place every kind of handle passes."""
    decim, fs_in = 16, 1200000
    rng = np.random.default_rng(31)
    n = 100000
    raw = rng.integers(96, 160, size=(n, 2)).astype(np.uint8)
    raw[30000:52000] = rng.integers(0, 256, size=(22000, 2)).astype(np.uint8)  # a louder stretch
    _iq, chans, taps = AC.definition_case(decim)
    cap = CH.Capture(fs_in=fs_in, fmt="cu8", taps_per_phase=16)
    whole = CH.Channeliser(decim, chans, taps=taps, max_write_iq=n, capture=cap)
    pieces = CH.Channeliser(decim, chans, taps=taps, max_write_iq=40000, capture=cap)
    for c in (whole, pieces):
        c.survey_enable()
        c.activity_enable()
    whole.write(raw)
    pos = 0
    for k in (1, 8191, 8193, 3 * 8192 + 5, 0, 40000, 7, n):
        pieces.write(raw[pos:pos + k])
        pos += k
    a, b = outputs(whole), outputs(pieces)
    assert a[1] == n * 16 // 25 // HP == 7 and (a[2].n == 7).all() and (a[2].emax > a[2].emin).all()
    assert same_outputs(a, b), "the activity of a capture handle depends on how the writes were cut"
    assert np.array_equal(whole.read_psd_sums()[0], pieces.read_psd_sums()[0]) and np.array_equal(whole.read_level_sums()[0], pieces.read_level_sums()[0])
    whole.close(); pieces.close()


# ---------------------------------------------------------------------------------------------- 4. the product is left alone
def test_activity_leaves_the_product_alone(CH):
    """D = 64, 19 channels, ragged writes, three handles: survey + activity, survey alone, nothing.  PCM is the same bytes on all three, S
    and E the same bits with and without the activity; the survey-only handle counts its launches where it always did and none under
    the activity's slots; on the handle with both, every launch is fused and counted once, under the activity's slots."""
    decim = 64
    iq, chans, taps = AC.definition_case(decim)
    sizes = [1, 8191, 8193, 3 * 8192 + 5, 0, 2 * HP]
    both, survey, plain = (CH.Channeliser(decim, chans, taps=taps, max_write_iq=4 * HP) for _ in range(3))
    both.survey_enable(); both.activity_enable()
    survey.survey_enable()
    for c in (both, survey, plain):
        c.profile_enable(True)
    pos = producing = 0
    for n in sizes:
        nout = both.write(iq[pos:pos + n])
        assert survey.write(iq[pos:pos + n]) == nout and plain.write(iq[pos:pos + n]) == nout
        pos += n
        producing += nout > 0
        pcm = both.read_pcm()
        assert pcm.shape == (len(chans), nout) and pcm.tobytes() == survey.read_pcm().tobytes() == plain.read_pcm().tobytes()
    assert producing == 4
    assert np.array_equal(both.read_psd_sums()[0], survey.read_psd_sums()[0]) and both.read_psd_sums()[1] == survey.read_psd_sums()[1] == 7
    assert np.array_equal(both.read_level_sums()[0], survey.read_level_sums()[0])
    for which in (0, 1):
        assert survey.survey_profile_read(which)[1] == producing and survey.activity_profile_read(which) == (0.0, 0)
        assert plain.survey_profile_read(which) == (0.0, 0) and plain.activity_profile_read(which) == (0.0, 0)
        assert both.activity_profile_read(which)[1] == producing and both.survey_profile_read(which) == (0.0, 0)
        assert all(c.profile_read(which)[1] == producing for c in (both, survey, plain))
    for c in (both, survey, plain):
        c.close()


# ---------------------------------------------------------------------------------------------- 5. control plane
def test_retune_resets_enable(CH):
    from jaero_amd import capi

    decim, fs = 32, 48000.0 * 32
    iq, chans, taps = AC.definition_case(decim)
    chans = chans[:5]
    x = CO.as_complex(iq)
    ch = CH.Channeliser(decim, chans, taps=taps, max_write_iq=4 * HP)
    o = AO.ChanActivityOracle(decim, chans, taps)
    ch.survey_enable(); ch.activity_enable()

    def step(a, b):
        ch.write(iq[a * HP:b * HP]); o.survey(x[a * HP:b * HP])

    step(0, 2)
    # retune: a moved tune word restarts that channel's statistics with its level; audio- and gain-only retunes keep everything
    moved = (CH.tune_word(-0.2 * fs, fs), AUDIO, 1.0)
    ch.retune(1, *moved); o.retune(1, *moved)
    ch.retune(0, chans[0][0], AUDIO + 77, 0.25); o.retune(0, chans[0][0], AUDIO + 77, 0.25)
    a = ch.read_activity()
    assert a.n.tolist() == [2, 0, 2, 2, 2] and np.isnan(a.emax[1]) and np.isnan(a.emin[1]) and a.when[1] == -1 and not a.hist[1].any()
    assert ch.read_level_sums()[1].tolist() == [2, 0, 2, 2, 2]
    step(2, 4)
    assert_activity(ch, o, "behind retune")
    assert o.an.tolist() == [4, 2, 4, 4, 4] and o.when[1] >= 2
    # retune_all: channel 3 moves, channel 2 changes its gain only
    allnew = [tuple(c) for c in o.channels]
    allnew[3] = (CH.tune_word(0.3 * fs, fs), AUDIO, 1.0)
    allnew[2] = (allnew[2][0], allnew[2][1], 2.5)
    ch.retune_all(allnew); o.retune_all(allnew)
    step(4, 5)
    assert_activity(ch, o, "behind retune_all")
    assert o.an.tolist() == [5, 3, 5, 1, 5] and o.when[3] == 4
    E, n = ch.read_level_sums()
    assert n.tolist() == [5, 3, 5, 1, 5]
    # the two resets are independent
    S5 = ch.read_psd_sums()
    ch.activity_reset(); o.activity_reset()
    P, nb = ch.read_peak_sums()
    a = ch.read_activity()
    assert nb == 0 and not P.any() and not a.n.any() and not a.hist.any() and (a.when == -1).all() and np.isnan(a.emax).all()
    assert np.isnan(ch.read_peak_psd()[0]).all()
    with pytest.raises(ValueError):
        ch.suggest_gains(peak=True)  # no block yet: no gain to suggest
    assert ch.read_psd_sums()[1] == 5 and np.array_equal(ch.read_psd_sums()[0], S5[0]) and np.array_equal(ch.read_level_sums()[0], E)
    step(5, 6)
    assert_activity(ch, o, "behind activity_reset")
    assert (o.when == 5).all() and (o.an == 1).all()  # block indices count from create, not from the reset
    kept = outputs(ch)
    ch.survey_reset(); o.reset()
    assert ch.read_psd_sums()[1] == 0 and not ch.read_level_sums()[0].any()
    assert same_outputs(outputs(ch), kept)
    # a read of a part that is off; disabling and enabling again clears
    ch.activity_enable(peak=True, blocks=False)
    with pytest.raises(capi.JaeroError) as e:
        ch.read_activity()
    assert e.value.code == capi.E_INVAL
    assert ch.read_peak_sums()[1] == 0
    ch.activity_enable(peak=False, blocks=True)
    with pytest.raises(capi.JaeroError) as e:
        ch.read_peak_sums()
    assert e.value.code == capi.E_INVAL
    assert not ch.read_activity().n.any()
    ch.activity_enable(peak=False, blocks=False)
    for read in (ch.read_peak_sums, ch.read_activity):
        with pytest.raises(capi.JaeroError) as e:
            read()
        assert e.value.code == capi.E_INVAL
    ch.activity_enable()
    o = AO.ChanActivityOracle(decim, [tuple(c) for c in allnew], taps, psd=False, levels=False)
    o.pblk = 6
    o.sbuf = x[5 * HP:6 * HP].copy()  # the oracle's history: the hop before
    step(6, 7)
    assert_activity(ch, o, "enabled again")
    assert (o.when == 6).all()
    assert ch.L.jaero_activity_enable(ch.h, 4) == capi.E_INVAL and ch.read_activity().n.tolist() == [1] * 5  # refused: nothing changes
    ch.close()


# ---------------------------------------------------------------------------------------------- 6. blind burst discovery
def test_blind_burst_discovery(CH):
    """The discovery capture (tests/chan_activity_cases.py: a carrier that is always on, one that is on in hops 30 .. 32 of 64) through a
    real handle of three placeholder channels, nothing given but the carriers' width: pass 1 read_peak_psd -> find_carriers (both
    carriers, within 250 Hz) -> retune_all; pass 2 read_activity -> duty_cycle (4 / 64 for the burst channel, 0 for the other two) and
    suggest_gains(peak=True) -> retune_all; pass 3: the int16 RMS of the burst channel over the two blocks that lie wholly inside the
    burst is within 10 % of the target.  (The block term covers the whole circular block, the output its second half, and emax is the
    larger of the two blocks' terms.)  The same chain on the oracle on the CPU gives 0.984 of the target for the burst channel (0.969
    and 0.999 for the two blocks), so the issue's 10 % stands."""
    target = 0.1 * 32768
    iq = AC.discovery_capture()
    fs, hops = AC.DISC_FS, AC.DISC_HOPS
    ch = CH.Channeliser(AC.DISC_DECIM, [(0, AUDIO, 1.0)] * 3, max_write_iq=hops * HP)
    ch.activity_enable(peak=True, blocks=False)
    assert ch.write(iq) == hops * ch.Mo
    peak, nb = ch.read_peak_psd()
    assert nb == hops
    found = CH.find_carriers(peak, fs, 10500.0)
    print("found centres:", np.round(found, 1))
    assert len(found) == 2 and abs(found[0] - AC.DISC_BURST_HZ) <= 250.0 and abs(found[1] - AC.DISC_ON_HZ) <= 250.0
    centres = list(found) + [AC.DISC_EMPTY_HZ]
    ch.retune_all(AC.discovery_channels(centres))
    ch.activity_enable(peak=False, blocks=True)
    ch.survey_enable(psd=False, levels=True)
    assert ch.write(iq) == hops * ch.Mo
    a = ch.read_activity()
    level, cnt = ch.read_levels()
    duty = CH.duty_cycle(a.hist)
    ratio = a.emax / level
    print("duty:", duty, " emax / level:", np.round(ratio, 3), " when:", a.when)
    assert (a.n == hops).all() and (cnt == hops).all()
    assert duty[0] == 4 / 64 and duty[1] == 0.0 and duty[2] == 0.0
    assert ratio[0] > 4.0 and ratio[1] < 1.5 and ratio[2] < 1.5
    assert a.when[0] in (hops + 31, hops + 32)  # absolute, counted from create: the second pass
    o = AO.ChanActivityOracle(AC.DISC_DECIM, AC.discovery_channels(centres), CH.design_taps(AC.DISC_DECIM), psd=False, peak=False)
    o.survey(CO.as_complex(iq)); o.activity_reset(); o.reset()
    o.survey(CO.as_complex(iq))
    AC.assert_terms_comparable(o.block_terms(CO.as_complex(iq)))
    assert np.array_equal(a.hist, o.hist) and np.array_equal(a.when, o.when)
    gains = ch.suggest_gains(target, peak=True)
    assert np.array_equal(gains, target / np.sqrt(a.emax / 2.0))
    mean_gains = ch.suggest_gains(target)
    assert gains[0] < 0.5 * mean_gains[0]  # the mean level would set the burst channel's gain more than twice too high
    ch.retune_all(AC.discovery_channels(centres, gains))
    assert ch.write(iq) == hops * ch.Mo
    pcm = ch.read_pcm()
    ch.close()
    burst = pcm[0, 31 * ch.Mo:33 * ch.Mo].astype(float)
    rms = float(np.sqrt(np.mean(burst ** 2)))
    print(f"burst channel: gain {gains[0]:.3f}, RMS over the burst's blocks {rms:.0f} LSB = {rms / target:.3f} of the target")
    assert abs(rms / target - 1.0) <= 0.10


# ---------------------------------------------------------------------------------------------- 7. capture -> burst bank
def test_capture_to_burst_bank(CH, oracle_mod):
    """The first capture in the tree that is fed to a burst bank.  `chan_activity_cases.burst_capture` (two 10.5 kbps OQPSK bursts, one per
    second, lifted to D = 16 at -181.25 kHz over white noise) through one placeholder channel, nothing given but the carrier's width: pass
    1 read_peak_psd -> find_carriers -> retune_all; pass 2 read_activity -> suggest_gains(peak=True) -> retune_all; pass 3 is fed to a
    JAERO_KIND_BURST_OQPSK bank in writes of 8 hops (4096 samples a channel).  The device's PCM is the numpy definition's for the found
    centre and gain (chan_cases.assert_rule), and jaero_read_events shows the JAERO_EV_SIGNAL rows of oracle.run_burst on that PCM: signal
    on in each second.  On the CPU the oracle reports both bursts on this PCM (signal on at samples 32 216 and 80 704, off at 68 541 between
    them; the found centre was 341 Hz off -- the peak-hold spectrum of a burst is dominated by its carrier and tone preamble -- which the
    demodulator's own acquisition takes up: it reports 7658 Hz for the 8 kHz audio carrier).  With the noise 14 dB lower the oracle
    missed the first burst; that one adjustment of the capture is recorded in tests/chan_activity_cases.py."""
    from chan_cases import assert_rule
    from jaero_amd import capi
    from jaero_amd import demodulator as B

    O = oracle_mod
    iq = AC.burst_capture()
    decim, fs, step = AC.BURST_DECIM, 48000.0 * AC.BURST_DECIM, 8 * HP
    target = 0.1 * 32768
    ch = CH.Channeliser(decim, [(0, AUDIO, 1.0)], max_write_iq=step)

    def one_pass(sink=None):
        out = []
        for s in range(0, len(iq), step):
            if sink is None:
                ch.write(iq[s:s + step])
            else:
                assert ch.feed(sink, iq[s:s + step]) == min(step, len(iq) - s) // HP * ch.Mo
                out.append(ch.read_pcm())
        return out

    ch.activity_enable(peak=True, blocks=False)
    one_pass()
    peak, nb = ch.read_peak_psd()
    assert nb == len(iq) // HP
    found = CH.find_carriers(peak, fs, 10500.0)
    print("found centre:", np.round(found, 1))
    # a burst's peak-hold spectrum is led by its preamble's three lines, the carrier and the tones fb / 4 either side of it: the centroid
    # lies between the tones, and the burst demodulator's own estimate (over its locking bandwidth of 10.5 kHz) takes up what is left
    assert len(found) == 1 and abs(found[0] - AC.BURST_HZ) <= 10500.0 / 4
    tune = CH.tune_word(found[0], fs)
    ch.retune_all([(tune, AUDIO, 1.0)])
    ch.activity_enable(peak=False, blocks=True)
    one_pass()
    a = ch.read_activity()
    duty = CH.duty_cycle(a.hist)
    gain = float(ch.suggest_gains(target, peak=True)[0])
    print(f"duty {duty[0]:.3f}, gain {gain:.4f}, strongest block {a.when[0]} (absolute)")
    assert 0.25 < duty[0] < 0.45  # two bursts of 0.33 s in 2 s, seen through two-hop blocks
    ch.retune_all([(tune, AUDIO, gain)])
    ch.activity_enable(peak=False, blocks=False)
    bank = B.DemodulatorBank(B.BurstOqpskSettings(), 1, max_write_samples=9 * ch.Mo, softbit_capacity=20000)
    pcm = np.concatenate(one_pass(bank), axis=1)
    ev = bank.read_events(0)
    bank.close(); ch.close()
    # the numpy definition for the same centre and gain, behind the same history (two passes)
    o = CO.ChanOracle(decim, [(tune, AUDIO, gain)], CH.design_taps(decim))
    x = CO.as_complex(iq)
    o.write(x); o.write(x)
    ystar = o.write(x)
    assert pcm.shape == ystar.shape == (1, len(iq) // HP * ch.Mo)
    assert_rule(pcm[0], ystar[0], gain, "burst channel")
    ref = O.run_burst(O.burst_oqpsk_settings(), CO.to_int16(ystar[0]), chunk=8 * ch.Mo)
    want = ref["events"][ref["events"][:, 1] == capi.EV_SIGNAL]
    got = ev[ev[:, 1] == capi.EV_SIGNAL]
    print("JAERO_EV_SIGNAL rows:", got[:, [0, 2]].tolist())
    on = want[want[:, 2] == 1.0][:, 0]
    assert ((on >= 20000) & (on < 48000)).any() and ((on >= 68000) & (on < 96000)).any(), "the oracle does not report both bursts"
    assert np.array_equal(got, want)
