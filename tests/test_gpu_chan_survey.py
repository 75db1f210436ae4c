"""GPU (-m gpu): the channeliser survey (jaero_survey_*, k_chan_psd / k_chan_level in jaero_amd/csrc/k_chan.h) against its definition
(tests/chan_survey_oracle.py), and the blind chain it exists for: capture -> surveyed centres and gains -> demodulator bank.

Tolerance against the oracle, both quantities (`assert_close`): |got - want| <= 1e-12 (want + ref), ref = mean_k(want) for the spectrum and
max_c(want) for the levels.  numpy against a long-double direct DFT differs by <= 3.8e-16 in that measure; the 2 600 x margin is for the
other summation orders of wg_fft14_e32 and of the q reduction.  Every level test holds a strong channel, so that ref means something.
Cut independence is exact: np.array_equal on the float64."""
import numpy as np
import pytest

import chan_oracle as CO
import chan_survey_oracle as SO
from chan_cases import AUDIO, CH, CHAIN_CENTRES, FS_OUT, channel_set, pchannel_chain_capture, synthetic_capture, white_full_scale
from conftest import assert_soft_bytes

pytestmark = pytest.mark.gpu

N, HP = SO.N, SO.HP
RTOL = 1e-12


def assert_close(got, want, ref, where):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    assert ref > 0 and np.isfinite(got).all(), where
    err = float(np.max(np.abs(got - want) / (want + ref)))
    print(f"{where}: largest |got - want| / (want + ref) = {err:.2e} over {got.size} values")
    assert err <= RTOL, (where, err)


def tone(nhops, k, amp_i=20000.0, amp_q=12000.0):
    """int16 I/Q of a tone on bin k of the N-point grid (k = 0: a constant)"""
    n = np.arange(nhops * HP)
    z = (amp_i + 1j * amp_q) * np.exp(2j * np.pi * ((k * n) % N) / N)
    return np.stack([np.rint(z.real), np.rint(z.imag)], axis=1).astype(np.int16)


# ---------------------------------------------------------------------------------------------- 1. spectrum
@pytest.mark.parametrize("case", ["white", "capture", "tone0", "toneN-1", "one_hop", "nblk_max_hops"])
def test_spectrum_equals_definition(CH, case):
    """One channel at D = 64, all 16 384 bins.  The tones sit on bins 0 and N - 1: their Hann neighbours are (k +- 1) mod N across the
    ends.  'nblk_max_hops': a write of max_write_iq behind Hp - 1 waiting samples completes max_write_iq / Hp + 1 blocks in one launch."""
    decim, chans, taps = 64, [(12345678, AUDIO, 1.0)], np.ones(1)
    if case == "white":
        iq, cuts = white_full_scale(3 * HP, 11), [3 * HP]
    elif case == "capture":
        iq, cuts = synthetic_capture(decim, 3, 264)[0], [3 * HP]
    elif case == "tone0":
        iq, cuts = tone(3, 0), [3 * HP]
    elif case == "toneN-1":
        iq, cuts = tone(3, N - 1), [3 * HP]
    elif case == "one_hop":
        iq, cuts = white_full_scale(HP, 12), [HP]
    else:
        iq, cuts = white_full_scale(4 * HP, 13), [HP - 1, 3 * HP + 1]
    ch = CH.Channeliser(decim, chans, taps=taps, max_write_iq=max(cuts))
    ch.survey_enable(psd=True, levels=False)
    ch.profile_enable(True)
    pos = 0
    for n in cuts:
        ch.write(iq[pos:pos + n])
        pos += n
    S, nblocks = ch.read_psd_sums()
    psd, nb2 = ch.read_psd()
    launches = ch.survey_profile_read(0)[1]
    ch.close()
    o = SO.ChanSurveyOracle(decim, chans, taps, levels=False)
    o.survey(CO.as_complex(iq))
    assert nblocks == nb2 == o.nblocks == len(iq) // HP
    assert launches == 1  # all the blocks of the one write that completed any
    assert_close(S, o.S, float(o.S.mean()), f"spectrum, {case}")
    assert np.array_equal(psd, SO.normalise_psd(S, nblocks))
    if case.startswith("tone"):
        k = 0 if case == "tone0" else N - 1
        assert sorted(np.argsort(S)[-3:]) == sorted([(k - 1) % N, k, (k + 1) % N])  # the Hann main lobe, across the ends


# ---------------------------------------------------------------------------------------------- 2. levels
@pytest.mark.parametrize("decim", [16, 32, 64, 128, 256])
@pytest.mark.parametrize("ntaps", [1, 2049, 8193])
@pytest.mark.parametrize("source", ["white", "capture"])
def test_levels_equal_definition(CH, decim, ntaps, source):
    """Every D x taps of 1 / 2049 / 8193 entries x (white full-scale I/Q, a synthetic capture whose strongest carrier two of the channels
    sit on) x the twelve-channel set: after a write of one hop, and on a second handle after one write of three hops."""
    fs_out = FS_OUT[decim]
    nhops = 3
    if source == "white":
        iq, strong = white_full_scale(nhops * HP, 300 + decim), 54321.0
    else:
        iq, centres = synthetic_capture(decim, nhops, 400 + decim)
        strong = centres[2]
    taps = np.ones(1) if ntaps == 1 else CH.design_taps(decim, cutoff_hz=fs_out * 5 / 12, ntaps=ntaps, beta=8.0 if ntaps == 2049 else 16.0,
                                                         fs_out=fs_out)
    chans = [tuple(c) for c in channel_set(CH, decim, strong, 0.1)]
    x = CO.as_complex(iq)
    for hops in (1, 3):
        ch = CH.Channeliser(decim, chans, taps=taps, max_write_iq=hops * HP, fs_out=fs_out)
        ch.survey_enable(psd=False, levels=True)
        assert ch.write(iq[:hops * HP]) == hops * ch.Mo
        E, n = ch.read_level_sums()
        level, n2 = ch.read_levels()
        ch.close()
        o = SO.ChanSurveyOracle(decim, chans, taps, psd=False)
        o.survey(x[:hops * HP])
        assert np.array_equal(n, o.n) and np.array_equal(n2, o.n) and (n == hops).all()
        assert_close(E, o.E, float(o.E.max()), f"levels D={decim} L={ntaps} {source} {hops} hop(s)")
        assert np.array_equal(level, E / n)
        if source == "capture":
            assert o.E[2] == o.E[3] and o.E[2] > 4 * o.E.min()  # the channels on the strong carrier stand out


# ---------------------------------------------------------------------------------------------- 3. cut independence
@pytest.mark.parametrize("nch,decim", [(1, 16), (7, 32), (64, 64), (67, 32), (1, 128), (7, 256), (64, 256), (67, 128)])
def test_cut_independence(CH, nch, decim):
    """tests/test_gpu_chan.py's ragged write sizes against one write per hop: both sums equal bit for bit, and equal the definition.
    Channel counts 1, 7, 64, 67: the level kernel's last workgroup has spare groups at all but 64."""
    rng = np.random.default_rng(nch)
    fs_out = FS_OUT[decim]
    fs = fs_out * decim
    chans = [(CH.tune_word(float(rng.uniform(-fs / 2, fs / 2)), fs), AUDIO, 1.0) for _ in range(nch)]
    mw = 4 * HP
    sizes = [1, 8191, 8193, 3 * 8192 + 5, mw, 0, 8191 - 5, 2 * HP, 3]
    total = sum(sizes)
    iq = rng.integers(-32768, 32768, size=(total, 2)).astype(np.int16)
    taps = CH.design_taps(decim, ntaps=2049, beta=10.0, fs_out=fs_out)
    ragged = CH.Channeliser(decim, chans, taps=taps, max_write_iq=mw, fs_out=fs_out)
    hop = CH.Channeliser(decim, chans, taps=taps, max_write_iq=HP, fs_out=fs_out)
    for c in (ragged, hop):
        c.survey_enable()
    pos = 0
    for n in sizes:
        ragged.write(iq[pos:pos + n])
        pos += n
    for k in range(total // HP):
        hop.write(iq[k * HP:(k + 1) * HP])
    (S, nb), (E, n) = ragged.read_psd_sums(), ragged.read_level_sums()
    (S1, nb1), (E1, n1) = hop.read_psd_sums(), hop.read_level_sums()
    ragged.close(); hop.close()
    assert nb == nb1 == total // HP == 12 and np.array_equal(n, n1) and (n == 12).all()
    assert np.array_equal(S, S1), "the spectrum depends on how the writes were cut"
    assert np.array_equal(E, E1), "the levels depend on how the writes were cut"
    o = SO.ChanSurveyOracle(decim, chans, taps)
    o.survey(CO.as_complex(iq))
    assert_close(S, o.S, float(o.S.mean()), f"spectrum, ragged, {nch} channels D={decim}")
    assert_close(E, o.E, float(o.E.max()), f"levels, ragged, {nch} channels D={decim}")


# ---------------------------------------------------------------------------------------------- 4. retune, retune_all, reset
def test_retune_retune_all_reset(CH):
    """Three handles over the same 8 hops: `ch` gets every call below, `same` every call but the refused retune_all, `plain` none."""
    from jaero_amd import capi

    decim, fs = 32, 48000.0 * 32
    iq = white_full_scale(8 * HP, 7)
    x = CO.as_complex(iq)
    taps = CH.design_taps(decim, cutoff_hz=20000.0)
    chans = [(CH.tune_word(-50000.0, fs), AUDIO, 1.0), (CH.tune_word(123456.7, fs), AUDIO, 1.0), (CH.tune_word(123460.0, fs), AUDIO, 0.5)]
    ch, same, plain = (CH.Channeliser(decim, chans, taps=taps, max_write_iq=4 * HP) for _ in range(3))
    o = SO.ChanSurveyOracle(decim, chans, taps)
    for c in (ch, same, plain):
        c.survey_enable()

    def step(a, b):
        for c in (ch, same, plain):
            c.write(iq[a:b])
        o.survey(x[a:b])

    def retune(k, *words):
        ch.retune(k, *words); same.retune(k, *words); o.retune(k, *words)

    def same_as_oracle(where):
        E, n = ch.read_level_sums()
        assert np.array_equal(n, o.n), (where, n, o.n)
        assert_close(E, o.E, float(o.E.max()), where)
        return E, n

    cut = 3 * HP + 100
    step(0, cut)
    # a tune word changes: that channel starts again with the next write; audio- and gain-only retunes restart nothing
    retune(1, CH.tune_word(-400000.3, fs), CH.tune_word(5000.0, 48000.0), 0.25)
    retune(0, chans[0][0], CH.tune_word(3000.0, 48000.0), 0.5)
    retune(2, chans[2][0], chans[2][1], 2.0)
    E, n = ch.read_level_sums()
    assert list(n) == [3, 0, 3] and E[1] == 0.0 and np.isnan(ch.read_levels()[0][1])
    step(cut, 6 * HP)
    E, n = same_as_oracle("levels behind three retunes")
    Ep, npl = plain.read_level_sums()
    assert list(n) == [6, 3, 6] and list(npl) == [6, 6, 6]
    assert E[0] == Ep[0] and E[2] == Ep[2] and E[1] != Ep[1]  # the neighbours are the unretuned twin's, bit for bit
    # retune_all with one bad gain changes nothing: not the words the synthesis uses, not the sums, not the counts
    bad = [(CH.tune_word(1000.0, fs), AUDIO, 1.0), (CH.tune_word(2000.0, fs), AUDIO, 1.0), (CH.tune_word(3000.0, fs), AUDIO, 0.0)]
    with pytest.raises(capi.JaeroError) as e:
        ch.retune_all(bad)
    assert e.value.code == capi.E_INVAL
    with pytest.raises(ValueError):
        ch.retune_all(bad[:2])
    step(6 * HP, 7 * HP)
    E, n = same_as_oracle("levels behind a refused retune_all")
    assert list(n) == [7, 4, 7]
    assert np.array_equal(E, same.read_level_sums()[0])
    pcm = ch.read_pcm()
    assert pcm.tobytes() == same.read_pcm().tobytes() and pcm.astype(float).std(axis=1).min() > 100.0
    # retune_all: channel 2 moves, channel 0 changes its gain only, channel 1 stays
    allnew = [(o.channels[0][0], o.channels[0][1], 3.0), tuple(o.channels[1]), (CH.tune_word(250000.0, fs), AUDIO, 1.0)]
    ch.retune_all(allnew); o.retune_all(allnew)
    for k in range(3):
        same.retune(k, *allnew[k])  # one channel at a time: the same words, the same restarts
    step(7 * HP, 8 * HP)
    E, n = same_as_oracle("levels behind retune_all")
    assert list(n) == [8, 5, 1]
    Es, ns = same.read_level_sums()
    assert np.array_equal(E, Es) and np.array_equal(n, ns)
    pcm = ch.read_pcm()
    assert pcm.tobytes() == same.read_pcm().tobytes() and pcm.tobytes() != plain.read_pcm().tobytes()
    S, nb = ch.read_psd_sums()
    assert nb == 8
    assert_close(S, o.S, float(o.S.mean()), "spectrum across the retunes")
    assert np.array_equal(S, plain.read_psd_sums()[0])  # no retune touches the spectrum
    # reset
    ch.survey_reset()
    S, nb = ch.read_psd_sums()
    E, n = ch.read_level_sums()
    assert nb == 0 and not S.any() and not E.any() and not n.any()
    assert np.isnan(ch.read_psd()[0]).all() and np.isnan(ch.read_levels()[0]).all()
    with pytest.raises(ValueError):
        ch.suggest_gains()  # no block yet: no gain to suggest
    assert plain.read_psd_sums()[1] == 8  # another handle's survey is its own
    # a read of a part that is not enabled
    ch.survey_enable(psd=True, levels=False)
    with pytest.raises(capi.JaeroError) as e:
        ch.read_levels()
    assert e.value.code == capi.E_INVAL
    ch.survey_enable(psd=False, levels=True)
    with pytest.raises(capi.JaeroError) as e:
        ch.read_psd()
    assert e.value.code == capi.E_INVAL
    assert ch.read_level_sums()[1].tolist() == [0, 0, 0]
    ch.survey_enable(psd=False, levels=False)
    for read in (ch.read_psd, ch.read_levels):
        with pytest.raises(capi.JaeroError) as e:
            read()
        assert e.value.code == capi.E_INVAL
    for c in (ch, same, plain):
        c.close()


# ---------------------------------------------------------------------------------------------- 5. the product is left alone
def test_survey_leaves_the_product_alone(CH):
    """D = 32, 67 channels, ragged writes: read_pcm with the survey on is byte for byte a twin's with it off; off, the survey kernels are
    never launched and the channeliser's own profile counts stay one launch per write that completed a block."""
    nch, decim = 67, 32
    rng = np.random.default_rng(5)
    fs = 48000.0 * decim
    chans = [(CH.tune_word(float(rng.uniform(-fs / 2, fs / 2)), fs), AUDIO, 1.0) for _ in range(nch)]
    mw = 4 * HP
    sizes = [1, 8191, 8193, 3 * 8192 + 5, mw, 0, 8191 - 5, 2 * HP, 3]
    iq = rng.integers(-32768, 32768, size=(sum(sizes), 2)).astype(np.int16)
    taps = CH.design_taps(decim, ntaps=2049, beta=10.0)
    on = CH.Channeliser(decim, chans, taps=taps, max_write_iq=mw)
    off = CH.Channeliser(decim, chans, taps=taps, max_write_iq=mw)
    on.survey_enable()
    for c in (on, off):
        c.profile_enable(True)
    pos, producing = 0, 0
    for n in sizes:
        nout = on.write(iq[pos:pos + n])
        assert off.write(iq[pos:pos + n]) == nout
        pos += n
        producing += nout > 0
        a, b = on.read_pcm(), off.read_pcm()
        assert a.shape == (nch, nout) and a.tobytes() == b.tobytes()
    assert producing == 6
    for which in (0, 1):
        assert off.survey_profile_read(which) == (0.0, 0)
        assert on.survey_profile_read(which)[1] == producing
        assert off.profile_read(which)[1] == producing and on.profile_read(which)[1] == producing
    on.close(); off.close()


# ---------------------------------------------------------------------------------------------- 6. scale
@pytest.mark.parametrize("decim", [256, 32])
def test_scale_33091_channels(CH, decim):
    """33 091 channels x 16 hops in one write: the levels of 16 spread channels and the whole spectrum against the definition, one launch
    of each survey kernel."""
    fs_out, nch, nhops = FS_OUT[decim], 33091, 16
    rng = np.random.default_rng(33091)
    tune = rng.integers(0, 1 << 32, size=nch, dtype=np.uint64)
    chans = [(int(t), AUDIO, 1.0) for t in tune]
    iq = rng.integers(-32768, 32768, size=(nhops * HP, 2)).astype(np.int16)
    ch = CH.Channeliser(decim, chans, max_write_iq=nhops * HP, fs_out=fs_out)
    ch.survey_enable()
    ch.profile_enable(True)
    assert ch.write(iq) == nhops * ch.Mo
    E, n = ch.read_level_sums()
    S, nb = ch.read_psd_sums()
    print("k_chan_synth ms, launches:", ch.profile_read(1), " k_chan_psd:", ch.survey_profile_read(0), " k_chan_level:", ch.survey_profile_read(1))
    assert ch.survey_profile_read(0)[1] == 1 and ch.survey_profile_read(1)[1] == 1
    ch.close()
    assert nb == nhops and (n == nhops).all() and np.isfinite(E).all() and E.min() > 0
    pick = sorted({0, 1, 15, 16, nch - 1, nch - 2} | set(int(v) for v in rng.integers(0, nch, size=10)))
    assert len(pick) == 16
    o = SO.ChanSurveyOracle(decim, [chans[c] for c in pick], CH.design_taps(decim, fs_out=fs_out))
    o.survey(CO.as_complex(iq))
    assert_close(E[pick], o.E, float(o.E.max()), f"levels of 16 of {nch} channels, D={decim}")
    assert_close(S, o.S, float(o.S.mean()), f"spectrum, D={decim}")


# ---------------------------------------------------------------------------------------------- 7. the blind chain
def test_blind_capture_to_signal_units(CH, oracle_mod):
    """Nothing about the capture is given to the chain but the carriers' width.  Four placeholder channels (tune 0, gain 1) survey the
    first 16 hops for the spectrum; find_carriers gives the centres, retune_all sets them at gain 1; the next 8 hops are surveyed for
    the levels, retune_all applies suggest_gains(); the rest is fed to a DemodulatorBank -> AeroLBank.write_from_bank on the device.
    The found centres are within 250 Hz, every channel's PCM RMS within 0.08 .. 0.13 of full scale, a second bank on the same device
    PCM gives the oracle demodulator's soft bytes on the PCM read back, and every channel's CRC-clean signal units are a contiguous
    in-order run of the transmitted ones.  The same chain in numpy + oracle on the CPU gives 78, 78, 78 and 51 of them, and so
    does the device; the floors only keep the check from passing empty: two whole frames (52) where the CPU run has them, one (26) for
    the fourth channel, whose CPU count of 51 is one short of two."""
    from jaero_amd import capi
    from jaero_amd import demodulator as B

    O = oracle_mod
    pays, iq, _ = pchannel_chain_capture()
    decim, fb, nch = 16, 10500, 4
    fs = 48000.0 * decim
    hops = 40
    ch = CH.Channeliser(decim, [(0, AUDIO, 1.0)] * nch, max_write_iq=hops * HP)
    ch.survey_enable(psd=True, levels=False)
    assert ch.write(iq[:16 * HP]) == 16 * ch.Mo
    psd, nb = ch.read_psd()
    assert nb == 16
    found = CH.find_carriers(psd, fs, 10500.0)
    print("found centres:", np.round(found, 1))
    assert len(found) == nch
    errs = np.array(found) - np.array(sorted(CHAIN_CENTRES))
    print("centre errors, Hz:", np.round(errs, 1))
    assert np.all(np.abs(errs) <= 250.0)
    ch.retune_all([(CH.tune_word(f, fs), AUDIO, 1.0) for f in found])
    ch.survey_enable(psd=False, levels=True)
    assert ch.write(iq[16 * HP:24 * HP]) == 8 * ch.Mo
    level, cnt = ch.read_levels()
    assert (cnt == 8).all()
    gains = ch.suggest_gains()
    assert np.array_equal(gains, 0.1 * 32768 / np.sqrt(level / 2.0)) and np.isfinite(gains).all()
    print("suggested gains:", np.round(gains, 3))
    ch.retune_all([(CH.tune_word(f, fs), AUDIO, float(g)) for f, g in zip(found, gains)])
    ch.survey_enable(psd=False, levels=False)

    mws = (hops + 1) * ch.Mo
    demod = B.DemodulatorBank(B.OqpskSettings(), nch, max_write_samples=mws, softbit_capacity=8192)
    demod2 = B.DemodulatorBank(B.OqpskSettings(), nch, max_write_samples=mws, softbit_capacity=1 << 16)
    aerol = B.AeroLBank(nch, fb, max_softbits_per_write=8192, su_capacity=26 * 8 + 8)
    rest = iq[24 * HP:]
    pcm, sizes = [], []
    for s in range(0, len(rest), hops * HP):
        nout = ch.feed(demod, rest[s:s + hops * HP])
        assert nout == (min(len(rest), s + hops * HP) - s) // HP * ch.Mo
        aerol.write_from_bank(demod, 8192)
        ptr, n = ch.pcm_view()
        assert n == nout
        capi.check(demod2.L.jaero_write(demod2.h, ptr, n, capi.PCM_CHANNEL_MAJOR, 1, None))
        pcm.append(ch.read_pcm())
        sizes.append(nout)
    pcm = np.concatenate(pcm, axis=1)
    assert pcm.shape == (nch, len(rest) // HP * ch.Mo)
    for c in range(nch):
        rms = pcm[c].astype(float).std()
        print(f"channel {c}: gain {gains[c]:.3f}, PCM rms {rms:.0f} LSB = {rms / 32768:.4f} of full scale")
        assert 0.08 * 32768 < rms < 0.13 * 32768
        sus = aerol.read_sus(c)
        good = [bytes(r[2:12].astype(np.uint8)) for r in sus if r[14]]
        sent = [p for fr in pays[c] for p in fr]
        print(f"channel {c}: {len(good)} CRC-clean signal units of {len(sent)}")
        assert len(good) >= (52, 52, 52, 26)[c], (c, len(good))
        i0 = sent.index(good[0])
        assert good == sent[i0:i0 + len(good)], c
        ref = O.run_demod(O.oqpsk_settings(), pcm[c], chunk=sizes)
        soft = demod2.read_softbits(c)
        n = len(ref["soft"])
        assert n > 0.9 * fb * len(rest) / fs and len(soft) == n + ref.get("pending", len(soft) - n)
        assert np.array_equal(soft[:n] >= 128, ref["soft"] >= 128), "hard decisions differ"
        assert_soft_bytes(soft[:n], ref["soft"], where=f"channel {c}", allow=0)
    for h in (ch, demod, demod2, aerol):
        h.close()
