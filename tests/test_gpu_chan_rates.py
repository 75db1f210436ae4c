"""GPU (-m gpu): the channeliser at total decimations 128 / 256 and output rates 24 / 12 kHz (jaero_chan2_create, k_chan_synth<128> / <256>)
against its definition (tests/chan_oracle.py), and the capture -> channeliser -> MSK bank chain at the reference's default MSK rates.

Every comparison of int16 output uses `chan_cases.assert_rule`; the inputs and the twelve channels are tests/chan_cases.py's, at the output
rate."""
import numpy as np
import pytest

import chan_oracle as CO
from chan_cases import AUDIO, CH, FS_OUT, assert_rule, channel_set, synthetic_capture, white_full_scale
from conftest import assert_soft_bytes
from jaero_amd import signalgen as G

pytestmark = pytest.mark.gpu

HP = CO.HP


def definition_case(CHm, decim, ntaps, source):
    """(iq, taps, channels, y*) of one case of test_kernel_equals_definition: 768 samples per channel."""
    fs_out = FS_OUT[decim]
    nhops = 768 // (CO.N // decim // 2)
    if source == "white":
        iq, strong = white_full_scale(nhops * HP, 100 + decim), 54321.0
    else:
        iq, centres = synthetic_capture(decim, nhops, 200 + decim)
        strong = centres[2]
    taps = np.ones(1) if ntaps == 1 else CHm.design_taps(decim, cutoff_hz=fs_out * 5 / 12, ntaps=ntaps, beta=8.0 if ntaps == 2049 else 16.0,
                                                         fs_out=fs_out)
    chans = channel_set(CHm, decim, strong, 0.1)
    x = CO.as_complex(iq)
    y1 = CO.block_form(x, decim, [tuple(chans[3])], taps)[0]
    chans[3][2] = 32767.5 / np.quantile(np.abs(y1), 0.99)  # 1 % of the oracle's own samples lie beyond the rails
    ystar = CO.block_form(x, decim, [tuple(c) for c in chans], taps)
    return iq, taps, chans, ystar, nhops


@pytest.mark.parametrize("decim", [128, 256])
@pytest.mark.parametrize("ntaps", [1, 2049, 8193])
@pytest.mark.parametrize("source", ["white", "capture"])
def test_kernel_equals_definition(CH, decim, ntaps, source):
    """Taps: [1] (all-pass: the whole band aliases into the output), 2049 and 8193 entries with the cut-off at 5 / 12 of the output rate
    (the 48 kHz test's 20 kHz in proportion).  12 hops at D = 128, 24 at D = 256."""
    iq, taps, chans, ystar, nhops = definition_case(CH, decim, ntaps, source)
    assert nhops == {128: 12, 256: 24}[decim]
    ch = CH.Channeliser(decim, chans, taps=taps, max_write_iq=nhops * HP, fs_out=FS_OUT[decim])
    assert ch.fs_out == FS_OUT[decim] and ch.Mo == CO.N // decim // 2
    assert ch.write(iq) == nhops * ch.Mo == 768
    got = ch.read_pcm()
    ptr, n = ch.pcm_view()
    assert ptr and n == nhops * ch.Mo
    ch.close()
    assert got.shape == ystar.shape
    for c in range(len(chans)):
        assert_rule(got[c], ystar[c], chans[c][2], f"D={decim} L={ntaps} {source} ch{c}")
    clipped = np.mean(np.abs(got[3].astype(int)) >= 32767)
    print(f"clipping channel: {100 * clipped:.2f} % of samples at the rails")
    assert 0.001 < clipped < 0.05
    assert (got[3] == 32767).any() or (got[3] == -32768).any()


@pytest.mark.parametrize("nch,decim", [(1, 128), (7, 256), (64, 256), (67, 128)])
def test_ragged_writes(CH, nch, decim):
    import torch

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
    dev = CH.Channeliser(decim, chans, taps=taps, max_write_iq=mw, fs_out=fs_out)
    hop = CH.Channeliser(decim, chans, taps=taps, max_write_iq=HP, fs_out=fs_out)
    diq = torch.from_numpy(iq).cuda()
    Mo = ragged.Mo
    parts, dparts, pos, produced = [], [], 0, 0
    for n in sizes:
        nout = ragged.write(iq[pos:pos + n])
        assert nout == ((pos + n) // HP) * Mo - produced
        assert dev.write(diq[pos:pos + n].contiguous()) == nout
        pos += n
        produced += nout
        parts.append(ragged.read_pcm())
        dparts.append(dev.read_pcm())
        assert parts[-1].shape == (nch, nout)
    with pytest.raises(Exception):
        ragged.write(np.zeros((mw + 1, 2), np.int16))  # refused, nothing consumed
    assert ragged.write(iq[:0]) == 0
    ref = []
    for k in range(total // HP):
        assert hop.write(iq[k * HP:(k + 1) * HP]) == Mo
        ref.append(hop.read_pcm())
    got, dgot, ref = np.concatenate(parts, axis=1), np.concatenate(dparts, axis=1), np.concatenate(ref, axis=1)
    assert got.shape == ref.shape == (nch, (total // HP) * Mo)
    assert got.tobytes() == ref.tobytes() and dgot.tobytes() == ref.tobytes()
    assert got.astype(float).std(axis=1).min() > 100.0
    for c in (ragged, dev, hop):
        c.close()


def test_retune_mid_stream(CH):
    decim, fs_out = 256, 12000.0
    fs = fs_out * decim
    nhops = 12
    iq = white_full_scale(nhops * HP, 7)
    x = CO.as_complex(iq)
    taps = CH.design_taps(decim, cutoff_hz=fs_out * 5 / 12, fs_out=fs_out)
    chans = [(CH.tune_word(-50000.0, fs), AUDIO, 1.0), (CH.tune_word(123456.7, fs), AUDIO, 1.0), (CH.tune_word(123460.0, fs), AUDIO, 0.5)]
    new = (CH.tune_word(-400000.3, fs), CH.tune_word(1250.0, fs_out), 0.25)
    plain = CH.Channeliser(decim, chans, taps=taps, max_write_iq=8 * HP, fs_out=fs_out)
    ch = CH.Channeliser(decim, chans, taps=taps, max_write_iq=8 * HP, fs_out=fs_out)
    o = CO.ChanOracle(decim, chans, taps)
    cut = 6 * HP + 100  # the write ends inside a hop: the new words hold from block 6 on, whose input began under the old ones
    outs, refs, base = [], [], []
    for a, b in ((0, cut), (cut, nhops * HP)):
        assert ch.write(iq[a:b]) == plain.write(iq[a:b])
        outs.append(ch.read_pcm()); base.append(plain.read_pcm()); refs.append(o.write(x[a:b]))
        if b == cut:
            ch.retune(1, *new)
            o.retune(1, *new)
    got, base, ystar = np.concatenate(outs, axis=1), np.concatenate(base, axis=1), np.concatenate(refs, axis=1)
    n0 = outs[0].shape[1]
    assert n0 == 6 * ch.Mo and got.shape[1] == nhops * ch.Mo
    assert_rule(got[1, :n0], ystar[1, :n0], 1.0, "retuned channel, before")
    assert_rule(got[1, n0:], ystar[1, n0:], 0.25, "retuned channel, after")
    assert np.array_equal(got[1, :n0], base[1, :n0]) and not np.array_equal(got[1, n0:], base[1, n0:])
    assert got[0].tobytes() == base[0].tobytes() and got[2].tobytes() == base[2].tobytes()
    with pytest.raises(Exception):
        ch.retune(3, *new)
    with pytest.raises(Exception):
        ch.retune(0, new[0], new[1], 0.0)
    ch.close(); plain.close()


def test_the_rate_is_a_label(CH):
    """fs_out enters no arithmetic: the same decim, taps and words give the same bytes whatever the output is called.  What the label does:
    feed accepts a bank whose Fs it names and refuses every other one before anything advances."""
    from jaero_amd import capi
    from jaero_amd import demodulator as B

    decim, nhops = 64, 24
    fs = 12000.0 * decim
    iq = white_full_scale(nhops * HP, 11)
    taps = CH.design_taps(decim, fs_out=12000.0)
    chans = [(CH.tune_word(-50000.0, fs), AUDIO, 1.0), (CH.tune_word(123456.7, fs), CH.tune_word(1000.0, 12000.0), 0.5),
             (CH.tune_word(fs / 2 - 2500.0, fs), AUDIO, 0.25)]
    nch = len(chans)
    a = CH.Channeliser(decim, chans, taps=taps, max_write_iq=nhops * HP, fs_out=12000.0)
    b = CH.Channeliser(decim, chans, taps=taps, max_write_iq=nhops * HP)
    assert a.fs_out == 12000.0 and b.fs_out == 48000.0
    assert a.write(iq) == b.write(iq) == nhops * a.Mo
    pa, pb = a.read_pcm(), b.read_pcm()
    assert pa.tobytes() == pb.tobytes() and pa.astype(float).std(axis=1).min() > 100.0
    a.close(); b.close()

    mw = 9 * HP
    mk = lambda rate: CH.Channeliser(decim, chans, taps=taps, max_write_iq=mw, fs_out=rate)
    bank = lambda rate: B.DemodulatorBank(B.MskSettings(fb=600.0, lockingbw=900.0, Fs=rate), nch, max_write_samples=(mw // HP + 1) * (CO.N // decim // 2),
                                          softbit_capacity=4096)
    c12, twin, c48 = mk(12000.0), mk(12000.0), mk(48000.0)
    b12, btwin, b48 = bank(12000.0), bank(12000.0), bank(48000.0)

    def refused(ch, bk, piece):
        with pytest.raises(capi.JaeroError) as e:
            ch.feed(bk, piece)
        assert e.value.code == capi.E_INVAL and "Fs" in str(e.value)

    cuts = [0, 8 * HP - 100, 16 * HP + 3, nhops * HP]
    refused(c12, b48, iq[:HP])   # a 12 kHz channeliser into a 48 kHz bank
    refused(c48, b12, iq[:HP])   # a 48 kHz channeliser into a 12 kHz bank
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        n = c12.feed(b12, iq[lo:hi])
        assert n == twin.feed(btwin, iq[lo:hi]) == (hi // HP - lo // HP) * c12.Mo
        assert c12.read_pcm().tobytes() == twin.read_pcm().tobytes()
        refused(c12, b48, iq[lo:hi])  # consumes nothing: the next piece continues where the accepted one ended
    assert c48.feed(b48, iq[:mw]) == (mw // HP) * c48.Mo  # and the refusals left the 48 kHz pair usable
    for c in range(nch):
        s, t = b12.read_softbits(c), btwin.read_softbits(c)
        assert len(s) > 50 and np.array_equal(s, t), c
        assert np.isfinite(b12.read_status(c).mse)
    for h in (c12, twin, c48, b12, btwin, b48):
        h.close()


# ---------------------------------------------------------------------------------------------- the chains
MSK_CHAIN_CENTRES = [-150000.0, 200003.0]
MSK_CHAIN_AMPS = [1.0, 2.0]


def msk_chain_capture(fb, fs_out, decim, seconds):
    """Two continuous MSK channels of amplitudes 1 and 2, Eb/N0 13 dB on the weaker, 0.1 of full scale RMS; whole hops, at most 8 M samples."""
    fs = fs_out * decim
    n = int(seconds * fs) // HP * HP
    assert n <= 8_000_000
    rng = np.random.default_rng(int(fb + decim))
    bits = [rng.integers(0, 2, size=int(n / (fs / fb)) + 20, dtype=np.uint8) for _ in MSK_CHAIN_CENTRES]
    iq, info = G.wideband_msk(bits, MSK_CHAIN_CENTRES, MSK_CHAIN_AMPS, fs, fb=fb, ebno_db=13.0, rms=0.1, seed=7, nsamples=n, return_info=True)
    return bits, iq, info


def chain_channels(CHm, fb, fs_out, decim, info):
    fs = fs_out * decim
    audio_hz = 1000.0 if fb == 600 else 2000.0
    # a channel's audio is the real part of amp * scale * e^(j phase): RMS amp * scale * sqrt(p_unit / 2); brought to 0.1 of full scale
    gains = [0.1 * 32768.0 / (a * info["scale"] * np.sqrt(info["p_unit"] / 2.0)) for a in MSK_CHAIN_AMPS]
    return [(CHm.tune_word(f, fs), CHm.tune_word(audio_hz, fs_out), g) for f, g in zip(MSK_CHAIN_CENTRES, gains)], audio_hz, gains


def bits_match(hard, sent, fb, where):
    """From 1 s in, the hard decisions are the transmitted bits at ONE lag within +-40 and ONE polarity: returns (lag, inverted)."""
    i0 = int(fb)
    hard = np.asarray(hard).astype(np.uint8)
    assert len(hard) > i0 + 200, (where, len(hard))
    idx = np.arange(i0, len(hard))
    hits = [(lag, inv) for lag in range(-40, 41) for inv in (0, 1)
            if idx[-1] + lag < len(sent) and np.array_equal(hard[idx], sent[idx + lag] ^ inv)]
    print(f"{where}: {len(hard) - i0} bits from 1 s on, (lag, inverted) = {hits}")
    assert len(hits) == 1, (where, hits)
    return hits[0]


@pytest.mark.parametrize("fb,fs_out,decim,seconds", [(600, 12000.0, 256, 2.5), (600, 12000.0, 128, 4.0), (1200, 24000.0, 128, 2.5)])
def test_capture_to_msk_soft_bits_on_device(CH, oracle_mod, fb, fs_out, decim, seconds):
    """Channeliser.feed -> DemodulatorBank at the reference's default MSK rates (Fs = 12000 for 600 bps, 24000 for 1200 bps), nothing
    through the host, in 40-hop writes, at the default taps.  Per channel the bank's soft bits are the oracle demodulator's on the PCM read
    back from the channeliser (hard decisions equal, soft bytes equal); and from 1 s in the hard bits are the transmitted ones at one lag
    and polarity -- shown for the oracle's own output first."""
    from jaero_amd import demodulator as B

    O = oracle_mod
    bits, iq, info = msk_chain_capture(fb, fs_out, decim, seconds)
    chans, audio_hz, gains = chain_channels(CH, fb, fs_out, decim, info)
    nch, hops = len(chans), 40
    ch = CH.Channeliser(decim, chans, max_write_iq=hops * HP, fs_out=fs_out)
    assert ch.Mo == CO.N // decim // 2
    st = B.MskSettings(fb=float(fb), lockingbw=1.5 * fb, freq_center=audio_hz, Fs=fs_out)
    demod = B.DemodulatorBank(st, nch, max_write_samples=(hops + 1) * ch.Mo, softbit_capacity=1 << 14)
    pcm, sizes = [], []
    for s in range(0, len(iq), hops * HP):
        nout = ch.feed(demod, iq[s:s + hops * HP])
        assert nout == (min(len(iq), s + hops * HP) - s) // HP * ch.Mo
        pcm.append(ch.read_pcm())
        sizes.append(nout)
    pcm = np.concatenate(pcm, axis=1)
    assert pcm.shape == (nch, len(iq) // HP * ch.Mo)
    for c in range(nch):
        rms = pcm[c].astype(float).std()
        print(f"channel {c}: gain {gains[c]:.2f}, PCM rms {rms:.0f} LSB")
        assert 0.08 * 32768 < rms < 0.13 * 32768
        ref = O.run_demod(O.msk_settings(freq_center=audio_hz, lockingbw=1.5 * fb, fb=float(fb), Fs=fs_out), pcm[c], chunk=sizes)
        n = len(ref["soft"])
        lag = bits_match(ref["soft"] >= 128, bits[c], fb, f"oracle, channel {c}")
        soft = demod.read_softbits(c)
        assert n > seconds * fb * 0.9 and len(soft) == n + ref.get("pending", len(soft) - n)
        assert np.array_equal(soft[:n] >= 128, ref["soft"] >= 128), "hard decisions differ"
        assert_soft_bytes(soft[:n], ref["soft"], where=f"channel {c}", allow=0)
        assert bits_match(soft[:n] >= 128, bits[c], fb, f"bank, channel {c}") == lag
    ch.close(); demod.close()


def test_scale_33091_channels(CH):
    """33 091 channels at D = 256 and 12 kHz, 16 hops in one write: 16 spread channels against the oracle, one launch of each kernel; then a
    feed into a 600 bps / 12 kHz MSK bank of that size."""
    from jaero_amd import demodulator as B

    decim, fs_out, nch, nhops = 256, 12000.0, 33091, 16
    rng = np.random.default_rng(33091)
    tune = rng.integers(0, 1 << 32, size=nch, dtype=np.uint64)
    chans = [(int(t), AUDIO, 1.0) for t in tune]
    iq = rng.integers(-32768, 32768, size=(nhops * HP, 2)).astype(np.int16)
    ch = CH.Channeliser(decim, chans, max_write_iq=nhops * HP, fs_out=fs_out)
    ch.profile_enable(True)
    assert ch.write(iq) == nhops * ch.Mo
    got = ch.read_pcm()
    print("k_chan_fwd ms, launches:", ch.profile_read(0), " k_chan_synth:", ch.profile_read(1))
    assert ch.profile_read(0)[1] == 1 and ch.profile_read(1)[1] == 1
    pick = sorted({0, 1, 63, 64, nch - 1, nch - 2} | set(int(v) for v in rng.integers(0, nch, size=10)))
    assert len(pick) == 16
    ystar = CO.block_form(CO.as_complex(iq), decim, [chans[c] for c in pick], CH.design_taps(decim, fs_out=fs_out))
    for k, c in enumerate(pick):
        assert_rule(got[c], ystar[k], 1.0, f"scale ch{c}")
    del got
    bank = B.DemodulatorBank(B.MskSettings(fb=600.0, lockingbw=900.0, Fs=fs_out), nch, max_write_samples=(nhops + 1) * ch.Mo,
                             softbit_capacity=2048, ebno=False)
    assert ch.feed(bank, iq) == nhops * ch.Mo
    st = bank.read_status(nch - 1)  # synchronises
    assert np.isfinite(st.mse)
    bank.close()
    ch.close()
