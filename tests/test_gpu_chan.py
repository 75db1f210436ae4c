"""GPU (-m gpu): the wideband I/Q channeliser (jaero_chan_*, jaero_amd/csrc/k_chan.h) against its definition (tests/chan_oracle.py).

Every comparison of int16 output uses `chan_cases.assert_rule`: got == rint(y*), or off by one where the oracle's unrounded y* lies within
tau = 1e-7 max(1, g) LSB of a half-integer; and an output RMS above 100 LSB.  The inputs and the twelve channels are tests/chan_cases.py's."""
import numpy as np
import pytest

import chan_oracle as CO
from chan_cases import AUDIO, CH, CHAIN_AMPS, CHAIN_CENTRES, assert_rule, channel_set, pchannel_chain_capture, synthetic_capture, white_full_scale
from conftest import assert_soft_bytes

pytestmark = pytest.mark.gpu

HP = CO.HP


@pytest.mark.parametrize("decim", [16, 32, 64])
@pytest.mark.parametrize("ntaps", [1, 2049, 8193])
@pytest.mark.parametrize("source", ["white", "capture"])
def test_kernel_equals_definition(CH, decim, ntaps, source):
    """Taps: [1] (all-pass: the whole band aliases into the output), 2049 and 8193 entries with a 20 kHz cut-off (wide, so that the channel of
    gain 0.04 stays above 100 LSB RMS at every D; the default 9 kHz prototype runs in the chain and scale tests below)."""
    nhops = 6
    if source == "white":
        iq, strong = white_full_scale(nhops * HP, 100 + decim), 54321.0
    else:
        iq, centres = synthetic_capture(decim, nhops, 200 + decim)
        strong = centres[2]
    taps = np.ones(1) if ntaps == 1 else CH.design_taps(decim, cutoff_hz=20000.0, ntaps=ntaps, beta=8.0 if ntaps == 2049 else 16.0)
    chans = channel_set(CH, decim, strong, 0.04)
    x = CO.as_complex(iq)
    y1 = CO.block_form(x, decim, [tuple(chans[3])], taps)[0]
    chans[3][2] = 32767.5 / np.quantile(np.abs(y1), 0.99)  # 1 % of the oracle's own samples lie beyond the rails
    ystar = CO.block_form(x, decim, [tuple(c) for c in chans], taps)
    ch = CH.Channeliser(decim, chans, taps=taps, max_write_iq=nhops * HP)
    assert ch.write(iq) == nhops * ch.Mo
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


@pytest.mark.parametrize("nch,decim", [(1, 16), (7, 32), (64, 64), (67, 32)])
def test_ragged_writes(CH, nch, decim):
    import torch

    rng = np.random.default_rng(nch)
    fs = 48000.0 * decim
    chans = [(CH.tune_word(float(rng.uniform(-fs / 2, fs / 2)), fs), AUDIO, 1.0) for _ in range(nch)]
    mw = 4 * HP
    sizes = [1, 8191, 8193, 3 * 8192 + 5, mw, 0, 8191 - 5, 2 * HP, 3]
    total = sum(sizes)
    iq = rng.integers(-32768, 32768, size=(total, 2)).astype(np.int16)
    taps = CH.design_taps(decim, ntaps=2049, beta=10.0)
    ragged = CH.Channeliser(decim, chans, taps=taps, max_write_iq=mw)
    dev = CH.Channeliser(decim, chans, taps=taps, max_write_iq=mw)
    hop = CH.Channeliser(decim, chans, taps=taps, max_write_iq=HP)
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
    decim, fs = 32, 48000.0 * 32
    iq = white_full_scale(6 * HP, 7)
    x = CO.as_complex(iq)
    taps = CH.design_taps(decim, cutoff_hz=20000.0)
    chans = [(CH.tune_word(-50000.0, fs), AUDIO, 1.0), (CH.tune_word(123456.7, fs), AUDIO, 1.0), (CH.tune_word(123460.0, fs), AUDIO, 0.5)]
    new = (CH.tune_word(-400000.3, fs), CH.tune_word(5000.0, 48000.0), 0.25)
    plain = CH.Channeliser(decim, chans, taps=taps, max_write_iq=4 * HP)
    ch = CH.Channeliser(decim, chans, taps=taps, max_write_iq=4 * HP)
    o = CO.ChanOracle(decim, chans, taps)
    cut = 3 * HP + 100  # the write ends inside a hop: the new words hold from block 3 on, whose input began under the old ones
    outs, refs, base = [], [], []
    for a, b in ((0, cut), (cut, 6 * HP)):
        assert ch.write(iq[a:b]) == plain.write(iq[a:b])
        outs.append(ch.read_pcm()); base.append(plain.read_pcm()); refs.append(o.write(x[a:b]))
        if b == cut:
            ch.retune(1, *new)
            o.retune(1, *new)
    got, base, ystar = np.concatenate(outs, axis=1), np.concatenate(base, axis=1), np.concatenate(refs, axis=1)
    n0 = outs[0].shape[1]
    assert n0 == 3 * ch.Mo and got.shape[1] == 6 * ch.Mo
    assert_rule(got[1, :n0], ystar[1, :n0], 1.0, "retuned channel, before")
    assert_rule(got[1, n0:], ystar[1, n0:], 0.25, "retuned channel, after")
    assert np.array_equal(got[1, :n0], base[1, :n0]) and not np.array_equal(got[1, n0:], base[1, n0:])
    assert got[0].tobytes() == base[0].tobytes() and got[2].tobytes() == base[2].tobytes()
    with pytest.raises(Exception):
        ch.retune(3, *new)
    with pytest.raises(Exception):
        ch.retune(0, new[0], new[1], 0.0)
    ch.close(); plain.close()


# ---------------------------------------------------------------------------------------------- the chain
def test_capture_to_signal_units_on_device(CH, oracle_mod):
    """Channeliser.feed -> DemodulatorBank -> AeroLBank.write_from_bank, nothing through the host: every channel yields >= 52 CRC-clean
    signal units that are a contiguous, in-order run of the transmitted ones (the same chain in numpy + oracle gives 78; 52 = two whole
    frames only keeps the check from passing empty).  And a second bank handed the same device PCM gives the oracle demodulator's soft bits
    on the PCM read back from the channeliser: hard decisions equal, soft bytes equal."""
    import ctypes as C

    from jaero_amd import capi
    from jaero_amd import demodulator as B

    O = oracle_mod
    pays, iq, info = pchannel_chain_capture()
    decim, fb, nch = 16, 10500, 4
    fs = 48000.0 * decim
    # the level signalgen.oqpsk produces: RMS = 0.1 of full scale; a channel's audio is the real part of amp * scale * (i + j q)
    gains = [0.1 * 32768.0 / (a * info["scale"] * np.sqrt(info["p_unit"] / 2.0)) for a in CHAIN_AMPS]
    chans = [(CH.tune_word(f, fs), AUDIO, g) for f, g in zip(CHAIN_CENTRES, gains)]
    hops = 40
    ch = CH.Channeliser(decim, chans, max_write_iq=hops * HP)
    mws = (hops + 1) * ch.Mo
    demod = B.DemodulatorBank(B.OqpskSettings(), nch, max_write_samples=mws, softbit_capacity=8192)
    demod2 = B.DemodulatorBank(B.OqpskSettings(), nch, max_write_samples=mws, softbit_capacity=1 << 16)
    aerol = B.AeroLBank(nch, fb, max_softbits_per_write=8192, su_capacity=26 * 8 + 8)
    small = B.DemodulatorBank(B.OqpskSettings(), nch, max_write_samples=mws - 1, softbit_capacity=8192)
    other = B.DemodulatorBank(B.OqpskSettings(), nch + 1, max_write_samples=mws, softbit_capacity=8192)
    for bad in (small, other):  # refused before anything advances
        with pytest.raises(capi.JaeroError) as e:
            ch.feed(bad, iq[:HP])
        assert e.value.code == capi.E_INVAL
        bad.close()
    pcm, sizes = [], []
    for s in range(0, len(iq), hops * HP):
        nout = ch.feed(demod, iq[s:s + hops * HP])
        assert nout == (min(len(iq), s + hops * HP) - s) // HP * ch.Mo
        aerol.write_from_bank(demod, 8192)
        ptr, n = ch.pcm_view()
        assert n == nout
        capi.check(demod2.L.jaero_write(demod2.h, ptr, n, capi.PCM_CHANNEL_MAJOR, 1, None))
        pcm.append(ch.read_pcm())
        sizes.append(nout)
    pcm = np.concatenate(pcm, axis=1)
    assert pcm.shape == (nch, len(iq) // HP * ch.Mo)
    for c in range(nch):
        rms = pcm[c].astype(float).std()
        print(f"channel {c}: gain {gains[c]:.2f}, PCM rms {rms:.0f} LSB")
        assert 0.08 * 32768 < rms < 0.13 * 32768
        sus = aerol.read_sus(c)
        good = [bytes(r[2:12].astype(np.uint8)) for r in sus if r[14]]
        sent = [p for fr in pays[c] for p in fr]
        print(f"channel {c}: {len(good)} CRC-clean signal units of {len(sent)}")
        assert len(good) >= 52, (c, len(good))
        i0 = sent.index(good[0])
        assert good == sent[i0:i0 + len(good)], c
        ref = O.run_demod(O.oqpsk_settings(), pcm[c], chunk=sizes)
        soft = demod2.read_softbits(c)
        n = len(ref["soft"])
        assert n > 8 * 5250 * 0.9 and len(soft) == n + ref.get("pending", len(soft) - n)
        assert np.array_equal(soft[:n] >= 128, ref["soft"] >= 128), "hard decisions differ"
        assert_soft_bytes(soft[:n], ref["soft"], where=f"channel {c}", allow=0)
    for h in (ch, demod, demod2, aerol):
        h.close()


def test_scale_33091_channels(CH):
    """33 091 channels at D = 32, 16 hops in one write: 16 spread channels against the oracle; then a feed into a bank of that size."""
    from jaero_amd import demodulator as B

    decim, nch, nhops = 32, 33091, 16
    fs = 48000.0 * decim
    rng = np.random.default_rng(33091)
    tune = rng.integers(0, 1 << 32, size=nch, dtype=np.uint64)
    chans = [(int(t), AUDIO, 1.0) for t in tune]
    iq = rng.integers(-32768, 32768, size=(nhops * HP, 2)).astype(np.int16)
    ch = CH.Channeliser(decim, chans, max_write_iq=nhops * HP)
    ch.profile_enable(True)
    assert ch.write(iq) == nhops * ch.Mo
    got = ch.read_pcm()
    print("k_chan_fwd ms, launches:", ch.profile_read(0), " k_chan_synth:", ch.profile_read(1))
    assert ch.profile_read(0)[1] == 1 and ch.profile_read(1)[1] == 1
    pick = sorted({0, 1, 63, 64, nch - 1, nch - 2} | set(int(v) for v in rng.integers(0, nch, size=10)))
    ystar = CO.block_form(CO.as_complex(iq), decim, [chans[c] for c in pick], CH.design_taps(decim))
    for k, c in enumerate(pick):
        assert_rule(got[c], ystar[k], 1.0, f"scale ch{c}")
    del got
    bank = B.DemodulatorBank(B.OqpskSettings(), nch, max_write_samples=(nhops + 1) * ch.Mo, softbit_capacity=2048, ebno=False)
    assert ch.feed(bank, iq) == nhops * ch.Mo
    st = bank.read_status(nch - 1)  # synchronises
    assert np.isfinite(st.mse)
    bank.close()
    ch.close()
