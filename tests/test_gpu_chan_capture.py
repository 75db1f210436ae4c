"""GPU (-m gpu): the channeliser's capture front end (jaero_chan3_*, jaero_amd/csrc/k_chan_capture.h) against its definition
(tests/chan_capture_oracle.py): the staged stream bit for bit where no rotation is involved, within 2^-46 S X where one is, and the int16
output by `chan_cases.assert_rule`.

CAP_RUN = 256 is the staging kernel's run of outputs per workgroup; write sizes are chosen around it."""
import ctypes as C

import numpy as np
import pytest

import chan_capture_oracle as CC
import chan_oracle as CO
import chan_survey_oracle as SO
from chan_cases import AUDIO, CH, CHAIN_AMPS, CHAIN_CENTRES, assert_rule, channel_set, pchannel_chain_capture

pytestmark = pytest.mark.gpu

HP = CO.HP
CAP_RUN = 256
ONE = [(12345678, AUDIO, 1.0)]


def raw_samples(fmt, n, seed, full_scale=False):
    """n raw I/Q pairs of the format.  cf32 holds NaN, +-Inf, values beyond +-1 and -0.0 among values of 0.3 RMS."""
    rng = np.random.default_rng(seed)
    if fmt == "cu8":
        if full_scale:
            k, s = rng.integers(0, 3, size=(n, 2)), rng.integers(0, 2, size=(n, 2))
            return np.where(s == 1, 255 - k, k).astype(np.uint8)
        return rng.integers(0, 256, size=(n, 2), dtype=np.uint8)
    if fmt == "cs8":
        return rng.integers(-128, 128, size=(n, 2), dtype=np.int8)
    if fmt == "cs16":
        if full_scale:
            k, s = rng.integers(0, 256, size=(n, 2)), rng.integers(0, 2, size=(n, 2))
            return np.where(s == 1, 32767 - k, -32768 + k).astype(np.int16)
        return rng.integers(-32768, 32768, size=(n, 2), dtype=np.int16)
    a = (0.3 * rng.normal(size=(n, 2))).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 1.5, -7.25, -0.0, 1.0, -1.0, 2.0 ** -140], np.float32)
    pos = rng.choice(n * 2, size=min(200, n // 4), replace=False)
    a.reshape(-1)[pos] = special[np.arange(len(pos)) % len(special)]
    return a


def ragged_sizes(K, L, Mr, max_write_iq, total):
    """0, 1, K - 2, K - 1, K, the inputs that stage one sample less than, exactly and one more than a workgroup's run (and two runs),
    max_write_iq, and odd sizes in between; the last piece takes what is left of `total`."""
    around = [(-(-k * Mr // L)) for k in (CAP_RUN - 1, CAP_RUN, CAP_RUN + 1, 2 * CAP_RUN - 1, 2 * CAP_RUN, 2 * CAP_RUN + 1)]
    sizes = [1, 0, max(K - 2, 0), max(K - 1, 0), K, 1, 1, 2] + around + [7777, 3, max_write_iq, 12345, 0, 5]
    assert sum(sizes) < total
    left = total - sum(sizes)
    while left > 0:
        sizes.append(min(left, max_write_iq - 1))
        left -= sizes[-1]
    return sizes


def make(CHm, decim, fs_in, fmt, K=32, shift_hz=0.0, max_write_iq=40000, chans=ONE, taps=None, rtaps=None):
    cap = CHm.Capture(fs_in=fs_in, fmt=fmt, shift_hz=shift_hz, taps_per_phase=K, rtaps=rtaps)
    return CHm.Channeliser(decim, chans, taps=np.ones(1) if taps is None else taps, max_write_iq=max_write_iq, capture=cap)


def oracle_for(CHm, ch, fmt, K):
    fs_in, fs_c = int(ch.fs_in), int(ch.fs_c)
    rt = getattr(ch, "rtaps", None)
    return CC.CaptureOracle(fmt, fs_in, fs_c, ch.shift_word, K, rt)


# ---------------------------------------------------------------------------------------------- 1. staged stream, bit for bit
STAGED_CASES = [
    # decim, fs_in, format, K                   L / Mr
    (16, 1200000, "cu8", 32),                 # 16 / 25
    (16, 1200000, "cs16", 1),
    (16, 1200000, "cs8", 64),
    (16, 1200000, "cf32", 32),
    (64, 2400000, "cu8", 64),                 # 32 / 25
    (32, 2048000, "cs8", 32),                 # 3 / 4
    (64, 2500000, "cs16", 32),                # 768 / 625
    (64, 10000000, "cf32", 1),                # 192 / 625
    (64, 10000000, "cu8", 32),
]


@pytest.mark.parametrize("decim,fs_in,fmt,K", STAGED_CASES)
def test_staged_stream_bit_for_bit(CH, decim, fs_in, fmt, K):
    """shift = 0: convert and resample only, every product and sum rounded once on both sides -> np.array_equal.  Ragged writes from the
    host, the same from device memory, and the whole input in one write give the same stream; the count after every write is
    ceil(T L / Mr)."""
    import torch

    total, mw = 100003, 40000
    raw = raw_samples(fmt, total, 1000 + K + decim)
    host, dev = make(CH, decim, fs_in, fmt, K, max_write_iq=mw), make(CH, decim, fs_in, fmt, K, max_write_iq=mw)
    once = make(CH, decim, fs_in, fmt, K, max_write_iq=total)
    L, Mr = CC.ratio(fs_in, host.fs_c)
    assert (L, Mr) != (1, 1)
    o = oracle_for(CH, host, fmt, K)
    draw = torch.from_numpy(raw).cuda()
    parts, pos, staged_counts = [], 0, set()
    for n in ragged_sizes(K, L, Mr, mw, total):
        nout = host.write(raw[pos:pos + n])
        assert dev.write(draw[pos:pos + n].contiguous()) == nout
        want = o.write(raw[pos:pos + n])
        pos += n
        got, first = host.read_staged()
        dgot, dfirst = dev.read_staged()
        assert first == dfirst == o.first and len(got) == len(want) and o.first + len(want) == -(-pos * L // Mr), (pos, n)
        assert np.array_equal(got.real, want.real) and np.array_equal(got.imag, want.imag), (pos, n)
        assert np.array_equal(dgot.real, want.real) and np.array_equal(dgot.imag, want.imag), (pos, n, "device pointer")
        staged_counts.add(len(got))
        parts.append(got)
    assert pos == total
    with pytest.raises(Exception):
        host.write(raw[:mw + 1])  # refused, nothing consumed
    whole = np.concatenate(parts)
    once.write(raw)
    z, first = once.read_staged()
    assert first == 0 and np.array_equal(z.real, whole.real) and np.array_equal(z.imag, whole.imag)
    assert np.isfinite(whole.real).all() and np.isfinite(whole.imag).all() and whole.real.std() > 100.0
    print(f"{fmt} {fs_in} -> {int(host.fs_c)} (L / Mr = {L} / {Mr}, K = {K}): {len(whole)} staged samples equal; staged per write "
          f"{sorted(staged_counts)[:12]} ...")
    for h in (host, dev, once):
        h.close()


# ---------------------------------------------------------------------------------------------- 2. pure conversion
@pytest.mark.parametrize("fmt", ["cs16", "cu8", "cs8", "cf32"])
def test_pure_conversion(CH, fmt):
    """Equal rates, shift = 0: the staged stream IS the conversion."""
    raw = raw_samples(fmt, 30001, 7)
    ch = make(CH, 16, 768000, fmt, K=-5, max_write_iq=20000)  # K is ignored at equal rates
    re, im = CC.convert(raw, CC.FORMATS[fmt])
    pos = 0
    for n in (1, 0, 255, 256, 257, 20000, 9232):
        ch.write(raw[pos:pos + n])
        z, first = ch.read_staged()
        assert first == pos and np.array_equal(z.real, re[pos:pos + n]) and np.array_equal(z.imag, im[pos:pos + n]), (fmt, pos, n)
        if fmt == "cf32":
            assert np.array_equal(np.signbit(z.real), np.signbit(re[pos:pos + n]))  # -0.0 stays -0.0
        pos += n
    assert pos == len(raw)
    ch.close()


def test_cs16_capture_handle_equals_plain_handle(CH):
    """A CS16 capture handle at the channeliser's own rate gives the int16 output of a jaero_chan2_create handle byte for byte, through
    jaero_chan3_write and through jaero_chan_write (which works on it)."""
    import torch

    from jaero_amd import capi

    decim, fs = 32, 48000.0 * 32
    rng = np.random.default_rng(11)
    chans = [(CH.tune_word(float(rng.uniform(-fs / 2, fs / 2)), fs), AUDIO, 1.0) for _ in range(7)]
    taps = CH.design_taps(decim, ntaps=2049, beta=10.0)
    mw = 4 * HP
    sizes = [1, 8191, 8193, 3 * 8192 + 5, mw, 0, 8191 - 5, 2 * HP, 3]
    iq = rng.integers(-32768, 32768, size=(sum(sizes), 2)).astype(np.int16)
    plain = CH.Channeliser(decim, chans, taps=taps, max_write_iq=mw)
    cap = make(CH, decim, int(fs), "cs16", chans=chans, taps=taps, max_write_iq=mw)
    old = make(CH, decim, int(fs), "cs16", chans=chans, taps=taps, max_write_iq=mw)
    diq = torch.from_numpy(iq).cuda()
    pos, outs = 0, [[], [], []]
    for i, n in enumerate(sizes):
        want = plain.write(iq[pos:pos + n])
        assert cap.write(diq[pos:pos + n].contiguous() if i % 2 else iq[pos:pos + n]) == want
        a = np.ascontiguousarray(iq[pos:pos + n])
        nout = C.c_int(-1)
        capi.check(old.L.jaero_chan_write(old.h, a.ctypes.data, n, 0, None, C.byref(nout)))
        assert nout.value == want
        old.last_nout = nout.value
        pos += n
        for k, h in enumerate((plain, cap, old)):
            outs[k].append(h.read_pcm())
    ref, got, got_old = (np.concatenate(o, axis=1) for o in outs)
    assert ref.shape == (7, (pos // HP) * plain.Mo) and ref.astype(float).std(axis=1).min() > 100.0
    assert np.array_equal(got, ref) and np.array_equal(got_old, ref)
    for h in (plain, cap, old):
        h.close()


def test_chan_write_refuses_a_cu8_handle_and_changes_nothing(CH):
    from jaero_amd import capi

    K = 32
    raw = raw_samples("cu8", 9000, 5)
    ch = make(CH, 16, 1200000, "cu8", K)
    o = oracle_for(CH, ch, "cu8", K)
    ch.write(raw[:4000])
    z, _ = ch.read_staged()
    want = o.write(raw[:4000])
    assert np.array_equal(z.real, want.real) and np.array_equal(z.imag, want.imag)
    bank_less = C.c_int(5)
    bad = np.zeros((100, 2), np.int16)
    rc = ch.L.jaero_chan_write(ch.h, bad.ctypes.data, 100, 0, None, C.byref(bank_less))
    assert rc == capi.E_INVAL and b"jaero_chan_write" in ch.L.jaero_last_error()
    ch.write(raw[4000:])
    z, first = ch.read_staged()
    want = o.write(raw[4000:])
    assert first == o.first and np.array_equal(z.real, want.real) and np.array_equal(z.imag, want.imag)
    ch.close()


# ---------------------------------------------------------------------------------------------- 3. shift != 0
@pytest.mark.parametrize("decim,fs_in,fmt,shift_hz", [
    (16, 768000, "cu8", 123456.7), (16, 768000, "cs16", -250000.3),      # equal rates
    (16, 1200000, "cs16", 250000.3), (16, 1200000, "cu8", -123456.7),    # 16 / 25
    (16, 1200000, "cf32", -599999.9),                                    # a word next to -2^31
])
def test_shift_within_bound(CH, decim, fs_in, fmt, shift_hz):
    """|z_gpu - z_oracle| <= 2^-46 S X, S = max_phi sum_j |h[phi + j L]| (1 at equal rates), X = sqrt(2) max |component|: 64 ulp of the
    largest possible sum (two libm-grade rotations differ by a few ulp per input sample; the same-order sums add under K 2^-53).
    Measured on an MI355X: see the table in DESIGN 18."""
    K = 32
    raw = raw_samples(fmt, 100003, 31, full_scale=fmt != "cf32")
    if fmt == "cf32":
        raw = np.where(np.isfinite(raw), np.clip(raw, -1.0, 1.0), raw).astype(np.float32)
    ch = make(CH, decim, fs_in, fmt, K, shift_hz=shift_hz)
    word = ch.shift_word
    assert word != 0 and (word >= 1 << 31) == (shift_hz < 0)
    L, Mr = CC.ratio(fs_in, ch.fs_c)
    S = 1.0 if (L, Mr) == (1, 1) else CC.gain_bound(ch.rtaps, L)
    re, im = CC.convert(raw, CC.FORMATS[fmt])
    X = np.sqrt(2.0) * max(np.abs(re).max(), np.abs(im).max())
    bound = 2.0 ** -46 * S * X
    o = oracle_for(CH, ch, fmt, K)
    worst, pos, rms = 0.0, 0, []
    for n in ragged_sizes(K, L, Mr, 40000, len(raw)):
        ch.write(raw[pos:pos + n])
        want = o.write(raw[pos:pos + n])
        pos += n
        z, first = ch.read_staged()
        assert first == o.first and len(z) == len(want)
        if len(z):
            worst = max(worst, float(np.abs(z - want).max()))
            rms.append(float(np.abs(want).std()))
    print(f"{fmt} {fs_in} shift {shift_hz} Hz (word {word}): max |z_gpu - z_oracle| = {worst:.3g} LSB = {worst / bound:.3g} of the bound "
          f"{bound:.3g} (S = {S:.4f}, X = {X:.0f})")
    assert max(rms) > 100.0
    assert worst <= bound
    ch.close()


# ---------------------------------------------------------------------------------------------- 4. output against the definition
OUTPUT_CASES = [(16, 1200000, "cu8"), (64, 4800000, "cs16"), (16, 600000, "cs16"), (64, 2400000, "cu8")]  # 16 / 25 twice, 32 / 25 twice


def output_case(CHm, decim, fs_in, fmt):
    """(raw, channels, taps, K, rtaps): white full-scale input (every sample within 1 % of a rail), 6 hops of staged samples and a bit,
    the 20 kHz prototype; channel 3's gain from the oracle's own output."""
    K = 32
    fs_c = 48000 * decim
    L, Mr = CC.ratio(fs_in, fs_c)
    n = -(-6 * HP * Mr // L) + 100
    raw = raw_samples(fmt, n, 100 + decim, full_scale=True)
    taps = CHm.design_taps(decim, cutoff_hz=20000.0, ntaps=8193, beta=16.0)
    rtaps = CHm.design_resampler(fs_in, fs_c, K)[0]
    chans = channel_set(CHm, decim, 54321.0, 0.04, fs_in=fs_in)
    z = CC.CaptureOracle(fmt, fs_in, fs_c, 0, K, rtaps).write(raw)
    y1 = CO.block_form(z, decim, [tuple(chans[3])], taps)[0]
    chans[3][2] = 32767.5 / np.quantile(np.abs(y1), 0.99)
    return raw, chans, taps, K, rtaps, z


@pytest.mark.parametrize("decim,fs_in,fmt", OUTPUT_CASES)
def test_output_equals_definition(CH, decim, fs_in, fmt):
    """Oracle staging -> ChanOracle -> the int16 rule, every channel, no share of samples written off.  Ragged writes."""
    raw, chans, taps, K, rtaps, z = output_case(CH, decim, fs_in, fmt)
    ystar = CO.block_form(z, decim, [tuple(c) for c in chans], taps)
    ch = make(CH, decim, fs_in, fmt, K, chans=chans, taps=taps, max_write_iq=len(raw), rtaps=rtaps)
    outs, pos, produced = [], 0, 0
    for n in (1, 31, 32, 4999, len(raw) // 2, 0, len(raw)):
        n = min(n, len(raw) - pos)
        nout = ch.write(raw[pos:pos + n])
        pos += n
        L, Mr = CC.ratio(fs_in, ch.fs_c)
        assert nout == (-(-pos * L // Mr)) // HP * ch.Mo - produced
        produced += nout
        outs.append(ch.read_pcm())
    got = np.concatenate(outs, axis=1)
    ch.close()
    assert got.shape == ystar.shape and got.shape[1] == 6 * ch.Mo
    for c in range(len(chans)):
        assert_rule(got[c], ystar[c], chans[c][2], f"D={decim} {fmt} {fs_in} ch{c}")
    clipped = np.mean(np.abs(got[3].astype(int)) >= 32767)
    print(f"clipping channel: {100 * clipped:.2f} % of samples at the rails")
    assert 0.001 < clipped < 0.05


# ---------------------------------------------------------------------------------------------- 5. survey on a capture handle
def test_survey_on_a_capture_handle(CH):
    """16 / 25, cu8: spectrum and levels against tests/chan_survey_oracle.py fed the oracle's staged stream; the bound is that file's
    (tests/test_gpu_chan_survey.py): |got - want| <= 1e-12 (want + ref), ref = mean_k(want) / max_c(want)."""
    decim, fs_in, fmt = 16, 1200000, "cu8"
    raw, chans, taps, K, rtaps, z = output_case(CH, decim, fs_in, fmt)
    so = SO.ChanSurveyOracle(decim, [tuple(c) for c in chans], taps)
    nblk = so.survey(z)
    assert nblk == 6
    ch = make(CH, decim, fs_in, fmt, K, chans=chans, taps=taps, max_write_iq=len(raw), rtaps=rtaps)
    ch.survey_enable(psd=True, levels=True)
    half = len(raw) // 2 + 17
    ch.write(raw[:half])
    ch.write(raw[half:])
    S, nb = ch.read_psd_sums()
    E, cnt = ch.read_level_sums()
    ch.close()
    assert nb == nblk and (cnt == so.n).all()
    for name, got, want, ref in (("spectrum", S, so.S, float(so.S.mean())), ("levels", E, so.E, float(so.E.max()))):
        err = float(np.max(np.abs(got - want) / (want + ref)))
        print(f"{name}: largest |got - want| / (want + ref) = {err:.2e} over {got.size} values")
        assert np.isfinite(got).all() and err <= 1e-12, (name, err)


# ---------------------------------------------------------------------------------------------- 6. the chain, from an RTL-style capture
def chain_capture_cu8(CHm):
    """`chan_cases.pchannel_chain_capture` (768 kS/s) raised to 1.2 MS/s by the ORACLE resampler at 25 / 16 and quantised to cu8 (the inverse
    of the format's conversion, rounded).  Returns (payloads, raw cu8 [n, 2], info)."""
    pays, iq, info = pchannel_chain_capture()
    h, L, Mr = CHm.design_resampler(768000, 1200000, 32)
    assert (L, Mr) == (25, 16)
    re, im = CC.Resampler(h, L, Mr, 32).write(iq[:, 0].astype(np.float64), iq[:, 1].astype(np.float64))
    raw = np.empty((len(re), 2), np.uint8)
    raw[:, 0] = np.clip(np.rint((re / 128.0 + 255.0) / 2.0), 0, 255)
    raw[:, 1] = np.clip(np.rint((im / 128.0 + 255.0) / 2.0), 0, 255)
    return pays, raw, info


def chain_channels(CHm, info):
    fs = 768000.0
    gains = [0.1 * 32768.0 / (a * info["scale"] * np.sqrt(info["p_unit"] / 2.0)) for a in CHAIN_AMPS]
    return [(CHm.tune_word(f, fs), AUDIO, g) for f, g in zip(CHAIN_CENTRES, gains)]


def test_rtl_style_capture_to_signal_units_on_device(CH):
    """Channeliser(capture = cu8 @ 1 200 000).feed -> OQPSK bank -> AeroLBank.write_from_bank, nothing through the host: every channel
    yields a contiguous, in-order run of >= 52 CRC-clean signal units (52 = two frames only keeps the check from passing empty; the same
    capture through oracle staging -> ChanOracle -> oracle demodulator -> Aero-L on the CPU gives the counts in DESIGN 18)."""
    from jaero_amd import demodulator as B

    pays, raw, info = chain_capture_cu8(CH)
    chans = chain_channels(CH, info)
    nch, fb = 4, 10500
    step = 40 * HP * 25 // 16  # 40 hops of staged samples per feed
    ch = make(CH, 16, 1200000, "cu8", 32, chans=chans, taps=CH.design_taps(16), max_write_iq=step)
    mws = (40 + 1) * ch.Mo
    demod = B.DemodulatorBank(B.OqpskSettings(), nch, max_write_samples=mws, softbit_capacity=8192)
    aerol = B.AeroLBank(nch, fb, max_softbits_per_write=8192, su_capacity=26 * 8 + 8)
    total = 0
    for s in range(0, len(raw), step):
        total += ch.feed(demod, raw[s:s + step])
        aerol.write_from_bank(demod, 8192)
    assert total == (-(-len(raw) * 16 // 25)) // HP * ch.Mo
    for c in range(nch):
        sus = aerol.read_sus(c)
        good = [bytes(r[2:12].astype(np.uint8)) for r in sus if r[14]]
        sent = [p for fr in pays[c] for p in fr]
        print(f"channel {c}: {len(good)} CRC-clean signal units of {len(sent)}")
        assert len(good) >= 52, (c, len(good))
        i0 = sent.index(good[0])
        assert good == sent[i0:i0 + len(good)], c
    for h in (ch, demod, aerol):
        h.close()


# ---------------------------------------------------------------------------------------------- 7. scale and time
def test_scale_4096_channels_cu8_at_2400000(CH):
    """4096 channels, D = 64, cu8 at 2.4 MS/s, one write of 16 hops' worth (102 400 capture samples -> 131 072 staged): 16 spread channels
    by the rule, one launch of each of the two new kernels.  Nothing is asserted about time; the milliseconds are printed beside
    k_chan_fwd and k_chan_synth of a plain handle fed 16 hops in the same run."""
    decim, nch, nhops, fs_in, K = 64, 4096, 16, 2400000, 32
    fs_c = 48000.0 * decim
    rng = np.random.default_rng(4096)
    chans = [(CH.tune_word(float(f), fs_c), AUDIO, 1.0) for f in rng.uniform(-1.1e6, 1.1e6, size=nch)]
    n = nhops * HP * 25 // 32
    raw = raw_samples("cu8", n, 4096)
    ch = make(CH, decim, fs_in, "cu8", K, chans=chans, taps=CH.design_taps(decim), max_write_iq=n)
    ch.profile_enable(True)
    assert ch.write(raw) == nhops * ch.Mo
    got = ch.read_pcm()
    stage, fwd, syn = ch.capture_profile_read(0), ch.capture_profile_read(1), ch.profile_read(1)
    assert stage[1] == 1 and fwd[1] == 1 and syn[1] == 1 and ch.profile_read(0)[1] == 0
    z = CC.CaptureOracle("cu8", fs_in, int(fs_c), 0, K, ch.rtaps).write(raw)
    assert len(z) == nhops * HP
    pick = sorted({0, 1, 63, 64, nch - 1, nch - 2} | set(int(v) for v in rng.integers(0, nch, size=10)))
    ystar = CO.block_form(z, decim, [chans[c] for c in pick], CH.design_taps(decim))
    for k, c in enumerate(pick):
        assert_rule(got[c], ystar[k], 1.0, f"scale ch{c}")
    ch.close()
    plain = CH.Channeliser(decim, chans, max_write_iq=nhops * HP)
    plain.profile_enable(True)
    assert plain.write(rng.integers(-32768, 32768, size=(nhops * HP, 2)).astype(np.int16)) == nhops * plain.Mo
    plain.read_pcm()
    pf, ps = plain.profile_read(0), plain.profile_read(1)
    plain.close()
    print(f"capture handle: k_capture_stage {stage[0]:.4f} ms, k_capture_fwd {fwd[0]:.4f} ms, k_chan_synth {syn[0]:.4f} ms; "
          f"plain handle: k_chan_fwd {pf[0]:.4f} ms, k_chan_synth {ps[0]:.4f} ms (single un-warmed writes of 16 hops, 4096 channels, D = 64)")
