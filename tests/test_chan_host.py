"""CPU: the channeliser's C ABI without a device (exports, refusals, no CPU fallback), the integer frequency arithmetic of the Python
helpers against the oracle's, and the oracle against itself at every total decimation 16 .. 256: the block (fast-convolution) form the
kernels implement against the ideal mix -> FIR -> decimate form, and fed in pieces against fed at once."""
import ctypes as C

import numpy as np
import pytest

import chan_oracle as CO
from chan_cases import FS_OUT, boundary_words, tone_capture
from jaero_amd import capi, channeliser as CH

CHAN_SYMBOLS = [s for s in capi.EXPORTS if s.startswith("jaero_chan_")]


def test_library_exports_every_chan_symbol():
    assert sorted(CHAN_SYMBOLS) == sorted(
        "jaero_chan_" + n for n in ("create", "destroy", "write", "pcm_view", "read_pcm", "retune", "feed", "profile_enable", "profile_read"))
    L = capi.lib()
    for name in CHAN_SYMBOLS:
        assert hasattr(L, name), name
    assert C.sizeof(capi.ChanChannel) == 16  # 2 uint32 + double
    assert L.jaero_abi_version() == 1


def _create(L, decim=32, nch=2, gains=(1.0, 1.0), taps=None, ntaps=None, max_write_iq=8192, ch_null=False, taps_null=False, out_null=False):
    arr = (capi.ChanChannel * max(nch, 1))(*[capi.ChanChannel(1000 * i, 715827883, g) for i, g in zip(range(max(nch, 1)), gains)])
    t = np.ones(3) / 3 if taps is None else np.asarray(taps, dtype=np.float64)
    h = C.c_void_p()
    rc = L.jaero_chan_create(0, decim, nch, None if ch_null else C.cast(arr, C.c_void_p), None if taps_null else t.ctypes.data,
                             t.size if ntaps is None else ntaps, max_write_iq, None if out_null else C.byref(h))
    return rc, h


@pytest.mark.parametrize("kw,word", [
    (dict(decim=8), b"decim"), (dict(decim=48), b"decim"), (dict(decim=0), b"decim"), (dict(decim=128), b"decim"),
    (dict(nch=0), b"nchannels"), (dict(nch=-3), b"nchannels"),
    (dict(ntaps=0), b"ntaps"), (dict(taps=np.ones(8194)), b"ntaps"), (dict(ntaps=-1), b"ntaps"),
    (dict(max_write_iq=0), b"max_write_iq"), (dict(max_write_iq=-5), b"max_write_iq"),
    (dict(ch_null=True), b"null"), (dict(taps_null=True), b"null"), (dict(out_null=True), b"null"),
    (dict(gains=(1.0, 0.0)), b"gain"), (dict(gains=(1.0, -2.0)), b"gain"), (dict(gains=(float("nan"), 1.0)), b"gain"),
    (dict(gains=(1.0, float("inf"))), b"gain"),
    (dict(taps=[0.5, float("nan"), 0.5]), b"tap"), (dict(taps=[float("inf")]), b"tap"),
])
def test_create_refusals_need_no_device(kw, word):
    """Every refusal of jaero_chan_create is JAERO_EINVAL before a device is looked for, and says what was wrong."""
    L = capi.lib()
    rc, h = _create(L, **kw)
    assert rc == capi.E_INVAL and not h.value
    assert word in L.jaero_last_error(), L.jaero_last_error()


def test_null_handles_are_refused():
    L = capi.lib()
    n, p = C.c_int(7), C.c_void_p()
    ms = C.c_double()
    ch = capi.ChanChannel(0, 0, 1.0)
    buf = np.zeros(8, np.int16)
    assert L.jaero_chan_write(None, buf.ctypes.data, 4, 0, None, C.byref(n)) == capi.E_INVAL
    assert b"jaero_chan_write" in L.jaero_last_error()
    assert L.jaero_chan_pcm_view(None, C.byref(p), C.byref(n)) == capi.E_INVAL
    assert L.jaero_chan_read_pcm(None, buf.ctypes.data, 4, C.byref(n)) == capi.E_INVAL
    assert L.jaero_chan_retune(None, 0, C.byref(ch)) == capi.E_INVAL
    assert L.jaero_chan_feed(None, None, buf.ctypes.data, 4, 0, None, C.byref(n)) == capi.E_INVAL
    assert L.jaero_chan_profile_enable(None, 1) == capi.E_INVAL
    assert L.jaero_chan_profile_read(None, 0, C.byref(ms), C.byref(n), 0) == capi.E_INVAL
    L.jaero_chan_destroy(None)  # a no-op


def test_no_cpu_fallback():
    """Without a HIP device a valid jaero_chan_create fails with ENODEV (never computes on the host)."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    L = capi.lib()
    rc, h = _create(L)
    assert rc == capi.E_NODEV and not h.value
    with pytest.raises(capi.JaeroError) as e:
        CH.Channeliser(16, [(0, 0, 1.0)], taps=np.ones(1))
    assert e.value.code == capi.E_NODEV


# ---------------------------------------------------------------------------------------------- words
@pytest.mark.parametrize("fs", [768000.0, 1536000.0, 3072000.0])
def test_tune_word_round_trip(fs):
    for hz in (0.0, 33.3, -123456.7, fs / 2 - 10000.0, -(fs / 2 - 10000.0), 200003.0, -0.01):
        w = CH.tune_word(hz, fs)
        assert 0 <= w < 1 << 32
        assert abs(CH.word_hz(w, fs) - hz) <= fs / 2 ** 33 * 1.0000001  # the nearest word
        assert CH.tune_word(CH.word_hz(w, fs), fs) == w
    assert CH.word_hz(1 << 31, fs) == -fs / 2 and CH.word_hz((1 << 32) - 1, fs) == -fs / 2 ** 32 and CH.word_hz(0, fs) == 0.0


@pytest.mark.parametrize("decim", CO.DECIMS)
def test_channel_words_agree_with_the_oracle_at_every_boundary(decim):
    for t in boundary_words():
        for audio in (0, 715827883, (1 << 32) - 1, 1 << 31):
            got = CH.channel_words(t, audio, decim)
            assert got == CO.words(t, audio, decim), (t, audio)
            b, rho, w = got
            ts = t - (1 << 32) if t >= 1 << 31 else t
            assert b * (1 << 18) + rho == ts and -(1 << 17) <= rho < (1 << 17) and -8192 <= b <= 8192 and 0 <= w < 1 << 32
            # the requested centre lands on the audio offset: bin b of the grid + w / D per output sample = tune, in words of the capture rate
            assert (b * (1 << 18) * decim + audio - w) % (1 << 32) == (ts * decim) % (1 << 32)


def test_design_taps():
    for decim in (16, 32, 64):
        h = CH.design_taps(decim)
        assert h.shape == (8193,) and abs(h.sum() - 1.0) < 1e-12 and np.allclose(h, h[::-1], rtol=0, atol=1e-18)
        H = np.abs(np.fft.rfft(h, 1 << 18))
        f = np.arange(len(H)) * 48000.0 * decim / (1 << 18)
        assert H[f < 6000.0].min() > 0.999 and H[f > 24000.0].max() < 1e-6  # flat over an OQPSK channel, gone where the next one aliases
    assert CH.design_taps(32, ntaps=1).tolist() == [1.0]


# ---------------------------------------------------------------------------------------------- oracle against itself
@pytest.mark.parametrize("decim", CO.DECIMS)
@pytest.mark.parametrize("centre", ["off_grid", "negative", "wrap_high", "wrap_low"])
def test_block_form_equals_direct_form(decim, centre):
    """max |block - direct| <= 1e-3 output LSB at the default taps of the output rate, at every decimation (measured: at most 5.2e-6 at
    48 kHz, 2.9e-5 at D = 128 and 1.3e-4 at D = 256; the bound keeps the two forms on the same int16 in all but ~0.2 % of samples).
    wrap_*: centres at +-(Fs_in / 2 - fs_out 10 / 48), 10 kHz from the edge at 48 kHz, whose run of bins wraps at N."""
    fs_out = FS_OUT[decim]
    fs = fs_out * decim
    edge = fs / 2 - fs_out * 10 / 48
    fc = {"off_grid": 33.3, "negative": -123456.7, "wrap_high": edge, "wrap_low": -edge}[centre]
    rng = np.random.default_rng(decim)
    nhops = 6
    x = tone_capture(decim, fs_out, CH.word_hz(CH.tune_word(fc, fs), fs), nhops, rng)
    tune, audio = CH.tune_word(fc, fs), CH.tune_word(fs_out / 6, fs_out)
    b, _, _ = CO.words(tune, audio, decim)
    M = CO.N // decim
    if centre.startswith("wrap"):
        assert b - M // 2 < -CO.N // 2 or b + M // 2 > CO.N // 2  # the run of bins crosses the seam of the spectrum
    h = CH.design_taps(decim, fs_out=fs_out)
    yb = CO.block_form(x, decim, [(tune, audio, 2.0)], h)[0]
    assert len(yb) == nhops * (M // 2)
    yd = CO.direct_form(x, decim, tune, audio, 2.0, h, len(yb))
    err = np.abs(yb - yd).max()
    print(f"D={decim} {centre}: max |block - direct| = {err:.3g} LSB, rms out {yb.std():.1f}")
    assert yb.std() > 100.0
    assert err <= 1e-3


@pytest.mark.parametrize("decim,audio_hz,gain", [(64, 8000.0, 0.04), (256, 2000.0, 0.1)])
def test_oracle_in_pieces_equals_oracle_at_once(decim, audio_hz, gain):
    rng = np.random.default_rng(5)
    fs_out = FS_OUT[decim]
    x = rng.integers(-32768, 32768, 5 * CO.HP + 77) + 1j * rng.integers(-32768, 32768, 5 * CO.HP + 77)
    chans = [(CH.tune_word(-300000.3, fs_out * decim), CH.tune_word(audio_hz, fs_out), gain), (12345678, 999, 1.0)]
    h = CH.design_taps(decim, ntaps=2049, beta=10.0, fs_out=fs_out)
    whole = CO.block_form(x, decim, chans, h)
    o = CO.ChanOracle(decim, chans, h)
    parts, pos, total = [], 0, 0
    for n in (1, 8191, 8193, 0, 3 * 8192 + 5, 77, 8000, 10 ** 6):
        parts.append(o.write(x[pos:pos + n]))
        pos = min(len(x), pos + n)
        total += parts[-1].shape[1]
        assert total == (pos // CO.HP) * o.Mo
    got = np.concatenate(parts, axis=1)
    assert got.shape == whole.shape and np.array_equal(got, whole)
