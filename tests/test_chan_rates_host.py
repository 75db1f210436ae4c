"""CPU: the channeliser at total decimations 128 / 256 and output rates 24 / 12 kHz (jaero_chan2_create) without a device: the export, the
refusals, no CPU fallback, the integer frequency arithmetic and the default taps of the Python helpers, and the oracle at the new
decimations against itself (block form against mix -> FIR -> decimate, fed in pieces against fed at once)."""
import ctypes as C

import numpy as np
import pytest

import chan_rates_oracle as RO
from jaero_amd import capi, channeliser as CH
from test_chan_host import _boundary_words


def test_library_exports_the_new_entry():
    assert "jaero_chan2_create" in capi.EXPORTS
    assert hasattr(capi.lib(), "jaero_chan2_create")
    assert capi.lib().jaero_abi_version() == 1
    assert CH.DECIMS == (16, 32, 64, 128, 256)


def _create2(L, decim=128, out_rate=24000, nch=2, gains=(1.0, 1.0), taps=None, ntaps=None, max_write_iq=8192, ch_null=False,
             taps_null=False, out_null=False):
    arr = (capi.ChanChannel * max(nch, 1))(*[capi.ChanChannel(1000 * i, 715827883, g) for i, g in zip(range(max(nch, 1)), gains)])
    t = np.ones(3) / 3 if taps is None else np.asarray(taps, dtype=np.float64)
    h = C.c_void_p()
    rc = L.jaero_chan2_create(0, decim, out_rate, nch, None if ch_null else C.cast(arr, C.c_void_p), None if taps_null else t.ctypes.data,
                              t.size if ntaps is None else ntaps, max_write_iq, None if out_null else C.byref(h))
    return rc, h


@pytest.mark.parametrize("kw,word", [
    (dict(decim=8), b"decim"), (dict(decim=48), b"decim"), (dict(decim=512), b"decim"),
    (dict(out_rate=0), b"out_rate"), (dict(out_rate=44100), b"out_rate"), (dict(out_rate=96000), b"out_rate"),
    (dict(nch=0), b"nchannels"), (dict(nch=-3), b"nchannels"),
    (dict(ntaps=0), b"ntaps"), (dict(taps=np.ones(8194)), b"ntaps"), (dict(ntaps=-1), b"ntaps"),
    (dict(max_write_iq=0), b"max_write_iq"), (dict(max_write_iq=-5), b"max_write_iq"),
    (dict(ch_null=True), b"null"), (dict(taps_null=True), b"null"), (dict(out_null=True), b"null"),
    (dict(gains=(1.0, 0.0)), b"gain"), (dict(gains=(1.0, -2.0)), b"gain"), (dict(gains=(float("nan"), 1.0)), b"gain"),
    (dict(gains=(1.0, float("inf"))), b"gain"),
    (dict(taps=[0.5, float("nan"), 0.5]), b"tap"), (dict(taps=[float("inf")]), b"tap"),
])
def test_create2_refusals_need_no_device(kw, word):
    """Every refusal of jaero_chan2_create is JAERO_EINVAL before a device is looked for, and says what was wrong."""
    L = capi.lib()
    rc, h = _create2(L, **kw)
    assert rc == capi.E_INVAL and not h.value
    assert word in L.jaero_last_error(), L.jaero_last_error()


@pytest.mark.parametrize("decim,out_rate", [(16, 48000), (64, 12000), (128, 24000), (128, 12000), (256, 12000), (256, 48000)])
def test_no_cpu_fallback(decim, out_rate):
    """Without a HIP device a valid jaero_chan2_create fails with ENODEV (never computes on the host)."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    L = capi.lib()
    rc, h = _create2(L, decim=decim, out_rate=out_rate)
    assert rc == capi.E_NODEV and not h.value
    with pytest.raises(capi.JaeroError) as e:
        CH.Channeliser(decim, [(0, 0, 1.0)], taps=np.ones(1), fs_out=float(out_rate))
    assert e.value.code == capi.E_NODEV


def test_python_wrapper_passes_the_rate_on():
    """Channeliser(fs_out=...) is refused for a rate that is none of the three, by the library, before a device is looked for."""
    for bad in (44100.0, 12000.5, 0.0):
        with pytest.raises(capi.JaeroError) as e:
            CH.Channeliser(128, [(0, 0, 1.0)], taps=np.ones(1), fs_out=bad)
        assert e.value.code == capi.E_INVAL and "out_rate" in str(e.value)
    with pytest.raises(capi.JaeroError) as e:
        CH.Channeliser(512, [(0, 0, 1.0)], taps=np.ones(1), fs_out=12000.0)
    assert e.value.code == capi.E_INVAL and "decim" in str(e.value)


# ---------------------------------------------------------------------------------------------- words
@pytest.mark.parametrize("decim", [128, 256])
def test_channel_words_agree_with_the_oracle_at_every_boundary(decim):
    for t in _boundary_words():
        for audio in (0, 715827883, (1 << 32) - 1, 1 << 31):
            got = CH.channel_words(t, audio, decim)
            assert got == RO.words(t, audio, decim), (t, audio)
            b, rho, w = got
            ts = t - (1 << 32) if t >= 1 << 31 else t
            assert b * (1 << 18) + rho == ts and -(1 << 17) <= rho < (1 << 17) and -8192 <= b <= 8192 and 0 <= w < 1 << 32
            assert (b * (1 << 18) * decim + audio - w) % (1 << 32) == (ts * decim) % (1 << 32)


@pytest.mark.parametrize("decim,fs_out", [(64, 12000.0), (128, 12000.0), (256, 12000.0), (32, 24000.0), (128, 24000.0)])
def test_default_taps(decim, fs_out):
    h = CH.design_taps(decim, fs_out=fs_out)
    assert h.shape == (8193,) and abs(h.sum() - 1.0) < 1e-12 and np.allclose(h, h[::-1], rtol=0, atol=1e-18)
    H = np.abs(np.fft.rfft(h, 1 << 18))
    f = np.arange(len(H)) * fs_out * decim / (1 << 18)
    print(f"D={decim} fs_out={fs_out}: pass band min {H[f < fs_out / 8].min():.9f}, stop band max {H[f > fs_out / 2].max():.3g}")
    assert H[f < fs_out / 8].min() > 0.999 and H[f > fs_out / 2].max() < 1e-6
    assert np.array_equal(h, CH.design_taps(decim, cutoff_hz=0.3125 * fs_out, fs_out=fs_out))


def test_default_taps_at_48_khz_are_unchanged():
    """design_taps(32) is what it was before the output rate became an argument: 2 fc sinc(2 fc k) kaiser(16) with fc = 9000 / (48000 x 32)."""
    fc = 9000.0 / (48000.0 * 32)
    k = np.arange(8193) - (8193 - 1) / 2
    old = 2 * fc * np.sinc(2 * fc * k) * np.kaiser(8193, 16.0)
    old = old / old.sum()
    assert np.array_equal(CH.design_taps(32), old)
    assert np.array_equal(CH.design_taps(32, 9000.0), old) and np.array_equal(CH.design_taps(32, fs_out=48000.0), old)
    assert CH.design_taps(256, ntaps=1, fs_out=12000.0).tolist() == [1.0]


# ---------------------------------------------------------------------------------------------- oracle against itself
def _capture(decim, fs_out, fc, nhops, rng):
    """tests/test_chan_host.py's input scaled to the output rate: a tone of 3000 LSB fs_out / 32 above the centre, one of 9000 LSB
    fs_out 40 / 48 above it (outside the +-fs_out / 2 the channel keeps), noise of 300 LSB per rail; rounded to integers."""
    fs = fs_out * decim
    n = RO.HP * nhops
    t = np.arange(n)
    x = (3000 * np.exp(2j * np.pi * (((fc + fs_out / 32) / fs * t) % 1.0)) + 9000 * np.exp(2j * np.pi * (((fc + fs_out * 40 / 48) / fs * t) % 1.0))
         + 300 * (rng.normal(size=n) + 1j * rng.normal(size=n)))
    return np.rint(x.real) + 1j * np.rint(x.imag)


@pytest.mark.parametrize("decim,fs_out", [(128, 24000.0), (256, 12000.0)])
@pytest.mark.parametrize("centre", ["off_grid", "negative", "wrap_high", "wrap_low"])
def test_block_form_equals_direct_form(decim, fs_out, centre):
    """max |block - direct| <= 1e-3 output LSB at the default taps, the bound of the 48 kHz test (measured: at most 2.9e-5 at D = 128 and
    1.3e-4 at D = 256).  wrap_*: centres at +-(Fs_in / 2 - fs_out 10 / 48), whose run of bins wraps at N."""
    fs = fs_out * decim
    edge = fs / 2 - fs_out * 10 / 48
    fc = {"off_grid": 33.3, "negative": -123456.7, "wrap_high": edge, "wrap_low": -edge}[centre]
    rng = np.random.default_rng(decim)
    nhops = 6
    x = _capture(decim, fs_out, CH.word_hz(CH.tune_word(fc, fs), fs), nhops, rng)
    tune, audio = CH.tune_word(fc, fs), CH.tune_word(fs_out / 6, fs_out)
    b, _, _ = RO.words(tune, audio, decim)
    M = RO.N // decim
    if centre.startswith("wrap"):
        assert b - M // 2 < -RO.N // 2 or b + M // 2 > RO.N // 2  # the run of bins crosses the seam of the spectrum
    h = CH.design_taps(decim, fs_out=fs_out)
    yb = RO.block_form(x, decim, [(tune, audio, 2.0)], h)[0]
    assert len(yb) == nhops * (M // 2)
    yd = RO.direct_form(x, decim, tune, audio, 2.0, h, len(yb))
    err = np.abs(yb - yd).max()
    print(f"D={decim} {centre}: max |block - direct| = {err:.3g} LSB, rms out {yb.std():.1f}")
    assert yb.std() > 100.0
    assert err <= 1e-3


def test_oracle_in_pieces_equals_oracle_at_once():
    rng = np.random.default_rng(5)
    decim, fs_out = 256, 12000.0
    x = rng.integers(-32768, 32768, 5 * RO.HP + 77) + 1j * rng.integers(-32768, 32768, 5 * RO.HP + 77)
    chans = [(CH.tune_word(-300000.3, fs_out * decim), CH.tune_word(2000.0, fs_out), 0.1), (12345678, 999, 1.0)]
    h = CH.design_taps(decim, ntaps=2049, beta=10.0, fs_out=fs_out)
    whole = RO.block_form(x, decim, chans, h)
    o = RO.ChanRatesOracle(decim, chans, h)
    parts, pos, total = [], 0, 0
    for n in (1, 8191, 8193, 0, 3 * 8192 + 5, 77, 8000, 10 ** 6):
        parts.append(o.write(x[pos:pos + n]))
        pos = min(len(x), pos + n)
        total += parts[-1].shape[1]
        assert total == (pos // RO.HP) * o.Mo
    got = np.concatenate(parts, axis=1)
    assert got.shape == whole.shape and np.array_equal(got, whole)
