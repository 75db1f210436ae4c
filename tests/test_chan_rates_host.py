"""CPU: the channeliser at total decimations 128 / 256 and output rates 24 / 12 kHz (jaero_chan2_create) without a device: the export, the
refusals, no CPU fallback and the default taps of the Python helpers.  The integer frequency arithmetic and the oracle against itself at
these decimations are cases of tests/test_chan_host.py's tests."""
import ctypes as C

import numpy as np
import pytest

from jaero_amd import capi, channeliser as CH


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


# ---------------------------------------------------------------------------------------------- taps
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
