"""CPU: the capture front end's C ABI without a device (exports, refusals in their documented order, no CPU fallback), the resampler design,
and the oracle (tests/chan_capture_oracle.py) against itself -- fed in ragged pieces against fed at once -- and against ideal tones."""
import ctypes as C

import numpy as np
import pytest

import chan_capture_oracle as CC
from jaero_amd import capi, channeliser as CH

SYMBOLS = ["jaero_chan3_create", "jaero_chan3_write", "jaero_chan3_feed", "jaero_chan3_read_staged", "jaero_chan3_profile_read"]


def test_library_exports_the_five_symbols():
    L = capi.lib()
    for name in SYMBOLS:
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert C.sizeof(capi.Capture) == 24  # 2 int + uint32 + int + pointer
    assert L.jaero_abi_version() == 1


def _create(L, fmt=capi.IQ_CU8, fs_in=1200000, K=32, rtaps="design", cap_null=False, decim=16, out_rate=48000, nch=2, gains=(1.0, 1.0),
            taps=None, max_write_iq=8192, out_null=False, ch_null=False):
    arr = (capi.ChanChannel * max(nch, 1))(*[capi.ChanChannel(1000 * i, 715827883, g) for i, g in zip(range(max(nch, 1)), gains)])
    t = np.ones(3) / 3 if taps is None else np.asarray(taps, dtype=np.float64)
    if isinstance(rtaps, str):
        Lr = CC.ratio(max(fs_in, 1), 768000)[0]
        rt = np.ones(min(Lr, 4096) * max(K, 1)) / max(K, 1)
    else:
        rt = rtaps
    cap = capi.Capture(fmt, fs_in, 0, K, None if rt is None else rt.ctypes.data)
    h = C.c_void_p()
    rc = L.jaero_chan3_create(0, None if cap_null else C.byref(cap), decim, out_rate, nch, None if ch_null else C.cast(arr, C.c_void_p),
                              t.ctypes.data, t.size, max_write_iq, None if out_null else C.byref(h))
    return rc, h


BAD_RT = np.ones(16 * 32)
BAD_RT[100] = np.nan


@pytest.mark.parametrize("kw,word", [
    (dict(out_null=True, cap_null=True), b"out is null"),
    (dict(cap_null=True, fmt=9, decim=7), b"cap is null"),
    (dict(fmt=4, fs_in=0), b"format"), (dict(fmt=-1), b"format"),
    (dict(fs_in=0, K=0), b"fs_in"), (dict(fs_in=-5), b"fs_in"),
    (dict(fs_in=1200001, K=0), b"L above 1024"),          # 768000 / 1200001 is in lowest terms
    (dict(fs_in=95999, K=0), b"L above 1024"),            # L is checked before the ratio
    (dict(fs_in=768000 * 8 + 768, K=0), b"beyond 8"),     # 1000 / 8001
    (dict(fs_in=95000, K=0), b"beyond 8"),                # 768 / 95: Fs_c > 8 fs_in
    (dict(K=0, rtaps=None), b"taps_per_phase"), (dict(K=65), b"taps_per_phase"), (dict(K=-1), b"taps_per_phase"),
    (dict(rtaps=None, decim=7), b"rtaps"),
    (dict(rtaps=BAD_RT, nch=0), b"resampler tap 100"),
    # behind the capture's checks: jaero_chan2_create's own, in its order
    (dict(ch_null=True, decim=16), b"null"),
    (dict(fs_in=1280, decim=128, out_rate=5), b"out_rate"),   # Fs_c = 640: 1 / 2
    (dict(fs_in=768000, decim=8), b"decim"),
    (dict(nch=0), b"nchannels"), (dict(taps=np.ones(8194)), b"ntaps"), (dict(max_write_iq=0), b"max_write_iq"),
    (dict(gains=(1.0, 0.0)), b"gain"), (dict(taps=[0.5, float("nan")]), b"tap 1"),
    # last, still without a device: a write that would stage 2^31 samples or more (8 / 1 x 2^28; equal rates x (2^31 - 1))
    (dict(fs_in=96000, max_write_iq=1 << 28), b"stages"), (dict(fs_in=768000, max_write_iq=(1 << 31) - 1), b"stages"),
    (dict(fs_in=96000, max_write_iq=1 << 28, gains=(1.0, -1.0)), b"gain"),
])
def test_create_refusals_need_no_device_and_come_in_order(kw, word):
    """Every refusal is JAERO_EINVAL before a device is looked for; where two things are wrong the documented order decides which is named."""
    L = capi.lib()
    rc, h = _create(L, **kw)
    assert rc == capi.E_INVAL and not h.value
    assert word in L.jaero_last_error(), L.jaero_last_error()


def test_equal_rates_ignore_k_and_rtaps():
    """fs_in == out_rate x decim: K and rtaps are not looked at; the valid call then needs a device."""
    L = capi.lib()
    rc, h = _create(L, fs_in=768000, K=-3, rtaps=None)
    assert rc in (capi.E_OK, capi.E_NODEV)
    if rc == capi.E_OK:
        L.jaero_chan_destroy(h)


def test_null_handles_are_refused():
    L = capi.lib()
    n, first, ms = C.c_int(7), C.c_longlong(0), C.c_double()
    buf = np.zeros(8, np.float64)
    assert L.jaero_chan3_write(None, buf.ctypes.data, 2, 0, None, C.byref(n)) == capi.E_INVAL
    assert b"jaero_chan3_write" in L.jaero_last_error()
    assert L.jaero_chan3_feed(None, None, buf.ctypes.data, 2, 0, None, C.byref(n)) == capi.E_INVAL
    assert b"jaero_chan3_feed" in L.jaero_last_error()
    assert L.jaero_chan3_read_staged(None, buf.ctypes.data, 4, C.byref(n), C.byref(first)) == capi.E_INVAL
    assert L.jaero_chan3_profile_read(None, 0, C.byref(ms), C.byref(n), 0) == capi.E_INVAL


def test_no_cpu_fallback():
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
        CH.Channeliser(16, [(0, 0, 1.0)], taps=np.ones(1), capture=CH.Capture(fs_in=2400000, fmt="cu8"))
    assert e.value.code == capi.E_NODEV
    with pytest.raises(capi.JaeroError) as e:
        CH.Channeliser(16, [(0, 0, 1.0)], taps=np.ones(1), capture=CH.Capture(fs_in=768001, fmt="cf32"))
    assert e.value.code == capi.E_INVAL


# ---------------------------------------------------------------------------------------------- design
@pytest.mark.parametrize("fs_in,fs_c,want", [(2400000, 3072000, (32, 25)), (2500000, 3072000, (768, 625)), (10000000, 3072000, (192, 625)),
                                             (1200000, 768000, (16, 25)), (2048000, 1536000, (3, 4)), (768000, 768000, (1, 1))])
def test_design_resampler_reduces_the_ratio(fs_in, fs_c, want):
    h, L, Mr = CH.design_resampler(fs_in, fs_c, 32)
    assert (L, Mr) == want == CC.ratio(fs_in, fs_c) == CH.resample_ratio(fs_in, fs_c)
    assert h.shape == (L * 32,) and abs(h.sum() - L) < 1e-9 * L
    assert np.allclose(h, h[::-1], rtol=0, atol=1e-15)


@pytest.mark.parametrize("fs_in,fs_c", [(2400000, 3072000), (2048000, 1536000), (1200000, 768000), (2500000, 3072000), (10000000, 3072000),
                                        (1920000, 768000), (6000000, 3072000)])
def test_every_phase_has_unit_dc_gain(fs_in, fs_c):
    """sum_j h[phi + j L] = 1 within the prototype's ripple: the images of DC at multiples of fs_in lie in the stop band of a Kaiser window
    of beta = 10 (about -100 dB, 1e-5); the bound is 1e-4.  And S = max_phi sum_j |h| stays below 2.5 (2.32 was the largest met)."""
    h, L, Mr = CH.design_resampler(fs_in, fs_c, 32, 10.0)
    dc = h.reshape(-1, L).sum(axis=0)
    S = CC.gain_bound(h, L)
    print(f"{fs_in} -> {fs_c}: L / Mr = {L} / {Mr}, max |phase DC gain - 1| = {np.abs(dc - 1).max():.3g}, S = {S:.4f}")
    assert np.abs(dc - 1.0).max() < 1e-4
    assert 1.0 <= S < 2.5


# ---------------------------------------------------------------------------------------------- oracle against itself
@pytest.mark.parametrize("K", [1, 2, 32, 64])
@pytest.mark.parametrize("fs_in,fs_c", [(1200000, 768000), (2400000, 3072000)])
def test_oracle_resampler_in_pieces_equals_at_once(K, fs_in, fs_c):
    rng = np.random.default_rng(K)
    h, L, Mr = CH.design_resampler(fs_in, fs_c, K)
    n = 20000
    re, im = rng.integers(-32768, 32768, n).astype(float), rng.integers(-32768, 32768, n).astype(float)
    wr, wi = CC.Resampler(h, L, Mr, K).write(re, im)
    assert len(wr) == -(-n * L // Mr)
    r = CC.Resampler(h, L, Mr, K)
    pr, pi, pos = [], [], 0
    for k in [0, 1, max(K - 2, 0), max(K - 1, 0), K, 1, 0, 3, 2 * K + 1, 777, 1, 1, 1, 5000, 24, 25, 26, 10 ** 9]:
        a, b = r.write(re[pos:pos + k], im[pos:pos + k])
        pos = min(n, pos + k)
        pr.append(a); pi.append(b)
        assert r.m == sum(len(p) for p in pr) == -(-pos * L // Mr), (pos, r.m)  # ceil(T L / Mr) after every piece
        assert r.T == pos
    assert pos == n
    assert np.array_equal(np.concatenate(pr), wr) and np.array_equal(np.concatenate(pi), wi)


def test_capture_oracle_in_pieces_with_shift():
    """convert, mix and resample together: the phase is a function of the absolute index, so the pieces see the same rotation."""
    rng = np.random.default_rng(3)
    K = 32
    h, L, Mr = CH.design_resampler(1200000, 768000, K)
    raw = rng.integers(0, 256, size=(9000, 2), dtype=np.uint8)
    shift = CH.tune_word(-123456.7, 1200000.0)
    whole = CC.CaptureOracle("cu8", 1200000, 768000, shift, K, h).write(raw)
    o = CC.CaptureOracle("cu8", 1200000, 768000, shift, K, h)
    parts, firsts, pos = [], [], 0
    for k in (1, 30, 31, 32, 0, 4000, 4906):
        parts.append(o.write(raw[pos:pos + k]))
        firsts.append(o.first)
        pos += k
    assert pos == len(raw) and firsts[0] == 0 and firsts[-1] == sum(len(p) for p in parts[:-1])
    assert np.array_equal(np.concatenate(parts), whole)
    # shift == 0 leaves the converted samples untouched, -0.0 included
    re, im = CC.mix(np.array([-0.0, 3.0]), np.array([1.0, -0.0]), 0, 12345)
    assert np.signbit(re[0]) and np.signbit(im[1])


def test_conversions():
    assert [c.tolist() for c in CC.convert(np.array([[0, 255], [127, 128]], np.uint8), CC.CU8)] == [[-32640.0, -128.0], [32640.0, 128.0]]
    assert [c.tolist() for c in CC.convert(np.array([[-128, 127], [0, -1]], np.int8), CC.CS8)] == [[-32768.0, 0.0], [32512.0, -256.0]]
    assert [c.tolist() for c in CC.convert(np.array([[-32768, 32767]], np.int16), CC.CS16)] == [[-32768.0], [32767.0]]
    re, im = CC.convert(np.array([[np.nan, np.inf], [-np.inf, 1.5], [-0.0, 2.0 ** -20]], np.float32), CC.CF32)
    assert re.tolist() == [0.0, 0.0, -0.0] and im.tolist() == [0.0, 49152.0, 2.0 ** -5] and np.signbit(re[2])


# ---------------------------------------------------------------------------------------------- oracle against ideal tones
def _tone_levels(K=32, beta=10.0):
    """1.2 MS/s -> 768 kS/s.  (a) a tone at 100 kHz of amplitude 10000 against the ideal tone at the output rate, delayed by the group delay
    (L K - 1) / (2 L fs_in): max |z - ideal| / amplitude over the settled part.  (b) a tone at 500 kHz (beyond the new Nyquist frequency of
    384 kHz; it would alias to -268 kHz): RMS out / amplitude, in dB."""
    fs_in, fs_c, A = 1200000, 768000, 10000.0
    h, L, Mr = CH.design_resampler(fs_in, fs_c, K, beta)
    n = np.arange(60000)
    out = []
    for f in (100000.0, 500000.0):
        x = A * np.exp(2j * np.pi * ((f / fs_in * n) % 1.0))
        zr, zi = CC.Resampler(h, L, Mr, K).write(x.real, x.imag)
        out.append((f, (zr + 1j * zi)[2 * K:]))
    f, z = out[0]
    m = np.arange(len(out[0][1])) + 2 * K
    delay = (L * K - 1) / (2.0 * L * fs_in)
    ideal = A * np.exp(2j * np.pi * (f * (m / fs_c - delay)))
    follow = float(np.abs(z - ideal).max() / A)
    alias_db = float(20 * np.log10(np.sqrt(np.mean(np.abs(out[1][1]) ** 2)) / A))
    return follow, alias_db


def test_tone_follows_the_ideal_and_alias_is_suppressed():
    """Measured with this numpy oracle at K = 32, beta = 10: the pass-band tone follows the ideal delayed tone within 8.96e-6 of its
    amplitude, the 500 kHz tone comes out at -83.5 dB.  Asserted with a factor 2: 1.8e-5 and -77.5 dB (a factor 2 in amplitude is 6 dB)."""
    follow, alias_db = _tone_levels()
    print(f"pass-band tone: max |z - ideal| / A = {follow:.3g}; 500 kHz tone: {alias_db:.1f} dB")
    assert follow <= 1.8e-5
    assert alias_db <= -77.5
