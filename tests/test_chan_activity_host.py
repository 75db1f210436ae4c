"""CPU: the channeliser's activity (jaero_activity_*) without a device -- the exports and what is refused before a device is looked
for -- then its numpy definition (tests/chan_activity_oracle.py) against itself, and the case it exists for: a carrier that is on in three
hops of 64, which the survey's mean spectrum does not show and the peak-hold spectrum does."""
import ctypes as C

import numpy as np
import pytest

import chan_activity_cases as AC
import chan_activity_oracle as AO
import chan_oracle as CO
from chan_cases import AUDIO
from jaero_amd import capi, channeliser as CH

N, HP = AO.N, AO.HP
ACTIVITY_SYMBOLS = ("jaero_activity_enable", "jaero_activity_reset", "jaero_activity_read_peak", "jaero_activity_read_blocks",
                    "jaero_activity_profile_read")


def test_exports_and_refusals_without_a_device():
    L = capi.lib()
    for name in ACTIVITY_SYMBOLS:
        assert name in capi.EXPORTS and hasattr(L, name), name
        assert not name.startswith("jaero_chan_")  # tests/test_chan_host.py pins that set
    assert L.jaero_abi_version() == 1
    assert (capi.ACT_PEAK, capi.ACT_BLOCKS, capi.ACT_BINS) == (1, 2, 64)
    buf, n = np.zeros(N), C.c_longlong(0)
    hist = np.zeros(64, dtype=np.uint32)
    ms, k = C.c_double(0), C.c_int(0)
    for bad in (4, -1, 7):
        assert L.jaero_activity_enable(None, bad) == capi.E_INVAL
        assert "outside 0..3" in L.jaero_last_error().decode()  # the bits are checked before the null ctx, as jaero_survey_enable does
    assert L.jaero_activity_enable(None, 3) == capi.E_INVAL
    assert "null" in L.jaero_last_error().decode()
    assert L.jaero_activity_reset(None) == capi.E_INVAL
    assert L.jaero_activity_read_peak(None, buf.ctypes.data, C.byref(n)) == capi.E_INVAL
    p = buf.ctypes.data
    assert L.jaero_activity_read_blocks(None, p, p, p, p, hist.ctypes.data) == capi.E_INVAL
    assert L.jaero_activity_read_blocks(None, p, p, p, p, None) == capi.E_INVAL
    assert L.jaero_activity_profile_read(None, 0, C.byref(ms), C.byref(k), 0) == capi.E_INVAL
    # the survey's own refusals are what they were
    assert L.jaero_survey_enable(None, 4) == capi.E_INVAL and "jaero_survey_enable: what 4 has bits outside 0..3" in L.jaero_last_error().decode()
    for name in ("activity_enable", "activity_reset", "read_peak_sums", "read_peak_psd", "read_activity", "activity_profile_read"):
        assert callable(getattr(CH.Channeliser, name))
    assert CH.Activity._fields == ("emax", "emin", "when", "n", "hist") and callable(CH.duty_cycle)


def test_bin_is_the_exponent():
    """bin(e) = min(63, max(0, ilogb(e) + 32)), bin(0) = 0, on both sides of every edge"""
    assert AO.act_bin(0.0) == 0 and AO.act_bin(5e-324) == 0 and AO.act_bin(2.0 ** -33) == 0 and AO.act_bin(2.0 ** -32) == 0
    assert AO.act_bin(np.nextafter(2.0 ** -31, 0)) == 0 and AO.act_bin(2.0 ** -31) == 1
    for i in range(1, 63):
        assert AO.act_bin(2.0 ** (i - 32)) == i and AO.act_bin(np.nextafter(2.0 ** (i - 32), 0)) == i - 1
        assert AO.act_bin(1.5 * 2.0 ** (i - 32)) == i
    assert AO.act_bin(2.0 ** 31) == 63 and AO.act_bin(2.0 ** 40) == 63 and AO.act_bin(1e300) == 63


def white(n, seed, amp=8000.0):
    rng = np.random.default_rng(seed)
    return np.rint(amp * (rng.normal(size=n) + 1j * rng.normal(size=n)) / np.sqrt(2.0))


def same_activity(a, b):
    return (np.array_equal(a.P, b.P) and a.peak_blocks == b.peak_blocks and np.array_equal(a.emax, b.emax) and np.array_equal(a.emin, b.emin)
            and np.array_equal(a.when, b.when) and np.array_equal(a.an, b.an) and np.array_equal(a.hist, b.hist))


def test_fed_in_pieces_equals_fed_at_once_exactly():
    decim, fs = 64, 48000.0 * 64
    x = white(6 * HP + 77, 2)
    x[2 * HP:3 * HP] *= 3.0  # a louder hop, so that the extremes are not an accident of the noise
    chans = [(CH.tune_word(f, fs), AUDIO, 1.0) for f in (33.3, -123456.7, fs / 2 - 1.0)]
    taps = CH.design_taps(decim, ntaps=2049, beta=10.0)
    whole, pieces = AO.ChanActivityOracle(decim, chans, taps), AO.ChanActivityOracle(decim, chans, taps)
    assert whole.survey(x) == 6
    pos = 0
    for n in AC.CUTS:
        pieces.survey(x[pos:pos + n])
        pos += n
    assert same_activity(whole, pieces) and whole.peak_blocks == 6 and (whole.an == 6).all()
    assert np.array_equal(pieces.S, whole.S) and np.array_equal(pieces.E, whole.E)  # the survey beside it is what it was
    base = AO.SO.ChanSurveyOracle(decim, chans, taps)
    base.survey(x)
    assert np.array_equal(base.S, whole.S) and np.array_equal(base.E, whole.E) and np.array_equal(base.n, whole.n)
    # what the definition implies
    assert (whole.hist.sum(axis=1) == whole.an).all()
    assert (whole.P >= whole.S / whole.nblocks).all() and (whole.P <= whole.S).all()
    mean = whole.E / whole.n
    assert (whole.emin <= mean).all() and (mean <= whole.emax).all() and (whole.emin < whole.emax).all()
    assert set(whole.when.tolist()) <= {2, 3}  # the louder hop lies in blocks 2 and 3
    terms = whole.block_terms(x)
    assert np.array_equal(terms.max(axis=1), whole.emax) and np.array_equal(terms.min(axis=1), whole.emin)
    assert np.array_equal(terms.argmax(axis=1), whole.when)
    # after one block everything is that block's term
    one = AO.ChanActivityOracle(decim, chans, taps)
    assert one.survey(x[:HP]) == 1
    assert np.array_equal(one.P, one.S) and np.array_equal(one.emax, one.E) and np.array_equal(one.emin, one.E) and (one.when == 0).all()
    # the restart of exactly the channel whose tune word changes; audio- and gain-only retunes restart nothing
    twin = AO.ChanActivityOracle(decim, chans, taps)
    twin.survey(x[:2 * HP])
    twin.retune(0, chans[0][0], AUDIO + 5, 0.5)
    twin.retune(1, CH.tune_word(50000.0, fs), AUDIO, 1.0)
    assert twin.an.tolist() == [2, 0, 2] and twin.emax[1] == 0.0 and twin.emin[1] == np.inf and twin.when[1] == -1 and not twin.hist[1].any()
    twin.survey(x[2 * HP:])
    assert twin.an.tolist() == [6, 4, 6] and twin.n.tolist() == [6, 4, 6]
    for c in (0, 2):
        assert twin.emax[c] == whole.emax[c] and twin.emin[c] == whole.emin[c] and twin.when[c] == whole.when[c]
        assert np.array_equal(twin.hist[c], whole.hist[c])
    assert twin.emax[1] != whole.emax[1] and twin.when[1] >= 2 and twin.hist[1].sum() == 4
    assert np.array_equal(twin.P, whole.P)  # no retune touches the peak-hold spectrum
    # the two resets are independent; the values of a channel without a block
    twin.activity_reset()
    assert twin.nblocks == 6 and np.array_equal(twin.S, whole.S) and twin.n.tolist() == [6, 4, 6]
    assert not twin.P.any() and twin.peak_blocks == 0 and not twin.an.any() and not twin.hist.any()
    assert (twin.emax == 0.0).all() and (twin.emin == np.inf).all() and (twin.when == -1).all()
    assert np.isnan(CH.duty_cycle(twin.hist)).all()
    twin.survey(x[:HP])
    twin.reset()
    assert twin.nblocks == 0 and not twin.S.any() and twin.peak_blocks == 1 and (twin.an == 1).all() and (twin.when == 6).all()


def test_duty_cycle():
    h = np.zeros((5, 64), dtype=np.uint32)
    h[0, 46], h[0, 48], h[0, 49] = 60, 2, 2          # a floor and four blocks two and three bins above it
    h[1, 50] = 64                                      # always on: its own signal is its floor
    h[2, 10], h[2, 11], h[2, 12] = 5, 5, 1             # a tie: the lower bin is the floor
    h[4, 63], h[4, 0] = 1, 3
    d = CH.duty_cycle(h)
    assert d[0] == 4 / 64 and d[1] == 0.0 and d[2] == 1 / 11 and np.isnan(d[3]) and d[4] == 0.25
    assert CH.duty_cycle(h, rise_bins=3)[0] == 2 / 64 and CH.duty_cycle(h, rise_bins=1)[2] == 6 / 11
    assert CH.duty_cycle(h[0]) == 4 / 64 and np.isnan(CH.duty_cycle(h[3]))


@pytest.fixture(scope="module")
def discovery():
    """The discovery capture through the oracle, once: channels on the burst carrier, on the carrier that is always on, on noise."""
    o = AO.ChanActivityOracle(AC.DISC_DECIM, AC.discovery_channels(), CH.design_taps(AC.DISC_DECIM))
    assert o.survey(CO.as_complex(AC.discovery_capture())) == AC.DISC_HOPS
    return o


def test_discovery_of_a_burst_carrier(discovery):
    """D = 16, 64 blocks of white noise, two band-limited 8 kHz carriers 15 dB above the noise per bin: +100 kHz always on, -150 kHz on in
    hops 30 .. 32 only.  find_carriers at its default threshold finds one carrier in the mean spectrum and both in the peak-hold spectrum,
    each within 250 Hz.  The peak-hold result was checked on the oracle at thresholds of 3, 4, 6 and 8 dB and holds at all four (at
    12 dB per bin it holds at 3 .. 6 and not at 8, which is why the carriers are 15 dB); at 10 dB the burst carrier is lost.  The centroid of a
    noise-like carrier seen for three hops is itself noisy: over the capture's seeds 1 .. 12 the burst carrier was found 38 .. 260 Hz
    off (RMS 180 Hz, 9 of 12 within 250 Hz; both carriers were found at 3 .. 8 dB at all 12); the capture is seed 1, 72 Hz off.
    Block terms: the burst channel's largest is 8.8 x its mean, the other two channels' 1.13 x."""
    o = discovery
    mean = CH.find_carriers(o.psd(), AC.DISC_FS, 10500.0)
    peak = CH.find_carriers(o.peak_psd(), AC.DISC_FS, 10500.0)
    print("mean spectrum:", np.round(mean, 1), " peak-hold spectrum:", np.round(peak, 1))
    assert len(mean) == 1 and abs(mean[0] - AC.DISC_ON_HZ) <= 250.0
    assert len(peak) == 2 and abs(peak[0] - AC.DISC_BURST_HZ) <= 250.0 and abs(peak[1] - AC.DISC_ON_HZ) <= 250.0
    for thr in (3.0, 4.0, 8.0):
        f = CH.find_carriers(o.peak_psd(), AC.DISC_FS, 10500.0, thr)
        assert len(f) == 2 and abs(f[0] - AC.DISC_BURST_HZ) <= 250.0 and abs(f[1] - AC.DISC_ON_HZ) <= 250.0, (thr, f)
    ratio = o.emax / (o.E / o.n)
    print("emax / (E / n):", np.round(ratio, 3), " when:", o.when)
    assert ratio[0] > 4.0 and ratio[1] < 1.5 and ratio[2] < 1.5
    assert o.when[0] in (31, 32)  # the two blocks that lie wholly inside the burst
    duty = CH.duty_cycle(o.hist)
    print("duty:", duty, " bins of the burst channel:", {int(i): int(o.hist[0, i]) for i in np.nonzero(o.hist[0])[0]})
    assert duty[0] == 4 / 64 and duty[1] == 0.0 and duty[2] == 0.0  # the window is 2 hops: a 3-hop burst touches 4 blocks
    AC.assert_terms_comparable(o.block_terms(CO.as_complex(AC.discovery_capture())))
