"""CPU: the channeliser survey (jaero_survey_*, jaero_chan2_retune_all) without a device -- the exports and what is refused before a device
is looked for -- then its numpy definition (tests/chan_survey_oracle.py) against itself, against the time-domain Hann window and against
the channeliser's own output, and `channeliser.find_carriers` on the definition's spectrum."""
import ctypes as C

import numpy as np
import pytest

import chan_oracle as CO
import chan_survey_oracle as SO
from chan_cases import AUDIO, CHAIN_CENTRES, pchannel_chain_capture
from jaero_amd import capi, channeliser as CH
from jaero_amd import signalgen as G

N, HP = SO.N, SO.HP
SURVEY_SYMBOLS = ("jaero_survey_enable", "jaero_survey_reset", "jaero_survey_read_psd", "jaero_survey_read_levels",
                  "jaero_survey_profile_read", "jaero_chan2_retune_all")


def test_exports_and_refusals_without_a_device():
    L = capi.lib()
    for name in SURVEY_SYMBOLS:
        assert name in capi.EXPORTS and hasattr(L, name), name
        assert not name.startswith("jaero_chan_")  # tests/test_chan_host.py pins that set
    assert L.jaero_abi_version() == 1
    buf, n = np.zeros(N), C.c_longlong(0)
    ms, k = C.c_double(0), C.c_int(0)
    ch = capi.ChanChannel(0, 0, 1.0)
    assert L.jaero_survey_enable(None, 3) == capi.E_INVAL
    for bad in (4, -1, 7, 1 << 20):
        assert L.jaero_survey_enable(None, bad) == capi.E_INVAL
        assert "outside 0..3" in L.jaero_last_error().decode()
    assert L.jaero_survey_reset(None) == capi.E_INVAL
    assert L.jaero_survey_read_psd(None, buf.ctypes.data, C.byref(n)) == capi.E_INVAL
    assert L.jaero_survey_read_levels(None, buf.ctypes.data, buf.ctypes.data) == capi.E_INVAL
    assert L.jaero_survey_profile_read(None, 0, C.byref(ms), C.byref(k), 0) == capi.E_INVAL
    assert L.jaero_chan2_retune_all(None, C.cast(C.pointer(ch), C.c_void_p)) == capi.E_INVAL
    for name in ("survey_enable", "survey_reset", "read_psd", "read_levels", "suggest_gains", "retune_all", "survey_profile_read"):
        assert callable(getattr(CH.Channeliser, name))


@pytest.fixture(scope="module")
def chain_iq():
    return pchannel_chain_capture()[1]


def white(n, seed, amp=8000.0):
    rng = np.random.default_rng(seed)
    return np.rint(amp * (rng.normal(size=n) + 1j * rng.normal(size=n)) / np.sqrt(2.0))


def test_frequency_domain_hann_is_the_time_domain_window():
    """S of the definition = sum_p |DFT(s_p (1/2 - 1/2 cos 2 pi n / N))|^2; largest |d| / (want + mean) measured 7.8e-16."""
    x = white(3 * HP, 1)
    o = SO.ChanSurveyOracle(64, [(0, AUDIO, 1.0)], np.ones(1), levels=False)
    assert o.survey(x) == 3 and o.nblocks == 3
    padded = np.concatenate([np.zeros(HP), x])
    want = sum(SO.hann_spectrum_time(padded[p * HP: p * HP + N]) for p in range(3))
    err = float(np.max(np.abs(o.S - want) / (want + want.mean())))
    print(f"frequency-domain against time-domain Hann: {err:.2e}")
    assert err <= 1e-13


def test_fed_in_pieces_equals_fed_at_once_exactly():
    decim, fs = 64, 48000.0 * 64
    x = white(6 * HP + 77, 2)
    chans = [(CH.tune_word(f, fs), AUDIO, 1.0) for f in (33.3, -123456.7, fs / 2 - 1.0)]
    taps = CH.design_taps(decim, ntaps=2049, beta=10.0)
    whole, pieces = SO.ChanSurveyOracle(decim, chans, taps), SO.ChanSurveyOracle(decim, chans, taps)
    assert whole.survey(x) == 6
    pos = 0
    for n in (1, 8191, 8193, 3 * 8192 + 5, 0, 8191 - 5, 10 ** 9):
        pieces.survey(x[pos:pos + n])
        pos += n
    assert pieces.nblocks == whole.nblocks == 6 and np.array_equal(pieces.n, whole.n) and (whole.n == 6).all()
    assert np.array_equal(pieces.S, whole.S) and np.array_equal(pieces.E, whole.E)
    assert whole.S.min() > 0 and whole.E.min() > 0
    # reset, and the restart of a channel whose tune word changes; audio- and gain-only retunes restart nothing
    twin = SO.ChanSurveyOracle(decim, chans, taps)
    twin.survey(x[:2 * HP])
    twin.retune(0, chans[0][0], AUDIO + 5, 0.5)
    twin.retune(1, CH.tune_word(50000.0, fs), AUDIO, 1.0)
    twin.survey(x[2 * HP:])
    assert list(twin.n) == [6, 4, 6] and twin.E[0] == whole.E[0] and twin.E[2] == whole.E[2] and twin.E[1] != whole.E[1]
    twin.reset()
    assert not twin.S.any() and not twin.E.any() and not twin.n.any() and twin.nblocks == 0
    assert np.isnan(twin.levels()).all()


def test_psd_sums_to_the_mean_square_of_white_noise():
    x = white(9 * HP, 3)
    o = SO.ChanSurveyOracle(64, [(0, AUDIO, 1.0)], np.ones(1), levels=False)
    o.survey(x[:HP])
    o.reset()  # block 0's window is half zeros
    o.survey(x[HP:])
    assert o.nblocks == 8
    total, want = float(o.psd().sum()), float(np.mean(np.abs(x) ** 2))
    print(f"sum psd / mean |x|^2 = {total / want:.4f}")
    assert abs(total / want - 1.0) <= 0.02


def level_against_output(decim, chans, taps, x):
    o = SO.ChanSurveyOracle(decim, chans, taps, psd=False)
    y = o.write(x)
    rms = np.sqrt(np.mean(y ** 2, axis=1))
    ratio = o.predicted_rms(1.0) / rms
    print(f"D = {decim}: predicted / measured output RMS {np.round(ratio, 4)}, measured {np.round(rms, 1)} LSB")
    return ratio


def test_level_predicts_the_output_rms_chain_capture(chain_iq):
    """The first 48 hops at D = 16; measured 0.9945 .. 0.9957 (the shortfall is block 0's half window of zeros)."""
    fs = 48000.0 * 16
    chans = [(CH.tune_word(f, fs), AUDIO, 1.0) for f in CHAIN_CENTRES]
    ratio = level_against_output(16, chans, CH.design_taps(16), CO.as_complex(chain_iq[:48 * HP]))
    assert np.all(np.abs(ratio - 1.0) <= 0.03)


def test_level_predicts_the_output_rms_msk_capture_d256():
    decim, fs_out = 256, 12000.0
    fs, fb, nhops = fs_out * decim, 600.0, 48
    centres, amps = [-150000.0, 33.3, 200003.0], [1.0, 2.0, 3.0]
    rng = np.random.default_rng(256)
    n = nhops * HP
    bits = [rng.integers(0, 2, size=int(n / (fs / fb)) + 20, dtype=np.uint8) for _ in centres]
    iq = G.wideband_msk(bits, centres, amps, fs, fb=fb, ebno_db=13.0, rms=0.1, seed=7, nsamples=n)
    chans = [(CH.tune_word(f, fs), CH.tune_word(1000.0, fs_out), 1.0) for f in centres]
    ratio = level_against_output(decim, chans, CH.design_taps(decim, fs_out=fs_out), CO.as_complex(iq))
    assert np.all(np.abs(ratio - 1.0) <= 0.03)


def test_find_carriers_on_the_chain_capture(chain_iq):
    """16 hops of the definition's spectrum: exactly the four carriers, each within 250 Hz (measured: 110 Hz at the most; beyond 250 Hz
    the demodulator's own acquisition takes over)."""
    fs = 48000.0 * 16
    o = SO.ChanSurveyOracle(16, [(0, AUDIO, 1.0)], np.ones(1), levels=False)
    o.survey(CO.as_complex(chain_iq[:16 * HP]))
    assert o.nblocks == 16
    found = CH.find_carriers(o.psd(), fs, 10500.0)
    print("found", np.round(found, 1), "errors", np.round(np.array(found) - np.array(sorted(CHAIN_CENTRES)), 1) if len(found) == 4 else None)
    assert len(found) == 4
    assert np.all(np.abs(np.array(found) - np.array(sorted(CHAIN_CENTRES))) <= 250.0)


def test_find_carriers_on_noise_finds_nothing():
    o = SO.ChanSurveyOracle(16, [(0, AUDIO, 1.0)], np.ones(1), levels=False)
    o.survey(white(16 * HP, 5, amp=3000.0))
    assert CH.find_carriers(o.psd(), 48000.0 * 16, 10500.0) == []
