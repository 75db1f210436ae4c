"""What the activity's tests share (tests/test_chan_activity_host.py on the CPU, tests/test_gpu_chan_activity.py on the GPU): the blind
discovery capture (white noise, one carrier that is always on, one that is on for three hops of 64), the 19-channel definition case at
every total decimation, the checks on the oracle's block terms that make `when` and `hist` comparable exactly, and the burst capture
that is fed to a burst bank.  Nothing here touches a GPU."""
import functools

import numpy as np

import chan_activity_oracle as AO
import chan_oracle as CO
from chan_cases import AUDIO, FS_OUT
from jaero_amd import channeliser as CHN
from jaero_amd import signalgen as G

N, HP = CO.N, CO.HP
CUTS = (1, 8191, 8193, 3 * 8192 + 5, 0, 8191 - 5, 10 ** 9)  # tests/test_chan_survey_host.py's test_fed_in_pieces_equals_fed_at_once_exactly


def to_iq(x):
    """complex -> int16 [n, 2], rounded"""
    return np.stack([np.rint(x.real), np.rint(x.imag)], axis=1).astype(np.int16)


def band_noise(n, fs, centre, bw, rng):
    """A band-limited noise-like carrier: complex white noise of unit variance, brick-walled to +-bw / 2 in the frequency domain over the
    whole length, shifted to `centre`.  Inside the band its spectral density is that of white noise of unit variance; its power is
    bw / fs."""
    w = (rng.normal(size=n) + 1j * rng.normal(size=n)) / np.sqrt(2.0)
    W = np.fft.fft(w)
    W[np.abs(np.fft.fftfreq(n, 1.0 / fs)) > bw / 2] = 0.0
    t = np.arange(n, dtype=np.float64)
    return np.fft.ifft(W) * np.exp(2j * np.pi * ((centre / fs * t) % 1.0))


# ---------------------------------------------------------------------------------------------- the discovery case
DISC_DECIM, DISC_HOPS = 16, 64
DISC_FS = 48000.0 * DISC_DECIM
DISC_BURST_HZ, DISC_ON_HZ, DISC_EMPTY_HZ = -150000.0, 100000.0, 250000.0   # the burst carrier, the one that is always on, a channel of noise
DISC_BW = 8000.0
DISC_BURST_HOPS = (30, 33)     # on in hops 30, 31, 32: blocks 30 .. 33 see it (a block is two hops), blocks 31 and 32 wholly
DISC_SIGMA = 1000.0            # noise, LSB RMS (complex): a noise channel's block term is 384 / 16384 sigma^2 = 2^14.5, the middle of a bin
DISC_DB = 15.0                 # the carriers' spectral density above the noise's


@functools.lru_cache(maxsize=None)
def discovery_capture(db=DISC_DB, seed=1):
    """int16 I/Q [64 Hp, 2] at D = 16 (768 kS/s): white noise, a band-limited 8 kHz carrier `db` above the noise per bin at +100 kHz that is
    always on, another at -150 kHz that is on only in hops 30 .. 32.  Read-only (shared)."""
    rng = np.random.default_rng(seed)
    n = DISC_HOPS * HP
    amp = DISC_SIGMA * 10.0 ** (db / 20.0)
    x = DISC_SIGMA * (rng.normal(size=n) + 1j * rng.normal(size=n)) / np.sqrt(2.0)
    x = x + amp * band_noise(n, DISC_FS, DISC_ON_HZ, DISC_BW, rng)
    gate = np.zeros(n)
    gate[DISC_BURST_HOPS[0] * HP: DISC_BURST_HOPS[1] * HP] = 1.0
    x = x + amp * gate * band_noise(n, DISC_FS, DISC_BURST_HZ, DISC_BW, rng)
    iq = to_iq(x)
    iq.flags.writeable = False
    return iq


def discovery_channels(centres=(DISC_BURST_HZ, DISC_ON_HZ, DISC_EMPTY_HZ), gains=(1.0, 1.0, 1.0)):
    return [(CHN.tune_word(f, DISC_FS), AUDIO, float(g)) for f, g in zip(centres, gains)]


# ---------------------------------------------------------------------------------------------- the definition case
DEF_NCH, DEF_HOPS = 19, 7
DEF_GATE_HOPS = (2, 4)


def definition_case(decim, seed=None):
    """(iq int16 [7 Hp, 2], channels, taps) at total decimation `decim`: 19 channels (three more than a workgroup of the level kernel
    holds, so that its second workgroup runs with 13 spare groups) -- one whose run of bins wraps at the seam of the spectrum, one on bin
    0, two that share a tune word (different audio and gain), one on the gated carrier, the rest drawn -- over white noise plus a carrier
    that is on in hops 2 and 3 only, so that every channel's emax != emin and the gated channel's differ by far; taps of 2049 entries."""
    fs_out = FS_OUT[decim]
    fs = fs_out * decim
    rng = np.random.default_rng(1000 + decim if seed is None else seed)
    n = DEF_HOPS * HP
    carrier_hz = 0.11 * fs
    x = 1500.0 * (rng.normal(size=n) + 1j * rng.normal(size=n)) / np.sqrt(2.0)
    gate = np.zeros(n)
    gate[DEF_GATE_HOPS[0] * HP: DEF_GATE_HOPS[1] * HP] = 1.0
    x = x + 1500.0 * 10.0 ** (15.0 / 20.0) * gate * band_noise(n, fs, carrier_hz, fs_out / 6, rng)
    hz = [fs / 2 - 1.0, 0.0, 33.3, 33.3, carrier_hz, -fs / 2 + fs_out / 8] + [float(v) for v in rng.uniform(-fs / 2, fs / 2, size=DEF_NCH - 6)]
    chans = [(CHN.tune_word(f, fs), AUDIO, 1.0) for f in hz]
    chans[3] = (chans[2][0], CHN.tune_word(fs_out / 16, fs_out), 0.5)  # the same tune word, another audio word and gain
    M = N // decim
    assert abs(CO.words(chans[0][0], AUDIO, decim)[0]) + M // 2 > N // 2 and CO.words(chans[1][0], AUDIO, decim)[0] == 0
    assert len(chans) == DEF_NCH
    taps = CHN.design_taps(decim, ntaps=2049, beta=10.0, fs_out=fs_out)
    return to_iq(x), chans, taps


def assert_terms_comparable(terms):
    """The conditions under which `when` and `hist` of two correct implementations are EQUAL although their block terms differ in the last
    bits: no e_{c,p} has an frexp mantissa within 1e-9 of 0.5 or 1 (a bin edge), and every channel's two largest terms differ by more
    than 1e-9 relative (the index of the maximum).  Returns the smaller margin."""
    terms = np.asarray(terms)
    assert terms.shape[1] >= 2 and (terms > 0).all()
    mant = np.frexp(terms)[0]  # in [0.5, 1)
    edge = float(np.min(np.minimum(mant - 0.5, 1.0 - mant)))
    top = np.sort(terms, axis=1)[:, -2:]
    gap = float(np.min((top[:, 1] - top[:, 0]) / top[:, 1]))
    print(f"block terms: nearest mantissa to a bin edge {edge:.3g}, smallest relative gap between a channel's two largest {gap:.3g}")
    assert edge > 1e-9 and gap > 1e-9, (edge, gap)
    return min(edge, gap)


# ---------------------------------------------------------------------------------------------- capture -> burst bank
BURST_DECIM, BURST_HZ = 16, -181250.0
BURST_SECONDS, BURST_STARTS = 2, (20000, 68000)   # samples at 48 kHz: one burst per second
BURST_SIGMA = 3000.0   # wideband noise, LSB RMS (complex): 20 dB below the burst in the channel.  (At 600 the reference's detector, whose
#                        thresholds ride on the level between bursts, missed the first burst on the CPU; this is the one adjustment.)


@functools.lru_cache(maxsize=None)
def burst_capture():
    """`signalgen.burst_oqpsk` (two bursts, one per second, 2 s at 48 kHz, no noise of its own) lifted to D = 16: the analytic signal by FFT,
    FFT interpolation x 16, a shift to BURST_HZ, white noise.  int16 I/Q [n, 2], n a whole number of hops; read-only (shared)."""
    n48 = BURST_SECONDS * 48000
    pcm, _ = G.burst_oqpsk(n48, burst_starts=list(BURST_STARTS), ndata_sym=1500, ebno_db=None, peak=0.3, seed=G.SEED_BASE + 77)
    X = np.fft.fft(pcm.astype(np.float64))
    X[n48 // 2:] = 0.0          # analytic signal: the positive frequencies, twice
    X[1:n48 // 2] *= 2.0
    n = n48 * BURST_DECIM
    Z = np.zeros(n, dtype=np.complex128)
    Z[:n48 // 2] = X[:n48 // 2]  # FFT interpolation: the same spectrum on a grid 16 times as long
    z = np.fft.ifft(Z) * BURST_DECIM
    fs = 48000.0 * BURST_DECIM
    t = np.arange(n, dtype=np.float64)
    z = z * np.exp(2j * np.pi * (((BURST_HZ - 8000.0) / fs * t) % 1.0))  # the burst's 8 kHz audio carrier lands on BURST_HZ
    rng = np.random.default_rng(78)
    x = z + BURST_SIGMA * (rng.normal(size=n) + 1j * rng.normal(size=n)) / np.sqrt(2.0)
    n = n // HP * HP
    iq = to_iq(x[:n])
    iq.flags.writeable = False
    return iq
