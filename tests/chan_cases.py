"""What the channeliser's tests share (tests/test_gpu_chan*.py on the GPU, tests/test_chan_*host.py on the CPU): the rule every comparison
of int16 output rests on, the inputs (white full-scale I/Q, the synthetic captures, the tones of the oracle-against-itself tests, the
P-channel chain capture), the twelve edge-case channels, the boundary tune words, the CPU model of one item of k_chan_synth's transform
(tests/test_chan_fft_model.py, tests/test_chan_rates_fft_model.py), and the `CH` fixture.  Each is defined here once, at every total
decimation 16 .. 256; a test file that needs one imports it by name.  Nothing here touches a GPU but `CH`."""
import functools

import numpy as np
import pytest

import chan_oracle as CO
from jaero_amd import aerol_frames as AF
from jaero_amd import signalgen as G

N, HP = CO.N, CO.HP
AUDIO = 715827883  # round(2^32 / 6): 8 kHz at 48 kHz, 4 kHz at 24 kHz, 2 kHz at 12 kHz
FS_OUT = {16: 48000.0, 32: 48000.0, 64: 48000.0, 128: 24000.0, 256: 12000.0}  # D = 128 and 256 both cut a 3.072 MS/s capture


@pytest.fixture(scope="module")
def CH():
    """jaero_amd.channeliser with the library loaded.  A test module imports the fixture by name; pytest finds it there."""
    from jaero_amd import capi
    from jaero_amd import channeliser

    capi.lib()
    return channeliser


def assert_rule(got, ystar, gain, where=""):
    """got == rint(y*), or |got - rint(y*)| == 1 AND the oracle's unrounded y* lies within tau = 1e-7 max(1, g) LSB of a half-integer.  tau
    is 10^4 x the round-off measured between two fp64 summation orders of the definition on the CPU (1.0e-11 LSB at gain 1); it says WHERE
    a difference may occur, so no share of samples is written off.  Every compared channel must have an output RMS above 100 LSB, so that
    nothing passes empty."""
    got = np.asarray(got).astype(np.int64)
    ref = CO.to_int16(ystar).astype(np.int64)
    assert got.shape == ref.shape, (where, got.shape, ref.shape)
    d = np.abs(got - ref)
    assert d.max(initial=0) <= 1, (where, "differs by more than one", int(d.max()))
    tau = 1e-7 * max(1.0, gain)
    off = np.nonzero(d)[0]
    edge = np.abs(ystar[off] - (np.floor(ystar[off]) + 0.5))  # distance to the half-integer between the two candidates
    print(f"{where}: {got.size} samples, {off.size} differ by one, rms {got.astype(float).std():.1f}")
    assert (edge <= tau).all(), (where, "a sample differs away from a rounding edge", float(edge.max(initial=0)), int(off.size))
    assert got.astype(float).std() > 100.0, (where, "output RMS below 100 LSB")


def white_full_scale(n, seed):
    """White I/Q whose every sample is within 1 % of full scale (either sign, -32768 included): the strongest input there is, so that a
    channel of gain 0.04 keeps an RMS above 100 LSB behind the narrowest filter at D = 64 (uniform white would leave it 58)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 256, size=(n, 2))
    s = rng.integers(0, 2, size=(n, 2))
    return np.where(s == 1, 32767 - k, -32768 + k).astype(np.int16)


def synthetic_capture(decim, nhops, seed):
    """Three carriers (amplitudes 1, 1, 3; Eb/N0 20 dB on the weak ones) at a quarter of full scale: OQPSK at 48 kHz x D for D <= 64, MSK
    (fb = fs_out / 20) at the 24 / 12 kHz rates above.  Returns (iq, centres)."""
    fs_out = FS_OUT[decim]
    fs = fs_out * decim
    rng = np.random.default_rng(seed)
    n = HP * nhops
    if decim <= 64:
        centres = [-123456.7, 33.3, fs / 2 - 10000.0]
        bits = [rng.integers(0, 2, size=2 * (int(n / (fs / 5250.0)) + 20), dtype=np.uint8) for _ in centres]
        return G.wideband_oqpsk(bits, centres, [1.0, 1.0, 3.0], decim, ebno_db=20.0, rms=0.25, seed=seed, nsamples=n), centres
    fb = fs_out / 20.0
    centres = [-123456.7, 33.3, fs / 2 - fs_out * 10 / 48]
    bits = [rng.integers(0, 2, size=int(n / (fs / fb)) + 20, dtype=np.uint8) for _ in centres]
    return G.wideband_msk(bits, centres, [1.0, 1.0, 3.0], fs, fb=fb, ebno_db=20.0, rms=0.25, seed=seed, nsamples=n), centres


def channel_set(CHm, decim, strong_hz, weak_gain, fs_in=None):
    """12 channels as a list of [tune, audio, gain]: centres off grid, negative, at the edges of the occupied band, two on one bin with
    different words; gains 1 except channel 2 (`weak_gain`, on `strong_hz` like channel 3) and channel 3 (set by the caller so that about
    1 % of its samples clip).  Offsets scale with the output rate (10 kHz, 3 Hz, 11 Hz and 11 kHz at 48 kHz).

    The occupied band is B = min(fs_in, Fs_c), Fs_c = fs_out x decim; fs_in = None: the capture fills Fs_c.  Where B == Fs_c the edge
    channels sit at +-(Fs_c / 2 - fs_out 10 / 48) and +-(Fs_c / 2 - 1) and their runs of bins wrap at N; where the capture is narrower (one
    that is raised to Fs_c) they sit on the capture's own edges, since nothing lies beyond."""
    fs_out = FS_OUT[decim]
    fs, r = fs_out * decim, fs_out / 48000.0
    B = fs if fs_in is None else min(float(fs_in), fs)
    edge = B / 2 - fs_out * 10 / 48
    hz = [33.3, -123456.7, strong_hz, strong_hz, edge, -edge, 200003.0, -0.01, 7 * fs / N + 3.0 * r, 7 * fs / N - 11.0 * r, -B / 2 + 1.0,
          B / 2 - 1.0]
    chans = [[CHm.tune_word(f, fs), AUDIO, 1.0] for f in hz]
    assert CO.words(chans[8][0], AUDIO, decim)[0] == CO.words(chans[9][0], AUDIO, decim)[0] == 7 and chans[8][0] != chans[9][0]
    for i in (4, 5, 10, 11):
        b = CO.words(chans[i][0], AUDIO, decim)[0]
        if B == fs:
            assert abs(b) + N // decim // 2 > N // 2  # wraps
        else:  # on the capture's own edge, inside the band it fills, and no run of bins wraps
            assert abs(hz[i]) <= B / 2 < fs / 2 and abs(b) + N // decim // 2 <= N // 2
    chans[6][1] = CHm.tune_word(11000.0 * r, fs_out)
    chans[2][2] = weak_gain
    return chans


# ---------------------------------------------------------------------------------------------- the P-channel chain
CHAIN_CENTRES = [-150000.0, -137500.0, -125000.0, 200003.0]
CHAIN_AMPS = [1.0, 1.5, 2.0, 2.5]


@functools.lru_cache(maxsize=None)
def pchannel_chain_capture():
    """D = 16, four 10.5 kbps P channels of 8 frames each, Eb/N0 13 dB on the weakest, 0.1 of full scale RMS: (payloads, iq, info).
    Built once per process (about half a minute on a CPU) and handed to every caller, so iq is read-only."""
    fb, nfr, decim = 10500, 8, 16
    pays, bits = [], []
    for c in range(4):
        pay = AF.random_payloads(nfr, fb, seed=50 + c)
        b, _ = AF.p_channel_bits(pay, fb)
        pays.append(pay)
        bits.append(np.concatenate([b, np.zeros(64, np.uint8)]))
    n48 = int(len(bits[0]) / 2 * 48000 / 5250) + 2000
    n = (n48 * decim // HP) * HP
    iq, info = G.wideband_oqpsk(bits, CHAIN_CENTRES, CHAIN_AMPS, decim, fb=fb, ebno_db=13.0, rms=0.1, seed=7, nsamples=n, return_info=True)
    iq.flags.writeable = False
    return pays, iq, info


# ---------------------------------------------------------------------------------------------- the host tests' inputs
def boundary_words():
    """Tune words at every edge of the split into (bin, remainder): the ends of the 32-bit range, and +-1 around each half-bin boundary of
    bins 0, +-1, +-5, the middle and the two ends of the grid."""
    ws = {0, 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, (1 << 32) - 2}
    for b in (0, 1, -1, 5, -5, 8191, -8191, 8192 - 1, -8192, 4096, -4097):
        for d in (-(1 << 17) - 1, -(1 << 17), -(1 << 17) + 1, -1, 0, 1, (1 << 17) - 1, 1 << 17, (1 << 17) + 1):
            ws.add((b * (1 << 18) + d) % (1 << 32))
    return sorted(ws)


def tone_capture(decim, fs_out, fc, nhops, rng):
    """The input the definition was checked on: a tone of 3000 LSB fs_out / 32 above the centre (1.5 kHz at 48 kHz), one of 9000 LSB
    fs_out 40 / 48 above it (40 kHz at 48 kHz: outside the +-fs_out / 2 the channel keeps), noise of 300 LSB per rail; rounded to integers."""
    fs = fs_out * decim
    n = HP * nhops
    t = np.arange(n)
    x = (3000 * np.exp(2j * np.pi * (((fc + fs_out / 32) / fs * t) % 1.0)) + 9000 * np.exp(2j * np.pi * (((fc + fs_out * 40 / 48) / fs * t) % 1.0))
         + 300 * (rng.normal(size=n) + 1j * rng.normal(size=n)))
    return np.rint(x.real) + 1j * np.rint(x.imag)


# ---------------------------------------------------------------------------------------------- k_chan_synth's transform, modelled
def model_item(S, X, G, b):
    """One (channel, block) item as the kernel computes it: returns (ml[T, P2 / 2], w[T, P2 / 2]): output index r - Mo and value held by
    thread u in its slot jj."""
    M, R1, R2, P2, T = S.M, S.R1, S.R2, S.P2, S.T
    u = np.arange(T)
    # gather + pass 1: thread n2 = u holds k = R2 n1 + u; planes swapped (inverse = forward of the swapped planes)
    a = np.zeros((T, R1), complex)
    for n1 in range(R1):
        k = R2 * n1 + u
        q = np.where(k < M // 2, k, k - M)
        Y = X[(b + q) % N] * G[q % N] / N
        a[:, n1] = Y.imag + 1j * Y.real
    A = np.fft.fft(a, axis=1) * np.exp(-2j * np.pi * u / M)[:, None] ** np.arange(R1)[None, :]
    # exchange
    L = np.full(S.XCH, np.nan, complex)
    for k in range(R1):
        L[S.xaddr(k, u)] = A[:, k]
    k1, h = u % R1, u // R1
    if S.SPLIT == 2:
        e = np.stack([L[S.xaddr(k1, n)] + np.where(h, -1.0, 1.0) * L[S.xaddr(k1, n + P2)] for n in range(P2)], axis=1)
        e = e * np.where(h, np.exp(-2j * np.pi / 32), 1.0)[:, None] ** np.arange(P2)[None, :]
    else:
        e = np.stack([L[S.xaddr(k1, n)] for n in range(P2)], axis=1)
    E = np.fft.fft(e, axis=1)
    ml = np.zeros((T, P2 // 2), int)
    w = np.zeros((T, P2 // 2), complex)
    for jj in range(P2 // 2):
        k2 = 2 * (jj + P2 // 2) + h if S.SPLIT == 2 else jj + P2 // 2 + 0 * h
        ml[:, jj] = k1 + R1 * (k2 - R2 // 2)
        s = E[:, jj + P2 // 2]
        w[:, jj] = s.imag + 1j * s.real
    return ml, w
