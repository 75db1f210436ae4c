"""What the rate meter's tests share (tests/test_gpu_rate.py on the GPU, tests/test_rate_host.py on the CPU): the rule every comparison of
R rests on, the nine case rows, and the blind chain capture -> channeliser -> rate lines -> classify_rates.  Each is defined here once
and built once per process.  Nothing here touches a GPU."""
import functools

import numpy as np

import chan_oracle as CO
import rate_oracle as RO
from jaero_amd import channeliser as CHm
from jaero_amd import signalgen as G

L, BINS = RO.L, RO.BINS
# The survey's bound (tests/test_gpu_chan_survey.py): R[k] is a sum of |H|^2 of fp64 transforms, as S[k] is.  It stands while the oracle
# itself lies within 1e-14 of a long-double DFT by the same rule (tests/test_rate_host.py asserts that, and prints the figure); it is
# never fitted to the GPU's output.
RTOL = 1e-12

ZERO, CONST = 5, 6  # the case rows that must give R == 0 exactly
NCASES = 9
N_PARITY = 3 * L + 100  # three segments and a tail
N_CUTS = 5 * L + 100    # the cut tests' rows, and how they are cut: a write of one sample, one that ends a sample short of a segment, one that
CUTS = [1, 4095, 4097, 1, 8197, N_CUTS - 16391]  # crosses one, two segments and a bit in one write, the rest (a segment and a tail)


@functools.lru_cache(maxsize=None)
def base_rows(n):
    """The nine case rows, int16 [9, n]: OQPSK at 10 500 and 8400 bps, MSK at 1200 and 600 bps (Eb/N0 13 dB), white full-scale noise with
    -32768 in it, zeros, a constant, a sine clipped at the rails, +-3 LSB noise."""
    rng = np.random.default_rng(11)
    t = np.arange(n)
    white = rng.integers(-32768, 32768, n)
    white[::97] = -32768
    rows = [
        G.oqpsk(n, fb=10500.0, fc=8000.0, ebno_db=13.0, seed=G.SEED_BASE + 1)[0],
        G.oqpsk(n, fb=8400.0, fc=8000.0, ebno_db=13.0, seed=G.SEED_BASE + 2)[0],
        G.msk(n, fb=1200.0, fc=2000.0, ebno_db=13.0, seed=G.SEED_BASE + 3)[0],
        G.msk(n, fb=600.0, fc=2000.0, ebno_db=13.0, seed=G.SEED_BASE + 4)[0],
        white,
        np.zeros(n),
        np.full(n, -12345),
        np.clip(np.rint(60000.0 * np.sin(2 * np.pi * 0.0371 * t)), -32768, 32767),
        rng.integers(-3, 4, n),
    ]
    out = np.stack([np.asarray(r).astype(np.int16) for r in rows])
    assert out.min() == -32768 and out.max() == 32767
    out.flags.writeable = False
    return out


def case_rows(nch, n):
    """int16 [nch, n]: row i is case row i mod 9, turned by 131 (i div 9) samples so that no two rows but the zero and constant ones are equal."""
    b = base_rows(n)
    return np.stack([np.roll(b[i % NCASES], 131 * (i // NCASES)) for i in range(nch)])


def exact_rows(nch):
    return [i for i in range(nch) if i % NCASES in (ZERO, CONST)]


def assert_rule(got, want, where=""):
    """Per row: |got - want| <= RTOL (want + mean_k want); the zero and the constant rows (want == 0 everywhere) are compared with ==.
    Returns the largest |got - want| / (want + mean_k want) over the other rows."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.shape[1] == BINS, (where, got.shape, want.shape)
    assert np.isfinite(got).all(), where
    worst = 0.0
    for c in range(want.shape[0]):
        if not want[c].any():
            assert (got[c] == 0.0).all(), (where, c, "a row whose sums are exactly zero is not", float(np.abs(got[c]).max()))
            continue
        ref = float(want[c].mean())
        err = float(np.max(np.abs(got[c] - want[c]) / (want[c] + ref)))
        worst = max(worst, err)
        assert err <= RTOL, (where, c, err)
    print(f"{where}: largest |got - want| / (want + mean) = {worst:.2e} over {want.shape[0]} rows")
    return worst


# ---------------------------------------------------------------------------------------------- the blind chain
CHAIN_DECIM, CHAIN_FS_OUT, CHAIN_SEGS = 16, 48000.0, 8
CHAIN_CARRIERS = [("oqpsk", 10500.0, -200000.0, 8000.0), ("oqpsk", 8400.0, -123456.0, 8000.0), ("msk", 1200.0, 150037.0, 2000.0),
                  ("msk", 600.0, 299989.0, 2000.0)]
CHAIN_EMPTY = (-300000.0, 8000.0)
CHAIN_RATES = [10500, 8400, 1200, 600, 0]
CHAIN_AUDIO = [8000.0, 8000.0, 2000.0, 2000.0]
CHAIN_EBNO_DB = 13.0


@functools.lru_cache(maxsize=None)
def chain():
    """A D = 16 capture (768 kS/s) of four carriers, each at Eb/N0 13 dB against ONE noise density (so amplitude ~ sqrt(fb)), and the five
    channels cut from it (the fifth is empty), 8 segments of output.  Every carrier is made alone by wideband_oqpsk / wideband_msk
    without noise, brought to unit amplitude by the scale they report, weighted, and the four are summed; the capture is scaled to 0.1
    of full scale.  The channels' gains put each output row at 0.1 of full scale (from the channeliser's oracle at gain 1).  Returns
    (iq int16 [n, 2], channels [(tune, audio, gain)], ystar [5, 8 L]: the channeliser oracle's unrounded output)."""
    decim, fs_out = CHAIN_DECIM, CHAIN_FS_OUT
    fs = fs_out * decim
    M = CO.N // decim
    n = CHAIN_SEGS * L // (M // 2) * CO.HP
    rng = np.random.default_rng(23)
    x = np.zeros(n, dtype=np.complex128)
    for kind, fb, centre, _ in CHAIN_CARRIERS:
        if kind == "oqpsk":
            bits = rng.integers(0, 2, size=2 * (int(n / (fs / (fb / 2))) + 20), dtype=np.uint8)
            iq, info = G.wideband_oqpsk([bits], [centre], [1.0], decim, fb=fb, ebno_db=None, rms=0.25, nsamples=n, return_info=True)
        else:
            bits = rng.integers(0, 2, size=int(n / (fs / fb)) + 20, dtype=np.uint8)
            iq, info = G.wideband_msk([bits], [centre], [1.0], fs, fb=fb, ebno_db=None, rms=0.25, nsamples=n, return_info=True)
        x += CO.as_complex(iq) / info["scale"] * np.sqrt(fb / info["p_unit"])  # power fb: Eb = 1 for every carrier
    sigma2 = fs / 10.0 ** (CHAIN_EBNO_DB / 10.0)  # N0 = Eb / 10^1.3 over the capture's bandwidth
    x += np.sqrt(sigma2 / 2.0) * (rng.normal(size=n) + 1j * rng.normal(size=n))
    x *= 0.1 * 32768.0 / np.sqrt(np.mean(np.abs(x) ** 2))
    iq = np.empty((n, 2), dtype=np.int16)
    iq[:, 0] = np.clip(np.rint(x.real), -32768, 32767)
    iq[:, 1] = np.clip(np.rint(x.imag), -32768, 32767)
    where = [(c, a) for _, _, c, a in CHAIN_CARRIERS] + [CHAIN_EMPTY]
    chans = [(CHm.tune_word(c, fs), CHm.tune_word(a, fs_out), 1.0) for c, a in where]
    y1 = CO.block_form(CO.as_complex(iq), decim, chans, CHm.design_taps(decim))
    assert y1.shape == (5, CHAIN_SEGS * L)
    gains = 0.1 * 32768.0 / np.sqrt(np.mean(y1 ** 2, axis=1))
    chans = [(t, a, float(g)) for (t, a, _), g in zip(chans, gains)]
    ystar = y1 * gains[:, None]
    iq.flags.writeable = False
    ystar.flags.writeable = False
    return iq, chans, ystar
