"""CPU: the rate meter's C ABI without a device (exports, refusals, no CPU fallback), its oracle against itself (the window's two forms,
cut independence, the exact zeros) and against a long-double DFT (the figure the GPU tolerance rests on), and classify_rates on the
oracle's sums: the case rows, the documented limits, and the blind chain's margins."""
import ctypes as C

import numpy as np
import pytest

import rate_cases as RC
import rate_oracle as RO
from jaero_amd import capi, ratemeter as RM
from jaero_amd import signalgen as G

L, BINS = RO.L, RO.BINS
RATE_SYMBOLS = [s for s in capi.EXPORTS if s.startswith("jaero_rate_")]


# ---------------------------------------------------------------------------------------------- the C ABI without a device
def test_library_exports_every_rate_symbol():
    assert sorted(RATE_SYMBOLS) == sorted(
        "jaero_rate_" + n for n in ("create", "destroy", "write", "reset", "read", "profile_enable", "profile_read"))
    Lb = capi.lib()
    for name in RATE_SYMBOLS:
        assert hasattr(Lb, name), name
    assert (capi.RATE_L, capi.RATE_BINS) == (L, BINS) == (4096, 2049)
    assert Lb.jaero_abi_version() == 1


@pytest.mark.parametrize("args,word", [((0, 4096, False), b"nchannels"), ((-2, 4096, False), b"nchannels"), ((3, 0, False), b"max_write_samples"),
                                       ((3, -1, False), b"max_write_samples"), ((3, 4096, True), b"null")])
def test_create_refusals_need_no_device(args, word):
    """Every refusal of jaero_rate_create is JAERO_EINVAL before a device is looked for, and says what was wrong."""
    Lb = capi.lib()
    nch, mw, out_null = args
    h = C.c_void_p()
    rc = Lb.jaero_rate_create(0, nch, mw, None if out_null else C.byref(h))
    assert rc == capi.E_INVAL and not h.value
    assert word in Lb.jaero_last_error(), Lb.jaero_last_error()


def test_null_handles_are_refused():
    Lb = capi.lib()
    n, nseg, ms = C.c_int(7), C.c_longlong(0), C.c_double()
    buf = np.zeros(8, np.int16)
    sums = np.zeros(BINS)
    assert Lb.jaero_rate_write(None, buf.ctypes.data, 4, 0, None, C.byref(n)) == capi.E_INVAL
    assert b"jaero_rate_write" in Lb.jaero_last_error()
    assert Lb.jaero_rate_reset(None) == capi.E_INVAL
    assert Lb.jaero_rate_read(None, sums.ctypes.data, C.byref(nseg)) == capi.E_INVAL
    assert Lb.jaero_rate_profile_enable(None, 1) == capi.E_INVAL
    assert Lb.jaero_rate_profile_read(None, 0, C.byref(ms), C.byref(n), 0) == capi.E_INVAL
    Lb.jaero_rate_destroy(None)  # a no-op


def test_no_cpu_fallback():
    """Without a HIP device a valid jaero_rate_create fails with ENODEV (never computes on the host)."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    Lb = capi.lib()
    h = C.c_void_p()
    assert Lb.jaero_rate_create(0, 3, 4096, C.byref(h)) == capi.E_NODEV and not h.value
    with pytest.raises(capi.JaeroError) as e:
        RM.RateMeter(3, 48000.0)
    assert e.value.code == capi.E_NODEV


# ---------------------------------------------------------------------------------------------- oracle against itself
N_PARITY = RC.N_PARITY


def oracle_of(pcm, cuts=None):
    o = RO.RateOracle(pcm.shape[0])
    pos = 0
    for n in (cuts or [pcm.shape[1]]):
        o.write(pcm[:, pos:pos + n])
        pos += n
        assert o.n == pos // L
    assert pos == pcm.shape[1]
    return o


def test_frequency_domain_hann_equals_time_domain_hann():
    """H[k] = Z[k] / 2 - (Z[k - 1] + Z[k + 1]) / 4 is the transform of q w, w[i] = (1 - cos(2 pi i / L)) / 2: the two agree to round-off,
    by the rule of the GPU comparison."""
    pcm = RC.case_rows(RC.NCASES, N_PARITY)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(L) / L)
    want = np.zeros((RC.NCASES, BINS))
    for j in range(3):
        y2 = pcm[:, j * L:(j + 1) * L].astype(np.int64) ** 2
        q = y2 - y2.sum(axis=1, keepdims=True) / L
        want += np.abs(np.fft.rfft(q * w, axis=1)) ** 2
    got = oracle_of(pcm).R
    for c in range(RC.NCASES):
        if c in (RC.ZERO, RC.CONST):
            continue
        err = float(np.max(np.abs(got[c] - want[c]) / (want[c] + want[c].mean())))
        print(f"row {c}: frequency-domain against time-domain Hann {err:.2e}")
        assert err <= RC.RTOL, (c, err)


def test_oracle_is_cut_independent():
    pcm = RC.case_rows(11, RC.N_CUTS)
    whole = oracle_of(pcm)
    cut = oracle_of(pcm, RC.CUTS)
    assert whole.n == cut.n == 5 and np.array_equal(whole.R, cut.R)


def test_zero_and_constant_rows_are_exact_zeros():
    pcm = RC.case_rows(RC.NCASES, N_PARITY)
    R = oracle_of(pcm).R
    assert (R[RC.ZERO] == 0.0).all() and (R[RC.CONST] == 0.0).all()
    assert all(R[c].min() >= 0.0 and R[c].max() > 0.0 for c in range(RC.NCASES) if c not in (RC.ZERO, RC.CONST))
    assert RC.exact_rows(20) == [5, 6, 14, 15]


def test_reset_keeps_the_grid():
    pcm = RC.case_rows(RC.NCASES, N_PARITY)
    o = RO.RateOracle(RC.NCASES)
    o.write(pcm[:, :L + 50])
    o.reset()
    o.write(pcm[:, L + 50:])
    assert o.n == 2 and np.array_equal(o.R, oracle_of(pcm[:, L:]).R)


def test_oracle_against_long_double_dft():
    """The figure the GPU tolerance rests on: the oracle (numpy's fp64 FFT) against the definition summed literally in long double, on 64
    bins of every case row -- 56 spread over 0 .. 2048 and the row's 8 strongest (its lines) -- over the parity case's three segments, by
    the rule |oracle - exact| <= f (exact + mean_k oracle).  Measured f = 4.2e-16; RTOL = 1e-12 stands while f <= 1e-14 (it would become
    100 f otherwise, DESIGN 18 "Rate lines")."""
    ld = np.longdouble
    assert np.finfo(ld).eps < 1e-18, "long double is no wider than double here"
    pcm = RC.case_rows(RC.NCASES, N_PARITY)
    R = oracle_of(pcm).R
    two_pi = ld(8) * np.arctan(ld(1))
    m = np.arange(L).astype(ld)
    cs, sn = np.cos(two_pi * m / L), np.sin(two_pi * m / L)
    w = ld(0.5) - ld(0.5) * cs
    i = np.arange(L)
    worst = 0.0
    for c in range(RC.NCASES):
        if c in (RC.ZERO, RC.CONST):
            continue
        bins = np.unique(np.concatenate([np.rint(np.linspace(0, L // 2, 56)).astype(int), np.argsort(R[c])[-8:]]))
        exact = np.zeros(len(bins), dtype=ld)
        for j in range(3):
            y2 = pcm[c, j * L:(j + 1) * L].astype(np.int64) ** 2
            qw = (y2.astype(ld) - ld(int(y2.sum())) / L) * w
            for b, k in enumerate(bins):
                e = (int(k) * i) % L
                re, im = (qw * cs[e]).sum(), (qw * sn[e]).sum()
                exact[b] += re * re + im * im
        err = float(np.max(np.abs(R[c, bins].astype(ld) - exact) / (exact + ld(R[c].mean()))))
        print(f"row {c}: oracle against long double {err:.2e} on {len(bins)} bins")
        worst = max(worst, err)
    print(f"oracle against long double, all rows: {worst:.2e}")
    assert worst <= 1e-14


# ---------------------------------------------------------------------------------------------- classify_rates
NSEG = 16


@pytest.fixture(scope="module")
def direct_R():
    """the oracle's sums over 16 segments of rows made by signalgen at 48 kHz: the four rates, white noise, one CW, two CWs 1200.3 Hz apart,
    600 bps MSK at 12 kHz (classified at fs = 12000), zeros"""
    n = NSEG * L
    t = np.arange(n)
    rng = np.random.default_rng(3)
    noise = rng.normal(0.0, 600.0, size=(3, n))
    cw = lambda f: 6000.0 * np.cos(2 * np.pi * ((f / 48000.0 * t) % 1.0))
    rows = [
        G.oqpsk(n, fb=10500.0, fc=8000.0, ebno_db=13.0, seed=G.SEED_BASE + 1)[0],
        G.oqpsk(n, fb=8400.0, fc=8000.0, ebno_db=13.0, seed=G.SEED_BASE + 2)[0],
        G.msk(n, fb=1200.0, fc=2000.0, ebno_db=13.0, seed=G.SEED_BASE + 3)[0],
        np.rint(noise[0] * 5),
        np.rint(cw(3000.0) + noise[1]),
        np.rint(cw(3000.0) + cw(4200.3) + noise[2]),
        G.msk(n, fb=600.0, Fs=12000.0, fc=2000.0, ebno_db=13.0, seed=G.SEED_BASE + 4)[0],
        np.zeros(n),
    ]
    o = RO.RateOracle(len(rows))
    o.write(np.stack(rows).astype(np.int16))
    assert o.n == NSEG
    return o.R


def test_classify_rates_on_direct_rows(direct_R):
    rate, audio, score = RM.classify_rates(direct_R[:6], 48000.0)
    print("scores, dB:\n", np.round(score, 1))
    assert rate.tolist() == [10500, 8400, 1200, 0, 0, 1200]  # one CW reads 0; two CWs fb apart read as fb: the documented limit
    bw = 48000.0 / L
    assert abs(audio[0] - 8000.0) <= bw and abs(audio[1] - 8000.0) <= bw and abs(audio[2] - 2000.0) <= bw
    assert np.isnan(audio[3]) and np.isnan(audio[4])
    assert score[3].max() < 7.0 and score[4].max() < 7.0  # noise and one CW stay 3 dB under the threshold
    assert score[0, 3] >= 13.0 and score[1, 2] >= 13.0 and score[2, 1] >= 13.0


def test_classify_rates_at_12_khz_and_on_empty_rows(direct_R):
    rate, audio, score = RM.classify_rates(direct_R[6], 12000.0)  # one row in, scalars out
    print("MSK 600 at 12 kHz, dB:", np.round(score, 1))
    assert rate == 600 and abs(audio - 2000.0) <= 12000.0 / L and score[0] >= 13.0
    assert np.isneginf(score[2]) and np.isneginf(score[3])  # 8400 and 10 500 bps do not fit into 6 kHz: skipped
    rate, audio, score = RM.classify_rates(direct_R[7:], 48000.0)
    assert rate.tolist() == [0] and np.isnan(audio[0]) and np.isneginf(score).all()


def test_classify_rates_literally():
    """the vectorised classify_rates against the definition written out per row"""
    rng = np.random.default_rng(9)
    R = rng.exponential(1.0, size=(6, BINS))
    R[0, [700, 700 + 896]] = 40.0
    R[1, [300, 300 + 51]] = 25.0
    R[2, [1000, 1000 + 102]] = 4.0
    R[3, 500] = 1e6                 # one line
    R[4, [2040, 8]] = 50.0          # at the ends
    rates, fs, thr, kmin = (600, 1200, 8400, 10500), 48000.0, 10.0, 8
    rate, audio, score = RM.classify_rates(R, fs)
    bw = fs / L
    for c in range(6):
        floor = np.median(R[c, kmin:])
        P = np.array([R[c, max(k - 1, 0):k + 2].max() for k in range(BINS)])
        best, best_db, best_a, best_d = 0, -np.inf, 0, 0
        for i, fb in enumerate(rates):
            d = int(round(fb / bw))
            s = [min(P[a], P[a + d]) for a in range(kmin, BINS - d)]
            a = int(np.argmax(s)) + kmin
            db = 10 * np.log10(max(s) / floor)
            assert abs(score[c, i] - db) < 1e-12
            if db > best_db:
                best, best_db, best_a, best_d = fb, db, a, d
        if best_db >= thr:
            assert rate[c] == best and audio[c] == (2 * best_a + best_d) * bw / 4
        else:
            assert rate[c] == 0 and np.isnan(audio[c])
    assert rate[0] == 10500 and rate[1] == 600 and rate[3] == 0  # two lines fb apart read as fb; one line, however strong, does not


# ---------------------------------------------------------------------------------------------- the blind chain, on the CPU alone
def test_chain_margins_on_the_oracle():
    """The condition of the GPU chain test (tests/test_gpu_rate.py), met by the oracles alone: capture -> channeliser oracle -> int16 ->
    rate oracle -> classify_rates names every carrier's rate with at least 3 dB to spare over the threshold, and the empty channel's best
    score lies at least 3 dB under it."""
    iq, chans, ystar = RC.chain()
    import chan_oracle as CO

    pcm = CO.to_int16(ystar)
    rms = pcm.astype(float).std(axis=1)
    assert np.allclose(rms, 3276.8, rtol=0.01), rms
    o = RO.RateOracle(5)
    assert o.write(pcm) == RC.CHAIN_SEGS
    rate, audio, score = RM.classify_rates(o.R, RC.CHAIN_FS_OUT)
    print("chain scores, dB:\n", np.round(score, 1), "\naudio:", audio)
    assert rate.tolist() == RC.CHAIN_RATES
    top = score.max(axis=1)
    assert (top[:4] >= 13.0).all() and top[4] <= 7.0, top
    assert (np.abs(audio[:4] - np.array(RC.CHAIN_AUDIO)) <= RC.CHAIN_FS_OUT / L).all() and np.isnan(audio[4])
