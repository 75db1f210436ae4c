"""What tests/test_gpu_coarse.py and tests/test_coarse_cases.py share: the six estimator configurations, the per-channel locking bandwidths of
the parity matrix, the input draws, a long-double restatement of CoarseFreqEstimate::ProcessBasebandData (coarsefreqestimate.cpp:90-137) and
the fp64 restatement of its fold and peak search (:116-131).  Nothing here touches a GPU."""
import functools
import math

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def c_round(x):
    """C's round(): halves away from zero."""
    return int(math.floor(x + 0.5)) if x >= 0 else int(math.ceil(x - 0.5))


class Cfg:
    def __init__(self, name, kind, fb, Fs, power, thr, lbw0, variant, lbws):
        self.name, self.kind, self.fb, self.Fs, self.power, self.thr, self.lbw0, self.variant = name, kind, fb, Fs, power, thr, lbw0, variant
        self.N = 1 << power
        self.NT = self.N // 32  # threads of the kernel's workgroup: 32 points each
        self.hz = Fs / self.N
        self.epb = c_round(fb / (2.0 * self.hz))  # expectedpeakbin
        self.lbws = lbws  # the parity matrix's channels

    def startbin(self, lbw):
        return int(max(c_round(lbw / self.hz), 1))

    def i0i1(self, lbw):
        return c_round((-lbw / self.hz) + self.N / 2), c_round((lbw / self.hz) + self.N / 2)

    def fold_inside(self, lbw):
        i0, i1 = self.i0i1(lbw)
        return (i0 - self.epb - 1 >= 0) and (i1 + self.epb < self.N) and i0 >= 0

    def pointers(self):
        return [0, 1, self.NT - 1, self.NT, self.N - 1, 4097, self.N // 2 + 333, 12345 % self.N]


# Per-channel locking bandwidths (all <= Fs / 2): the default; startbin == 1 (lockingbw < hzperbin / 2); neighbours with different startbin
# (8400 bps: the LDS window table is rebuilt, and rebuilt back); 8400 bps at startbin >= C4_TABN - 1 = 3583 (lockingbw >= 10 497 Hz: window
# built per estimate) next to channels below it; bandwidths from which the fold leaves the spectrum (fold_inside false); Fs / 2 exactly.
CONFIGS = {c.name: c for c in [
    Cfg("oqpsk_10500", "oqpsk", 10500.0, 48000.0, 14, 0.65, 10500.0, "k_coarse6",
        [10500.0, 1.0, 10500.0, 5000.0, 18750.0, 9000.0, 24000.0, 10250.0, 20000.0, 18740.0]),
    Cfg("oqpsk_8400", "oqpsk", 8400.0, 48000.0, 14, 0.65, 8400.0, "k_coarse6_w8400",
        [8400.0, 3000.0, 8400.0, 3000.0, 10600.0, 5000.0, 1.0, 10490.0, 20000.0, 7000.0, 24000.0, 8400.0]),
    Cfg("msk_1200", "msk", 1200.0, 48000.0, 13, 0.5, 1800.0, "k_coarse6_13", [1800.0, 2.0, 1500.0, 23500.0, 1800.0, 24000.0, 6000.0, 1740.0]),
    Cfg("msk_600", "msk", 600.0, 48000.0, 13, 0.5, 900.0, "k_coarse6_13", [900.0, 2.0, 750.0, 23800.0, 900.0, 24000.0, 3000.0, 870.0]),
    Cfg("msk_1200_24k", "msk", 1200.0, 24000.0, 13, 0.5, 1800.0, "k_coarse6_13", [1800.0, 1.0, 1500.0, 11500.0, 1800.0, 12000.0, 4000.0, 1740.0]),
    Cfg("msk_1200_12k", "msk", 1200.0, 12000.0, 13, 0.5, 1800.0, "k_coarse6_13", [1800.0, 0.5, 1500.0, 5400.0, 1800.0, 6000.0, 3000.0, 1740.0]),
]}


def check_index_ranges(cfg, lbw):
    """What has to hold before a bandwidth is given to the kernel (k_coarse6.h): startbin + 2 window entries fit the space they are built in,
    and every index of the unchecked fold lies in [0, N)."""
    N, sb = cfg.N, cfg.startbin(lbw)
    assert 0 < lbw <= cfg.Fs / 2 and 1 <= sb <= N // 2
    if cfg.fb == 8400.0:
        C4_TABN, C6_XCH = 3584, 16448
        assert sb + 2 <= (C4_TABN if sb < C4_TABN - 1 else C6_XCH)
    i0, i1 = cfg.i0i1(lbw)
    assert 0 <= i0 <= i1 <= N
    if cfg.fold_inside(lbw) and i1 > i0:
        assert i0 - cfg.epb - 1 >= 0 and (i1 - 1) + cfg.epb + 1 < N


def draw(cfg, lbw, rng, signal):
    """N complex baseband samples in time order: complex Gaussian noise 0.1 and, with `signal`, amplitude 0.3 of random symbols at fb / 2 per arm
    (half-sine shaped, the arms offset by half a symbol: continuous phase, +-90 degrees per bit) on a random carrier inside +-lockingbw / 4."""
    N = cfg.N
    x = 0.1 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    if signal:
        spb = cfg.Fs / cfg.fb
        n = np.arange(N)
        k = np.floor((n + rng.uniform(0, spb)) / spb).astype(int)
        bits = rng.choice([-1.0, 1.0], size=k[-1] + 2)
        phase = np.cumsum(bits[k] * (math.pi / 2) / spb)
        f0 = rng.uniform(-lbw / 4, lbw / 4)
        x = x + 0.3 * np.exp(1j * (phase + 2 * math.pi * f0 * n / cfg.Fs + rng.uniform(0, 2 * math.pi)))
    return x


@functools.lru_cache(maxsize=None)
def window(cfg, lbw):
    """The 8400 bps window in double, value by value as the reference's loop forms it (:61-74; startbin <= N / 2)."""
    N, sb = cfg.N, cfg.startbin(lbw)
    w = np.zeros(N)
    w[0] = 1.0
    for i in range(1, sb + 1):
        v = math.cos((math.pi / 2) * float(i) / float(sb))
        v *= v
        w[N - i] = v
        w[i] = v
    return w


def restate(cfg, lbw, x, y_in):
    """Long-double restatement: (|Z| clipped at 1, y_out) with Z the shifted third transform.  The inverse transform is unnormalised
    (FFTWrapper with kissfft scaling: ifft times N)."""
    import scipy.fft as sf

    N, sb = cfg.N, cfg.startbin(lbw)
    X = sf.fft(np.asarray(x, dtype=np.clongdouble))
    assert X.dtype == np.clongdouble
    if cfg.fb != 8400.0:
        X[sb:N - sb + 1] = 0
    else:
        X = X * window(cfg, lbw).astype(LD)
    v = sf.ifft(X) * LD(N)
    Z = sf.fftshift(sf.fft(v * v))
    L = np.maximum(np.abs(Z), LD(1))
    return L, LD(0.9) * np.asarray(y_in, dtype=LD) + np.log10(L)


def fold(cfg, lbw, y):
    """(candidate bins, folded values) of :116-131, term by term in the reference's order, in y's own precision."""
    N, e = cfg.N, cfg.epb
    i0, i1 = cfg.i0i1(lbw)
    i = np.arange(max(i0, 0), min(i1, N))
    val = np.zeros(len(i), dtype=y.dtype)
    for j in (-1, 0, 1):
        a, b = i - e - j, i + e + j
        ok = (a >= 0) & (b < N)
        val = val + np.where(ok, y[np.where(ok, a, 0)] + y[np.where(ok, b, 0)], 0)
    return i, val


def peak_bin(cfg, lbw, y):
    """zmaxloc: the first candidate whose folded value is the largest and > 0, else N / 2."""
    i, val = fold(cfg, lbw, y)
    if len(i) == 0 or not (val.max() > 0):
        return cfg.N // 2
    return int(i[int(np.argmax(val))])


def margin_ok(cfg, lbw, y_ld, y_oracle):
    """The condition under which kernel and oracle must name the same bin: best and second-best folded value of the restatement (0 standing
    for `no candidate`) differ by more than 1000 times the largest difference between the oracle's y and the restatement's.
    Returns (ok, ratio)."""
    i, val = fold(cfg, lbw, y_ld)
    if len(i) == 0:
        return True, math.inf
    d = float(np.max(np.abs(np.asarray(y_oracle, dtype=LD) - y_ld)))
    s = np.sort(val)
    gap = float(s[-1] - max(s[-2] if len(s) > 1 else LD(0), LD(0)))
    return gap > 1000.0 * d, (gap / d if d > 0 else math.inf)


def bump(cfg, y, c, amp):
    """Makes candidate c the only one that receives amp twice (its j = -1 term): c +- 1, c +- 2 and six candidates 2 epb away receive it once."""
    y[c - cfg.epb + 1] += amp
    y[c + cfg.epb - 1] += amp


def exact_cases(cfg):
    """[(name, lockingbw, y_in, expected bin or None)] on a zero ring: y_out = 0.9 y_in exactly, and the peak search runs on values known
    exactly.  `expected` is what the case was built to give (None: whatever restatement and oracle agree on)."""
    N, NT = cfg.N, cfg.NT
    main = {"oqpsk_10500": 10500.0, "oqpsk_8400": 7000.0, "msk_1200": 5000.0}.get(cfg.name, cfg.Fs / 9.6)
    assert cfg.fold_inside(main)
    i0, i1 = cfg.i0i1(main)
    nrows = -(-(i1 - i0) // NT)
    assert nrows >= 6 and nrows % 4 != 0  # two blocks of four candidate rows at least, the last one partial
    cand = lambda t, row: i0 + t + row * NT
    out = [("zero", main, np.zeros(N), N // 2), ("const", main, np.full(N, 7.0), i0)]
    edge = [b for b in cfg.lbws if not cfg.fold_inside(b)]
    assert len(edge) >= 2 and cfg.Fs / 2 in edge
    for b in edge:
        out.append((f"const_edge_{b:g}", b, np.full(N, 7.0), None))
    pairs = [("quad1", 8, 9), ("quad2", 8, 10), ("half_row", 1, 6), ("row", 3, 12), ("rows", 3, 20), ("halves", 5, 40),
             ("waves", 10, 64 * 3 + 7), ("last_wave", 70, NT - 1)]
    for name, ta, tb in pairs:
        for order, (ra, rb) in (("lower_first", (1, 2)), ("higher_first", (2, 1))):
            y = np.zeros(N)
            bump(cfg, y, cand(ta, ra), 10.0)
            bump(cfg, y, cand(tb, rb), 10.0)
            out.append((f"tie_{name}_{order}", main, y, min(cand(ta, ra), cand(tb, rb))))
    y = np.zeros(N)
    bump(cfg, y, cand(5, 1), 10.0)
    bump(cfg, y, cand(5, 5), 10.0)
    out.append(("tie_same_thread_two_blocks", main, y, cand(5, 1)))
    y = np.zeros(N)
    bump(cfg, y, i1 - 1, 10.0)
    bump(cfg, y, i1, 20.0)
    out.append(("i1_excluded", main, y, i1 - 1))
    y = np.zeros(N)
    bump(cfg, y, i0, 10.0)
    bump(cfg, y, i0 - 1, 20.0)
    out.append(("i0_first", main, y, i0))
    y = np.zeros(N)
    bump(cfg, y, i1 - 3, 10.0)
    assert (i1 - 3 - i0) // NT // 4 == (nrows - 1) // 4
    out.append(("last_partial_block", main, y, i1 - 3))
    return out


def folded_at(cfg, y, c):
    """The folded value of one bin, candidate or not (all indices inside the spectrum)."""
    e, v = cfg.epb, 0.0
    for j in (-1, 0, 1):
        v += y[c - e - j] + y[c + e + j]
    return v


# ---- the never-locked streams of test_gpu_coarse's public-API case: 64 channels carrying eight signals, four noise only and four at 0 dB Eb/N0
STREAM_NSIG = 8
STREAM_CHECK = [0, 1, 2, 3, 4, 5, 6, 7, 31, 63]
STREAM_NSAMP = {"oqpsk": 135000, "msk": 70000}  # an estimate per nfft / 4 samples: 32 and 34 of them
# signal thresholds under which these streams stay unlocked (mse > threshold): the oracle's mse on them is 0.38 - 0.76 for OQPSK from the third
# estimate on (the default 0.65 calls most of that locked) and climbs from 0.076 for MSK (a 600-symbol average that starts at zero)
STREAM_THR = {"oqpsk": 0.3, "msk": 0.05}
STREAM_MIN_UNLOCKED = 25


def stream_signals(kind):
    """[STREAM_NSIG, n] int16"""
    from jaero_amd import signalgen as G

    n = STREAM_NSAMP[kind]
    rows = []
    for k in range(STREAM_NSIG):
        seed = G.SEED_BASE + 7700 + 10 * (kind == "msk") + k
        if k < 4:
            rows.append(np.clip(np.round(np.random.default_rng(seed).normal(0.0, 2500.0, n)), -32768, 32767).astype(np.int16))
        elif kind == "oqpsk":
            rows.append(G.oqpsk(n, fc=8000.0 + 9.0 * (k - 5), ebno_db=0.0, seed=seed)[0])
        else:
            rows.append(G.msk(n, fb=1200.0, fc=1000.0 + 4.0 * (k - 5), ebno_db=0.0, seed=seed)[0])
    return np.stack(rows)
