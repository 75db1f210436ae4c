"""Shared by tests/test_burst_acq_cases.py (CPU) and tests/test_gpu_burst_acq.py (GPU): configurations, case generators, exact references and
checkers for the two transform kernels of the burst front end (jaero_amd/csrc/k_burst_front.h): k_trident<true> / k_trident<false>
(JAERO/burstoqpskdemodulator.cpp:412-481, JAERO/burstmskdemodulator.cpp:444-520) and k_hilbert_fft behind k_hist_push_frames /
k_hist_push_chmajor (JAERO/DSP.cpp:754-794).  No GPU code here.

Three things are compared.
  candidate  what is under test: the kernels' output; in the CPU test the oracle's own output, a plain numpy restatement (numpy_trident), or
             a deliberately wrong copy of either
  oracle     oracle.trident (jo_trident: the functions the oracle's burst demodulators call, so what tests/test_oracle_vs_ref.py pins to the
             unmodified reference) and oracle.hilbert_stream
  exact      long-double DFT sums X[k] = sum_n x[n] exp(-2 pi i k n / 32768) at the bins that decide a result, and the long-double direct form
             im y[m] = sum over odd k of g[k] x[m - L - k] / 32768 with g from oracle.hilbert_kernel, L = 6145

Trident (check_trident).  A window is tri_sz samples; the base part is its first nb samples, the top part the nt behind them.
  searches   restated in numpy on the oracle's |base| and |top| (admissible): the strongest base bin, for burst OQPSK the largest trident sum
             d[k - b] + d[k + b] - d[k] with d = |top| - |base|, for burst MSK the strongest top bin below and above the base peak.  First
             maximum, strict compare, as the reference scans.
  draws      carrier at f0 in the base part, two tones at f0 +- fb / 4 (OQPSK) or f0 +- fb / 2 (MSK) in the top part, level 1.414 (the AGC's
             target), random phase, Gaussian noise of 0 .. 0.5 of the level, f0 random inside the band.  A draw is ACCEPTED if every search's
             winner beats every other bin of its range (adjacent ones included) by more than MARGIN = 1e-9 of the winner, and the threshold
             term on a value (> 500) is clear by the same relative amount; the other two terms (< 20 Hz, < |psb / 20|) compare whole bins and
             are clear whenever the winners are.  At most 1 draw in 20 may be rejected per configuration (population asserts it; numpy
             transforms of 200 such draws per configuration had smallest margins of 2e-6, 7e-6 and 1e-4).
  ok, freq   equal to the oracle's exactly on accepted draws and on deliberate cases.  One kind of deliberate case cannot have an exact
             answer: a window that is a single sample away from index 0 has |X[k]| equal for ALL k up to rounding, so the oracle's own winner is
             decided by its last bits (bin 17 of 16384 equal ones in one such case).  There a search's admissible winners are all the bins within
             MARGIN of the maximum (when those bins are exactly equal the first one is the only admissible winner: the first-maximum rule is
             still tested, as on the all-zero window and the sample at index 0), ok is decided by the value terms alone (asserted clear), and
             the candidate's freq must be one an admissible winner gives.  The phase is then checked at the candidate's own bin (OQPSK; burst
             MSK's result does not tell the bin, its phase is not checked on those cases).
  values     metric, vol_gain and phase_deg against the exact values (exact_values).  For each, E_o = the oracle's largest error over the
             configuration's accepted draws, relative to the draw's strongest base magnitude (metric: |metric - exact| / |base|max, on a deliberate
             case whose top part is the stronger one / |top|max; vol_gain:
             its relative error, which is that of the strongest base magnitude; phase: radians).  The candidate's error on every draw and
             deliberate case must be <= 4 * E_o + 4 * 2^-52 in the same units: 4 is what pre8400_cases grants another factorisation of the same
             transform length class (the kernel splits 2^15 points into four 2^13-point transforms of 32 x 16 x 16, the oracle runs one radix-2
             plan), the additive term covers draws on which the oracle happens to be exact.  Values that are not finite or come from an
             all-zero part (vol_gain = inf, phase of 0 + 0j) must equal the oracle's bit for bit.
  lists      check_event_list: every listed channel holds its own result, nchanged == nlist, nothing else lost its sentinel.

Hilbert (check_hilbert).  Two real channels (2c, 2c + 1) ride one complex transform pair, so errors are relative to the peak of the PAIR:
  e_cand <= 8 * e_oracle + 4 * 2^-52 against the exact sum: 4 as above, 2 for the partner riding in the imaginary part; e_oracle = the oracle's
  own error against the exact sum on the same channels (the larger of the pair's two).  Channels without an exact sum (the sum is capped at MAX_EXACT_CHANNELS channels and
  MAX_EXACT_SAMPLES samples): |cand - oracle| <= (9 * e_oracle_worst + 4 * 2^-52) * pair peak, at most the two errors added.  Where both
  channels of a pair are silent the output is exactly zero.  A silent channel beside a live partner falls under the pair's bound; it is NOT a
  zero: the partner's rounding leaks across the pair (the same reason the reference's own FFT leaves ~1e-17 where the exact answer is zero,
  see the note in tests/test_gpu_burst.py::check_symbols_behind_sets).
Every module prints its errors in units of 2^-52 before it asserts."""
import math
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
N, NH = 32768, 16384
FS = 48000.0
HZ = FS / N
LEVEL = 1.414
MARGIN = 1e-9
KIND_BURST_MSK, KIND_BURST_OQPSK = 2, 3
HIL_LAT, HIL_TAPS = 6145, 2048
MAX_EXACT_CHANNELS, MAX_EXACT_SAMPLES = 4, 20000
HILBERT_SIZES = [1, 7, 2047, 2048, 2049, 100, 3000]  # and the bank's maximum
NDRAWS = 60  # accepted draws per configuration: with the deliberate cases a window of its own for each of 70 channels


def qround(x):
    return int(math.floor(x + 0.5))


def _cfg(name, kind, fb, f0):
    """The geometry BurstOqpskDemodulator::setSettings / BurstMskDemodulator::setSettings give at 48 kHz, restated (burst_fill_geometry)"""
    if kind == KIND_BURST_OQPSK:
        sps = 2.0 * FS / fb
        nb = nt = qround(128.0 * sps)
        tri_sz = qround(288.0 * sps)
        D1, D2, maxseg = int(sps * 128.0 * 2.5 - 190), tri_sz, 2048
        spacing = qround(0.25 * fb / HZ)
    else:
        sps = float(int(FS / fb))
        if fb >= 1200:
            nb, nt, tri_sz, D1, D2 = qround(126 * sps), qround(74 * sps), qround(200.0 * sps), int(289 * sps + 20), int(192 * sps)
        else:
            nb, nt, tri_sz, D1, D2 = qround(150 * sps), qround(74 * sps), qround(224 * sps), int(397 * sps + 20), qround(222 * sps)
        maxseg = 4096
        spacing = qround(0.5 * fb / HZ)
    return SimpleNamespace(name=name, kind=kind, oq=kind == KIND_BURST_OQPSK, fb=fb, sps=sps, nb=nb, nt=nt, tri_sz=tri_sz, D1=D1, D2=D2,
                           maxseg=maxseg, spacing=spacing, f0=f0, tone=fb / 4.0 if kind == KIND_BURST_OQPSK else fb / 2.0)


CONFIGS = {
    "oqpsk": _cfg("oqpsk", KIND_BURST_OQPSK, 10500.0, (6000.0, 10000.0)),
    "msk1200": _cfg("msk1200", KIND_BURST_MSK, 1200.0, (1000.0, 3000.0)),
    "msk600": _cfg("msk600", KIND_BURST_MSK, 600.0, (800.0, 3000.0)),
}
assert (CONFIGS["oqpsk"].nb, CONFIGS["oqpsk"].tri_sz) == (1170, 2633)
assert (CONFIGS["msk1200"].nb, CONFIGS["msk1200"].nt) == (5040, 2960)
assert (CONFIGS["msk600"].nb, CONFIGS["msk600"].nt) == (12000, 5920)


def geometry(cfg, nch, max_write):
    """What jaero_debug_burst_geom must report for a bank of nch channels (all but tri_grid and nsamples)"""
    maxseg = cfg.maxseg if cfg.maxseg <= max_write else (max_write + 15) // 16 * 16
    return dict(kind=cfg.kind, nch=nch, nchp=(nch + 63) // 64 * 64, maxseg=maxseg, hist_len=(HIL_LAT + 2 * HIL_TAPS + max_write + 64 + 3) & ~3,
                hil_lat=HIL_LAT, cv_len=cfg.D1 + max(cfg.D2, cfg.tri_sz) + maxseg + 64, D1=cfg.D1, tri_sz=cfg.tri_sz, nb=cfg.nb, nt=cfg.nt)


# ----------------------------------------------------------------------------------------------- windows
def make_window(cfg, rng, base_hz=None, top_hz=None, base_level=LEVEL, top_level=LEVEL, sigma=0.0, tone_hz=None, phase=None):
    """tri_sz samples: a carrier at base_hz in the base part, two tones at top_hz +- tone_hz in the top part (each top_level / sqrt 2), Gaussian
    noise of sigma * LEVEL over both.  What lies behind the two parts (burst OQPSK: 293 samples the check never reads) is noise of the level."""
    n = np.arange(cfg.tri_sz)
    ph = rng.uniform(0, 2 * np.pi) if phase is None else phase
    tone = cfg.tone if tone_hz is None else tone_hz
    w = rng.normal(0.0, LEVEL, cfg.tri_sz)
    nb, e = cfg.nb, cfg.nb + cfg.nt
    w[:nb] = base_level * np.cos(2 * np.pi * base_hz * n[:nb] / FS + ph) if base_level else 0.0
    w[nb:e] = top_level * (np.cos(2 * np.pi * (top_hz - tone) * n[nb:e] / FS + ph) + np.cos(2 * np.pi * (top_hz + tone) * n[nb:e] / FS + ph)) / np.sqrt(2) if top_level else 0.0
    if sigma:
        w[:e] += rng.normal(0.0, sigma * LEVEL, e)
    return w


def draw(cfg, rng):
    f0 = rng.uniform(*cfg.f0)
    return make_window(cfg, rng, f0, f0, sigma=rng.uniform(0.0, 0.5))


def single_sample(cfg, index, value=100.0):
    w = np.zeros(cfg.tri_sz)
    w[index] = value
    return w


# ----------------------------------------------------------------------------------------------- restated searches
def _winners(v, idx, from_zero):
    """Admissible winners of a first-maximum scan of v[idx] with a strict compare: (bins, margin).  from_zero: the scan starts from the value 0
    (nothing wins unless it exceeds 0: an empty list), else from its first entry.  One bin when the maximum is clear of every other bin by
    MARGIN, or when all bins within MARGIN of it are exactly equal (the first one wins, margin 0); otherwise every bin within MARGIN: the winner is
    decided by the last bits of whoever computes the values."""
    if len(idx) == 0:
        return [], 1.0
    vals = v[idx]
    m = vals.max()
    if from_zero and not m > 0.0:
        return [], 1.0
    near = idx[vals >= m - abs(m) * MARGIN]
    if len(near) == 1:
        rest = np.delete(vals, int(np.argmax(vals)))
        return [int(near[0])], (float((m - rest.max()) / abs(m)) if len(rest) and m != 0 else 1.0)
    if np.all(v[near] == m):
        return [int(near[0])], 0.0
    return [int(k) for k in near], 0.0


def admissible(cfg, B, T):
    """The restated searches on |base| and |top|: a namespace with the admissible winners of each search (base, top), the smallest winner margin,
    the value the > 500 term tests and whether it is clear, and the set of admissible (ok, freq) outcomes (one element unless a search is
    decided by rounding)."""
    out = SimpleNamespace(outcomes=set())
    if cfg.oq:
        mb, out.margin = _winners(B, np.arange(NH), False)  # starts from |base[0]|
        b = cfg.spacing
        d = T - B
        k = np.arange(b, NH - b)
        tv = np.full(NH, -np.inf)
        tv[k] = d[k - b] + d[k + b] - d[k]
        out.top, mt = _winners(tv, k, False)
        out.margin = min(out.margin, mt)
        mx = float(tv[out.top[0]])
        out.value, out.value_clear = mx, abs(mx - 500.0) > 500.0 * MARGIN
        if not mx > 500.0:
            out.outcomes = {(0, HZ * float(m)) for m in mb}
        else:
            assert len(out.top) * len(mb) <= 1 << 16, "two searches of a window decided by rounding among many bins"
            out.outcomes = {(int(abs(float(t - m) * HZ) < 20.0), HZ * float(m)) for t in out.top for m in mb}
    else:
        mb, out.margin = _winners(B, np.arange(NH), True)
        mb = mb or [0]
        psb = cfg.spacing
        out.value, out.value_clear = float(B.max()), abs(B.max() - 500.0) > 500.0 * MARGIN
        los, his = set(), set()
        for m in mb:
            lo, ml = _winners(T, np.arange(51, max(51, m - psb // 2)), True)
            hi, mh = _winners(T, np.arange(max(51, m + psb // 2 + 1), NH), True)
            out.margin = min(out.margin, ml, mh)
            assert len(lo) <= 1 or len(hi) <= 1, "both top searches of a window decided by rounding"
            for l in lo or [0]:
                for h in hi or [0]:
                    out.outcomes.add((int(B.max() > 500.0 and abs(abs(l - m) - psb) < abs(psb // 20)), float((h + l) // 2) * HZ))
                    los.add(l); his.add(h)
        out.top = sorted(los) + sorted(his)
    out.base = mb
    out.decided = len(out.outcomes) == 1 and len(mb) == 1 and (not cfg.oq or len(out.top) == 1)
    out.accepted = out.decided and out.margin > MARGIN and out.value_clear
    return out


# ----------------------------------------------------------------------------------------------- exact values
_cis = {}


def _dft_ld(x, k):
    """sum_n x[n] exp(-2 pi i k n / N) in long double: (re, im)"""
    if "c" not in _cis:
        a = np.arange(N, dtype=LD) * (LD(2) * np.arctan2(LD(0), LD(-1)) / LD(N))
        _cis["c"], _cis["s"] = np.cos(a), np.sin(a)
    idx = (np.arange(len(x), dtype=np.int64) * int(k)) % N
    xl = x.astype(LD)
    return np.sum(xl * _cis["c"][idx]), -np.sum(xl * _cis["s"][idx])


def _abs_ld(x, k):
    re, im = _dft_ld(x, k)
    return np.sqrt(re * re + im * im)


def exact_values(cfg, w, base_bin, top_bin=None):
    """(metric, vol_gain, phase_deg) in long double for the winners given (OQPSK: top_bin = the bin of the winning trident sum, whose six
    bins are summed; MSK: the metric is the strongest base magnitude)"""
    base, top = w[:cfg.nb], w[cfg.nb:cfg.nb + cfg.nt]
    re, im = _dft_ld(base, base_bin)
    minval = np.sqrt(re * re + im * im)
    pi = LD(2) * np.arctan2(LD(1), LD(0))
    phase_deg = (np.arctan2(im, re) - pi / 4) * 180 / pi
    with np.errstate(divide="ignore"):
        if cfg.oq:
            b = cfg.spacing
            d = lambda k: _abs_ld(top, k) - _abs_ld(base, k)
            return d(top_bin - b) + d(top_bin + b) - d(top_bin), LD(1.4142) * 500 / minval, phase_deg
        return minval, LD(1.4142) * (500 / (minval / 3)), phase_deg


def value_errors(cfg, res, exact, scale):
    """[metric, vol_gain, phase] errors of a result in the units of the module docstring; None where the exact value is not finite or the
    base part is all zero (those are compared bit for bit)"""
    em = float(abs(LD(res.metric) - exact[0]) / LD(scale))
    if not np.isfinite(exact[1]):
        return [em, None, None]
    ev = float(abs(LD(res.vol_gain) - exact[1]) / abs(exact[1]))
    dp = float((LD(res.phase_deg) - exact[2])) * math.pi / 180.0
    return [em, ev, abs((dp + math.pi) % (2 * math.pi) - math.pi)]


# ----------------------------------------------------------------------------------------------- cases
def make_case(O, cfg, w, label, deliberate=False):
    r, B, T = O.trident(cfg.kind, FS, cfg.fb, w)
    res = SimpleNamespace(ok=r.ok, freq=r.freq, phase_deg=r.phase_deg, vol_gain=r.vol_gain, metric=r.metric)
    a = admissible(cfg, B, T)
    c = SimpleNamespace(cfg=cfg, label=label, window=w, oracle=res, adm=a, deliberate=deliberate, bmax=float(B.max()), tmax=float(T.max()), exact=None, e_oracle=None)
    c.scale = max(c.bmax, c.tmax) or 1.0  # the strongest base magnitude on every draw (the top part's two tones are 3 dB down each)
    assert (res.ok, res.freq) in a.outcomes, (cfg.name, label, "the restated searches left the oracle's", (res.ok, res.freq), sorted(a.outcomes)[:4])
    if a.decided:
        c.exact = exact_values(cfg, w, a.base[0], a.top[0] if cfg.oq else None)
        c.e_oracle = value_errors(cfg, res, c.exact, c.scale)
    return c


_pop = {}


def population(O, name, n, seed=0xACC):
    """n ACCEPTED draws of a configuration with the oracle's results and the exact values, computed once per session:
    (cases, E_o = (metric, vol_gain, phase) worst oracle errors, rejected).  At most 1 draw in 20 may be rejected."""
    key = (name, n, seed)
    if key not in _pop:
        cfg = CONFIGS[name]
        rng = np.random.default_rng(seed + sum(map(ord, name)))
        cases, rejected = [], 0
        while len(cases) < n:
            c = make_case(O, cfg, draw(cfg, rng), f"draw {len(cases) + rejected}")
            if c.adm.accepted:
                cases.append(c)
            else:
                rejected += 1
            assert rejected * 20 <= max(20, len(cases) + rejected), (name, f"{rejected} draws rejected among {len(cases) + rejected}")
        E = tuple(max(c.e_oracle[i] for c in cases) for i in range(3))
        print(f"burst_acq {name}: {n} draws accepted, {rejected} rejected, smallest winner margin {min(c.adm.margin for c in cases):.2e}; oracle's worst "
              f"errors: metric {E[0] / EPS:.2f} eps, vol_gain {E[1] / EPS:.2f} eps, phase {E[2] / EPS:.2f} eps")
        _pop[key] = (cases, E, rejected)
    return _pop[key]


def _find_offset(O, cfg, rng, want):
    """burst OQPSK: a noise-free window with bin-centred tones whose trident winner lies `want` bins above its base winner.  The top part's centre
    is moved bin by bin until the restated searches say so (the weak base part's leakage pulls the sum's maximum a little)."""
    kb = 5461
    for o in range(want, want + 12):
        w = make_window(cfg, rng, kb * HZ, (kb + o) * HZ, base_level=0.25 * LEVEL)
        c = make_case(O, cfg, w, f"top {want} bins above the base (tones centred {o} bins up)", True)
        if c.adm.decided and c.adm.top[0] - c.adm.base[0] == want and c.adm.margin > MARGIN:
            return c
    raise AssertionError(f"no offset gives a winner {want} bins up")


_delib = {}


def deliberate_cases(O, name):
    """The cases of the module docstring's 'deliberate' kind for one configuration, computed once per session"""
    if name in _delib:
        return _delib[name]
    cfg = CONFIGS[name]
    rng = np.random.default_rng(0xDE11 + sum(map(ord, name)))
    f0 = 0.5 * (cfg.f0[0] + cfg.f0[1])
    ws = [
        ("all-zero window", np.zeros(cfg.tri_sz)),
        ("zero base, live top", make_window(cfg, rng, f0, f0, base_level=0.0, sigma=0.1)),
        ("live base, zero top", make_window(cfg, rng, f0, f0, top_level=0.0)),
        ("level 0.05: metric well below 500", make_window(cfg, rng, f0, f0, base_level=0.05, top_level=0.05, sigma=0.01)),
        ("single sample at index 0", single_sample(cfg, 0)),
        ("single sample at the base part's last index", single_sample(cfg, cfg.nb - 1)),
        ("single sample at the top part's first index", single_sample(cfg, cfg.nb)),
        ("single sample at the top part's last index", single_sample(cfg, cfg.nb + cfg.nt - 1)),
    ]
    ws[2] = (ws[2][0], np.where(np.arange(cfg.tri_sz) < cfg.nb, ws[2][1], 0.0))  # nothing behind the base part at all
    ws[1] = (ws[1][0], np.where(np.arange(cfg.tri_sz) >= cfg.nb, ws[1][1], 0.0))  # and nothing, noise included, in the base part
    cases = [make_case(O, cfg, w, label, True) for label, w in ws]
    if cfg.oq:
        cases += [_find_offset(O, cfg, rng, 13), _find_offset(O, cfg, rng, 14)]
        assert (cases[-2].oracle.ok, cases[-1].oracle.ok) == (1, 0), "13 bins are 19.04 Hz, 14 are 20.51 Hz"
    else:
        psb, kb = cfg.spacing, 1400
        edge = abs(psb // 20)
        for dlt in (edge - 1, edge):
            w = make_window(cfg, rng, kb * HZ, kb * HZ, tone_hz=(psb + dlt) * HZ)
            cases.append(make_case(O, cfg, w, f"tones {dlt} bins off the expected spacing", True))
        assert (cases[-2].oracle.ok, cases[-1].oracle.ok) == (1, 0), (psb, edge)
        w = make_window(cfg, rng, 100 * HZ, 100 * HZ + 2000.0)  # base peak at bin 100 < 50 + psb / 2: the lower search has no candidate
        cases.append(make_case(O, cfg, w, "base peak below bin 50 + psb / 2", True))
        assert 100 < 50 + psb // 2 and cases[-1].oracle.freq == float(cases[-1].adm.top[-1] // 2) * HZ
        if cfg.nb > 8192:
            cases.append(make_case(O, cfg, single_sample(cfg, 8192), "single sample at index 8192 of the base part", True))
            cases.append(make_case(O, cfg, single_sample(cfg, 8191), "single sample at index 8191 of the base part", True))
            w = make_window(cfg, rng, 1365 * HZ, 1365 * HZ)  # a base peak in residue class 1 of the four-way split
            cases.append(make_case(O, cfg, w, "bin-centred carrier at bin 1365 = 4 * 341 + 1", True))
            assert cases[-1].adm.base == [1365]
    for c in cases:
        if not c.adm.decided:
            assert c.adm.value_clear and c.adm.value < 500.0, (name, c.label, "a case decided by rounding must have ok decided by its value term")
    _delib[name] = cases
    return cases


# ----------------------------------------------------------------------------------------------- trident checker
def _bits(x):
    return np.float64(x).view(np.uint64)


def check_trident(case, cand, E, what=""):
    """The rules of the module docstring for one window; E = the configuration's (metric, vol_gain, phase) oracle errors.  Returns the candidate's
    three errors (None where the value is compared bit for bit or not at all)."""
    cfg, o, a = case.cfg, case.oracle, case.adm
    w = (cfg.name, case.label, what)
    assert cand.ok in (0, 1), w + ("ok", cand.ok)
    assert (int(cand.ok), float(cand.freq)) in a.outcomes, w + (f"(ok, freq) = {(cand.ok, cand.freq)}", "admissible", sorted(a.outcomes)[:4], "oracle", (o.ok, o.freq))
    exact, phase = case.exact, True
    if a.decided:
        assert (cand.ok, cand.freq) == (o.ok, o.freq), w
    elif cfg.oq:  # the base winner is one of many bins equal up to rounding: the values at the candidate's own bin
        kc = qround(cand.freq / HZ)
        assert kc in a.base, w
        exact = exact_values(cfg, case.window, kc, a.top[0])
    else:
        exact, phase = exact_values(cfg, case.window, a.base[0]), False
    errs = value_errors(cfg, cand, exact, case.scale)
    if errs[1] is None:  # an all-zero base part: vol_gain = inf and the phase of 0 + 0j, the same bits as the oracle's
        assert _bits(cand.vol_gain) == _bits(o.vol_gain) and _bits(cand.phase_deg) == _bits(o.phase_deg), w + (cand, o)
    if not phase:
        errs[2] = None
    for name, e, eo in zip(("metric", "vol_gain", "phase"), errs, E):
        assert e is None or e <= 4 * eo + 4 * EPS, w + (f"{name}: candidate {e / EPS:.2f} eps, oracle's worst {eo / EPS:.2f} eps, allowed {(4 * eo + 4 * EPS) / EPS:.2f}",)
    return errs


def check_event_list(listed, results, nchanged, expected, what=""):
    """One launch over `listed` channels: results[k] must be bit for bit expected[listed[k]] (the channel's result of a launch that was
    checked with check_trident) and exactly len(listed) entries of the bank may have lost their sentinel."""
    assert nchanged == len(listed), (what, f"{nchanged} results written for {len(listed)} events")
    for ch, r in zip(listed, results):
        e = expected[ch]
        got = (r.ok, _bits(r.freq), _bits(r.phase_deg), _bits(r.vol_gain), _bits(r.metric))
        assert got == (e.ok, _bits(e.freq), _bits(e.phase_deg), _bits(e.vol_gain), _bits(e.metric)), (what, f"channel {ch}", r, e)


def numpy_trident(cfg, w, wrong=None):
    """A plain numpy restatement of the trident check (numpy's transforms, first-maximum searches): what a right candidate looks like to the
    checker, and with `wrong` the mistakes the checker exists to catch: "last_max" (last maximum among equals), "shift1" (the window read one
    sample late), "nofold" (samples from 8192 on dropped), "sign_r1" (the (-j)^r factor of residue class 1 negated)."""
    if wrong == "shift1":
        w = np.concatenate([w[1:], [0.0]])
    base, top = w[:cfg.nb].copy(), w[cfg.nb:cfg.nb + cfg.nt]
    if wrong == "nofold":
        base[8192:] = 0.0
    Xb, Xt = np.fft.fft(base, N)[:NH], np.fft.fft(top, N)[:NH]
    if wrong == "sign_r1":
        hi = np.zeros(N)
        hi[8192:len(base)] = base[8192:]
        F1 = np.fft.fft(hi, N)[:NH]
        Xb[1::4] -= 2 * F1[1::4]
    B, T = np.abs(Xb), np.abs(Xt)
    first = (lambda v: int(np.flatnonzero(v == v.max())[-1])) if wrong == "last_max" else (lambda v: int(np.argmax(v)))
    mb = first(B) if (B.max() > 0 or wrong == "last_max") else 0
    ph = (180.0 / math.pi) * (math.atan2(Xb[mb].imag, Xb[mb].real) - math.pi / 4.0) if B.max() > 0 else -45.0
    with np.errstate(divide="ignore"):
        if cfg.oq:
            b = cfg.spacing
            d = T - B
            k = np.arange(b, NH - b)
            tv = d[k - b] + d[k + b] - d[k]
            t = first(tv) + b
            mx = float(tv[t - b])
            return SimpleNamespace(ok=int(mx > 500.0 and abs(float(t - mb) * HZ) < 20.0), freq=HZ * float(mb), phase_deg=ph,
                                   vol_gain=float(1.4142 * 500.0 / np.float64(B[mb])), metric=mx)
        psb = cfg.spacing
        lo_r, hi_r = np.arange(51, max(51, mb - psb // 2)), np.arange(max(51, mb + psb // 2 + 1), NH)
        lo = int(lo_r[first(T[lo_r])]) if len(lo_r) and T[lo_r].max() > 0 else 0
        hi = int(hi_r[first(T[hi_r])]) if len(hi_r) and T[hi_r].max() > 0 else 0
        mv = np.float64(B[mb])
        return SimpleNamespace(ok=int(mv > 500.0 and abs(abs(lo - mb) - psb) < abs(psb // 20)), freq=float((hi + lo) // 2) * HZ, phase_deg=ph,
                               vol_gain=float(1.4142 * (500.0 / (mv / 3))), metric=float(mv))


# ----------------------------------------------------------------------------------------------- Hilbert
def fullscale_pcm(nch, n, seed, silent=()):
    """Full-scale random int16 with -32768 and 32767 in every live channel, and the channels of `silent` all zero"""
    rng = np.random.default_rng(seed)
    pcm = rng.integers(-32768, 32768, size=(nch, n), dtype=np.int64).astype(np.int16)
    pcm[:, 0] = -32768
    if n > 3:
        pcm[:, 3] = 32767
    for c in silent:
        pcm[c] = 0
    return pcm


def hilbert_sizes(max_write, total):
    cyc, out = HILBERT_SIZES + [max_write], []
    while sum(out) < total:
        out.append(min(cyc[len(out) % len(cyc)], max_write))
    return out


_g = {}


def exact_hilbert(O, x):
    """im y[m] = sum over odd k of g[k] x[m - L - k] / 32768 in long double for a whole stream from a fresh filter (zeros before sample 0)"""
    assert len(x) <= MAX_EXACT_SAMPLES
    if "g" not in _g:
        k = O.hilbert_kernel(HIL_TAPS)
        assert not k.imag[0::2].any() and k.real[1024] == -1.0 and not np.delete(k.real, 1024).any()
        _g["g"] = k.imag.astype(LD)
    y = np.zeros(len(x), dtype=LD)
    if len(x) > HIL_LAT:
        y[HIL_LAT:] = np.convolve(x[:len(x) - HIL_LAT].astype(LD), _g["g"])[:len(x) - HIL_LAT]
    return y / LD(32768)


def oracle_hilbert(O, pcm, sizes):
    """oracle.hilbert_stream of every channel in the given writes: the imaginary parts [nch][n]"""
    out = np.empty(pcm.shape)
    for c in range(pcm.shape[0]):
        h = O.lib().jo_hilbert_create(HIL_TAPS)
        z = np.zeros(pcm.shape[1], dtype=np.complex128)
        s = 0
        for n in sizes:
            blk = np.ascontiguousarray(pcm[c, s:s + n])
            O.lib().jo_hilbert_update(h, blk.ctypes.data, n, z[s:].ctypes.data)
            s += n
        assert s == pcm.shape[1] and O.lib().jo_hilbert_latency(h) == HIL_LAT
        O.lib().jo_hilbert_destroy(h)
        out[c] = z.imag
    return out


def check_hilbert(cand, oracle, exact, name="", e_oracle_worst=None):
    """cand, oracle: [nch][n] imaginary parts; exact: {channel: long-double sum} for the capped channels.  The rules of the module docstring.
    e_oracle_worst: the bound's e_oracle for the channels without an exact sum when `exact` is empty (a stream's tail behind the capped part).
    Returns (rows (channel, kind, e_cand, e_oracle or None), the largest e_oracle)."""
    assert cand.shape == oracle.shape and len(exact) <= MAX_EXACT_CHANNELS, name
    nch = cand.shape[0]
    peak = lambda c: (float(np.abs(exact[c]).max()) if c in exact else float(np.abs(oracle[c]).max())) if c < nch else 0.0
    rows, worst = [], e_oracle_worst or 0.0
    pairs = [(a, a + 1) for a in range(0, nch, 2)]
    for a, b in pairs:  # the oracle's own error first: the bound of the channels without an exact sum comes from it
        pk = max(peak(a), peak(b))
        for c in (a, b):
            if c in exact:
                worst = max(worst, float(np.abs(oracle[c].astype(LD) - exact[c]).max()) / pk)
    for a, b in pairs:
        pk = max(peak(a), peak(b))
        for c in (a, b):
            if c >= nch:
                continue
            if pk == 0.0:
                rows.append((c, "both silent", 0.0 if not cand[c].any() else float("inf"), None))
            elif c in exact:  # e_oracle of the PAIR: the larger of its channels' errors (a silent channel's own oracle error is 0, its kernel output is not)
                eo = max(float(np.abs(oracle[x].astype(LD) - exact[x]).max()) / pk for x in (a, b) if x in exact)
                rows.append((c, "exact", float(np.abs(cand[c].astype(LD) - exact[c]).max()) / pk, eo))
            else:
                rows.append((c, "oracle", float(np.abs(cand[c] - oracle[c]).max()) / pk, None))
    for c, kind, ec, eo in rows if len(rows) <= 8 else [r for r in rows if r[1] != "oracle"] + [max((r for r in rows if r[1] == "oracle"), key=lambda r: r[2])]:
        print(f"burst_acq hilbert {name} channel {c} ({kind}): candidate {ec / EPS:.2f} eps" + (f", oracle {eo / EPS:.2f} eps of the pair's peak" if eo is not None else ""))
    for c, kind, ec, eo in rows:
        if kind == "both silent":
            assert ec == 0.0, (name, c, "a pair of silent channels must give exact zeros")
        elif kind == "exact":
            assert ec <= 8 * eo + 4 * EPS, (name, c, f"candidate {ec / EPS:.2f} eps, oracle {eo / EPS:.2f} eps, allowed {(8 * eo + 4 * EPS) / EPS:.2f}")
        else:
            assert (exact or e_oracle_worst is not None) and ec <= 9 * worst + 4 * EPS, (name, c, f"|cand - oracle| {ec / EPS:.2f} eps of the pair's peak, allowed {(9 * worst + 4 * EPS) / EPS:.2f}")
    return rows, worst
