"""Rate meter in front of the demodulator banks (jaero_rate_*, include/jaero_hip.h "rate lines").

`RateMeter` keeps, on the GPU, the Hann-windowed power spectrum of the SQUARED int16 signal of every channel, summed over consecutive
4096-sample segments: MSK (h = 0.5) and the reference's OQPSK both put two spectral lines fb apart there, at 2 f_audio +- fb / 2.
`classify_rates` (host numpy, no hot path) reads a channel's bit rate and audio offset off those sums.  The chain it closes:
capture -> `find_carriers` -> `suggest_gains` -> `duty_cycle` -> `classify_rates` -> the bank and `Channeliser(..., fs_out=...)` a
carrier belongs to.  All device arithmetic happens in libjaero_hip.so; there is no CPU fallback.

Burst channels (jaero_gate_*, include/jaero_hip.h "gated rate lines").  R is a sum over every segment, so the lines of a channel that
is mostly off drown in the segments in which it is off.  A gated meter adds a segment to a channel's R only where the segment's energy
E = sum y^2 reaches the channel's gate, and keeps emax, emin, njoin and ejoin per channel.  The flow:

    m.gate_enable()                            # every gate is 0 at create: everything joins
    ... m.write(...) ...                       # measure the energies
    emax, emin, njoin, ejoin, gate, nseg = m.read_gate()
    m.set_gate(suggest_gate(emax, emin))       # the midpoint for a channel whose segments differ, 0 for one that is continuous
    m.reset()                                  # keeps the gates and the segment grid
    ... m.write(...) ...                       # measure again
    R, nseg = m.read()
    rate, audio, score = classify_rates(R, m.fs)
    duty = m.read_gate()[2] / nseg             # njoin / nseg: how often a channel was on

Limits.  A single click sets emax, and with it the midpoint.  A burst's preamble (a carrier plus lines fb / 2 off it) puts lines fb / 2
apart into the squared signal, so a short 1200 bps burst can read 600: on the CPU oracle a 500-bit burst did exactly that, which is
why the bursts of the tests are long.

One-pass gates (jaero_gate2_*, include/jaero_hip.h "one-pass gates").  The flow above needs the signal twice.  Under
gate_enable(auto=True) the device chooses every gate itself, segment by segment, as suggest_gate would from emin and e2, the SECOND
largest segment energy: a channel runs under gate 0 until its segments differ by 3 / 2, then restarts -- R is assigned, not added to --
at the first segment that reaches the new gate, and `start` is that segment's number.  The one-pass flow:

    m.gate_enable(auto=True); ... m.write(...) ...; R, nseg = m.read(); classify_rates(R, m.fs); duty = njoin / (nseg - start)

with emax, emin, njoin, ejoin, e2, start, gate, nseg = m.read_gate_auto() (start is 2^64 - 1 for a channel that never restarted: its
duty cycle is njoin / nseg).  One click cannot move the gate, because it only ever becomes emax.  gate_enable(hist=True), alone or with
auto, also counts every completed segment's energy in a histogram of 321 bins, eight an octave (`energy_bin`, `bin_edge`), which gives
the click-proof two-pass flow for a caller who wants the gates fixed before the pass that counts:

    m.gate_enable(hist=True); ... m.write(...) ...; hist, nseg = m.read_gate_hist()
    m.set_gate(suggest_gate(*hist_extremes(hist))); m.reset(); ... m.write(...) ...; R, nseg = m.read()

hist_extremes takes the highest and the lowest bin that hold at least two segments, so one click and one dropout fall out.
gate_enable(auto=True) followed by gate_enable() freezes the device's gates for a second pass in the same way.

Limits of the one-pass gates.  Two clicks set e2.  A dropout (a segment of zeros) sets emin for good.  The segments joined while the
gate was still rising stay in R: on the burst rows of the tests that is one of 26.

Rate lines, read on the device (jaero_lines_classify, include/jaero_hip.h "rate lines, read on the device").  `read()` brings 16 KB a
channel to the host; everything `classify_rates` does to them before its log10 is selection -- a median, a three-bin maximum, a search
over pairs of bins -- and `classify_lines` does that where R lies, bit for bit, so that floor, nd scores and nd positions a channel
come back.  `decide_rates` finishes on those.  In every flow above

    R, nseg = m.read(); rate, audio, score = classify_rates(R, m.fs)      becomes      rate, audio, score = m.classify()

with equal results (np.array_equal), in every gate mode; classify_rates stays, and is the reference the one-call form is tested against.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import numpy as np

from . import capi

L = capi.RATE_L        # segment length, samples
BINS = capi.RATE_BINS  # bins 0 .. L / 2 of a channel's row
HBINS = capi.GATE_HBINS  # bins of a channel's histogram of segment energies
RATES = (600, 1200, 8400, 10500)


class RateMeter:
    """The rate lines of `nch` rows of int16 PCM (thin wrapper over jaero_rate).  fs: the rows' sample rate in Hz, a label kept
    for `classify_rates` -- it enters no device arithmetic.  max_write_samples: most samples per row one write may bring."""

    def __init__(self, nch: int, fs: float, device: int = 0, max_write_samples: int = 4 * L):
        self.lib = capi.lib()
        h = C.c_void_p()
        capi.check(self.lib.jaero_rate_create(device, int(nch), int(max_write_samples), C.byref(h)))
        self.h = h
        self.nch, self.fs, self.device, self.max_write_samples = int(nch), float(fs), device, int(max_write_samples)

    def close(self):
        if getattr(self, "h", None):
            self.lib.jaero_rate_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def write(self, pcm: np.ndarray, stream: int = 0) -> int:
        """Consumes a host int16 array [nch, n]; returns the segments this write completed."""
        a = np.ascontiguousarray(pcm, dtype=np.int16)
        if a.ndim != 2 or a.shape[0] != self.nch:
            raise ValueError(f"write takes [{self.nch}, n] int16, not {a.shape}")
        return self._write(a.ctypes.data, a.shape[1], 0, stream)

    def write_device(self, ptr: int, n: int, stream: int = 0) -> int:
        """The same for int16 [nch][n] in device memory at `ptr` (it must stay valid until the stream has passed the write)."""
        return self._write(ptr, n, 1, stream)

    def write_from(self, chan, stream: int = None) -> int:
        """Writes a channeliser's last output (`chan.pcm_view()`) with no host copy, on the stream the channeliser's last write used
        (stream None) -- behind that write, and in front of the channeliser's next one on that stream, which overwrites the output."""
        if chan.nch != self.nch:
            raise ValueError(f"the channeliser has {chan.nch} channels, the rate meter {self.nch}")
        ptr, n = chan.pcm_view()
        return self._write(ptr, n, 1, chan.last_stream if stream is None else stream) if n > 0 else 0

    def _write(self, ptr, n, dev, stream):
        done = C.c_int(0)
        capi.check(self.lib.jaero_rate_write(self.h, ptr, int(n), dev, C.c_void_p(stream), C.byref(done)))
        return done.value

    def read(self) -> Tuple[np.ndarray, int]:
        """(R [nch, 2049], nseg): the sums and the number of segments in them (synchronises)."""
        R = np.empty((self.nch, BINS), dtype=np.float64)
        n = C.c_longlong(0)
        capi.check(self.lib.jaero_rate_read(self.h, R.ctypes.data, C.byref(n)))
        return R, n.value

    def reset(self):
        """Clears the sums, the count and (gated) the four numbers (synchronises); the pending partial segment stays, so the segment grid
        stays absolute, and so do the gates."""
        capi.check(self.lib.jaero_rate_reset(self.h))

    def gate_enable(self, on: bool = True, auto: bool = False, hist: bool = False):
        """Switches between the gated meter and the ungated one it is at create (synchronises).  Either way the sums, the count and the
        four numbers are cleared as by reset(); the pending partial segment and the gates stay.  auto: the device chooses every gate,
        segment by segment (the gates start from 0; `set_gate` is refused).  hist: every completed segment's energy is also counted in
        a histogram (`read_gate_hist`), under the device's gates (auto) or the caller's.  Both need `on`."""
        if not auto and not hist:
            capi.check(self.lib.jaero_gate_enable(self.h, int(on)))
            return
        if not on:
            raise ValueError("gate_enable(False) takes neither auto nor hist")
        mode = (capi.GATE_AUTO if auto else capi.GATE_MANUAL) | (capi.GATE_HIST if hist else 0)
        capi.check(self.lib.jaero_gate2_enable(self.h, mode))

    def set_gate(self, g):
        """g: `nch` non-negative integers below 2^64, one gate per channel; they hold for the segments that later writes complete
        (synchronises, clears nothing).  A segment joins its channel's R iff its energy sum y^2 reaches the gate."""
        if np.ndim(g) != 1 or len(g) != self.nch or any(int(v) < 0 or int(v) >= 1 << 64 for v in g):
            raise ValueError(f"set_gate takes {self.nch} integers in [0, 2^64)")
        a = np.array([int(v) for v in g], dtype=np.uint64)
        capi.check(self.lib.jaero_gate_set(self.h, a.ctypes.data))

    def read_gate(self):
        """(emax, emin, njoin, ejoin, gate, nseg): per channel, as uint64 arrays, the largest and the smallest segment energy, the number
        of segments that joined and the sum of their energies since the last reset, and the gates; nseg counts every completed segment
        (synchronises).  With no segment yet: 0, 2^64 - 1, 0, 0."""
        st = np.empty((self.nch, 4), dtype=np.uint64)
        gate = np.empty(self.nch, dtype=np.uint64)
        n = C.c_longlong(0)
        capi.check(self.lib.jaero_gate_read(self.h, st.ctypes.data, gate.ctypes.data, C.byref(n)))
        return st[:, 0].copy(), st[:, 1].copy(), st[:, 2].copy(), st[:, 3].copy(), gate, n.value

    def read_gate_auto(self):
        """(emax, emin, njoin, ejoin, e2, start, gate, nseg) of a meter under gate_enable(auto=True): `read_gate`'s numbers, the second
        largest segment energy e2, the segment (counted from the last reset) at which the channel restarted -- 2^64 - 1: it never
        did --, and the gates the device holds now (synchronises).  njoin and ejoin count from the restart."""
        st = np.empty((self.nch, 6), dtype=np.uint64)
        gate = np.empty(self.nch, dtype=np.uint64)
        n = C.c_longlong(0)
        capi.check(self.lib.jaero_gate2_read(self.h, st.ctypes.data, gate.ctypes.data, C.byref(n)))
        return tuple(st[:, i].copy() for i in range(6)) + (gate, n.value)

    def read_gate_hist(self):
        """(hist uint32 [nch, 321], nseg) of a meter under gate_enable(hist=True): hist[c, b] counts the segments of channel c since the
        last reset, joined or not, whose energy fell into bin b (`energy_bin`); a row sums to nseg (synchronises)."""
        hist = np.empty((self.nch, HBINS), dtype=np.uint32)
        n = C.c_longlong(0)
        capi.check(self.lib.jaero_gate2_read_hist(self.h, hist.ctypes.data, C.byref(n)))
        return hist, n.value

    def classify_lines(self, d: Sequence[int], kmin: int = 8):
        """(floor [nch], score [nch, nd], where [nch, nd] int32, nseg): the rate lines read on the device (jaero_lines_classify).  d: 1 to
        8 line distances in bins (`rate_distances`).  floor is the median of R[kmin:]; score[i] the largest min(P[a], P[a + d[i]]) over
        kmin <= a < 2049 - d[i], P the three-bin maximum, and where[i] the smallest a that attains it; a distance with kmin + d[i] >= 2049
        is skipped (score 0, where -1).  floor and score are elements of R (or the mean of two) bit for bit.  Synchronises; changes nothing
        of the meter.  `kernel_ms` holds the HIP-event time of this call's launch."""
        dd = np.ascontiguousarray(d, dtype=np.int32).reshape(-1)
        if dd.size and not np.array_equal(dd, np.asarray(d).reshape(-1)):
            raise ValueError("classify_lines takes integer distances")
        nd = int(dd.size)
        floor = np.empty(self.nch, dtype=np.float64)
        score = np.empty((self.nch, max(nd, 1)), dtype=np.float64)
        where = np.empty((self.nch, max(nd, 1)), dtype=np.int32)
        n, ms = C.c_longlong(0), C.c_double(0.0)
        capi.check(self.lib.jaero_lines_classify(self.h, int(kmin), nd, dd.ctypes.data, floor.ctypes.data, score.ctypes.data, where.ctypes.data,
                                                 C.byref(n), C.byref(ms)))
        self.kernel_ms = ms.value
        return floor, score, where, n.value

    def classify(self, rates: Sequence[float] = RATES, threshold_db: float = 10.0, kmin: int = 8):
        """(rate [nch], audio_hz [nch], score_db [nch, len(rates)]): `classify_rates(self.read()[0], self.fs, ...)` without the copy of R --
        `classify_lines` on the device, `decide_rates` on its few numbers a channel.  The two are equal, not merely close."""
        d = rate_distances(self.fs, rates)
        floor, score, where, _ = self.classify_lines(d, kmin)
        return decide_rates(floor, score, where, d, self.fs, rates, threshold_db)

    def poke(self, R: np.ndarray, nseg: int):
        """Test hook (jaero_debug_rate_poke): overwrites the sums with R [nch, 2049] and the segment count with nseg (synchronises)."""
        a = np.ascontiguousarray(R, dtype=np.float64)
        if a.shape != (self.nch, BINS):
            raise ValueError(f"poke takes [{self.nch}, {BINS}] float64, not {a.shape}")
        capi.check(self.lib.jaero_debug_rate_poke(self.h, a.ctypes.data, int(nseg)))

    def profile_enable(self, on: bool = True):
        capi.check(self.lib.jaero_rate_profile_enable(self.h, int(on)))

    def profile_read(self, reset: bool = False) -> Tuple[float, int]:
        """(total ms, launches) of the line kernel since the last reset."""
        ms, n = C.c_double(0), C.c_int(0)
        capi.check(self.lib.jaero_rate_profile_read(self.h, 0, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value


def suggest_gate(emax, emin, min_ratio: float = 1.5):
    """Gates from `read_gate`'s emax and emin, in exact integer arithmetic (a list of Python ints, as `set_gate` takes them): the midpoint
    (emax + emin) // 2 where emax > 0 and emax >= min_ratio emin, else 0.  min_ratio is taken as the exact fraction it is written as
    (1.5 = 3 / 2: 2 emax >= 3 emin).  A channel whose strongest and weakest segment differ by less than 1.8 dB counts as continuous and
    joins everything: 256 segments of white noise or of continuous MSK differ by 1.15.  A single click sets emax; it does not move
    `hist_extremes`' pair, which this function takes as well (the empty pair 0, 2^64 - 1 gives gate 0)."""
    from fractions import Fraction

    r = Fraction(str(min_ratio))
    out = []
    for hi, lo in zip(emax, emin):
        hi, lo = int(hi), int(lo)
        out.append((hi + lo) // 2 if hi > 0 and hi * r.denominator >= lo * r.numerator else 0)
    return out


def energy_bin(E: int) -> int:
    """The histogram bin of a segment energy E >= 0, in exact integers as the device forms it: E itself below 8, else
    8 (e - 2) + ((E >> (e - 3)) & 7) with e = floor(log2 E) -- eight bins an octave -- and never past the last bin, 320, which is where
    the largest possible energy 4096 * 32768^2 = 2^42 lands."""
    E = int(E)
    if E < 0:
        raise ValueError("an energy is not negative")
    if E < 8:
        return E
    e = E.bit_length() - 1
    return min(8 * (e - 2) + ((E >> (e - 3)) & 7), HBINS - 1)


def bin_edge(b: int) -> int:
    """The smallest energy of bin b (0 .. 320): b below 8, else (8 + b mod 8) << (b div 8 - 1)."""
    b = int(b)
    if not 0 <= b < HBINS:
        raise ValueError(f"bins run 0 .. {HBINS - 1}")
    return b if b < 8 else (8 + b % 8) << (b // 8 - 1)


def hist_extremes(hist, min_count: int = 2):
    """(emax~, emin~) from `read_gate_hist`'s histogram [nch, 321] (or one row), as uint64 arrays: the lower edges of the highest and of the
    lowest bin that hold at least `min_count` segments; (0, 2^64 - 1), the empty pair, for a row with no such bin.  With min_count 2 one
    click and one dropout fall out, so suggest_gate(*hist_extremes(hist)) is a gate that one click cannot move."""
    h = np.atleast_2d(np.asarray(hist))
    if h.shape[1] != HBINS:
        raise ValueError(f"a histogram row has {HBINS} bins, not {h.shape[1]}")
    hi, lo = [], []
    for row in h:
        bins = np.flatnonzero(row >= min_count)
        hi.append(bin_edge(bins[-1]) if len(bins) else 0)
        lo.append(bin_edge(bins[0]) if len(bins) else (1 << 64) - 1)
    return np.array(hi, dtype=np.uint64), np.array(lo, dtype=np.uint64)


def classify_rates(R: np.ndarray, fs: float, rates: Sequence[float] = RATES, threshold_db: float = 10.0, kmin: int = 8):
    """(rate [nch], audio_hz [nch], score_db [nch, len(rates)]) from the rate lines R [nch, 2049] (or one row) of rows sampled at `fs`.

    Per row: bw = fs / L is a bin; floor = median(R[kmin:]); P[k] = max(R[k - 1], R[k], R[k + 1]) (clipped at the ends) lets a line sit
    between two bins.  For each rate fb, d = round(fb / bw) is the distance of its two lines; the rate is skipped (score_db = -inf) when
    kmin + d >= 2049.  score = max over kmin <= a < 2049 - d of min(P[a], P[a + d]), the first maximum; score_db = 10 log10(score /
    floor).  The row's rate is the one with the largest score if that reaches `threshold_db`, else 0; its audio offset is the lines'
    midpoint halved, (2 a + d) bw / 4, nan when the rate is 0.

    What the min of the two lines buys: one CW carrier (one line in the squared signal) does not read as a rate, however strong.  What
    it cannot tell: two CW carriers exactly fb apart read as that rate.  The lines must lie inside the measured band: 2 f_audio + fb / 2
    below fs / 2 and 2 f_audio - fb / 2 above kmin bw.  A burst channel's lines are diluted by its duty cycle, because the sums are
    means over every segment: its rate must be taken while it is on.  `RateMeter.gate_enable` / `set_gate` / `suggest_gate` do that
    (the module docstring has the flow); R of a gated meter is classified here like any other."""
    R2 = np.atleast_2d(np.asarray(R, dtype=np.float64))
    nch, nb = R2.shape
    bw = float(fs) / L
    P = np.maximum(R2, np.maximum(np.concatenate([R2[:, :1], R2[:, :-1]], axis=1), np.concatenate([R2[:, 1:], R2[:, -1:]], axis=1)))
    floor = np.median(R2[:, kmin:], axis=1)
    score_db = np.full((nch, len(rates)), -np.inf)
    where = np.zeros((nch, len(rates)), dtype=np.int64)
    ds = []
    for i, fb in enumerate(rates):
        d = int(round(fb / bw))
        ds.append(d)
        if kmin + d >= nb:
            continue
        m = np.minimum(P[:, kmin:nb - d], P[:, kmin + d:nb])
        a = np.argmax(m, axis=1)  # the first of equal maxima
        where[:, i] = a + kmin
        with np.errstate(divide="ignore", invalid="ignore"):
            s = 10.0 * np.log10(m[np.arange(nch), a] / floor)
        score_db[:, i] = np.where(np.isnan(s), -np.inf, s)  # an all-zero row scores nothing
    best = np.argmax(score_db, axis=1)
    top = score_db[np.arange(nch), best]
    hit = top >= threshold_db
    rate = np.where(hit, np.asarray(rates)[best], 0)
    audio = np.where(hit, (2 * where[np.arange(nch), best] + np.asarray(ds)[best]) * bw / 4.0, np.nan)
    if np.ndim(R) == 1:
        return rate[0], audio[0], score_db[0]
    return rate, audio, score_db


def rate_distances(fs: float, rates: Sequence[float] = RATES):
    """The distance in bins of each rate's two lines at sample rate `fs`, round(fb / (fs / 4096)) as `classify_rates` forms it: what
    `RateMeter.classify_lines` takes."""
    bw = float(fs) / L
    return [int(round(fb / bw)) for fb in rates]


def decide_rates(floor, score, where, d: Sequence[int], fs: float, rates: Sequence[float] = RATES, threshold_db: float = 10.0):
    """(rate [nch], audio_hz [nch], score_db [nch, len(rates)]) from `RateMeter.classify_lines`' floor [nch], score and where [nch, nd] for
    the distances d = rate_distances(fs, rates): what `classify_rates` does behind its search, on nd numbers a channel.  score_db = 10
    log10(score / floor), nan -> -inf, a skipped distance (where < 0) -inf; the winner is the first largest score_db -- taken here, on the
    dB values, as classify_rates takes it, so that two raw scores that round to one dB value tie in both --; then the threshold; audio =
    (2 where + d) bw / 4.  One row in (floor a scalar), scalars out."""
    one = np.ndim(floor) == 0
    floor = np.atleast_1d(np.asarray(floor, dtype=np.float64))
    score = np.atleast_2d(np.asarray(score, dtype=np.float64))
    where = np.atleast_2d(np.asarray(where)).astype(np.int64)
    nch = floor.shape[0]
    if len(d) != len(rates) or score.shape != (nch, len(rates)) or where.shape != score.shape:
        raise ValueError("decide_rates takes one distance, one score and one position per rate and channel")
    bw = float(fs) / L
    score_db = np.full((nch, len(rates)), -np.inf)
    for i in range(len(rates)):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            s = 10.0 * np.log10(score[:, i] / floor)
        score_db[:, i] = np.where(np.isnan(s) | (where[:, i] < 0), -np.inf, s)
    where = np.where(where < 0, 0, where)
    best = np.argmax(score_db, axis=1)  # the first of equal maxima
    top = score_db[np.arange(nch), best]
    hit = top >= threshold_db
    rate = np.where(hit, np.asarray(rates)[best], 0)
    audio = np.where(hit, (2 * where[np.arange(nch), best] + np.asarray(d)[best]) * bw / 4.0, np.nan)
    if one:
        return rate[0], audio[0], score_db[0]
    return rate, audio, score_db
