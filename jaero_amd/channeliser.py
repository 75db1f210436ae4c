"""Wideband I/Q channeliser in front of the demodulator banks (jaero_chan_*, include/jaero_hip.h).

`Channeliser` cuts one int16 I/Q capture at fs_out x decim into the int16 audio at fs_out (48, 24 or 12 kHz) of every channel
of a bank, on the GPU: `feed(bank, iq)` hands its output straight to `DemodulatorBank` (device to device), `write` / `read_pcm` give it to the
caller.  Frequencies are 32-bit words: `tune_word(hz, fs)` is the word nearest a frequency, `word_hz(word, fs)` the
frequency a word really is, `channel_words(tune, audio, decim)` the integers the kernels derive from a channel's words.
The survey (`survey_enable`, `read_psd`, `read_levels`) measures the capture's spectrum and every channel's level on the device;
`find_carriers` (host numpy, no hot path) turns the spectrum into centre frequencies, `suggest_gains` the levels into gains, and
`retune_all` applies both.  The activity (`activity_enable`, `read_peak_psd`, `read_activity`) keeps the extremes and the distribution of
the same per-block terms: the peak-hold spectrum finds carriers that are seldom on, `duty_cycle` says how often a channel is on and
`suggest_gains(peak=True)` sets a burst channel's gain from its strongest block.  `Channeliser(..., capture=Capture(fs_in=..., fmt=...))` takes an SDR capture in its own format (cs16, cu8, cs8,
cf32) and at its own integer rate: the device converts, shifts the centre by an exact phase word and resamples by the exact rational ratio
to fs_out x decim (jaero_chan3_*); `design_resampler` is the prototype it uses by default.  `Splitter(fs_c, outputs)` is one front end
(one copy, one staging launch, one forward transform per hop) in front of several outputs, each with its own rate, channels and taps and
each feeding its own bank (jaero_split_*); every output is bit for bit what a stand-alone `Channeliser` produces, and `plan_outputs` groups
surveyed carriers by the bit rate the rate meter named into such outputs.  All device arithmetic happens in
libjaero_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import capi

N = 16384          # transform length
HP = N // 2        # hop, input samples
DECIMS = (16, 32, 64, 128, 256)   # total decimation, capture to output
FS_OUT = 48000.0
FS_OUTS = (48000.0, 24000.0, 12000.0)


def tune_word(hz: float, fs: float) -> int:
    """The uint32 word nearest `hz` at sample rate `fs` (negative frequencies wrap: the word is read as a signed number)."""
    return int(round(hz / fs * 4294967296.0)) % (1 << 32)


def word_hz(word: int, fs: float) -> float:
    """The frequency a word stands for: the word as a signed 32-bit number times fs / 2^32."""
    w = int(word) % (1 << 32)
    if w >= 1 << 31:
        w -= 1 << 32
    return w * fs / 4294967296.0


def channel_words(tune: int, audio: int, decim: int) -> Tuple[int, int, int]:
    """(b, rho, w) of a channel: nearest bin of the tuning word, what is left of it, phase word per output sample."""
    t = int(tune) % (1 << 32)
    if t >= 1 << 31:
        t -= 1 << 32
    b = (t + (1 << 17)) >> 18
    rho = t - (b << 18)
    return b, rho, (int(audio) - rho * decim) % (1 << 32)


def design_taps(decim: int, cutoff_hz: Optional[float] = None, ntaps: int = 8193, beta: float = 16.0, fs_out: float = FS_OUT) -> np.ndarray:
    """Kaiser-windowed sinc low-pass at the capture rate fs_out x decim: 2 fc sinc(2 fc k) kaiser(beta), unit sum.
    cutoff_hz None: 9000 at 48 kHz, 0.3125 fs_out otherwise."""
    if cutoff_hz is None:
        cutoff_hz = 9000.0 if fs_out == FS_OUT else 0.3125 * fs_out
    fc = cutoff_hz / (fs_out * decim)
    k = np.arange(ntaps) - (ntaps - 1) / 2
    h = 2 * fc * np.sinc(2 * fc * k) * np.kaiser(ntaps, beta)
    return h / h.sum()


FORMATS = {"cs16": capi.IQ_CS16, "cu8": capi.IQ_CU8, "cs8": capi.IQ_CS8, "cf32": capi.IQ_CF32}
_FORMAT_DTYPE = {"cs16": np.int16, "cu8": np.uint8, "cs8": np.int8, "cf32": np.float32}


def resample_ratio(fs_in: int, fs_c: int) -> Tuple[int, int]:
    """(L, Mr): fs_c / fs_in in lowest terms."""
    fs_in, fs_c = int(fs_in), int(fs_c)
    g = math.gcd(fs_in, fs_c)
    return fs_c // g, fs_in // g


def design_resampler(fs_in: int, fs_c: int, taps_per_phase: int = 32, beta: float = 10.0) -> Tuple[np.ndarray, int, int]:
    """(h, L, Mr): the polyphase prototype of the capture front end (include/jaero_hip.h cites this).  L / Mr = fs_c / fs_in in lowest
    terms, n = L K taps at the rate fs_in L, cut-off fc = 0.5 min(fs_in, fs_c) / (fs_in L) cycles per sample:
    h[i] = 2 fc sinc(2 fc (i - (n - 1) / 2)) kaiser(n, beta), scaled so that sum h = L (every phase has a DC gain near 1)."""
    L, Mr = resample_ratio(fs_in, fs_c)
    n = L * int(taps_per_phase)
    fc = 0.5 * min(fs_in, fs_c) / (float(fs_in) * L)
    i = np.arange(n) - (n - 1) / 2
    h = 2 * fc * np.sinc(2 * fc * i) * np.kaiser(n, beta)
    return h * (L / h.sum()), L, Mr


@dataclass
class Capture:
    """What `Channeliser(capture=...)` is told about the capture: rate in Hz (an integer), format ("cs16", "cu8", "cs8", "cf32"), the shift
    of its centre in Hz (rounded to the nearest phase word of fs_in; positive moves the spectrum up), taps per phase of the resampler and
    its prototype (None: design_resampler(fs_in, fs_c, taps_per_phase))."""
    fs_in: int
    fmt: str = "cs16"
    shift_hz: float = 0.0
    taps_per_phase: int = 32
    rtaps: Optional[np.ndarray] = None


def _channel_array(channels: Sequence) -> "C.Array":
    rows = [c if isinstance(c, capi.ChanChannel) else capi.ChanChannel(int(c[0]) % (1 << 32), int(c[1]) % (1 << 32), float(c[2]))
            for c in channels]
    return (capi.ChanChannel * len(rows))(*rows)


def find_carriers(psd: np.ndarray, fs_in: float, bw_hz: float, threshold_db: float = 6.0) -> list:
    """Sorted centre frequencies in Hz (signed) of the carriers of width `bw_hz` in a spectrum of N bins in natural order (`read_psd`).

    Smooth by a circular boxcar mean of bw_hz (in bins, forced odd); the noise floor is the median of `psd`; repeatedly take the largest
    smoothed bin that lies at least `threshold_db` above the floor, refine it by the centroid of max(psd - floor, 0) over +-bw / 2 around
    it and once more around the rounded first estimate, blank +-bw around the pick.  The median is the noise floor only while carriers
    fill less than half of the band: in a fuller capture it lies on the carriers and nothing is found.  It may be handed the peak-hold
    spectrum (`read_peak_psd`) to find carriers that are seldom on: the median of a maximum over n blocks lies above the mean floor by
    the same factor in every bin, so the threshold keeps its meaning."""
    psd = np.asarray(psd, dtype=np.float64)
    n = psd.size
    w = int(round(bw_hz / fs_in * n)) | 1
    h = w // 2
    cs = np.concatenate([[0.0], np.cumsum(np.concatenate([psd[n - h:], psd, psd[:h]]))])
    smooth = (cs[w:] - cs[:-w]) / w
    floor = float(np.median(psd))
    excess = np.maximum(psd - floor, 0.0)
    off = np.arange(-h, h + 1)
    found = []
    while True:
        k = int(np.argmax(smooth))
        if not smooth[k] > 0.0 or not smooth[k] >= floor * 10.0 ** (threshold_db / 10.0):
            break
        centre = float(k)
        for _ in range(2):
            k0 = int(round(centre))
            e = excess[(k0 + off) % n]
            if e.sum() > 0.0:
                centre = k0 + float((e * off).sum() / e.sum())
        smooth[(k + np.arange(-w, w + 1)) % n] = -1.0
        c = centre % n
        found.append((c - n if c >= n / 2 else c) * fs_in / n)
    return sorted(found)


class Activity(NamedTuple):
    """What `Channeliser.read_activity` returns (the block statistics of include/jaero_hip.h's "activity")."""
    emax: np.ndarray   # [nch] largest block term e_{c,p}; nan where n == 0
    emin: np.ndarray   # [nch] smallest; nan where n == 0
    when: np.ndarray   # [nch] absolute index of the first block that reached emax; -1 where n == 0
    n: np.ndarray      # [nch] blocks counted
    hist: np.ndarray   # [nch, 64] uint32: blocks whose term has ilogb(e) + 32 == i (clamped to 0 .. 63)


def duty_cycle(hist: np.ndarray, rise_bins: int = 2) -> np.ndarray:
    """The share of a channel's blocks that stand out of its own floor, from the activity's histogram `hist` [nch, 64] (or one row).

    Per channel the floor bin is the most populated bin (the lowest on ties); the active blocks are those in bins >= floor + `rise_bins`
    (each bin is a factor of 2, 3.01 dB); the result is active / n, nan for an empty row.  What it cannot tell: a channel that is always
    on has its own signal as its floor and a duty of 0 here -- its level against the capture's noise floor (`read_levels` beside the
    other channels', or the spectrum) says that it is a carrier.  Nor does a channel that is on for more than half of its blocks read as
    its duty: the floor bin is then the signal's."""
    h = np.atleast_2d(np.asarray(hist)).astype(np.int64)
    n = h.sum(axis=1)
    floor = np.argmax(h, axis=1)  # the first of equal maxima: the lowest bin
    active = np.where(np.arange(h.shape[1])[None, :] >= (floor + int(rise_bins))[:, None], h, 0).sum(axis=1)
    out = np.where(n > 0, active / np.maximum(n, 1), np.nan)
    return out if np.ndim(hist) > 1 else out[0]


class Channeliser:
    """A bank of `len(channels)` channel filters over one capture (thin wrapper over jaero_chan).

    channels: (tune word, audio word, gain) per channel; the audio word is relative to fs_out.  taps: the prototype low-pass
    at the capture rate (None: design_taps(decim, fs_out=fs_out)).  max_write_iq: most I/Q pairs one write may bring.
    fs_out: the output rate, 48000, 24000 or 12000 -- a label (the capture rate is fs_out x decim) that `feed` checks
    against the bank's Fs; it enters no arithmetic."""

    def __init__(self, decim: int, channels: Sequence, taps: Optional[np.ndarray] = None, device: int = 0,
                 max_write_iq: int = 16 * HP, fs_out: float = FS_OUT, capture: Optional[Capture] = None):
        self.L = capi.lib()
        t = design_taps(decim, fs_out=fs_out) if taps is None else np.ascontiguousarray(taps, dtype=np.float64)
        arr = _channel_array(channels)
        h = C.c_void_p()
        rate = int(fs_out) if float(fs_out) == int(fs_out) else 0  # a rate that is no integer is none of the three
        self.capture = capture
        self.fmt = "cs16"
        self.shift_word = 0
        if capture is None:
            capi.check(self.L.jaero_chan2_create(device, int(decim), rate, len(arr), C.cast(arr, C.c_void_p), t.ctypes.data, int(t.size),
                                                 int(max_write_iq), C.byref(h)))
            self._fs_in = float(fs_out) * int(decim)
        else:
            if capture.fmt not in FORMATS:
                raise ValueError(f"capture format {capture.fmt!r} is none of {sorted(FORMATS)}")
            fs_in, fs_c = int(capture.fs_in), rate * int(decim)
            rt = capture.rtaps
            if rt is None and fs_in != fs_c and fs_in >= 1 and fs_c >= 1 and resample_ratio(fs_in, fs_c)[0] <= 1024:
                rt = design_resampler(fs_in, fs_c, capture.taps_per_phase)[0]
            rt = None if rt is None else np.ascontiguousarray(rt, dtype=np.float64)
            self.shift_word = tune_word(capture.shift_hz, float(fs_in)) if fs_in >= 1 else 0
            cs = capi.Capture(FORMATS[capture.fmt], fs_in, self.shift_word, int(capture.taps_per_phase), None if rt is None else rt.ctypes.data)
            capi.check(self.L.jaero_chan3_create(device, C.byref(cs), int(decim), rate, len(arr), C.cast(arr, C.c_void_p), t.ctypes.data,
                                                 int(t.size), int(max_write_iq), C.byref(h)))
            self.fmt = capture.fmt
            self._fs_in = float(fs_in)
            self.rtaps = rt
        self.h = h
        self.fs_out = float(fs_out)
        self.decim, self.nch, self.device, self.max_write_iq = int(decim), len(arr), device, int(max_write_iq)
        self.M = N // self.decim
        self.Mo = self.M // 2
        self.last_nout = 0
        self.last_stream = 0  # the stream of the last write / feed (RateMeter.write_from follows it)

    def close(self):
        if getattr(self, "h", None):
            self.L.jaero_chan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def fs_c(self) -> float:
        """The channeliser's own rate, fs_out x decim: what tune words are relative to."""
        return self.fs_out * self.decim

    @property
    def fs_in(self) -> float:
        """The capture's rate: fs_c unless a `Capture` said otherwise."""
        return self._fs_in

    def capture_tune_word(self, hz: float) -> int:
        """The tune word of a frequency `hz` of the CAPTURE (relative to its centre, at fs_in): the shift the device applies is added (the
        frequency its word really is), the sum is taken relative to fs_c."""
        return tune_word(hz + word_hz(self.shift_word, self._fs_in), self.fs_c)

    def _input(self, iq):
        """(pointer, I/Q pairs, is_device_ptr, keep-alive) of a numpy array [n, 2] / [2 n] of the handle's format (uint8, int8, int16,
        float32; complex64 [n] for cf32) or a torch tensor of that element size on the device."""
        want = _FORMAT_DTYPE[self.fmt]
        if isinstance(iq, np.ndarray):
            if iq.dtype == np.complex64:
                if self.fmt != "cf32":
                    raise TypeError(f"a complex64 array on a {self.fmt} channeliser")
                a = np.ascontiguousarray(iq).view(np.float32).reshape(-1)
            elif self.fmt == "cs16" and self.capture is None:
                a = np.ascontiguousarray(iq, dtype=np.int16).reshape(-1)
            else:
                if iq.dtype != want:
                    raise TypeError(f"a {iq.dtype} array on a {self.fmt} channeliser (takes {np.dtype(want)})")
                a = np.ascontiguousarray(iq).reshape(-1)
            assert a.size % 2 == 0
            return a.ctypes.data, a.size // 2, 0, a
        t = iq
        size = np.dtype(want).itemsize
        if t.is_complex():
            assert self.fmt == "cf32" and t.element_size() == 8 and t.is_cuda and t.is_contiguous()
            return t.data_ptr(), t.numel(), 1, t
        assert t.is_cuda and t.is_contiguous() and t.element_size() == size and t.numel() % 2 == 0
        return t.data_ptr(), t.numel() // 2, 1, t

    def write(self, iq, stream: int = 0) -> int:
        """Consumes the I/Q pairs; returns the samples per channel this write produced (a multiple of Mo, possibly 0)."""
        ptr, n, dev, _keep = self._input(iq)
        nout = C.c_int(0)
        fn = self.L.jaero_chan_write if self.capture is None else self.L.jaero_chan3_write
        capi.check(fn(self.h, ptr, n, dev, C.c_void_p(stream), C.byref(nout)))
        self.last_nout, self.last_stream = nout.value, stream
        return nout.value

    def feed(self, bank, iq, stream: int = 0) -> int:
        """write, then the bank's write of what came out (device to device, no synchronisation).  Returns samples per channel."""
        ptr, n, dev, _keep = self._input(iq)
        nout = C.c_int(0)
        fn = self.L.jaero_chan_feed if self.capture is None else self.L.jaero_chan3_feed
        capi.check(fn(self.h, bank.h, ptr, n, dev, C.c_void_p(stream), C.byref(nout)))
        self.last_nout, self.last_stream = nout.value, stream
        return nout.value

    def read_staged(self) -> Tuple[np.ndarray, int]:
        """(z, first): what the last write staged for the forward transform, complex128, and the absolute staged index of z[0]
        (synchronises; only on a channeliser with a `Capture`)."""
        L, Mr = resample_ratio(int(self._fs_in), int(self.fs_c))
        buf = np.empty((-(-self.max_write_iq * L // Mr) + 1, 2), dtype=np.float64)
        n, first = C.c_int(0), C.c_longlong(0)
        capi.check(self.L.jaero_chan3_read_staged(self.h, buf.ctypes.data, buf.shape[0], C.byref(n), C.byref(first)))
        z = np.empty(n.value, dtype=np.complex128)  # component by component: a sum with 1j would turn -0.0 into 0.0
        z.real, z.imag = buf[: n.value, 0], buf[: n.value, 1]
        return z, first.value

    def capture_profile_read(self, which: int, reset: bool = False):
        """(total ms, launches) of capture kernel `which`: 0 = staging (k_capture_stage), 1 = forward transform (k_capture_fwd)."""
        ms, n = C.c_double(0), C.c_int(0)
        capi.check(self.L.jaero_chan3_profile_read(self.h, which, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def read_pcm(self) -> np.ndarray:
        """The last write's output, int16 [nch, nout], on the host (synchronises)."""
        out = np.empty((self.nch, max(self.last_nout, 1)), dtype=np.int16)
        n = C.c_int(0)
        capi.check(self.L.jaero_chan_read_pcm(self.h, out.ctypes.data, out.shape[1], C.byref(n)))
        return out[:, : n.value].copy()

    def pcm_view(self) -> Tuple[int, int]:
        """(device pointer, samples per channel) of the last write's output, int16 [nch][nsamples]."""
        p, n = C.c_void_p(), C.c_int(0)
        capi.check(self.L.jaero_chan_pcm_view(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def retune(self, channel: int, tune: int, audio: int, gain: float):
        ch = capi.ChanChannel(int(tune) % (1 << 32), int(audio) % (1 << 32), float(gain))
        capi.check(self.L.jaero_chan_retune(self.h, channel, C.byref(ch)))

    def retune_all(self, channels: Sequence):
        """retune of every channel (tune word, audio word, gain) behind one synchronisation; nothing changes unless every gain is valid."""
        arr = _channel_array(channels)
        if len(arr) != self.nch:
            raise ValueError(f"retune_all takes {self.nch} channels, not {len(arr)}")
        capi.check(self.L.jaero_chan2_retune_all(self.h, C.cast(arr, C.c_void_p)))

    def survey_enable(self, psd: bool = True, levels: bool = True):
        """Switches the survey's two parts on or off; clears the sums and counts of what is on."""
        capi.check(self.L.jaero_survey_enable(self.h, int(bool(psd)) | int(bool(levels)) << 1))

    def survey_reset(self):
        capi.check(self.L.jaero_survey_reset(self.h))

    def read_psd_sums(self) -> Tuple[np.ndarray, int]:
        """(S[N] raw, nblocks) as the ABI returns them."""
        s, n = np.empty(N, dtype=np.float64), C.c_longlong(0)
        capi.check(self.L.jaero_survey_read_psd(self.h, s.ctypes.data, C.byref(n)))
        return s, n.value

    def read_psd(self) -> Tuple[np.ndarray, int]:
        """(psd[N], nblocks): S / (nblocks N^2 3 / 8), LSB^2 per bin in natural bin order (nan before the first block)."""
        s, n = self.read_psd_sums()
        return (s / (n * float(N) * N * 0.375) if n else np.full(N, np.nan)), n

    def read_level_sums(self) -> Tuple[np.ndarray, np.ndarray]:
        """(E[nch] raw, counts[nch]) as the ABI returns them."""
        e, n = np.empty(self.nch, dtype=np.float64), np.empty(self.nch, dtype=np.int64)
        capi.check(self.L.jaero_survey_read_levels(self.h, e.ctypes.data, n.ctypes.data))
        return e, n

    def read_levels(self) -> Tuple[np.ndarray, np.ndarray]:
        """(level[nch] = E / n, nan where n == 0; counts[nch]): the mean square of each channel's complex output before rotation and gain."""
        e, n = self.read_level_sums()
        return np.where(n > 0, e / np.maximum(n, 1), np.nan), n

    def suggest_gains(self, target_rms: float = 0.1 * 32768, peak: bool = False) -> np.ndarray:
        """The gain that brings each channel's int16 output to `target_rms`: target / sqrt(level / 2).  Raises ValueError for a
        channel that has no block yet or whose level is 0: it has no such gain (and retune_all would refuse the whole set for it).
        peak=True: target / sqrt(emax / 2) from the activity's block statistics, the gain that puts the STRONGEST BLOCK at the target
        (a burst channel's mean level is low by its duty cycle)."""
        if peak:
            act = self.read_activity()
            level, counts = act.emax, act.n
        else:
            level, counts = self.read_levels()
        empty = np.nonzero((counts == 0) | ~(level > 0.0))[0]
        if empty.size:
            raise ValueError(f"suggest_gains: channels {empty[:8].tolist()} have no surveyed block or a level of 0")
        return target_rms / np.sqrt(level / 2.0)

    def activity_enable(self, peak: bool = True, blocks: bool = True):
        """Switches the activity's two parts (peak-hold spectrum, per-channel block statistics) on or off; clears what is on."""
        capi.check(self.L.jaero_activity_enable(self.h, (capi.ACT_PEAK if peak else 0) | (capi.ACT_BLOCKS if blocks else 0)))

    def activity_reset(self):
        capi.check(self.L.jaero_activity_reset(self.h))

    def read_peak_sums(self) -> Tuple[np.ndarray, int]:
        """(P[N] raw, nblocks) as the ABI returns them."""
        p, n = np.empty(N, dtype=np.float64), C.c_longlong(0)
        capi.check(self.L.jaero_activity_read_peak(self.h, p.ctypes.data, C.byref(n)))
        return p, n.value

    def read_peak_psd(self) -> Tuple[np.ndarray, int]:
        """(peak[N], nblocks): P / (N^2 3 / 8), each bin's largest block in LSB^2 per bin, natural bin order (nan before the first block)."""
        p, n = self.read_peak_sums()
        return (p / (float(N) * N * 0.375) if n else np.full(N, np.nan)), n

    def read_activity(self) -> "Activity":
        """Activity(emax, emin, when, n, hist): every channel's largest and smallest block term (nan where n == 0), the absolute index of
        the block of the largest (-1 where n == 0), the blocks counted, and hist[nch, 64], the blocks per binary order of magnitude."""
        emax, emin = np.empty(self.nch, dtype=np.float64), np.empty(self.nch, dtype=np.float64)
        when, n = np.empty(self.nch, dtype=np.int64), np.empty(self.nch, dtype=np.int64)
        hist = np.empty((self.nch, capi.ACT_BINS), dtype=np.uint32)
        capi.check(self.L.jaero_activity_read_blocks(self.h, emax.ctypes.data, emin.ctypes.data, when.ctypes.data, n.ctypes.data, hist.ctypes.data))
        return Activity(np.where(n > 0, emax, np.nan), np.where(n > 0, emin, np.nan), when, n, hist)

    def activity_profile_read(self, which: int, reset: bool = False):
        """(total ms, launches) of the launches that serve the activity: which 0 = k_chan_psd keeping the peak, 1 = k_chan_level taking the
        block statistics.  A launch fused with the survey's part counts here and not in survey_profile_read."""
        ms, n = C.c_double(0), C.c_int(0)
        capi.check(self.L.jaero_activity_profile_read(self.h, which, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def survey_profile_read(self, which: int, reset: bool = False):
        """(total ms, launches) of survey kernel `which`: 0 = spectrum (k_chan_psd), 1 = levels (k_chan_level)."""
        ms, n = C.c_double(0), C.c_int(0)
        capi.check(self.L.jaero_survey_profile_read(self.h, which, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def profile_enable(self, on: bool = True):
        capi.check(self.L.jaero_chan_profile_enable(self.h, int(on)))

    def profile_read(self, which: int, reset: bool = False):
        """(total ms, launches) of kernel `which`: 0 = forward transform, 1 = per-channel synthesis."""
        ms, n = C.c_double(0), C.c_int(0)
        capi.check(self.L.jaero_chan_profile_read(self.h, which, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value


# ---------------------------------------------------------------------------------------------- splitter
RATE_FS_OUT = {10500: 48000.0, 8400: 48000.0, 1200: 24000.0, 600: 12000.0}  # the bank rate of each bit rate `decide_rates` names


class Plan(NamedTuple):
    """What `plan_outputs` returns."""
    outputs: list    # (fs_out, channels, None) per output: what `Splitter` takes
    indices: list    # per output, the indices into carriers_hz of the carriers it took, ascending
    rates: list      # per output, the bit rate of its carriers: what its bank is created for
    left_out: list   # indices of the carriers whose rate is none of RATE_FS_OUT's (0, "no rate", included)


def plan_outputs(carriers_hz: Sequence[float], rates_bps: Sequence[float], fs_c: float, audio_hz: Optional[float] = None,
                 gain: float = 1.0) -> Plan:
    """Groups surveyed carriers (`find_carriers`) by the bit rate the rate meter named (`decide_rates`): one output per rate that has a
    carrier, in the order 10500, 8400 (both at 48 kHz), 1200 (24 kHz), 600 (12 kHz); a rate without a carrier makes no output, a carrier with
    any other rate is left out and reported.  Each channel is (tune word of the carrier at fs_c, audio word of `audio_hz` at the output's
    rate -- None: fs_out / 6 --, gain).  A pure function: what a caller does between the rate meter and the banks."""
    if len(carriers_hz) != len(rates_bps):
        raise ValueError(f"plan_outputs takes one rate per carrier: {len(carriers_hz)} carriers, {len(rates_bps)} rates")
    outputs, indices, rates = [], [], []
    for rate, fs_out in RATE_FS_OUT.items():
        idx = [i for i, r in enumerate(rates_bps) if float(r) == rate]
        if not idx:
            continue
        audio = tune_word(fs_out / 6.0 if audio_hz is None else audio_hz, fs_out)
        outputs.append((fs_out, [(tune_word(float(carriers_hz[i]), float(fs_c)), audio, float(gain)) for i in idx], None))
        indices.append(idx)
        rates.append(rate)
    left = [i for i, r in enumerate(rates_bps) if float(r) not in RATE_FS_OUT]
    return Plan(outputs, indices, rates, left)


class _Output(Channeliser):
    """Output g of a `Splitter`: a `Channeliser` around the borrowed handle (jaero_split_output).  Every reader and retune method works as
    on a stand-alone channeliser; `nch`, `decim`, `Mo`, `fs_out`, `last_nout` and `last_stream` are kept current by the splitter.  The
    input goes to the splitter: `write`, `feed` and `close` raise."""

    def __init__(self, split: "Splitter", h, decim: int, nch: int, fs_out: float):
        self.L, self.h, self.split = split.L, h, split
        self.capture, self.fmt, self.shift_word = split.capture, split.fmt, split.shift_word
        self._fs_in = split._fs_in
        self.fs_out = float(fs_out)
        self.decim, self.nch, self.device, self.max_write_iq = int(decim), int(nch), split.device, split.max_write_iq
        self.M = N // self.decim
        self.Mo = self.M // 2
        self.last_nout = 0
        self.last_stream = 0

    def write(self, iq, stream: int = 0):
        raise RuntimeError("an output of a Splitter takes no input of its own: use Splitter.write")

    def feed(self, bank, iq, stream: int = 0):
        raise RuntimeError("an output of a Splitter takes no input of its own: use Splitter.feed")

    def read_staged(self):
        raise RuntimeError("a Splitter has no read_staged")

    def close(self):
        raise RuntimeError("an output of a Splitter is closed with it: use Splitter.close")

    def __del__(self):
        pass


class Splitter:
    """One capture into several banks at their own rates (thin wrapper over jaero_split): one front end, one spectrum per hop, and
    `len(outputs)` outputs that are each, bit for bit, what a stand-alone `Channeliser(fs_c / fs_out, channels, taps, fs_out=fs_out,
    capture=capture)` fed the same writes produces.

    fs_c: the rate the front end runs at (an integer; fs_c / fs_out must be one of DECIMS for every output).  outputs: a list of
    (fs_out, channels, taps-or-None); taps None: design_taps(fs_c / fs_out, fs_out=fs_out).  capture: a `Capture` whose rate and format the
    writes are in (None: int16 I/Q at fs_c); max_write_iq then counts capture samples.  `outputs[g]` is the `Channeliser` object of
    output g."""

    def __init__(self, fs_c: int, outputs: Sequence, capture: Optional[Capture] = None, device: int = 0, max_write_iq: int = 16 * HP):
        self.L = capi.lib()
        fs_c = int(fs_c) if float(fs_c) == int(fs_c) else 0  # a rate that is no integer is none
        keep, rows = [], []
        for fs_out, channels, taps in outputs:
            rate = int(fs_out) if float(fs_out) == int(fs_out) else 0
            if taps is None:
                if rate < 1 or fs_c % rate or fs_c // rate not in DECIMS:
                    raise ValueError(f"Splitter: fs_c {fs_c} / fs_out {fs_out} is none of {DECIMS}; no default taps")
                taps = design_taps(fs_c // rate, fs_out=float(fs_out))
            t = np.ascontiguousarray(taps, dtype=np.float64)
            arr = _channel_array(channels)
            keep.append((t, arr))
            rows.append(capi.ChanOutput(rate, len(arr), C.cast(arr, C.c_void_p), t.ctypes.data, int(t.size)))
        outs = (capi.ChanOutput * max(len(rows), 1))(*rows)
        self.capture, self.fmt, self.shift_word, self.rtaps = capture, "cs16", 0, None
        self._fs_in = float(fs_c)
        cs = None
        if capture is not None:
            if capture.fmt not in FORMATS:
                raise ValueError(f"capture format {capture.fmt!r} is none of {sorted(FORMATS)}")
            fs_in = int(capture.fs_in)
            rt = capture.rtaps
            if rt is None and fs_in != fs_c and fs_in >= 1 and fs_c >= 1 and resample_ratio(fs_in, fs_c)[0] <= 1024:
                rt = design_resampler(fs_in, fs_c, capture.taps_per_phase)[0]
            rt = None if rt is None else np.ascontiguousarray(rt, dtype=np.float64)
            self.shift_word = tune_word(capture.shift_hz, float(fs_in)) if fs_in >= 1 else 0
            cs = capi.Capture(FORMATS[capture.fmt], fs_in, self.shift_word, int(capture.taps_per_phase), None if rt is None else rt.ctypes.data)
            self.fmt, self._fs_in, self.rtaps = capture.fmt, float(fs_in), rt
        h = C.c_void_p()
        capi.check(self.L.jaero_split_create(device, None if cs is None else C.byref(cs), fs_c, len(rows), outs, int(max_write_iq), C.byref(h)))
        self.h = h
        self.fs_c, self.device, self.max_write_iq = fs_c, device, int(max_write_iq)
        nblk = C.c_int(0)
        capi.check(self.L.jaero_split_info(self.h, None, None, C.byref(nblk)))
        self.nblk_max = nblk.value
        self.outputs = []
        for g, row in enumerate(rows):
            v = C.c_void_p()
            capi.check(self.L.jaero_split_output(self.h, g, C.byref(v)))
            self.outputs.append(_Output(self, v, fs_c // row.out_rate, row.nchannels, float(row.out_rate)))
        self._nout = (C.c_int * len(rows))()

    _input = Channeliser._input

    def close(self):
        if getattr(self, "h", None):
            self.L.jaero_split_destroy(self.h)
            self.h = None
            for o in getattr(self, "outputs", []):
                o.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _done(self, stream: int) -> list:
        nout = list(self._nout)
        for o, n in zip(self.outputs, nout):
            o.last_nout, o.last_stream = n, stream
        return nout

    def write(self, iq, stream: int = 0) -> list:
        """Consumes the I/Q pairs; returns, per output, the samples per channel this write produced (blocks x Mo of the output)."""
        ptr, n, dev, _keep = self._input(iq)
        capi.check(self.L.jaero_split_write(self.h, ptr, n, dev, C.c_void_p(stream), self._nout))
        return self._done(stream)

    def feed(self, banks: Sequence, iq, stream: int = 0) -> list:
        """write, then each bank's write of its output (device to device, no synchronisation), in output order.  banks: one
        `DemodulatorBank` per output; None: that output is produced and not fed."""
        if len(banks) != len(self.outputs):
            raise ValueError(f"feed takes {len(self.outputs)} banks (None where an output is not fed), not {len(banks)}")
        ptr, n, dev, _keep = self._input(iq)
        arr = (C.c_void_p * len(banks))(*[None if b is None else b.h for b in banks])
        capi.check(self.L.jaero_split_feed(self.h, arr, ptr, n, dev, C.c_void_p(stream), self._nout))
        return self._done(stream)

    def profile_enable(self, on: bool = True):
        """Switches the timers of the front end and of every output."""
        capi.check(self.L.jaero_split_profile_enable(self.h, int(on)))

    def profile_read(self, which: int, reset: bool = False):
        """(total ms, launches) of the front end's kernel `which`: 0 = forward transform (of either kind), 1 = staging kernel.  The
        outputs' kernels are read on `outputs[g]`."""
        ms, n = C.c_double(0), C.c_int(0)
        capi.check(self.L.jaero_split_profile_read(self.h, which, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value
