"""Wideband I/Q channeliser in front of the demodulator banks (jaero_chan_*, include/jaero_hip.h).

`Channeliser` cuts one int16 I/Q capture at fs_out x decim into the int16 audio at fs_out (48, 24 or 12 kHz) of every channel
of a bank, on the GPU: `feed(bank, iq)` hands its output straight to `DemodulatorBank` (device to device), `write` / `read_pcm` give it to the
caller.  Frequencies are 32-bit words: `tune_word(hz, fs)` is the word nearest a frequency, `word_hz(word, fs)` the
frequency a word really is, `channel_words(tune, audio, decim)` the integers the kernels derive from a channel's words.
The survey (`survey_enable`, `read_psd`, `read_levels`) measures the capture's spectrum and every channel's level on the device;
`find_carriers` (host numpy, no hot path) turns the spectrum into centre frequencies, `suggest_gains` the levels into gains, and
`retune_all` applies both.  All device arithmetic happens in libjaero_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

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


def _channel_array(channels: Sequence) -> "C.Array":
    rows = [c if isinstance(c, capi.ChanChannel) else capi.ChanChannel(int(c[0]) % (1 << 32), int(c[1]) % (1 << 32), float(c[2]))
            for c in channels]
    return (capi.ChanChannel * len(rows))(*rows)


def find_carriers(psd: np.ndarray, fs_in: float, bw_hz: float, threshold_db: float = 6.0) -> list:
    """Sorted centre frequencies in Hz (signed) of the carriers of width `bw_hz` in a spectrum of N bins in natural order (`read_psd`).

    Smooth by a circular boxcar mean of bw_hz (in bins, forced odd); the noise floor is the median of `psd`; repeatedly take the largest
    smoothed bin that lies at least `threshold_db` above the floor, refine it by the centroid of max(psd - floor, 0) over +-bw / 2 around
    it and once more around the rounded first estimate, blank +-bw around the pick.  The median is the noise floor only while carriers
    fill less than half of the band: in a fuller capture it lies on the carriers and nothing is found."""
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


class Channeliser:
    """A bank of `len(channels)` channel filters over one capture (thin wrapper over jaero_chan).

    channels: (tune word, audio word, gain) per channel; the audio word is relative to fs_out.  taps: the prototype low-pass
    at the capture rate (None: design_taps(decim, fs_out=fs_out)).  max_write_iq: most I/Q pairs one write may bring.
    fs_out: the output rate, 48000, 24000 or 12000 -- a label (the capture rate is fs_out x decim) that `feed` checks
    against the bank's Fs; it enters no arithmetic."""

    def __init__(self, decim: int, channels: Sequence, taps: Optional[np.ndarray] = None, device: int = 0,
                 max_write_iq: int = 16 * HP, fs_out: float = FS_OUT):
        self.L = capi.lib()
        t = design_taps(decim, fs_out=fs_out) if taps is None else np.ascontiguousarray(taps, dtype=np.float64)
        arr = _channel_array(channels)
        h = C.c_void_p()
        rate = int(fs_out) if float(fs_out) == int(fs_out) else 0  # a rate that is no integer is none of the three
        capi.check(self.L.jaero_chan2_create(device, int(decim), rate, len(arr), C.cast(arr, C.c_void_p), t.ctypes.data, int(t.size),
                                             int(max_write_iq), C.byref(h)))
        self.h = h
        self.fs_out = float(fs_out)
        self.decim, self.nch, self.device, self.max_write_iq = int(decim), len(arr), device, int(max_write_iq)
        self.M = N // self.decim
        self.Mo = self.M // 2
        self.last_nout = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.jaero_chan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _input(iq):
        """(pointer, I/Q pairs, is_device_ptr, keep-alive) of a numpy int16 array [n, 2] / [2 n] or a torch int16 tensor on the device."""
        if isinstance(iq, np.ndarray):
            a = np.ascontiguousarray(iq, dtype=np.int16).reshape(-1)
            assert a.size % 2 == 0
            return a.ctypes.data, a.size // 2, 0, a
        t = iq
        assert t.is_cuda and t.is_contiguous() and t.element_size() == 2 and t.numel() % 2 == 0
        return t.data_ptr(), t.numel() // 2, 1, t

    def write(self, iq, stream: int = 0) -> int:
        """Consumes the I/Q pairs; returns the samples per channel this write produced (a multiple of Mo, possibly 0)."""
        ptr, n, dev, _keep = self._input(iq)
        nout = C.c_int(0)
        capi.check(self.L.jaero_chan_write(self.h, ptr, n, dev, C.c_void_p(stream), C.byref(nout)))
        self.last_nout = nout.value
        return nout.value

    def feed(self, bank, iq, stream: int = 0) -> int:
        """write, then the bank's write of what came out (device to device, no synchronisation).  Returns samples per channel."""
        ptr, n, dev, _keep = self._input(iq)
        nout = C.c_int(0)
        capi.check(self.L.jaero_chan_feed(self.h, bank.h, ptr, n, dev, C.c_void_p(stream), C.byref(nout)))
        self.last_nout = nout.value
        return nout.value

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

    def suggest_gains(self, target_rms: float = 0.1 * 32768) -> np.ndarray:
        """The gain that brings each channel's int16 output to `target_rms`: target / sqrt(level / 2).  Raises ValueError for a
        channel that has no block yet or whose level is 0: it has no such gain (and retune_all would refuse the whole set for it)."""
        level, counts = self.read_levels()
        empty = np.nonzero((counts == 0) | ~(level > 0.0))[0]
        if empty.size:
            raise ValueError(f"suggest_gains: channels {empty[:8].tolist()} have no surveyed block or a level of 0")
        return target_rms / np.sqrt(level / 2.0)

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
