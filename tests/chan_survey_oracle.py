"""The channeliser survey's definition (include/jaero_hip.h, "survey of a channeliser's capture") in numpy, literally, streaming, on top of
`chan_oracle.ChanOracle`: the Welch spectrum S with the Hann window applied in the frequency domain, the per-channel levels E_c
with their block counts n_c, reset, and the restart of a channel whose tune word a retune changes.  The GPU kernels (k_chan_psd,
k_chan_level) are tested against this (tests/test_gpu_chan_survey.py); this against itself and the time-domain Hann on the CPU
(tests/test_chan_survey_host.py)."""
import numpy as np

import chan_oracle as CO

N, HP = CO.N, CO.HP


def hann_spectrum_time(s):
    """|DFT(s w)|^2, w[n] = 1/2 - 1/2 cos(2 pi n / N): what the frequency-domain form of `ChanSurveyOracle` equals."""
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)
    H = np.fft.fft(np.asarray(s) * w)
    return H.real ** 2 + H.imag ** 2


def normalise_psd(S, nblocks):
    """psd[k] = S[k] / (nblocks N^2 3 / 8): LSB^2 per bin, summing to the mean |x|^2 of a stationary input."""
    return S / (nblocks * float(N) * N * 0.375)


class ChanSurveyOracle(CO.ChanOracle):
    """write() is ChanOracle's (the unrounded output) and surveys the blocks it completes; survey() only surveys (for tests that
    need no output).  Use one of the two on an instance: each advances its own copy of the input history."""

    def __init__(self, decim, channels, taps, psd=True, levels=True):
        super().__init__(decim, channels, taps)
        self.want_psd, self.want_levels = psd, levels
        self.sbuf = np.zeros(HP, dtype=np.complex128)
        self.reset()

    def reset(self):
        self.S = np.zeros(N)
        self.nblocks = 0
        self.E = np.zeros(len(self.channels))
        self.n = np.zeros(len(self.channels), dtype=np.int64)

    def retune(self, channel, tune, audio, gain):
        if int(tune) % (1 << 32) != int(self.channels[channel][0]) % (1 << 32):
            self.E[channel] = 0.0
            self.n[channel] = 0
        self.channels[channel] = (tune, audio, gain)

    def retune_all(self, channels):
        assert len(channels) == len(self.channels)
        for c, ch in enumerate(channels):
            self.retune(c, *ch)

    def survey(self, x):
        self.sbuf = np.concatenate([self.sbuf, np.asarray(x, dtype=np.complex128)])
        nblk = (len(self.sbuf) - HP) // HP
        M = self.M
        q = np.arange(-M // 2, M // 2)
        for j in range(nblk):
            X = np.fft.fft(self.sbuf[j * HP: j * HP + N])
            if self.want_psd:
                H = 0.5 * X - 0.25 * (np.roll(X, 1) + np.roll(X, -1))  # X[(k - 1) mod N] + X[(k + 1) mod N]
                self.S += H.real ** 2 + H.imag ** 2
                self.nblocks += 1
            if self.want_levels:
                for c, (tune, audio, _gain) in enumerate(self.channels):
                    b = CO.words(tune, audio, self.D)[0]
                    Y = X[(b + q) % N] * self.G[q % N] / N
                    self.E[c] += np.sum(Y.real ** 2 + Y.imag ** 2)
                    self.n[c] += 1
        self.sbuf = self.sbuf[nblk * HP:]
        return nblk

    def write(self, x):
        self.survey(x)
        return super().write(x)

    def psd(self):
        return normalise_psd(self.S, self.nblocks)

    def levels(self):
        """E / n, nan where n == 0"""
        return np.where(self.n > 0, self.E / np.maximum(self.n, 1), np.nan)

    def predicted_rms(self, gain=1.0):
        """RMS of the real output at `gain`: g sqrt(E_c / (2 n_c))"""
        return gain * np.sqrt(self.levels() / 2.0)
