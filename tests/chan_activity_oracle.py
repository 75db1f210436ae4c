"""The activity's definition (include/jaero_hip.h, "activity: the second, independent part of the survey") in numpy, literally,
streaming, on top of `chan_survey_oracle.ChanSurveyOracle`: the peak-hold spectrum P with its block count, per channel the largest and
smallest block term emax / emin, the absolute block index `when` of the largest, the count n and the 64-bin histogram of the terms' binary
exponents, activity_reset, and the restart of a channel whose tune word a retune changes.  The survey's own sums (S, E) are formed beside
them from the same terms, as on the device.  The GPU kernels (k_chan_psd<SUM, PEAK>, k_chan_level<D, LEVEL, ACT>) are tested against this
(tests/test_gpu_chan_activity.py); this against itself on the CPU (tests/test_chan_activity_host.py)."""
import math

import numpy as np

import chan_oracle as CO
import chan_survey_oracle as SO

N, HP = SO.N, SO.HP
BINS = 64


def act_bin(e):
    """bin(e) = min(63, max(0, ilogb(e) + 32)), bin(0) = 0"""
    e = float(e)
    if e == 0.0:
        return 0
    return min(BINS - 1, max(0, math.frexp(e)[1] - 1 + 32))  # ilogb(e) = frexp's exponent - 1


class ChanActivityOracle(SO.ChanSurveyOracle):
    """survey() measures the blocks it completes for the survey (psd, levels) and the activity (peak, blocks); write() is ChanOracle's
    behind survey().  Block indices count from the oracle's creation, as the handle's blocks_done."""

    def __init__(self, decim, channels, taps, psd=True, levels=True, peak=True, blocks=True):
        self.want_peak, self.want_blocks = peak, blocks
        self.pblk = 0
        super().__init__(decim, channels, taps, psd=psd, levels=levels)  # calls reset()
        self.activity_reset()

    def activity_reset(self):
        nch = len(self.channels)
        self.P = np.zeros(N)
        self.peak_blocks = 0
        self.emax = np.zeros(nch)
        self.emin = np.full(nch, np.inf)
        self.when = np.full(nch, -1, dtype=np.int64)
        self.an = np.zeros(nch, dtype=np.int64)
        self.hist = np.zeros((nch, BINS), dtype=np.uint32)

    def retune(self, channel, tune, audio, gain):
        if int(tune) % (1 << 32) != int(self.channels[channel][0]) % (1 << 32):
            self.emax[channel], self.emin[channel], self.when[channel], self.an[channel] = 0.0, np.inf, -1, 0
            self.hist[channel] = 0
        super().retune(channel, tune, audio, gain)

    def survey(self, x):
        self.sbuf = np.concatenate([self.sbuf, np.asarray(x, dtype=np.complex128)])
        nblk = (len(self.sbuf) - HP) // HP
        M = self.M
        q = np.arange(-M // 2, M // 2)
        for j in range(nblk):
            p = self.pblk + j
            X = np.fft.fft(self.sbuf[j * HP: j * HP + N])
            if self.want_psd or self.want_peak:
                H = 0.5 * X - 0.25 * (np.roll(X, 1) + np.roll(X, -1))  # X[(k - 1) mod N] + X[(k + 1) mod N]
                term = H.real ** 2 + H.imag ** 2
                if self.want_psd:
                    self.S += term
                    self.nblocks += 1
                if self.want_peak:
                    self.P = np.maximum(self.P, term)
                    self.peak_blocks += 1
            if self.want_levels or self.want_blocks:
                for c, (tune, audio, _gain) in enumerate(self.channels):
                    b = CO.words(tune, audio, self.D)[0]
                    Y = X[(b + q) % N] * self.G[q % N] / N
                    e = np.sum(Y.real ** 2 + Y.imag ** 2)
                    if self.want_levels:
                        self.E[c] += e
                        self.n[c] += 1
                    if self.want_blocks:
                        if self.an[c] == 0 or e > self.emax[c]:  # strictly above: the smallest block index of the maximum stays
                            self.emax[c], self.when[c] = e, p
                        if e < self.emin[c]:
                            self.emin[c] = e
                        self.hist[c, act_bin(e)] += 1
                        self.an[c] += 1
        self.sbuf = self.sbuf[nblk * HP:]
        self.pblk += nblk
        return nblk

    def peak_psd(self):
        """P / (N^2 3 / 8): LSB^2 per bin"""
        return self.P / (float(N) * N * 0.375)

    def block_terms(self, x):
        """e_{c,p} [nch, nblk] of all whole blocks of x from a fresh history, with the channels as they are now (for the tests' checks
        of how far the terms lie from a bin edge and from each other; changes nothing)."""
        buf = np.concatenate([np.zeros(HP, dtype=np.complex128), np.asarray(x, dtype=np.complex128)])
        nblk = (len(buf) - HP) // HP
        q = np.arange(-self.M // 2, self.M // 2)
        out = np.zeros((len(self.channels), nblk))
        for j in range(nblk):
            X = np.fft.fft(buf[j * HP: j * HP + N])
            for c, (tune, audio, _gain) in enumerate(self.channels):
                b = CO.words(tune, audio, self.D)[0]
                Y = X[(b + q) % N] * self.G[q % N] / N
                out[c, j] = np.sum(Y.real ** 2 + Y.imag ** 2)
        return out
