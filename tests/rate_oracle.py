"""The rate lines' definition (include/jaero_hip.h, "rate lines") in numpy, literally.  The GPU kernel (k_rate_lines) is tested against
`RateOracle`; the oracle against a long-double DFT and against the time-domain form of its window on the CPU (tests/test_rate_host.py)."""
import numpy as np

L = 4096
BINS = L // 2 + 1


def segment_terms(y):
    """|H[k]|^2, k <= L / 2, of the segments y [nch, L] (integers)."""
    y2 = np.asarray(y).astype(np.int64) ** 2
    q = y2.astype(np.float64) - (y2.sum(axis=1, keepdims=True).astype(np.float64) / L)  # exact: integers below 2^43, a multiple of 2^-12
    Z = np.fft.fft(q, axis=1)
    H = Z / 2 - (np.roll(Z, 1, axis=1) + np.roll(Z, -1, axis=1)) / 4
    return (H.real ** 2 + H.imag ** 2)[:, :BINS]


class RateOracle:
    """Streaming form: write() takes int16 [nch, n] for any n and returns the segments it completed; `R` [nch, 2049] and `n` are the sums
    and the segment count since create or the last reset()."""

    def __init__(self, nch):
        self.nch = nch
        self.buf = np.zeros((nch, 0), dtype=np.int64)
        self.R = np.zeros((nch, BINS))
        self.n = 0

    def write(self, pcm):
        pcm = np.asarray(pcm)
        assert pcm.ndim == 2 and pcm.shape[0] == self.nch
        self.buf = np.concatenate([self.buf, pcm.astype(np.int64)], axis=1)
        nseg = self.buf.shape[1] // L
        for j in range(nseg):
            self.R = self.R + segment_terms(self.buf[:, j * L:(j + 1) * L])
        self.buf = self.buf[:, nseg * L:]
        self.n += nseg
        return nseg

    def reset(self):
        """clears the sums and the count; the pending partial segment stays"""
        self.R = np.zeros((self.nch, BINS))
        self.n = 0
