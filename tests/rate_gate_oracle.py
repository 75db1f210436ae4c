"""The gated rate lines' definition (include/jaero_hip.h, "gated rate lines") in numpy, literally, on rate_oracle.segment_terms.  The GPU
kernel (k_rate_lines_gated) is tested against `GatedRateOracle`; the oracle against `RateOracle` on the CPU (tests/test_rate_gate_host.py)."""
import numpy as np

import rate_oracle as RO

L, BINS = RO.L, RO.BINS
U64_MAX = (1 << 64) - 1


def segment_energy(y):
    """E = sum y^2 of the segments y [nch, L] (integers), as Python ints"""
    return [int(e) for e in (np.asarray(y).astype(np.int64) ** 2).sum(axis=1)]


class GatedRateOracle:
    """Streaming form, as RateOracle: write() takes int16 [nch, n] for any n and returns the segments it completed.  `R` [nch, 2049] sums
    the terms of the segments that joined (E_j >= gate, with the gate in force at the write that completes the segment), `n` counts every
    completed segment; `emax`, `emin`, `njoin`, `ejoin` are lists of Python ints per channel since create or the last reset(); `joined[c]`
    lists the segments of channel c that joined since then, counted from the last reset."""

    def __init__(self, nch):
        self.nch = nch
        self.buf = np.zeros((nch, 0), dtype=np.int64)
        self.gate = [0] * nch
        self.reset()

    def set_gate(self, g):
        assert len(g) == self.nch and all(0 <= int(v) <= U64_MAX for v in g)
        self.gate = [int(v) for v in g]

    def write(self, pcm):
        pcm = np.asarray(pcm)
        assert pcm.ndim == 2 and pcm.shape[0] == self.nch
        self.buf = np.concatenate([self.buf, pcm.astype(np.int64)], axis=1)
        nseg = self.buf.shape[1] // L
        for j in range(nseg):
            seg = self.buf[:, j * L:(j + 1) * L]
            E = segment_energy(seg)
            terms = RO.segment_terms(seg)
            for c in range(self.nch):
                self.emax[c] = max(self.emax[c], E[c])
                self.emin[c] = min(self.emin[c], E[c])
                if E[c] >= self.gate[c]:
                    self.R[c] = self.R[c] + terms[c]
                    self.njoin[c] += 1
                    self.ejoin[c] += E[c]
                    self.joined[c].append(self.n + j)
        self.buf = self.buf[:, nseg * L:]
        self.n += nseg
        return nseg

    def reset(self):
        """clears the sums, the count and the four numbers; the pending partial segment and the gates stay"""
        self.R = np.zeros((self.nch, BINS))
        self.n = 0
        self.emax, self.emin = [0] * self.nch, [U64_MAX] * self.nch
        self.njoin, self.ejoin = [0] * self.nch, [0] * self.nch
        self.joined = [[] for _ in range(self.nch)]

    def stats(self):
        """(emax, emin, njoin, ejoin) as uint64 arrays, what RateMeter.read_gate returns first"""
        return tuple(np.array(v, dtype=np.uint64) for v in (self.emax, self.emin, self.njoin, self.ejoin))
