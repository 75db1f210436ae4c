"""The one-pass gates' definition (include/jaero_hip.h, "one-pass gates") in Python integers, literally, on rate_oracle.segment_terms.  The
GPU kernel (k_rate_lines_auto) is tested against `AutoRateOracle`; the oracle against `RateOracle`, against the tables of energy sequences
and against itself on the CPU (tests/test_rate_auto_host.py)."""
import numpy as np

import rate_gate_oracle as GO
import rate_oracle as RO

L, BINS = RO.L, RO.BINS
U64_MAX = GO.U64_MAX
HBINS = 321
MANUAL, AUTO, HIST = 1, 2, 4


def energy_bin(E):
    """the histogram bin of E, by the definition's shifts (jaero_amd.ratemeter.energy_bin is tested against the same spot values)"""
    E = int(E)
    if E < 8:
        return E
    e = E.bit_length() - 1
    return 8 * (e - 2) + ((E >> (e - 3)) & 7)


class AutoRateOracle:
    """Streaming form, as GatedRateOracle: write() takes int16 [nch, n] for any n and returns the segments it completed.  mode: AUTO or
    MANUAL, with or without HIST (the histogram is kept either way; HIST says whether a handle would hand it out).  Per channel, as lists
    of Python ints since create or the last reset(): emax, emin, njoin, ejoin, e2, start (U64_MAX: never restarted), gate; `joined[c]`
    lists the segments that are in R[c] -- after a restart only those from `start[c]` on --, counted from the last reset; `gates[c]` the
    gate after every segment; `hist` [nch][321] counts every completed segment."""

    def __init__(self, nch, mode=AUTO):
        assert mode & ~HIST in (MANUAL, AUTO)
        self.nch, self.mode = nch, mode
        self.buf = np.zeros((nch, 0), dtype=np.int64)
        self.gate = [0] * nch
        self.reset()

    def set_gate(self, g):
        assert not self.mode & AUTO and len(g) == self.nch and all(0 <= int(v) <= U64_MAX for v in g)
        self.gate = [int(v) for v in g]

    def set_mode(self, mode):
        """as jaero_gate2_enable: clears as reset() does; the gates stay unless the new mode has AUTO"""
        assert mode & ~HIST in (MANUAL, AUTO)
        self.mode = mode
        self.reset()

    def step(self, c, s, E, term):
        """segment number s of channel c, with energy E and terms |H_s|^2: the definition, line by line"""
        if self.mode & AUTO:
            if E > self.emax[c]:
                self.e2[c] = self.emax[c]
                self.emax[c] = E
            elif E > self.e2[c]:
                self.e2[c] = E
            self.emin[c] = min(self.emin[c], E)
            e2, emin = self.e2[c], self.emin[c]
            g1 = (e2 + emin) // 2 if e2 > 0 and 2 * e2 >= 3 * emin else 0
        else:
            self.emax[c] = max(self.emax[c], E)
            self.emin[c] = min(self.emin[c], E)
            g1 = self.gate[c]
        join = E >= g1
        restart = self.gate[c] == 0 and g1 > 0 and join
        if restart:
            self.R[c] = term.copy()
            self.njoin[c], self.ejoin[c], self.start[c] = 1, E, s
            self.joined[c] = [s]
        elif join:
            self.R[c] = self.R[c] + term
            self.njoin[c] += 1
            self.ejoin[c] += E
            self.joined[c].append(s)
        self.gate[c] = g1
        self.gates[c].append(g1)
        self.hist[c][energy_bin(E)] += 1

    def write(self, pcm):
        pcm = np.asarray(pcm)
        assert pcm.ndim == 2 and pcm.shape[0] == self.nch
        self.buf = np.concatenate([self.buf, pcm.astype(np.int64)], axis=1)
        nseg = self.buf.shape[1] // L
        for j in range(nseg):
            seg = self.buf[:, j * L:(j + 1) * L]
            E = GO.segment_energy(seg)
            terms = RO.segment_terms(seg)
            for c in range(self.nch):
                self.step(c, self.n + j, E[c], terms[c])
        self.buf = self.buf[:, nseg * L:]
        self.n += nseg
        return nseg

    def reset(self):
        """clears the sums, the count, the six numbers and the histogram; the pending partial segment stays; the gates stay but under AUTO"""
        nch = self.nch
        self.R = np.zeros((nch, BINS))
        self.n = 0
        self.emax, self.emin = [0] * nch, [U64_MAX] * nch
        self.njoin, self.ejoin = [0] * nch, [0] * nch
        self.e2, self.start = [0] * nch, [U64_MAX] * nch
        if self.mode & AUTO:
            self.gate = [0] * nch
        self.joined = [[] for _ in range(nch)]
        self.gates = [[] for _ in range(nch)]
        self.hist = [[0] * HBINS for _ in range(nch)]

    def stats(self):
        """(emax, emin, njoin, ejoin, e2, start) as uint64 arrays, what RateMeter.read_gate_auto returns first"""
        return tuple(np.array(v, dtype=np.uint64) for v in (self.emax, self.emin, self.njoin, self.ejoin, self.e2, self.start))

    def hist_array(self):
        return np.array(self.hist, dtype=np.uint32)
