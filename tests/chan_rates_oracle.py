"""The channeliser's definition (tests/chan_oracle.py) at every total decimation 16 .. 256: the arithmetic of `ChanOracle.write`, `words` and
`direct_form` depends on decim only through M = N / decim, so the subclass only widens what the constructor accepts.  The output rate
(48, 24 or 12 kHz) is a label and does not appear."""
import numpy as np

import chan_oracle as CO

N, HP = CO.N, CO.HP
DECIMS = (16, 32, 64, 128, 256)
words, rotation, to_int16, as_complex, direct_form = CO.words, CO.rotation, CO.to_int16, CO.as_complex, CO.direct_form


class ChanRatesOracle(CO.ChanOracle):
    def __init__(self, decim, channels, taps):
        assert decim in DECIMS
        taps = np.asarray(taps, dtype=np.float64)
        assert 1 <= len(taps) <= N // 2 + 1
        self.D, self.M = decim, N // decim
        self.Mo = self.M // 2
        self.G = np.fft.fft(np.concatenate([taps, np.zeros(N - len(taps))]))
        self.channels = [tuple(c) for c in channels]
        self.buf = np.zeros(HP, dtype=np.complex128)
        self.p = 0


def block_form(x, decim, channels, taps):
    """All whole blocks of x at once: unrounded y* [nch, floor(len(x) / Hp) Mo]."""
    return ChanRatesOracle(decim, channels, taps).write(x)
