"""The channeliser's definition (include/jaero_hip.h, "wideband I/Q channeliser") in numpy, literally, and the ideal form it is measured
against: mix -> np.convolve -> decimate.  The GPU kernels are tested against `ChanOracle`; the two forms against each other on the CPU
(tests/test_chan_host.py)."""
import numpy as np

N = 16384
HP = N // 2
DECIMS = (16, 32, 64, 128, 256)  # the arithmetic depends on decim only through M = N / decim; the output rate (48, 24 or 12 kHz) is a label


def words(tune, audio, decim):
    """(b, rho, w): nearest bin of the tuning word read as a signed number, what is left, phase word per output sample."""
    t = int(tune) % (1 << 32)
    if t >= 1 << 31:
        t -= 1 << 32
    b = (t + (1 << 17)) >> 18  # Python's >> is arithmetic
    rho = t - b * (1 << 18)
    return b, rho, (int(audio) - rho * decim) % (1 << 32)


def rotation(w, m0, n):
    """e^(j 2 pi ((w m) mod 2^32) / 2^32) for m = m0 .. m0 + n - 1, m an absolute count (Python integers: no overflow)."""
    m = (np.arange(n, dtype=np.uint64) + np.uint64(m0 % (1 << 32))) % np.uint64(1 << 32)
    ph = (np.uint64(w) * m) % np.uint64(1 << 32)  # w, m < 2^32: the product fits in 64 bits
    return np.exp(2j * np.pi * (ph.astype(np.float64) / 4294967296.0))


def to_int16(y):
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)


def as_complex(iq):
    """int16 [n, 2] (or [2 n]) -> complex128 [n]"""
    a = np.asarray(iq).reshape(-1, 2).astype(np.float64)
    return a[:, 0] + 1j * a[:, 1]


class ChanOracle:
    """Streaming form: write() takes any number of complex samples and returns the unrounded y* [nch, nout] the blocks completed by
    this write produce.  channels: (tune, audio, gain) per channel; retune() replaces one from the next write on."""

    def __init__(self, decim, channels, taps):
        assert decim in DECIMS
        taps = np.asarray(taps, dtype=np.float64)
        assert 1 <= len(taps) <= N // 2 + 1
        self.D, self.M = decim, N // decim
        self.Mo = self.M // 2
        self.G = np.fft.fft(np.concatenate([taps, np.zeros(N - len(taps))]))
        self.channels = [tuple(c) for c in channels]
        self.buf = np.zeros(HP, dtype=np.complex128)  # x[n] = 0 for n < 0; then: previous hop + what waits
        self.p = 0

    def retune(self, channel, tune, audio, gain):
        self.channels[channel] = (tune, audio, gain)

    def write(self, x):
        self.buf = np.concatenate([self.buf, np.asarray(x, dtype=np.complex128)])
        nblk = (len(self.buf) - HP) // HP
        M, Mo = self.M, self.Mo
        out = np.zeros((len(self.channels), nblk * Mo))
        q = np.arange(-M // 2, M // 2)
        for j in range(nblk):
            p = self.p + j
            X = np.fft.fft(self.buf[j * HP: j * HP + N])
            for c, (tune, audio, gain) in enumerate(self.channels):
                b, _, w = words(tune, audio, self.D)
                Y = X[(b + q) % N] * self.G[q % N]
                wr = np.fft.ifft(np.fft.ifftshift(Y)) * (M / N)  # (1 / N) sum_q Y[q] e^(+j 2 pi q r / M)
                v = wr[Mo:] * (-1.0 if (b * (p - 1)) % 2 else 1.0)
                out[c, j * Mo:(j + 1) * Mo] = gain * (v * rotation(w, p * Mo, Mo)).real
        self.buf = self.buf[nblk * HP:]
        self.p += nblk
        return out


def block_form(x, decim, channels, taps):
    """All whole blocks of x at once: unrounded y* [nch, floor(len(x) / Hp) Mo]."""
    return ChanOracle(decim, channels, taps).write(x)


def direct_form(x, decim, tune, audio, gain, taps, nout):
    """The ideal the block form approximates to the level of the taps' stop band: shift bin b to zero, FIR, keep every D-th sample,
    rotate by the phase word, real part."""
    b, _, w = words(tune, audio, decim)
    n = np.arange(len(x))
    xm = np.asarray(x) * np.exp(-2j * np.pi * ((b * n) % N) / N)
    u = np.convolve(xm, taps)[:len(x)][::decim][:nout]
    return gain * (u * rotation(w, 0, len(u))).real
