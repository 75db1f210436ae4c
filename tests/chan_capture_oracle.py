"""The capture front end's definition (include/jaero_hip.h, "capture front end of the channeliser") in numpy, literally: the conversions of
the four raw formats, the mix by an integer phase word, the streaming rational resampler, and their composition with
`chan_oracle.ChanOracle` (which accepts any complex input).  The GPU kernels (k_capture_stage, k_capture_fwd) are tested against this
(tests/test_gpu_chan_capture.py); this against itself and against ideal tones on the CPU (tests/test_chan_capture_host.py).

Every product and every sum below is one whole-array numpy operation on float64, so each rounds once, as the definition says; real and
imaginary parts are kept in separate arrays."""
from math import gcd

import numpy as np

CS16, CU8, CS8, CF32 = 0, 1, 2, 3
FORMATS = {"cs16": CS16, "cu8": CU8, "cs8": CS8, "cf32": CF32}
DTYPES = {CS16: np.int16, CU8: np.uint8, CS8: np.int8, CF32: np.float32}


def ratio(fs_in, fs_c):
    """(L, Mr): fs_c / fs_in in lowest terms."""
    g = gcd(int(fs_in), int(fs_c))
    return int(fs_c) // g, int(fs_in) // g


def convert(raw, fmt):
    """raw [n, 2] (or [2 n]) of the format's dtype -> (re, im) float64 in int16 LSB units, exact."""
    a = np.asarray(raw)
    assert a.dtype == DTYPES[fmt], (a.dtype, fmt)
    a = a.reshape(-1, 2)
    if fmt == CS16:
        x = a.astype(np.float64)
    elif fmt == CU8:
        x = ((2 * a.astype(np.int64) - 255) * 128).astype(np.float64)
    elif fmt == CS8:
        x = (a.astype(np.int64) * 256).astype(np.float64)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            x = a.astype(np.float64) * 32768.0
        x = np.where(np.isfinite(a), x, 0.0)
    return x[:, 0].copy(), x[:, 1].copy()


def mix(re, im, shift, n0):
    """x'[n] = x[n] e^(j 2 pi ((shift n) mod 2^32) / 2^32) for n = n0 .. n0 + len - 1 (absolute), the phase read as a signed word;
    shift == 0: the input itself."""
    shift = int(shift) % (1 << 32)
    if shift == 0:
        return re, im
    n = (np.arange(len(re), dtype=np.uint64) + np.uint64(n0 % (1 << 32))) % np.uint64(1 << 32)
    ph = (np.uint64(shift) * n) % np.uint64(1 << 32)  # shift, n < 2^32: the product fits in 64 bits
    s = ph.astype(np.int64)
    s = np.where(s >= 1 << 31, s - (1 << 32), s).astype(np.float64) / 2147483648.0  # [-1, 1): the angle / pi
    c, sn = np.cos(np.pi * s), np.sin(np.pi * s)
    return re * c - im * sn, re * sn + im * c


class Resampler:
    """z[m] = sum_{j < K} h[phi_m + j L] x'[n_m - j], n_m = floor(m Mr / L), phi_m = (m Mr) mod L, x'[n] = 0 for n < 0; streaming: write()
    takes any number of samples (re, im) and returns the z[m] that now exist (n_m <= T - 1), m and T absolute counts from creation."""

    def __init__(self, h, L, Mr, K):
        self.h = np.asarray(h, dtype=np.float64)
        assert self.h.shape == (L * K,)
        self.L, self.Mr, self.K = int(L), int(Mr), int(K)
        self.T = 0  # input samples taken
        self.m = 0  # outputs made
        self.hr = np.zeros(K - 1)  # x'[T - (K - 1) .. T)
        self.hi = np.zeros(K - 1)

    def write(self, re, im):
        L, Mr, K = self.L, self.Mr, self.K
        xr = np.concatenate([self.hr, np.asarray(re, dtype=np.float64)])
        xi = np.concatenate([self.hi, np.asarray(im, dtype=np.float64)])
        base = self.T - (K - 1)  # absolute index of xr[0]
        T1 = self.T + len(re)
        m1 = -(-T1 * L // Mr)  # ceil(T1 L / Mr), Python integers
        m = np.arange(self.m, m1, dtype=np.int64)
        n_m = (m * Mr) // L
        phi = (m * Mr) % L
        zr, zi = np.zeros(len(m)), np.zeros(len(m))
        for j in range(K):
            hj = self.h[phi + j * L]
            zr = zr + hj * xr[n_m - j - base]
            zi = zi + hj * xi[n_m - j - base]
        if K > 1:
            self.hr, self.hi = xr[len(xr) - (K - 1):].copy(), xi[len(xi) - (K - 1):].copy()
        self.T, self.m = T1, m1
        return zr, zi


class CaptureOracle:
    """convert -> mix -> resample, streaming: write(raw) returns the staged samples (complex128) this write made; `first` is the absolute
    index of the first of them."""

    def __init__(self, fmt, fs_in, fs_c, shift=0, K=1, rtaps=None):
        self.fmt = FORMATS[fmt] if isinstance(fmt, str) else fmt
        self.L, self.Mr = ratio(fs_in, fs_c)
        self.shift = int(shift) % (1 << 32)
        self.T = 0
        self.first = 0
        self.rs = None
        if (self.L, self.Mr) != (1, 1):
            self.rs = Resampler(rtaps, self.L, self.Mr, K)

    def write(self, raw):
        re, im = convert(raw, self.fmt)
        re, im = mix(re, im, self.shift, self.T)
        self.first = self.rs.m if self.rs else self.T
        self.T += len(re)
        if self.rs:
            re, im = self.rs.write(re, im)
        z = np.empty(len(re), dtype=np.complex128)  # component by component: a sum with 1j would turn -0.0 into 0.0
        z.real, z.imag = re, im
        return z


def gain_bound(h, L):
    """S = max_phi sum_j |h[phi + j L]|: the most a unit input can make of one output."""
    return float(np.abs(np.asarray(h)).reshape(-1, L).sum(axis=0).max())
