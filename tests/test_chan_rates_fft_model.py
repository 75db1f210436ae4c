"""CPU model of k_chan_synth's M-point transform (jaero_amd/csrc/k_chan.h) for the two small shapes, M = 128 (D = 128) and M = 64 (D = 256),
as built: tests/test_chan_fft_model.py's three tests with ChanShape<128> / <256>'s constants.

  M = 128 = 8 x 16, T = 16, SPLIT = 2, P2 = 8: the 512 case with 8-point transforms; the radix-2 step that shares a row's 16-point FFT
            between threads (k1, 0) and (k1, 1) multiplies by W_16^(h n)
  M =  64 = 8 x 8,  T = 8,  SPLIT = 1, P2 = 8: the 256 case with 8-point transforms
Every thread ends with 4 outputs; the item's Mo int16 are T 8-byte words of the staging buffer and lane u stores word u."""
import numpy as np
import pytest

from chan_cases import N, model_item


class Shape:
    def __init__(self, D):
        self.D, self.M = D, N // D
        self.MO = self.M // 2
        self.R1 = 8
        self.R2 = 16 if self.M == 128 else 8
        self.P2 = 8
        self.SPLIT = self.R2 // self.P2
        self.T = self.R2
        self.ITEMS = 256 // self.T
        self.THREADS = self.ITEMS * self.T
        self.ROW = self.R2 + 1
        self.XCH = self.R1 * self.ROW
        self.OUTS = self.MO // self.T

    def xaddr(self, k1, n2):
        return k1 * self.ROW + n2


def model_item_small(S, X, G, b):
    """chan_cases.model_item with the split step's twiddle W_R2^(h n) instead of its literal W_32^(h n)."""
    if S.SPLIT == 1:
        return model_item(S, X, G, b)
    M, R1, R2, P2, T = S.M, S.R1, S.R2, S.P2, S.T
    u = np.arange(T)
    a = np.zeros((T, R1), complex)
    for n1 in range(R1):
        k = R2 * n1 + u
        q = np.where(k < M // 2, k, k - M)
        Y = X[(b + q) % N] * G[q % N] / N
        a[:, n1] = Y.imag + 1j * Y.real
    A = np.fft.fft(a, axis=1) * np.exp(-2j * np.pi * u / M)[:, None] ** np.arange(R1)[None, :]
    L = np.full(S.XCH, np.nan, complex)
    for k in range(R1):
        L[S.xaddr(k, u)] = A[:, k]
    k1, h = u % R1, u // R1
    e = np.stack([L[S.xaddr(k1, n)] + np.where(h, -1.0, 1.0) * L[S.xaddr(k1, n + P2)] for n in range(P2)], axis=1)
    e = e * np.where(h, np.exp(-2j * np.pi / R2), 1.0)[:, None] ** np.arange(P2)[None, :]
    E = np.fft.fft(e, axis=1)
    ml = np.zeros((T, P2 // 2), int)
    w = np.zeros((T, P2 // 2), complex)
    for jj in range(P2 // 2):
        k2 = 2 * (jj + P2 // 2) + h
        ml[:, jj] = k1 + R1 * (k2 - R2 // 2)
        s = E[:, jj + P2 // 2]
        w[:, jj] = s.imag + 1j * s.real
    return ml, w


@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("b", [0, 1234, -8000, 8190, -8192])
def test_item_is_the_second_half_of_the_definition(D, b):
    S = Shape(D)
    rng = np.random.default_rng(D + b % 97)
    X = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    G = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    ml, w = model_item_small(S, X, G, b)
    assert ml.shape == (S.T, 4)
    assert sorted(ml.reshape(-1).tolist()) == list(range(S.MO))  # every output sample of the block once
    q = np.arange(-S.M // 2, S.M // 2)
    Y = X[(b + q) % N] * G[q % N]
    r = np.arange(S.M)
    ref = (Y[None, :] * np.exp(2j * np.pi * q[None, :] * r[:, None] / S.M)).sum(axis=1) / N   # w[r], literally
    assert np.max(np.abs(w - ref[S.MO + ml])) < 1e-10 * np.abs(ref).max()


@pytest.mark.parametrize("D,lds", [(128, 17408), (256, 18432)])
def test_shapes(D, lds):
    S = Shape(D)
    assert S.R1 * S.R2 == S.M and S.SPLIT * S.P2 == S.R2 and S.T * (S.P2 // 2) == S.MO
    assert S.THREADS == 256 and 64 % S.T == 0                                    # an item never straddles two wavefronts
    assert S.ITEMS * S.XCH * 8 == lds and (S.XCH * 8) % 16 == 0                  # static LDS; every item's int16 staging is 16-byte aligned
    # the generalised store: a thread's outputs are whole 16-byte words (the three large shapes) or, here, one 8-byte word: the item's
    # Mo int16 are exactly T such words, lane u stores word u, and the item's run in pcm starts on an 8-byte boundary
    assert S.OUTS == 4 and S.OUTS % 8 != 0 and S.MO * 2 == S.T * 8 and (S.MO * 2) % 8 == 0
    assert S.MO * 2 <= S.XCH * 8                                                  # the staging fits
    assert S.R1 <= 8 and S.T <= 32                                                # regfft<8>; the 32-entry W_M^k table covers twm[u]


@pytest.mark.parametrize("D", [128, 256])
def test_lds_accesses_are_conflict_free(D):
    S = Shape(D)
    tid = np.arange(S.THREADS)
    u, li = tid % S.T, tid // S.T
    k1 = u % S.R1
    base = li * S.XCH

    def conflicts(addr, lanes, banks):
        worst = 1
        for g in range(0, S.THREADS, lanes):
            distinct = set(addr[g:g + lanes].tolist())             # identical addresses broadcast
            per_bank = {}
            for a in distinct:
                per_bank[a % banks] = per_bank.get(a % banks, 0) + 1
            worst = max(worst, max(per_bank.values()))
        return worst

    for k in range(S.R1):      # writes: thread u stores (k, u)
        assert conflicts(base + S.xaddr(k, u), 16, 16) == 1, ("write", k)
    for n in range(S.R2):      # reads: thread (k1, h) loads (k1, n)
        assert conflicts(base + S.xaddr(k1, n), 32, 32) == 1, ("read", n)
    # an even row stride (items R1 R2 doubles apart) would put a read's rows on a few banks: what the + 1 is for
    assert conflicts(li * S.R1 * S.R2 + k1 * S.R2 + 0, 32, 32) >= 4
    # the staging buffer read back as 8-byte words, lane u word u of its item, once per item: free at M = 64; at M = 128 two items' words
    # (bases 136 doubles apart) share 8 of 32 banks
    assert conflicts(base + u, 32, 32) == (2 if D == 128 else 1)
