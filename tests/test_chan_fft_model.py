"""CPU model of k_chan_synth's M-point transform (jaero_amd/csrc/k_chan.h) for the three M = N / D.

The kernel only runs on the GPU (tests/test_gpu_chan.py); what can be pinned without one is its index arithmetic: (i) the gather order,
the two passes, the twiddles, the exchange map and -- for 512 = 16 x 32 -- the radix-2 step that shares a row's 32-point FFT between two
threads turn "bins b - M/2 .. b + M/2 - 1 of the spectrum" into the second half of the definition's w[r], each thread holding the output
samples the kernel says it holds; (ii) every thread's outputs together are the block's Mo samples, once each; (iii) the LDS addresses: a
64-bit read is served 32 lanes at a time from 32 eight-byte banks, a 64-bit write 16 lanes at a time from 16, identical addresses
broadcast."""
import numpy as np
import pytest

from chan_cases import N, model_item


class Shape:
    def __init__(self, D):
        self.D, self.M = D, N // D
        self.MO = self.M // 2
        self.R1 = 32 if self.M == 1024 else 16
        self.R2 = 16 if self.M == 256 else 32
        self.P2 = 32 if self.M == 1024 else 16
        self.SPLIT = self.R2 // self.P2
        self.T = self.R2
        self.ITEMS = 4 if self.M == 1024 else 256 // self.T
        self.THREADS = self.ITEMS * self.T
        self.ROW = self.R2 + 1
        self.XCH = self.R1 * self.ROW

    def xaddr(self, k1, n2):
        return k1 * self.ROW + n2


@pytest.mark.parametrize("D", [16, 32, 64])
@pytest.mark.parametrize("b", [0, 1234, -8000, 8190, -8192])
def test_item_is_the_second_half_of_the_definition(D, b):
    S = Shape(D)
    rng = np.random.default_rng(D + b % 97)
    X = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    G = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    ml, w = model_item(S, X, G, b)
    # every output sample of the block once
    assert sorted(ml.reshape(-1).tolist()) == list(range(S.MO))
    q = np.arange(-S.M // 2, S.M // 2)
    Y = X[(b + q) % N] * G[q % N]
    r = np.arange(S.M)
    ref = (Y[None, :] * np.exp(2j * np.pi * q[None, :] * r[:, None] / S.M)).sum(axis=1) / N   # w[r], literally
    assert np.max(np.abs(w - ref[S.MO + ml])) < 1e-10 * np.abs(ref).max()


@pytest.mark.parametrize("D", [16, 32, 64])
def test_shapes(D):
    S = Shape(D)
    assert S.R1 * S.R2 == S.M and S.SPLIT * S.P2 == S.R2 and S.T * (S.P2 // 2) == S.MO
    assert S.THREADS in (128, 256) and S.THREADS % 64 == 0 and 64 % S.T == 0     # an item never straddles two wavefronts
    assert S.ITEMS * S.XCH * 8 <= 65536 and (S.XCH * 8) % 16 == 0                # static LDS; every item's int16 staging is 16-byte aligned
    assert S.MO * 2 <= S.XCH * 8 and (S.MO // S.T) % 8 == 0                       # the staging fits; whole 16-byte stores per thread


@pytest.mark.parametrize("D", [16, 32, 64])
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
    # an even row stride would put the 16 k1 of a read on a few banks: what the + 1 is for
    assert conflicts(base + k1 * S.R2 + 0, 32, 32) > 4
