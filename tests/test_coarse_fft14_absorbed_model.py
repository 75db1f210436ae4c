"""CPU model of the absorbed-twiddle form of the workgroup transforms of k_coarse6 (jaero_amd/csrc/wg_fft.h: wg_fft14_e32 and
wg_fft13_e32 with C6_ABSORB 2, and C6_ABSORB 1), in the style of tests/test_coarse_fft14_e32_model.py, whose exchange-1 maps and split-order
first pass it shares.

The twiddle a pass applied to its outputs is moved to the inputs of the pass behind the exchange, where one thread's factors are r^j, and a
decimation-in-frequency butterfly absorbs them: for a block of length M whose input j is meant times rho^j,
    u = a + rho^(M/2) b,   v = 2 a - u,   and the halves are blocks of length M / 2 with ratios rho and rho W_M.
The multiplier of block b at level lv of an L-point transform is r^half W_64^(half (S q + Z)) with half = L >> (lv + 1), S = 64 / L,
q = brev(b, lv) and W_64^Z the constant part of the ratio (W_32 for the upper half of k2 / k1); an index >= 16 is -i times the product for
index - 16.  Outputs stay in place in bit-reversed order.  This file restates those index maps, the ratio table and the exchange addresses
and checks them against numpy's FFT, and every LDS access against the 16-lane bank rule of the existing model."""
import numpy as np
import pytest

import test_coarse_fft14_e32_model as M0

W64 = np.exp(-2j * np.pi * np.arange(64) / 64)


def brev(v, bits):
    return sum(((v >> i) & 1) << (bits - 1 - i) for i in range(bits))


def root_mul(p, idx):
    """c6_root_mul: p W_64^idx for 0 <= idx < 32 from the product with W_64^(idx & 15)"""
    assert 0 <= idx < 32
    r = p * W64[idx & 15]
    return -1j * r if idx & 16 else r


def ratio_powers(r):
    P = [r]
    for _ in range(4):
        P.append(P[-1] * P[-1])
    return P


def afft(x, L, off, Z, P):
    """c6_afft<L, OFF, Z>: x[:, off:off+L] in place; returns the list of W_64 indices used (the ratio table)"""
    LG, S = {32: 5, 16: 4}[L], 64 // L
    used = []
    for lv in range(LG):
        half = L >> (lv + 1)
        for b in range(1 << lv):
            idx = half * (S * brev(b, lv) + Z)
            used.append(idx)
            w = root_mul(P[LG - 1 - lv], idx)
            for j in range(half):
                ia = off + 2 * half * b + j
                ib = ia + half
                a = x[:, ia].copy()
                u = a + w * x[:, ib]
                x[:, ia] = u
                x[:, ib] = 2 * a - u
    return used


def afft16x2(x, r):
    P = ratio_powers(r)
    return afft(x, 16, 0, 0, P) + afft(x, 16, 16, 2, P)


def pass3(x, r, absorbed):
    out = np.zeros_like(x)
    if absorbed:
        afft16x2(x, r)
        for k3 in range(16):
            out[:, 2 * k3] = x[:, brev(k3, 4)]
            out[:, 2 * k3 + 1] = x[:, 16 + brev(k3, 4)]
    else:
        for h in range(2):
            o = np.fft.fft(x[:, 16 * h:16 * h + 16], axis=1)
            for k3 in range(16):
                out[:, 2 * k3 + h] = o[:, k3]
    return out


def twiddle_brev(x, L, off, c, s):
    LG = {32: 5, 16: 4}[L]
    for k in range(L):
        x[:, off + brev(k, LG)] *= c * s ** k


# ------------------------------------------------------------------------------------------------------------------ 2^14 = 32 x 32 x 16
N, T, TW, XLEN = M0.N, M0.T, M0.TW, M0.XLEN


def ex2_write(s):   # pass-2 thread (k1, n3) holds k2 = brev(s, 5)
    k1, n3, k2 = T >> 4, T & 15, brev(s, 5)
    return (k2 & 15) * 32 + k1 + n3 * 513 + (k2 >> 4) * 8208


def model_fft14(x, ab=2):
    d = x.reshape(32, 512).T.copy()
    o = M0.fft32_split(d)                                          # pass 1: no twiddle
    L = np.full(N, np.nan, complex)
    for s in range(32):
        L[M0.ex1_write(s)] = o[:, s]
    d2 = np.stack([L[M0.ex1_read(m)] for m in range(32)], axis=1)
    k1, n3 = T >> 4, T & 15
    afft(d2, 32, 0, 0, ratio_powers(TW[16 * k1]))                  # x W_1024^(k1 n2) absorbed
    if ab == 1:
        twiddle_brev(d2, 32, 0, TW[k1 * n3], TW[32 * n3])          # x W_N^(k1 n3) W_512^(k2 n3)
    L = np.full(XLEN, np.nan, complex)
    for s in range(32):
        L[ex2_write(s)] = d2[:, s]
    d3 = np.stack([L[M0.ex2_read(m & 15, m >> 4)] for m in range(32)], axis=1)   # slot m = n3 + 16 k2hi
    return pass3(d3, TW[T], ab == 2).T.reshape(N)                  # ratio W_N^(k1 + 32 k2lo) = W_N^t, upper half x W_32


# ------------------------------------------------------------------------------------------------------------------ 2^13 = 32 x 16 x 16
N13, T13, TW13, XLEN13 = M0.N13, M0.T13, M0.TW13, M0.XLEN13


def e13_ex2_write(s):        # pass-2 thread (k1a, n3) holds slot s = 16 g + brev(k2, 4)
    return (s >> 4) * 16 + brev(s & 15, 4) * 32 + (T13 >> 4) + 513 * (T13 & 15)


def model_fft13(x, ab=2):
    d = x.reshape(32, 256).T.copy()
    o = M0.fft32_split(d)
    L = np.full(N13, np.nan, complex)
    for s in range(32):
        L[M0.e13_ex1_write(s)] = o[:, s]
    d2 = np.stack([L[M0.e13_ex1_read(m)] for m in range(32)], axis=1)
    k1a, n3 = T13 >> 4, T13 & 15
    afft16x2(d2, TW13[16 * k1a])                                   # x W_512^(k1 n2), k1 = k1a + 16 g
    if ab == 1:
        twiddle_brev(d2, 16, 0, TW13[n3 * k1a], TW13[32 * n3])
        twiddle_brev(d2, 16, 16, TW13[n3 * (k1a + 16)], TW13[32 * n3])
    L = np.full(XLEN13, np.nan, complex)
    for s in range(32):
        L[e13_ex2_write(s)] = d2[:, s]
    d3 = np.stack([L[M0.e13_ex2_read(m)] for m in range(32)], axis=1)
    return pass3(d3, TW13[T13], ab == 2).T.reshape(N13)


CASES = [(14, N, model_fft14), (13, N13, model_fft13)]


def rel_err(got, x):
    want = np.fft.fft(x)
    return np.max(np.abs(got - want)) / np.max(np.abs(want))


@pytest.mark.parametrize("ab", [2, 1])
@pytest.mark.parametrize("log2n,n,model", CASES)
def test_transform_equals_numpy(log2n, n, model, ab):
    rng = np.random.default_rng(log2n)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    assert rel_err(model(x, ab), x) < 1e-12
    nt = n // 32
    for pos in (0, 1, 15, 16, 17, nt - 1, nt, nt + 1, 16 * nt + 5, n // 2, n - 1):   # a unit impulse: every output has modulus 1
        x = np.zeros(n, complex)
        x[pos] = 1.0
        assert rel_err(model(x, ab), x) < 1e-12, pos
    for k in (0, 1, 31, 32, 33, 1023, 1024, nt - 1, nt, n // 2, n // 2 + 1, n - 1):   # a tone on bin k: one output n, the others 0
        x = np.exp(2j * np.pi * k * np.arange(n) / n)
        got = model(x, ab)
        assert rel_err(got, x) < 1e-12 and int(np.argmax(np.abs(got))) == k, k


def test_ratio_table():
    """The multipliers' constant roots: every index lies in [0, 32), the 32-point pass needs 11 products with a root (1 + 3 + 7 of the
    indices 1 .. 15 once -i is free), the pair of 16-point passes 4 + 7."""
    x = np.zeros((1, 32), complex)
    u32 = afft(x, 32, 0, 0, ratio_powers(1.0 + 0j))
    assert len(u32) == 31 and all(0 <= i < 32 for i in u32)
    per_level = [u32[(1 << lv) - 1:(2 << lv) - 1] for lv in range(5)]
    assert [len({i & 15 for i in lv} - {0}) for lv in per_level] == [0, 0, 1, 3, 7]
    P = ratio_powers(1.0 + 0j)
    lo, hi = afft(x, 16, 0, 0, P), afft(x, 16, 16, 2, P)
    assert len(lo) == len(hi) == 15 and all(0 <= i < 32 for i in lo + hi)
    count = lambda u: sum(len({i & 15 for i in u[(1 << lv) - 1:(2 << lv) - 1]} - {0}) for lv in range(4))
    assert (count(lo), count(hi)) == (4, 7)


def test_exchange_addresses():
    """Exchange 1 is the existing model's; exchange 2's writers change with the order pass 2 leaves its outputs in.  Inside the buffer, a
    permutation that the readers invert, and conflict-free under the 16-lane rule."""
    w = np.concatenate([ex2_write(s) for s in range(32)])
    r = np.concatenate([M0.ex2_read(n3, h) for n3 in range(16) for h in range(2)])
    assert len(set(w.tolist())) == N and sorted(w) == sorted(r) and w.min() >= 0 and w.max() < XLEN
    w13 = np.concatenate([e13_ex2_write(s) for s in range(32)])
    r13 = np.concatenate([M0.e13_ex2_read(m) for m in range(32)])
    assert len(set(w13.tolist())) == N13 and sorted(w13) == sorted(r13) and w13.min() >= 0 and w13.max() < XLEN13
    for maps, waves in (([ex2_write(s) for s in range(32)], 8), ([e13_ex2_write(s) for s in range(32)], 4)):
        for a in maps:
            for q in range(4 * waves):
                assert len(set((a[16 * q:16 * q + 16] % 16).tolist())) == 16
    # the twiddle table entries the passes read: tw[16 k1], tw[t] (and for C6_ABSORB 1 tw[k1 n3], tw[32 n3]) stay below the thread count
    assert (16 * (T >> 4)).max() < 512 and ((T >> 4) * (T & 15)).max() < 512 and ((T13 & 15) * ((T13 >> 4) + 16)).max() < 512
