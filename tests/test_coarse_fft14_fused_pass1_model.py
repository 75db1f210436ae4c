"""CPU model of the fused first pass of the workgroup transforms of k_coarse6 (jaero_amd/csrc/wg_fft.h: c6_cfft32, P1; DESIGN 9
item 34), beside tests/test_coarse_fft14_absorbed_model.py, whose passes 2 and 3 and exchange 2 it shares.

The pass in front of exchange 1 has no twiddle to absorb: it is the absorbed butterfly network for the ratio 1, whose multiplier for block b at
level lv is the constant root W_64^(half 2 brev(b, lv)), half = 16 >> lv.  A root 1 or -i (index 0 or 16) makes the butterfly four
additions; every other one is u = a + w b, v = 2 a - u, six fused multiply-adds.  X[k] is left in slot brev(k, 5) instead of the split order
of the parent's pass, which changes which slot a thread writes to an address of exchange 1 and no address."""
import numpy as np
import pytest

import test_coarse_fft14_absorbed_model as M2
import test_coarse_fft14_e32_model as M0

brev = M2.brev


def cfft32(x):
    """c6_cfft32: x[:, 0:32] in place; returns [(index, trivial)] per butterfly"""
    kinds = []
    for lv in range(5):
        half = 16 >> lv
        for b in range(1 << lv):
            idx = half * 2 * brev(b, lv)
            assert 0 <= idx < 32
            e = idx & 15
            w = M2.W64[e]
            if idx & 16:
                w = complex(w.imag, -w.real)   # -i times the root of idx - 16
            for j in range(half):
                ia = 2 * half * b + j
                ib = ia + half
                a, bb = x[:, ia].copy(), x[:, ib].copy()
                if idx == 0:
                    x[:, ia], x[:, ib] = a + bb, a - bb
                elif idx == 16:
                    t = bb.imag - 1j * bb.real
                    x[:, ia], x[:, ib] = a + t, a - t
                else:
                    u = a + w * bb
                    x[:, ia], x[:, ib] = u, 2 * a - u
                kinds.append((idx, e == 0))
    return kinds


def ex1_write(s):       # pass-1 thread t = 16 n2 + n3 holds k1 = brev(s, 5): the address of M0.ex1_write for that k1
    k1 = brev(s, 5)
    return k1 * 512 + ((M0.T + 16 * (k1 & 1)) & 511)


def e13_ex1_write(s):
    return brev(s, 5) * 256 + M0.T13


def model_fft14(x):
    N, T, TW = M0.N, M0.T, M0.TW
    d = x.reshape(32, 512).T.copy()
    cfft32(d)
    L = np.full(N, np.nan, complex)
    for s in range(32):
        L[ex1_write(s)] = d[:, s]
    d2 = np.stack([L[M0.ex1_read(m)] for m in range(32)], axis=1)
    M2.afft(d2, 32, 0, 0, M2.ratio_powers(TW[16 * (T >> 4)]))
    L = np.full(M0.XLEN, np.nan, complex)
    for s in range(32):
        L[M2.ex2_write(s)] = d2[:, s]
    d3 = np.stack([L[M0.ex2_read(m & 15, m >> 4)] for m in range(32)], axis=1)
    return M2.pass3(d3, TW[T], True).T.reshape(N)


def model_fft13(x):
    N13, T13, TW13 = M0.N13, M0.T13, M0.TW13
    d = x.reshape(32, 256).T.copy()
    cfft32(d)
    L = np.full(N13, np.nan, complex)
    for s in range(32):
        L[e13_ex1_write(s)] = d[:, s]
    d2 = np.stack([L[M0.e13_ex1_read(m)] for m in range(32)], axis=1)
    M2.afft16x2(d2, TW13[16 * (T13 >> 4)])
    L = np.full(M0.XLEN13, np.nan, complex)
    for s in range(32):
        L[M2.e13_ex2_write(s)] = d2[:, s]
    d3 = np.stack([L[M0.e13_ex2_read(m)] for m in range(32)], axis=1)
    return M2.pass3(d3, TW13[T13], True).T.reshape(N13)


def test_pass_is_a_32_point_dft_in_bit_reversed_order():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((7, 32)) + 1j * rng.standard_normal((7, 32))
    want = np.fft.fft(x, axis=1)
    got = x.copy()
    kinds = cfft32(got)
    for k in range(32):
        assert np.max(np.abs(got[:, brev(k, 5)] - want[:, k])) < 1e-12 * np.max(np.abs(want)), k
    # 80 butterflies: 46 with a root 1 or -i (four additions), 34 fused; the fused ones use the roots 1 .. 15 of W_64 and -i times them
    assert len(kinds) == 80 and sum(t for _, t in kinds) == 46
    assert {i for i, t in kinds if t} == {0, 16} and all(i & 15 for i, t in kinds if not t)
    # the same network as the absorbed pass for the ratio 1
    ref = x.copy()
    used = M2.afft(ref, 32, 0, 0, M2.ratio_powers(1.0 + 0j))
    assert np.max(np.abs(ref - got)) < 1e-13 * np.max(np.abs(want))
    assert used == [(16 >> lv) * 2 * brev(b, lv) for lv in range(5) for b in range(1 << lv)]


@pytest.mark.parametrize("log2n,n,model", [(14, M0.N, model_fft14), (13, M0.N13, model_fft13)])
def test_transform_equals_numpy(log2n, n, model):
    rng = np.random.default_rng(log2n)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    assert M2.rel_err(model(x), x) < 1e-12
    nt = n // 32
    for pos in (0, 1, 15, 16, 17, nt - 1, nt, nt + 1, 16 * nt + 5, n // 2, n - 1):   # a unit impulse: every output has modulus 1
        x = np.zeros(n, complex)
        x[pos] = 1.0
        assert M2.rel_err(model(x), x) < 1e-12, pos
    for k in (0, 1, 31, 32, 33, 1023, 1024, nt - 1, nt, n // 2, n // 2 + 1, n - 1):   # a tone on bin k: one output n, the others 0
        x = np.exp(2j * np.pi * k * np.arange(n) / n)
        got = model(x)
        assert M2.rel_err(got, x) < 1e-12 and int(np.argmax(np.abs(got))) == k, k


def test_exchange_1_addresses_are_the_parents():
    """The same set of addresses per k1, so the readers and the bank behaviour of exchange 1 are the existing model's: only the slot that
    holds a k1 differs.  The 16-lane rule is checked again on the writers all the same."""
    K = M0.K
    for k1 in range(32):
        s_new, s_old = brev(k1, 5), next(s for s in range(32) if K(s) == k1)
        assert np.array_equal(ex1_write(s_new), M0.ex1_write(s_old))
        assert np.array_equal(e13_ex1_write(s_new), M0.e13_ex1_write(s_old))
    for maps, waves in (([ex1_write(s) for s in range(32)], 8), ([e13_ex1_write(s) for s in range(32)], 4)):
        assert sorted(np.concatenate(maps).tolist()) == list(range(32 * 64 * waves))
        for a in maps:
            for q in range(4 * waves):
                assert len(set((a[16 * q:16 * q + 16] % 16).tolist())) == 16
