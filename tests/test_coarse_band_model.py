"""CPU model of the band-aware estimate kernel k_coarse6_b7 (jaero_amd/csrc/k_coarse6.h: coarse6_body<false, 14, 7, 1792>; wg_fft.h: c6_cfft32_band;
DESIGN 9 item 35), beside tests/test_coarse_fft14_fused_pass1_model.py and tests/test_coarse_fft14_absorbed_model.py, whose networks it prunes.

A locking band of startbin = 7 * 512 makes the boxcar band limit zero slots 7 .. 24 of every thread of the 32 x 32 x 16 transform (and slot 25
of thread 0).  From the index maps of that transform this checks which registers of the first transform's pass 3 hold those slots, that a
network which never forms them gives the kept outputs of the full one bit for bit, and that pass 1 of the second transform with the zeros
followed through its butterflies equals the full pass on the same input.  The host's class expression is set against the kernel's own."""
import math

import numpy as np

import coarse_cases as CC
import test_coarse_fft14_absorbed_model as M2
import test_coarse_fft14_fused_pass1_model as M1

brev = M2.brev
SB, EPB, N, NT, E = 7, 1792, 1 << 14, 512, 32
ZERO = set(range(SB, E - SB))  # slots 7 .. 24


# ------------------------------------------------------------------------------------------------------------------ pass 3, first transform
def pass3_slot_of_register():
    """register (position in the thread's CV<32> behind c6_afft16x2) -> natural slot, from c6_pass3: slot 2 k3 + h <- 16 h + brev(k3, 4)"""
    m = {}
    for k3 in range(16):
        for h in range(2):
            m[16 * h + brev(k3, 4)] = 2 * k3 + h
    return m


def afft_pruned(x, L, off, Z, P, keep):
    """M2.afft that forms only what the registers in `keep` (positions behind the last level) depend on; returns the number of real fused
    multiply-adds spent (6 per full butterfly: u 4, v 2)"""
    LG, S = {32: 5, 16: 4}[L], 64 // L
    # needed[lv]: registers whose value in front of level lv is needed; walked from the outputs back
    need_after = set(keep)
    plan = []
    for lv in reversed(range(LG)):
        half = L >> (lv + 1)
        need_before, ops = set(), []
        for b in range(1 << lv):
            for j in range(half):
                ia = off + 2 * half * b + j
                ib = ia + half
                nu, nv = ia in need_after, ib in need_after
                if nu or nv:
                    need_before |= {ia, ib}
                    ops.append((lv, b, ia, ib, nv))  # v = 2 a - u needs u
        plan.append(ops)
        need_after = need_before
    fmas = 0
    for ops in reversed(plan):
        for lv, b, ia, ib, nv in ops:
            half = L >> (lv + 1)
            w = M2.root_mul(P[LG - 1 - lv], half * (S * brev(b, lv) + Z))
            a = x[:, ia].copy()
            u = a + w * x[:, ib]
            x[:, ia] = u
            fmas += 4
            if nv:
                x[:, ib] = 2 * a - u
                fmas += 2
            else:
                x[:, ib] = np.nan
    return fmas


def test_pass3_registers_of_the_zeroed_slots():
    m = pass3_slot_of_register()
    assert sorted(m.values()) == list(range(32))
    dead = {r for r, s in m.items() if s in ZERO}
    # h = 0 (registers 0 .. 15) gives the even slots 8 .. 24: k3 = 4 .. 12; h = 1 the odd slots 7 .. 23: k3 = 3 .. 11
    assert dead == {brev(k3, 4) for k3 in range(4, 13)} | {16 + brev(k3, 4) for k3 in range(3, 12)}
    assert len(dead) == 18
    # slot 25 (zeroed in thread 0 only, as data) and the slots beside the band are kept
    assert m[16 + brev(12, 4)] == 25 and 16 + brev(12, 4) not in dead
    assert {m[r] for r in range(32) if r not in dead} == set(range(0, 7)) | set(range(25, 32))


def test_pruned_pass3_gives_the_kept_outputs_of_the_full_one():
    rng = np.random.default_rng(35)
    x = rng.standard_normal((9, 32)) + 1j * rng.standard_normal((9, 32))
    r = np.exp(-2j * np.pi * 0.0123)
    full = x.copy()
    M2.afft16x2(full, r)
    m = pass3_slot_of_register()
    keep = {reg for reg, s in m.items() if s not in ZERO}
    got = x.copy()
    P = M2.ratio_powers(r)
    fmas = afft_pruned(got, 16, 0, 0, P, {k for k in keep if k < 16}) + afft_pruned(got, 16, 16, 2, P, {k for k in keep if k >= 16})
    for reg in sorted(keep):
        assert np.array_equal(got[:, reg].copy().view(np.float64), full[:, reg].copy().view(np.float64)), reg  # the same operations: the same bits
    # what the pruning saves: of 2 x 32 butterflies x 6 fused multiply-adds
    assert fmas < 2 * 32 * 6
    assert 2 * 32 * 6 - fmas == 30, fmas


# ------------------------------------------------------------------------------------------------------------------ pass 1, second transform
def cfft32_band(x, sb):
    """c6_cfft32_band<SB>: M1.cfft32 with the zero slots followed through the network; returns (renamings, products, full butterflies)"""
    zero = set(range(sb, 32 - sb))
    ren = prod = full = 0
    for lv in range(5):
        half = 16 >> lv
        for b in range(1 << lv):
            idx = half * 2 * brev(b, lv)
            w = M2.W64[idx & 15]
            if idx & 16:
                w = complex(w.imag, -w.real)
            for j in range(half):
                ia = 2 * half * b + j
                ib = ia + half
                za, zb = ia in zero, ib in zero
                a, bb = x[:, ia].copy(), x[:, ib].copy()
                if za and zb:
                    continue
                if zb:
                    x[:, ib] = a
                    zero.discard(ib)
                    ren += 1
                elif za:
                    if idx == 0:
                        u = bb
                        ren += 1
                    elif idx == 16:
                        u = bb.imag - 1j * bb.real
                        ren += 1
                    else:
                        u = w * bb
                        prod += 1
                    x[:, ia], x[:, ib] = u, -u
                    zero.discard(ia)
                elif idx == 0:
                    x[:, ia], x[:, ib] = a + bb, a - bb
                    full += 1
                elif idx == 16:
                    t = bb.imag - 1j * bb.real
                    x[:, ia], x[:, ib] = a + t, a - t
                    full += 1
                else:
                    u = a + w * bb
                    x[:, ia], x[:, ib] = u, 2 * a - u
                    full += 1
    assert not zero
    return ren, prod, full


def test_band_pass1_equals_the_full_pass_on_a_band_limited_input():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((11, 32)) + 1j * rng.standard_normal((11, 32))
    x[:, SB:E - SB] = 0.0
    x[0, E - SB] = 0.0  # thread 0: slot 25 zero as data
    want = x.copy()
    M1.cfft32(want)
    got = x.copy()
    ren, prod, full = cfft32_band(got, SB)
    # equal as numbers everywhere (numpy's complex product is not the kernel's fused one, so bits are the GPU test's matter); an exact zero may
    # differ in sign
    assert np.allclose(got, want, rtol=0, atol=1e-13 * np.max(np.abs(want)))
    assert np.array_equal(got == 0, want == 0)
    # level 0: 14 renamings and two butterflies of zeros; level 1: 4 renamings, 12 full; then 48 full ones
    assert (ren, prod, full) == (18, 0, 60)
    ref = np.fft.fft(x, axis=1)
    for k in range(32):
        assert np.max(np.abs(got[:, brev(k, 5)] - ref[:, k])) < 1e-12 * np.max(np.abs(ref)), k


def test_band_pass1_for_other_slot_aligned_bands():
    """The network is generic in SB: every zero is used up by level 1 or 2, and wide bands need the product form."""
    rng = np.random.default_rng(8)
    for sb in range(1, 16):
        x = rng.standard_normal((3, 32)) + 1j * rng.standard_normal((3, 32))
        x[:, sb:32 - sb] = 0.0
        want = x.copy()
        M1.cfft32(want)
        got = x.copy()
        cfft32_band(got, sb)
        assert np.allclose(got, want, rtol=0, atol=1e-13 * np.max(np.abs(want))), sb


# ------------------------------------------------------------------------------------------------------------------ epilogue constants
def test_slots_without_a_logarithm_and_rows_of_the_fold():
    cfg = CC.CONFIGS["oqpsk_10500"]
    assert cfg.startbin(10500.0) == SB * NT and cfg.epb == EPB and (cfg.N, cfg.NT) == (N, NT)
    # the band-limited signal occupies |k| <= startbin - 1, its square |k| <= 2 startbin - 2
    skip = [s for s in range(E) if ((s >= 2 * SB) if s < E // 2 else (E - 1 - s >= 2 * SB))]
    assert skip == [14, 15, 16, 17]
    for s in range(E):
        ks = np.arange(s * NT, (s + 1) * NT)
        absk = np.minimum(ks, N - ks)
        assert (s in skip) == bool(np.all(absk >= 2 * (SB * NT - 1) + 2)), s
    i0, i1 = cfg.i0i1(10500.0)
    assert (i0, i1) == (N // 2 - SB * NT, N // 2 + SB * NT) and cfg.fold_inside(10500.0)
    lo, hi = i0 - EPB - 1, (i1 - 1) + EPB + 1  # the fold's lowest and highest index
    assert (lo, hi) == (2815, 13568) and (lo // NT, hi // NT) == (5, 26)
    assert (lo // NT, hi // NT) == ((N // 2 - SB * NT - EPB - 1) // NT, (N // 2 + SB * NT + EPB) // NT)  # the kernel's expressions
    # y rows of the slots without a logarithm (the fftshift: row s ^ 16) are not among them
    assert all(not (lo // NT <= (s ^ 16) <= hi // NT) for s in skip)
    assert (i1 - i0 + 4 * NT - 1) // (4 * NT) == 4


# ------------------------------------------------------------------------------------------------------------------ host class
def kernel_class(Fs, fb, lbw):
    """coarse6_body's expressions in double (C's round: halves away from zero)"""
    hz = Fs * (1.0 / N)
    startbin = int(max(CC.c_round(lbw / hz), 1.0))
    epb = CC.c_round(fb / (2.0 * hz))
    i0, i1 = CC.c_round((-lbw / hz) + N / 2), CC.c_round((lbw / hz) + N / 2)
    return int(startbin == SB * NT and epb == EPB and i0 == N // 2 - startbin and i1 == N // 2 + startbin)


def test_host_class_is_the_kernels():
    from jaero_amd import capi

    L = capi.lib()
    cls = lambda power, Fs, fb, lbw: L.jaero_debug_coarse_band_class(power, float(Fs), float(fb), float(lbw))
    hz = 48000.0 / N
    # every whole and half hertz the settings allow (0 < lockingbw <= Fs / 2), the two edges of startbin 3584 and their neighbours in double
    lbws = [k / 2 for k in range(1, 48001)]
    for edge in (3583.5 * hz, 3584.5 * hz, 3584 * hz):
        lbws += [edge, math.nextafter(edge, 0.0), math.nextafter(edge, 1e9)]
    inside = 0
    for lbw in lbws:
        want = kernel_class(48000.0, 10500.0, lbw)
        assert cls(14, 48000.0, 10500.0, lbw) == want, lbw
        inside += want
    assert cls(14, 48000.0, 10500.0, 10500.0) == 1 and inside >= 4
    # startbin 3584 from its lower edge: the fold's i0 rounds another sum (8192 - 3583.5 -> 4609), so that bandwidth is not in the class
    assert kernel_class(48000.0, 10500.0, 3583.5 * hz) == 0 and cls(14, 48000.0, 10500.0, 3583.5 * hz) == 0
    assert cls(14, 48000.0, 10500.0, 9000.0) == 0 and cls(14, 48000.0, 10500.0, 10000.0) == 0
    # the other kernels' banks have no class: 2^13 points, 8400 bps, and MSK rates (another expectedpeakbin)
    assert cls(13, 48000.0, 10500.0, 10500.0) == 0 and cls(14, 48000.0, 8400.0, 10500.0) == 0 and cls(14, 48000.0, 1200.0, 10500.0) == 0
    assert cls(14, 24000.0, 10500.0, 5250.0) == 0
