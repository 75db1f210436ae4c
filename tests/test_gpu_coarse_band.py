"""GPU (-m gpu): the band-aware estimate kernel k_coarse6_b7 (coarse6_body<false, 14, 7, 1792> of jaero_amd/csrc/k_coarse6.h)
against the generic k_coarse6 on the same inputs, bit for bit.

Two banks of the same settings get the same rings, y and state; one has the generic kernel forced (jaero_debug_coarse_force_generic).  Every
comparison is np.array_equal on the raw 64-bit patterns: all 16 384 y values, the ring, the channel's state.  A poked bank refuses the public
readers, so the status rows are compared where the bank is driven by jaero_write (the mixed bank below), with the soft bits.

Five channels on a grid of two: the list is longer than the grid, so a workgroup runs several estimates with the ring prefetch between them
and the last one runs the dummy prefetch.  Ten estimates in a row per case, so that y's history and the prefetch chain are exercised."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import coarse_cases as CC
from test_gpu_coarse import Bank, oracle_estimate, visible_state

pytestmark = pytest.mark.gpu
CFG = CC.CONFIGS["oqpsk_10500"]
N, NT = CFG.N, CFG.NT
LBW = 10500.0
NEST = 10
# ring pointers on the quarter points and off them
PTRS = [0, N // 4, N // 2 + 1, 12345, N - 1]
# y rows of the spectrum slots that take no logarithm (slots 14 .. 17 of X, behind the fftshift rows 30, 31, 0, 1)
SKIP_ROWS = np.r_[0:2 * NT, 30 * NT:32 * NT]


def band_info(bank):
    buf = C.create_string_buffer(64)
    g, b = C.c_longlong(-1), C.c_longlong(-1)
    bank.capi.check(bank.L.jaero_debug_coarse_band(bank.h, buf, 64, C.byref(g), C.byref(b)))
    return buf.value.decode(), g.value, b.value


def tone(k, amp=0.3):
    return amp * np.exp(2j * np.pi * k * np.arange(N) / N)


def cases():
    """{name: [5 x (x in time order, y_in)]}"""
    rng = np.random.default_rng(0xB7)
    zeros, y0 = np.zeros(N, complex), np.zeros(N)
    sig = []
    n = np.arange(N)
    for f0 in (-2000.0, 0.0, 1700.0):  # three carrier offsets
        x = CC.draw(CFG, LBW, rng, signal=True)
        sig.append(x * np.exp(2j * np.pi * f0 * n / CFG.Fs))
    noise = CC.draw(CFG, LBW, rng, signal=False)
    out = {
        "signal_noise_bigchange": [(sig[0], y0), (sig[1], np.full(N, 3.0)), (sig[2], y0), (noise, y0), (zeros, np.full(N, 20.0))],
        # the band's edges and the thread-0 exception: 3583 kept, 3584 .. 12800 zeroed, 12801 kept
        "edge_tones": [(tone(3583), y0), (tone(3584), y0), (tone(12800), y0), (tone(12801), y0), (tone(3583) + tone(12801) + noise, y0)],
        # round-off of the empty part of the squared signal's spectrum above 1: the logarithm runs in slots 14 .. 17
        "scaled_1e7": [(1e7 * sig[0], y0), (1e7 * sig[1], y0), (1e7 * noise, y0), (1e7 * tone(100), y0), (1e7 * sig[2], np.full(N, 3.0))],
    }
    return out


def log_taken(y_in, y_out):
    """True if some y of the slots without a logarithm received a non-zero increment: y_out = y_in * 0.9 + lg, lg = +0.0 without it"""
    return not np.array_equal((y_in[SKIP_ROWS] * 0.9 + 0.0).view(np.uint64), y_out[SKIP_ROWS].view(np.uint64))


def run_case(bank, chans):
    """NEST estimates of every channel; [(ring, y, state) per channel] after each"""
    for ch, (x, y_in) in enumerate(chans):
        ptr = PTRS[ch]
        bank.poke(ch, ring=np.roll(x, ptr), y=y_in, **visible_state(CFG, ptr))
    out = []
    order = [3, 0, 4, 1, 2]
    for _ in range(NEST):
        assert bank.launch(order, 2) == 0, bank.L.jaero_last_error()
        out.append(bank.peek_all())
    return out


def test_band_kernel_equals_generic_bit_for_bit(oracle_mod):
    O = oracle_mod
    all_cases = cases()
    # on the CPU first: which cases leave the slots without a logarithm at +0.0 (the oracle's first estimate)
    expect_log = {}
    for name, chans in all_cases.items():
        expect_log[name] = [log_taken(y_in, oracle_estimate(O, CFG, LBW, x, y_in)[1]) for x, y_in in chans]
    assert all(expect_log["scaled_1e7"]) and not any(expect_log["signal_noise_bigchange"]) and not any(expect_log["edge_tones"]), expect_log
    band, gen = Bank(CFG, [LBW] * 5), Bank(CFG, [LBW] * 5)
    try:
        band.capi.check(gen.L.jaero_debug_coarse_force_generic(gen.h, 1))
        assert band_info(band) == ("k_coarse6_b7", 0, 0) and band_info(gen) == ("k_coarse6_b7", 0, 0)
        seen = {False: 0, True: 0}
        for name, chans in all_cases.items():
            rb, rg = run_case(band, chans), run_case(gen, chans)
            for k in range(NEST):
                for ch in range(5):
                    (r1, y1, s1), (r0, y0, s0) = rb[k][ch], rg[k][ch]
                    what = (name, f"estimate {k}", f"channel {ch}")
                    assert np.array_equal(y1.view(np.uint64), y0.view(np.uint64)), (what, "y", int(np.sum(y1.view(np.uint64) != y0.view(np.uint64))))
                    assert np.array_equal(r1.view(np.uint64), r0.view(np.uint64)), (what, "ring")
                    assert s1.keys() == s0.keys() and all(np.array([s1[f]]).tobytes() == np.array([s0[f]]).tobytes() for f in s0), (what, s1, s0)
            for ch, (x, y_in) in enumerate(chans):
                took = log_taken(y_in, rb[0][ch][1])
                assert took == expect_log[name][ch], (name, ch, "the logarithm of slots 14 .. 17", took)
                seen[took] += 1
            assert all(st["nest"] > 0 for _, _, st in rb[-1])
        assert seen[False] >= 5 and seen[True] >= 5, seen  # both sides of the skip were taken
        nrun = 5 * NEST * len(all_cases)
        assert band_info(band) == ("k_coarse6_b7", 0, nrun) and band_info(gen) == ("k_coarse6_b7", nrun, 0)
    finally:
        band.close()
        gen.close()


def test_banks_without_a_band_kernel():
    from jaero_amd import capi

    for name in ("oqpsk_8400", "msk_1200"):
        cfg = CC.CONFIGS[name]
        b = Bank(cfg, [cfg.lbw0])
        try:
            assert band_info(b) == ("", 0, 0)
            assert b.launch(None, 0) == 0
            assert band_info(b) == ("", 1, 0)
        finally:
            b.close()
    assert capi.lib().jaero_debug_coarse_band(None, None, 0, None, None) == capi.E_INVAL
    assert capi.lib().jaero_debug_coarse_force_generic(None, 1) == capi.E_INVAL


MIXED_LBW = [10500.0, 9000.0, 10000.0, 10500.0, 10500.0, 9000.0, 10000.0, 10500.0]
MOVING = 3


def run_mixed(force_generic):
    """Eight channels through jaero_write, channel MOVING taken from 10500 to 9000 Hz and back between writes.  Returns (per-channel soft bits,
    status rows, final (ring, y, state)), the status rows of MOVING per phase, and the hook's counts."""
    from jaero_amd import capi, signalgen
    from jaero_amd import demodulator as D

    nch, chunk, nchunks = len(MIXED_LBW), 4096, 12
    pcm, _, _ = signalgen.channel_bank("oqpsk", nch, chunk * nchunks, ebno_db=12.0)
    base = D.OqpskSettings()
    setts = [dataclasses.replace(base, lockingbw=b) for b in MIXED_LBW]
    bank = D.DemodulatorBank(setts, ebno=False, status_log=True, max_write_samples=chunk, softbit_capacity=chunk * nchunks)
    L, h = bank.L, bank.h
    try:
        capi.check(L.jaero_debug_coarse_force_generic(h, int(force_generic)))
        logs = [[] for _ in range(nch)]
        phase_rows = [0, 0, 0]
        for k in range(nchunks):
            if k == 4:
                bank.set_settings(dataclasses.replace(base, lockingbw=9000.0), channel=MOVING)
            if k == 8:
                bank.set_settings(dataclasses.replace(base, lockingbw=10500.0), channel=MOVING)
            bank.write(pcm[:, k * chunk:(k + 1) * chunk])
            for ch in range(nch):
                rows = bank.read_status_log(ch)
                logs[ch].append(rows)
                if ch == MOVING:
                    phase_rows[0 if k < 4 else 1 if k < 8 else 2] += len(rows)
        soft = [bank.read_softbits(ch) for ch in range(nch)]
        buf = C.create_string_buffer(64)
        g, b = C.c_longlong(-1), C.c_longlong(-1)
        capi.check(L.jaero_debug_coarse_band(h, buf, 64, C.byref(g), C.byref(b)))
        final = []
        for ch in range(nch):
            ring, y, s = np.empty(N, dtype=np.complex128), np.empty(N), capi.CoarseState()
            capi.check(L.jaero_debug_coarse_peek(h, ch, ring.ctypes.data, y.ctypes.data, C.byref(s)))
            final.append((ring, y, bytes(s)))
        logs = [np.concatenate(rows) for rows in logs]
        return soft, logs, final, phase_rows, (g.value, b.value)
    finally:
        bank.close()


def test_mixed_bank_follows_live_bandwidth_changes():
    assert [CFG.startbin(b) % NT == 0 for b in (10500.0, 9000.0, 10000.0)] == [True, True, False]  # 9000 Hz: aligned, not instantiated
    soft1, logs1, fin1, phases1, (g1, b1) = run_mixed(False)
    soft0, logs0, fin0, phases0, (g0, b0) = run_mixed(True)
    assert phases1 == phases0 and min(phases1) >= 1, phases1  # the moving channel ran estimates in each of its three phases
    for ch in range(len(MIXED_LBW)):
        assert np.array_equal(soft1[ch], soft0[ch]) and len(soft1[ch]) > 0, ch
        assert logs1[ch].shape == logs0[ch].shape and np.array_equal(logs1[ch].view(np.uint64), logs0[ch].view(np.uint64)), ch
        (r1, y1, s1), (r0, y0, s0) = fin1[ch], fin0[ch]
        assert np.array_equal(y1.view(np.uint64), y0.view(np.uint64)) and np.array_equal(r1.view(np.uint64), r0.view(np.uint64)) and s1 == s0, ch
    nest = [len(l) for l in logs1]
    total = sum(nest)
    want_band = sum(nest[ch] for ch, b in enumerate(MIXED_LBW) if b == 10500.0 and ch != MOVING) + phases1[0] + phases1[2]
    assert (g0, b0) == (total, 0)
    assert (g1, b1) == (total - want_band, want_band), (g1, b1, nest, phases1)
