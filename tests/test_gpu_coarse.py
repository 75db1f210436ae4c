"""GPU (-m gpu): the coarse-frequency estimate kernels (k_coarse6, k_coarse6_w8400, k_coarse6_13: coarse6_body of jaero_amd/csrc/k_coarse6.h)
run on their own through jaero_debug_coarse_poke / _launch / _peek, against the oracle's stand-alone estimator (jo_coarse_*) and a
long-double restatement (tests/coarse_cases.py).

Every case gives each channel of the bank its own ring, y and state, and channels that are not in the launch's list must come back bit for
bit.  The peak bin, which no buffer holds, is read through the slot: with emptying = 0, mse > threshold, mc_freq = Fs / 4 and m2_freq far
away, the slot stores m2_freq = mc_freq - (bin - N / 2) * hzperbin / 2, exactly at every rate here (hzperbin / 2 = 375 / 2^k Hz).

test_parity_matrix prints, per configuration, the largest |L - ref| / max|Z| of oracle and kernel in units of 2^-52 (L = 10^(y_out - 0.9 y_in)
against max(|Z|, 1) of the restatement); DESIGN.md section 6 keeps the table of an MI355X run."""
import ctypes as C
import math

import numpy as np
import pytest

import coarse_cases as CC
from test_gpu_parity import compare
from test_gpu_variants import write_sizes

pytestmark = pytest.mark.gpu
LD = np.longdouble
AFC, DCD = 1, 8


class Bank:
    """A continuous bank with one channel per locking bandwidth, driven through the three hooks."""

    def __init__(self, cfg, lbws):
        from jaero_amd import capi
        from jaero_amd import demodulator as D

        self.capi, self.cfg, self.lbws, self.nch = capi, cfg, list(lbws), len(lbws)
        for b in self.lbws:
            CC.check_index_ranges(cfg, b)  # nothing the kernel's own index checks do not cover reaches the GPU
        mk = D.OqpskSettings if cfg.kind == "oqpsk" else D.MskSettings
        fc = 8000.0 if cfg.kind == "oqpsk" else 1000.0
        setts = [mk(freq_center=fc, lockingbw=b, fb=cfg.fb, Fs=cfg.Fs, coarsefreqest_fft_power=cfg.power, signalthreshold=cfg.thr) for b in self.lbws]
        self.bank = D.DemodulatorBank(setts, ebno=False, status_log=True, max_write_samples=4096)
        self.L, self.h = self.bank.L, self.bank.h
        buf = C.create_string_buffer(128)
        capi.check(self.L.jaero_debug_kernel_variant(self.h, 1, buf, 128))
        assert buf.value.decode() == cfg.variant

    def close(self):
        self.bank.close()

    def poke(self, ch, ring=None, y=None, **st):
        s = None
        if st:
            s = self.capi.CoarseState(**st)
        ring = None if ring is None else np.ascontiguousarray(ring, dtype=np.complex128)
        y = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
        assert (ring is None or ring.shape == (self.cfg.N,)) and (y is None or y.shape == (self.cfg.N,))
        self.capi.check(self.L.jaero_debug_coarse_poke(self.h, ch, None if ring is None else ring.ctypes.data, None if y is None else y.ctypes.data,
                                                       None if s is None else C.byref(s)))

    def peek(self, ch):
        ring, y, s = np.empty(self.cfg.N, dtype=np.complex128), np.empty(self.cfg.N), self.capi.CoarseState()
        self.capi.check(self.L.jaero_debug_coarse_peek(self.h, ch, ring.ctypes.data, y.ctypes.data, C.byref(s)))
        return ring, y, {n: getattr(s, n) for n, _ in s._fields_}

    def peek_all(self):
        return [self.peek(ch) for ch in range(self.nch)]

    def launch(self, chans=None, grid=0):
        if chans is None:
            return self.L.jaero_debug_coarse_launch(self.h, None, self.nch, grid)
        a = np.ascontiguousarray(chans, dtype=np.int32)
        return self.L.jaero_debug_coarse_launch(self.h, a.ctypes.data, len(a), grid)


def visible_state(cfg, ptr):
    """Slot state that makes the estimate's bin visible in m2_freq (module docstring); countdowns and the sample counter away from what the
    slot sets them to."""
    return dict(bb_ptr=int(ptr), emptying=0, flags=0, countdown=2, countdown2=3, coarse_cnt=777, mse=cfg.thr + 1.0,
                m2_freq=cfg.Fs / 2 + 100.0, mc_freq=cfg.Fs / 4)


def bin_from_state(cfg, st):
    d = st["m2_freq"] - st["mc_freq"]
    k = CC.c_round(-d / (cfg.hz / 2))
    assert d == -k * (cfg.hz / 2), ("m2_freq - mc_freq is not a whole number of half bins", d)
    return cfg.N // 2 + k


def check_visible_after(cfg, before, after, what):
    """ring and pointer unchanged, I_COARSE_CNT 0, the countdowns as the slot leaves them while unlocked, one estimate and one row more"""
    (r0, _, s0), (r1, _, s1) = before, after
    assert np.array_equal(r0.view(np.float64), r1.view(np.float64)), (what, "ring changed")
    want = dict(s0, coarse_cnt=0, countdown=4, nest=s0["nest"] + 1, log_cnt=s0["log_cnt"] + 1, m2_freq=s1["m2_freq"])
    if cfg.kind == "oqpsk":
        want["countdown2"] = 5
    assert s1 == want, (what, s1, want)


def check_untouched(before, after, chans, what):
    for ch in chans:
        (r0, y0, s0), (r1, y1, s1) = before[ch], after[ch]
        assert np.array_equal(r0.view(np.uint64), r1.view(np.uint64)) and np.array_equal(y0.view(np.uint64), y1.view(np.uint64)) and s0 == s1, \
            (what, f"channel {ch} is not in the list and changed")


def oracle_estimate(O, cfg, lbw, x, y_in):
    """(bin, y_out) of jo_coarse_process on x (time order) from y_in; the construction's emptying countdown is used up on a zero block first"""
    oc = O.Coarse(cfg.power, lbw, cfg.fb, cfg.Fs)
    assert oc.process(np.zeros(cfg.N, dtype=np.complex128)) == 0.0
    oc.set_y(y_in)
    est = oc.process(x)
    return oc.peak_bin(est), oc.get_y()


def y_after_three(O, cfg, lbw, rng):
    oc = O.Coarse(cfg.power, lbw, cfg.fb, cfg.Fs)
    for k in range(3):
        oc.process(CC.draw(cfg, lbw, rng, signal=k != 1))
    return oc.get_y()


def matrix_lists(nch, rng):
    """(name, channel list or None, grid): the null list; one workgroup over every channel in order; permuted strict subsets on two and three
    workgroups, which get 3 + 2, 2 + 1 and (for nch - 1 entries) unequal shares with the last workgroup one short"""
    perm = [int(c) for c in rng.permutation(nch)]
    out = [("all", None, 0), ("all_one_workgroup", None, 1), ("subset5_grid2", perm[:5], 2), ("subset3_grid2", perm[2:5], 2)]
    n = nch - 1 if (nch - 1) % 3 else nch - 2
    out.append((f"subset{n}_grid3", perm[::-1][:n], 3))
    return out


@pytest.mark.parametrize("name", list(CC.CONFIGS))
def test_parity_matrix(oracle_mod, name):
    O, cfg = oracle_mod, CC.CONFIGS[name]
    N = cfg.N
    rng = np.random.default_rng(0xC0A5 + list(CC.CONFIGS).index(name))
    bank = Bank(cfg, cfg.lbws)
    ptrs = cfg.pointers()
    worst_o = worst_k = worst_ratio = 0.0
    ndraws = nrejected = 0
    try:
        for case, (lname, chans, grid) in enumerate(matrix_lists(bank.nch, rng)):
            inputs = []
            for ch, lbw in enumerate(cfg.lbws):
                x = CC.draw(cfg, lbw, rng, signal=(ch + case) % 2 == 0)
                ptr = ptrs[(ch + 3 * case) % len(ptrs)]
                ykind = (ch + case) % 3
                y_in = np.zeros(N) if ykind == 0 else np.full(N, 20.0) if ykind == 1 else y_after_three(O, cfg, lbw, rng)
                bank.poke(ch, ring=np.roll(x, ptr), y=y_in, **visible_state(cfg, ptr))  # ring[(ptr + j) % N] = x[j]
                inputs.append((x, y_in, ptr))
            before = bank.peek_all()
            listed = list(range(bank.nch)) if chans is None else chans
            # the CPU side first: oracle, restatement, and whether this draw binds the peak bin
            cpu = {}
            for ch in listed:
                x, y_in, _ = inputs[ch]
                lbw = cfg.lbws[ch]
                bin_o, y_o = oracle_estimate(O, cfg, lbw, x, y_in)
                L_ref, y_ld = CC.restate(cfg, lbw, x, y_in)
                ok, ratio = CC.margin_ok(cfg, lbw, y_ld, y_o)
                ndraws += 1
                nrejected += not ok
                if ok:
                    assert bin_o == CC.peak_bin(cfg, lbw, y_ld), (name, lname, ch, "oracle and restatement disagree on an accepted draw")
                cpu[ch] = (bin_o, y_o, L_ref, ok, ratio)
            assert bank.launch(chans, grid) == 0, bank.L.jaero_last_error()
            after = bank.peek_all()
            check_untouched(before, after, [c for c in range(bank.nch) if c not in listed], (name, lname))
            for ch in listed:
                what = (name, lname, f"channel {ch} lockingbw {cfg.lbws[ch]:g} ptr {inputs[ch][2]}")
                bin_o, y_o, L_ref, ok, ratio = cpu[ch]
                y_in = inputs[ch][1]
                check_visible_after(cfg, before[ch], after[ch], what)
                if ok:
                    assert bin_from_state(cfg, after[ch][2]) == bin_o, (what, f"peak bin (margin ratio {ratio:.3g})")
                zmax = float(L_ref.max())
                lin = lambda y: np.power(LD(10), np.asarray(y, dtype=LD) - LD(0.9) * np.asarray(y_in, dtype=LD))
                err_o = float(np.max(np.abs(lin(y_o) - L_ref)))
                err_k = float(np.max(np.abs(lin(after[ch][1]) - L_ref)))
                worst_o, worst_k = max(worst_o, err_o / zmax / CC.EPS), max(worst_k, err_k / zmax / CC.EPS)
                worst_ratio = max(worst_ratio, err_k / (err_o + 4 * CC.EPS * zmax))
                assert err_k <= 8 * err_o + 4 * CC.EPS * zmax, (what, f"y: kernel {err_k / zmax / CC.EPS:.1f} eps, oracle {err_o / zmax / CC.EPS:.1f} eps of max|Z| = {zmax:.3g}")
        print(f"\ncoarse parity {name}: {ndraws} estimates, {nrejected} draws without a binding peak; max|L - ref| / max|Z|: oracle {worst_o:.1f} eps, "
              f"kernel {worst_k:.1f} eps; largest kernel / (oracle + 4 eps max|Z|) = {worst_ratio:.2f}")
        assert nrejected * 20 <= ndraws, (name, f"{nrejected} of {ndraws} draws rejected")
    finally:
        bank.close()


@pytest.mark.parametrize("name", list(CC.CONFIGS))
def test_exact_cases_on_a_zero_ring(oracle_mod, name):
    """One channel per case of coarse_cases.exact_cases, all in one launch: y_out == 0.9 * y_in bit for bit, and the bin that the fp64
    restatement of the peak search and the oracle agree on."""
    O, cfg = oracle_mod, CC.CONFIGS[name]
    N = cfg.N
    cases = CC.exact_cases(cfg)
    zero = np.zeros(N, dtype=np.complex128)
    want = []
    for cname, lbw, y_in, built in cases:
        bin_o, y_o = oracle_estimate(O, cfg, lbw, zero, y_in)
        bin_n = CC.peak_bin(cfg, lbw, y_in * 0.9)
        assert np.array_equal(y_o, y_in * 0.9) and bin_o == bin_n and built in (None, bin_n), (name, cname, bin_o, bin_n, built)
        if cname.startswith("const_edge"):
            assert bin_n == cfg.epb + 1 > cfg.i0i1(lbw)[0]  # the first candidate with all six terms: the edge bins before it have fewer
        if cname == "i1_excluded":
            assert CC.folded_at(cfg, y_in * 0.9, bin_n + 1) > CC.folded_at(cfg, y_in * 0.9, bin_n)
        if cname == "i0_first":
            assert CC.folded_at(cfg, y_in * 0.9, bin_n - 1) > CC.folded_at(cfg, y_in * 0.9, bin_n)
        want.append(bin_n)
    bank = Bank(cfg, [c[1] for c in cases])
    try:
        ptrs = cfg.pointers()
        for ch, (cname, lbw, y_in, _) in enumerate(cases):
            bank.poke(ch, ring=zero, y=y_in, **visible_state(cfg, ptrs[ch % len(ptrs)]))
        before = bank.peek_all()
        assert bank.launch(None, 0) == 0, bank.L.jaero_last_error()
        after = bank.peek_all()
        bad = []
        for ch, (cname, lbw, y_in, _) in enumerate(cases):
            check_visible_after(cfg, before[ch], after[ch], (name, cname))
            assert np.array_equal(after[ch][1].view(np.uint64), (y_in * 0.9).view(np.uint64)), (name, cname, "y_out != 0.9 * y_in")
            got = bin_from_state(cfg, after[ch][2])
            if got != want[ch]:
                bad.append((cname, got, want[ch]))
            if cname == "zero":
                assert after[ch][2]["m2_freq"] == after[ch][2]["mc_freq"]  # estimate 0
        assert not bad, (name, "peak bin (case, kernel, expected)", bad)
        # the same cases once more as ONE workgroup's persistent list, in reverse order
        for ch, (cname, lbw, y_in, _) in enumerate(cases):
            bank.poke(ch, ring=zero, y=y_in, **visible_state(cfg, ptrs[(ch + 1) % len(ptrs)]))
        assert bank.launch(list(range(bank.nch))[::-1], 1) == 0, bank.L.jaero_last_error()
        bad = [(c[0], b, w) for c, b, w in zip(cases, (bin_from_state(cfg, bank.peek(ch)[2]) for ch in range(bank.nch)), want) if b != w]
        assert not bad, (name, "peak bin in one persistent workgroup (case, kernel, expected)", bad)
    finally:
        bank.close()


def recentre_expected(cfg, lbw, m2):
    """mixer_center.SetFreq(mixer2.GetFreq()) and the two clamps (oqpskdemodulator.cpp:660-672, mskdemodulator.cpp:505-515)"""
    mc = m2
    if mc < lbw / 2.0:
        mc = lbw / 2.0
    if mc > cfg.Fs / 2.0 - lbw / 2.0:
        mc = cfg.Fs / 2.0 - lbw / 2.0
    return mc


@pytest.mark.parametrize("name", ["oqpsk_10500", "oqpsk_8400", "msk_1200", "msk_1200_12k"])
def test_recentre_inside_a_persistent_list(oracle_mod, name):
    """The AFC recentre (bigchange) fires for the middle channel of a three-entry list that one workgroup runs: its y becomes all 20, its ring
    all zero, emptying 4, mc_freq = m2_freq within [lockingbw / 2, Fs / 2 - lockingbw / 2]; its neighbours -- the one behind it had its ring
    prefetched while the recentre was decided -- give what they give when the middle channel does not recentre."""
    cfg = CC.CONFIGS[name]
    N, lbw = cfg.N, cfg.lbw0
    rng = np.random.default_rng(0xB16 + list(CC.CONFIGS).index(name))
    lo, hi = lbw / 2.0, cfg.Fs / 2.0 - lbw / 2.0
    bank = Bank(cfg, [lbw] * 9)
    try:
        for k, m2 in enumerate([0.5 * (lo + hi) + 40.0, lo - 100.0, hi + 100.0]):  # inside, below the lower clamp, above the upper
            chans = [3 * k + 2, 3 * k + 1, 3 * k]  # run in this order: the middle entry is channel 3 k + 1
            mid = chans[1]
            data = {ch: (CC.draw(cfg, lbw, rng, signal=True), rng.uniform(0.0, 30.0, N), int(rng.integers(0, N))) for ch in chans}
            results = {}
            for recentre in (True, False):
                for ch in chans:
                    x, y_in, ptr = data[ch]
                    st = visible_state(cfg, ptr)
                    if ch == mid:
                        flags = (AFC if cfg.kind == "oqpsk" else AFC | DCD) if recentre else 0
                        st = dict(st, flags=flags, mse=cfg.thr / 2, m2_freq=m2, mc_freq=0.5 * (lo + hi), countdown=0, countdown2=5)
                    bank.poke(ch, ring=np.roll(x, ptr), y=y_in, **st)
                before = bank.peek_all()
                assert bank.launch(chans, 1) == 0, bank.L.jaero_last_error()
                after = bank.peek_all()
                check_untouched(before, after, [c for c in range(9) if c not in chans], (name, k, recentre))
                results[recentre] = (before, after)
            before, after = results[True]
            ring, y, st = after[mid]
            s0 = before[mid][2]
            assert np.array_equal(y, np.full(N, 20.0)) and not ring.any(), (name, k, "bigchange: y = 20 and an empty ring")
            want = dict(s0, emptying=4, countdown=0, coarse_cnt=0, nest=s0["nest"] + 1, log_cnt=s0["log_cnt"] + 1, mc_freq=recentre_expected(cfg, lbw, m2))
            if cfg.kind == "oqpsk":
                want["countdown2"] = 4  # locked and no DCD: the countdown runs, m2_freq stays
            assert st == want, (name, k, st, want)
            assert lo <= st["mc_freq"] <= hi and (st["mc_freq"] == m2) == (k == 0)
            # without the recentre the middle channel is an ordinary locked estimate
            assert results[False][1][mid][2]["emptying"] == 0 and results[False][1][mid][2]["mc_freq"] == 0.5 * (lo + hi)
            for ch in (chans[0], chans[2]):
                (r1, y1, s1), (r2, y2, s2) = results[True][1][ch], results[False][1][ch]
                assert np.array_equal(r1.view(np.uint64), r2.view(np.uint64)) and np.array_equal(y1.view(np.uint64), y2.view(np.uint64)), (name, k, ch)
                assert dict(s1, nest=0, log_cnt=0) == dict(s2, nest=0, log_cnt=0) and s2["nest"] == s1["nest"] + 1, (name, k, ch, s1, s2)
                check_visible_after(cfg, before[ch], after[ch], (name, k, ch))
    finally:
        bank.close()


def test_hook_argument_checks():
    """What the hooks refuse on a live bank (the null context is a CPU case of tests/test_capi_host.py), and that a poked bank takes no more writes."""
    from jaero_amd import capi
    from jaero_amd import demodulator as D

    cfg = CC.CONFIGS["msk_1200"]
    b = Bank(cfg, [1800.0] * 3)
    try:
        L, h = b.L, b.h
        st = capi.CoarseState(**visible_state(cfg, 0))
        assert L.jaero_debug_coarse_launch(h, None, 2, 0) == capi.E_INVAL  # the null list is all channels
        assert b.launch([0, 3]) == capi.E_INVAL and b.launch([0, -1]) == capi.E_INVAL and b.launch([1, 1]) == capi.E_INVAL
        assert b.launch([0, 1], 3) == capi.E_INVAL and b.launch([0, 1], -1) == capi.E_INVAL and b.launch(None, 4) == capi.E_INVAL
        for ch in (-1, 3):
            assert L.jaero_debug_coarse_poke(h, ch, None, None, C.byref(st)) == capi.E_INVAL
            assert L.jaero_debug_coarse_peek(h, ch, None, None, C.byref(st)) == capi.E_INVAL
        for bad in (dict(bb_ptr=cfg.N), dict(bb_ptr=-1), dict(flags=16), dict(m2_freq=-1.0), dict(mc_freq=math.nan), dict(emptying=-1)):
            s = capi.CoarseState(**dict(visible_state(cfg, 0), **bad))
            assert L.jaero_debug_coarse_poke(h, 0, None, None, C.byref(s)) == capi.E_INVAL, bad
        assert b.launch([2, 0], 2) == 0 and b.launch(None, 0) == 0
        pcm = np.zeros((3, 64), dtype=np.int16)
        with pytest.raises(capi.JaeroError) as e:
            b.bank.write(pcm)
        assert e.value.code == capi.E_HIP
    finally:
        b.close()
    burst = D.DemodulatorBank([D.BurstOqpskSettings()], max_write_samples=4096)
    try:
        st = capi.CoarseState()
        assert burst.L.jaero_debug_coarse_launch(burst.h, None, 1, 0) == capi.E_INVAL
        assert burst.L.jaero_debug_coarse_peek(burst.h, 0, None, None, C.byref(st)) == capi.E_INVAL
        assert burst.L.jaero_debug_coarse_poke(burst.h, 0, None, None, C.byref(st)) == capi.E_INVAL
    finally:
        burst.close()


@pytest.mark.parametrize("kind", ["oqpsk", "msk"])
def test_never_locked_stream(oracle_mod, kind):
    """No hook: 64 channels of noise only and of 0 dB Eb/N0 signals through jaero_write in ragged writes, with a signal threshold under which
    they stay unlocked, so that for 30 and more estimates per channel every estimate is the one the status log shows (a locked channel's
    estimates reach no output).  Ring fill, schedule and the y carried on the device, against the oracle's own run."""
    from jaero_amd import demodulator as D

    O = oracle_mod
    sig = CC.stream_signals(kind)
    nch, n = 64, sig.shape[1]
    thr = CC.STREAM_THR[kind]
    if kind == "oqpsk":
        st, ost = D.OqpskSettings(signalthreshold=thr), O.oqpsk_settings(threshold=thr)
    else:
        st, ost = D.MskSettings(fb=1200.0, lockingbw=1800.0, freq_center=1000.0, signalthreshold=thr), O.msk_settings(threshold=thr)
    sizes = write_sizes(n)
    pcm = sig[np.arange(nch) % CC.STREAM_NSIG]
    bank = D.DemodulatorBank([st] * nch, ebno=True, status_log=True, capture_symbols=True, max_write_samples=4096, softbit_capacity=n)
    try:
        s = 0
        for m in sizes:
            bank.write(np.ascontiguousarray(pcm[:, s:s + m]))
            s += m
        refs = {}
        for c in CC.STREAM_CHECK:
            k = c % CC.STREAM_NSIG
            if k not in refs:
                refs[k] = O.run_demod(ost, sig[k], chunk=sizes, capture_symbols=True)
                unlocked = int((refs[k]["status"][:, 5] == 0).sum())
                assert len(refs[k]["status"]) >= 30 and unlocked >= CC.STREAM_MIN_UNLOCKED, (kind, k, "the oracle locks on this stream", unlocked)
            log = bank.read_status_log(c)
            compare(bank.read_softbits(c), bank.read_symbols(c), log, refs[k])
            assert int((log[:, 5] == 0).sum()) >= CC.STREAM_MIN_UNLOCKED, (kind, c)
    finally:
        bank.close()
