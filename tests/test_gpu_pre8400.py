"""GPU (-m gpu): the 8400 bps prefilter kernels (k_pre8400_mix, k_pre8400_commit, k_pre8400_fft, k_pre8400_restart of jaero_amd/csrc/k_pre8400.h)
run on their own through jaero_debug_pre8400_write / _poke / _peek / _restart / _read_ring and jaero_debug_read_prefiltered -- the launch code of
jaero_write and jaero_set_settings, not a copy of it -- against the oracle's stand-alone prefilter (jo_pre8400_*) and an exact long-double sum
(tests/pre8400_cases.py, which states what is asserted and why).

The mix (ring contents, oscillator pointer and step) is compared as bit patterns after every write; the filtered output against the exact sum
with e_kernel <= 4 * e_oracle, against the oracle alone with 5 * the worst e_oracle of the test, and with exact zeros wherever the oracle has
them.  Every test prints its errors in units of 2^-52 of the peak; DESIGN.md section 14 keeps the table of an MI355X run."""
import ctypes as C

import numpy as np
import pytest

import pre8400_cases as PC

pytestmark = pytest.mark.gpu
CHANNEL_MAJOR, FRAME_MAJOR = 0, 1


class PreBank:
    """An 8400 bps bank driven through the prefilter hooks."""

    def __init__(self, nch, max_write=4096, **kw):
        from jaero_amd import capi
        from jaero_amd import demodulator as D

        self.capi, self.nch = capi, nch
        st = D.OqpskSettings(fb=8400.0, lockingbw=8400.0, coarsefreqest_fft_power=14)
        self.bank = D.DemodulatorBank([st] * nch, max_write_samples=max_write, **kw)
        self.L, self.h = self.bank.L, self.bank.h

    def close(self):
        self.bank.close()

    def write(self, blk, layout=CHANNEL_MAJOR, stretches=0):
        blk = np.asarray(blk, dtype=np.int16)
        assert blk.shape[0] == self.nch
        a = np.ascontiguousarray(blk if layout == CHANNEL_MAJOR else blk.T)
        return self.L.jaero_debug_pre8400_write(self.h, a.ctypes.data, layout, blk.shape[1], stretches)

    def peek(self, ch):
        s = self.capi.Pre8400State()
        self.capi.check(self.L.jaero_debug_pre8400_peek(self.h, ch, C.byref(s)))
        return s

    def poke(self, ch, **kw):
        s = self.peek(ch)
        for k, v in kw.items():
            setattr(s, k, v)
        self.capi.check(self.L.jaero_debug_pre8400_poke(self.h, ch, C.byref(s)))

    def restart(self, ch):
        self.capi.check(self.L.jaero_debug_pre8400_restart(self.h, ch))

    def ring(self, ch, first, n):
        out = np.empty(n, dtype=np.complex128)
        self.capi.check(self.L.jaero_debug_pre8400_read_ring(self.h, ch, first, n, out.ctypes.data))
        return out

    def out(self, ch, n):
        out = np.empty(n, dtype=np.complex128)
        self.capi.check(self.L.jaero_debug_read_prefiltered(self.h, ch, out.ctypes.data, n))
        return out


def drive(O, pb, pcm, sizes, chans, layout=CHANNEL_MAJOR, stretches=0, fsums=None, events=None, what=""):
    """The writes through the hook and through one oracle object per checked channel; after every write the mix bit for bit.
    fsums(ch, k, nprev): the sum poked in front of write k > 0 (None: what k_pre8400_commit left, 0); events[k](models): called in front of write
    k.  Returns (models, outputs of the kernel per channel, ring contents per channel)."""
    models = {ch: PC.Model(O) for ch in chans}
    gpu, rings = {ch: [] for ch in chans}, {ch: [] for ch in chans}
    s = 0
    for k, n in enumerate(sizes):
        if events and k in events:
            events[k](models)
        fs = {}
        if k > 0 and fsums is not None:
            for ch in chans:
                fs[ch] = fsums(ch, k, sizes[k - 1])
                pb.poke(ch, fsum=fs[ch])
        assert pb.write(pcm[:, s:s + n], layout, stretches) == 0, pb.L.jaero_last_error()
        for ch in chans:
            w = (what, f"write {k} of {n} at {s}, channel {ch}")
            down, _ = models[ch].write(pcm[ch, s:s + n], fs.get(ch))
            st = pb.peek(ch)
            assert (st.n0, st.nprev) == (s + n, n), w
            r = pb.ring(ch, s, n)
            PC.check_bits(r, down, w + ("down-mixed samples",))
            PC.check_bits(np.array([st.ptr, st.step]), np.array(models[ch].state), w + ("WTptr, WTstep",))
            rings[ch].append(r)
            gpu[ch].append(pb.out(ch, n))
        s += n
    return models, {ch: np.concatenate(v) for ch, v in gpu.items()}, {ch: np.concatenate(v) for ch, v in rings.items()}


def check_outputs(O, name, models, gpu, exact_chans):
    """Section 'what is asserted' of pre8400_cases: the exact sum for exact_chans (at most four), the oracle alone for the rest"""
    assert len(exact_chans) <= PC.MAX_EXACT_CHANNELS
    rows, worst, exact = [], 0.0, {}
    for ch in exact_chans:
        exact[ch] = PC.exact_prefilter(O, models[ch])
        e_o = PC.err_vs_exact(models[ch].all_out(), exact[ch])
        rows.append((f"channel {ch}", PC.err_vs_exact(gpu[ch], exact[ch]), e_o))
        worst = max(worst, e_o)
    PC.report(name, rows)  # every figure before any assertion
    for ch in exact_chans:
        PC.check_filtered(gpu[ch], models[ch].all_out(), exact=exact[ch], what=(name, ch))
    rest = []
    for ch in models:
        if ch not in exact_chans:
            o = models[ch].all_out()
            if not o.any():
                PC.check_zeros(gpu[ch], o, (name, ch))  # an all-zero channel: every output an exact zero
                rest.append((f"channel {ch} (silent)", 0.0, None))
                continue
            rest.append((f"channel {ch}", PC.check_filtered(gpu[ch], o, e_oracle_worst=worst, what=(name, ch))[0], None))
    PC.report(name, rest)


@pytest.mark.parametrize("nch", [1, 5, 67])
@pytest.mark.parametrize("layout", [CHANNEL_MAJOR, FRAME_MAJOR])
def test_mix_bit_for_bit(oracle_mod, nch, layout):
    """Both write-size sequences, every checked channel after every write; the second sequence again with one and with eight stretches forced
    (the single-stretch path for writes of 512 samples and more is otherwise taken from 524 288 channels on).  Every write but the first runs at
    a frequency of its own (poked sum / previous length), so that pointer and step are not the constructor's."""
    O = oracle_mod
    chans = PC.check_channels(nch)
    zc = chans[-1] if nch > 1 else None
    fsums = lambda ch, k, nprev: (7000.0 + 211.7 * ch + 13.3 * k) * nprev
    runs = {}
    for name, sizes, stretches in (("small", PC.SEQ_SMALL, 0), ("large", PC.SEQ_LARGE, 0), ("large_1", PC.SEQ_LARGE, 1), ("large_8", PC.SEQ_LARGE, 8),
                                   ("small_8", PC.SEQ_SMALL, 8)):
        pcm = PC.fullscale_pcm(nch, sum(sizes), 0x3100 + nch, zero_channel=zc)
        pb = PreBank(nch)
        try:
            runs[name] = drive(O, pb, pcm, sizes, chans, layout, stretches, fsums, what=(nch, layout, name))
        finally:
            pb.close()
    for a, b in (("large_1", "large_8"), ("large", "large_8")):
        for ch in chans:
            PC.check_bits(runs[a][2][ch], runs[b][2][ch], (nch, layout, a, b, ch, "ring"))
            PC.check_bits(runs[a][1][ch], runs[b][1][ch], (nch, layout, a, b, ch, "filtered output"))
    if zc is not None:
        assert not runs["large"][1][zc].any() and not runs["large"][2][zc].any()


def test_frequencies(oracle_mod):
    """fsum / nprev of every kind in every channel in turn (0, negative = clamped to 0, 7985.3 Hz, 23 999.9 Hz, an integer table step), the
    previous write never as long as the current one."""
    O = oracle_mod
    sizes = [2047, 2048, 513, 4096, 700, 3100, 512, 1]
    assert all(a != b for a, b in zip(sizes, sizes[1:]))
    pcm = PC.fullscale_pcm(5, sum(sizes), 0x3200)
    fsums = lambda ch, k, nprev: PC.freq_sum(PC.FREQS[(ch + k) % 5], ch, k, nprev)
    pb = PreBank(5)
    try:
        models, gpu, _ = drive(O, pb, pcm, sizes, list(range(5)), fsums=fsums, what="frequencies")
    finally:
        pb.close()
    steps = {round(m.state[1], 6) for m in models.values()}
    assert len(steps) >= 4
    check_outputs(O, "frequencies", models, gpu, [0, 1, 2, 3])


def test_filter_against_the_exact_sum_over_the_ring_wrap(oracle_mod):
    """67 channels, ring 16 384, ragged writes over more than two ring lengths: writes inside one transform block and writes spanning three."""
    O = oracle_mod
    sizes = PC.cycle_sizes(PC.FILTER_CYCLE, 36000)
    pcm = PC.fullscale_pcm(67, sum(sizes), 0x3300)
    fsums = lambda ch, k, nprev: (7985.3 + 0.37 * ch + 0.011 * k) * nprev
    pb = PreBank(67)
    try:
        st = pb.peek(0)
        assert (st.ring, st.cap, st.n0, st.nprev) == (16384, 4096, 0, 0)
        models, gpu, _ = drive(O, pb, pcm, sizes, PC.CHECK67, fsums=fsums, what="ring wrap")
    finally:
        pb.close()
    assert sum(sizes) > 2 * 16384
    check_outputs(O, "ring_wrap", models, gpu, [0, 3, 63, 66])


def test_tightest_ring(oracle_mod):
    """max_write_samples 2048: the ring is exactly max_write + 3 * 2048 = 8192.  2047 samples first, then six writes of 2048 that each start at
    n0 = 2047 (mod 2048), where the first transform block's window reaches 6143 samples back from the write's first sample."""
    O = oracle_mod
    sizes = [2047] + [2048] * 6
    pcm = PC.fullscale_pcm(5, sum(sizes), 0x3400)
    pb = PreBank(5, max_write=2048)
    try:
        assert pb.peek(0).ring == 8192
        models, gpu, _ = drive(O, pb, pcm, sizes, list(range(5)), fsums=lambda ch, k, nprev: (8000.0 - 3.1 * ch) * nprev, what="tightest ring")
    finally:
        pb.close()
    check_outputs(O, "tightest_ring", models, gpu, [0, 1, 2, 4])


def test_exact_zeros_and_channel_isolation(oracle_mod):
    """The first 2048 outputs of every channel are exact zeros; channel 5 of the group 4 .. 7 carries 8192 samples of digital silence (and channel
    2 nothing else) between three full-scale neighbours: exact zeros wherever the oracle has them -- the outputs behind two silent transform
    blocks --, and the neighbours as if nothing were beside them.  The writes (4096, 700, 3100) do not end on the block grid.

    The silence covers whole blocks (samples 4096 .. 12 287).  With 5000 .. 11 999 the rule cannot be met by anything but the oracle itself:
    at samples 9096 .. 10 239 and 12 288 .. 14 047 the exact output is 0 (no tap reaches a non-zero sample) while a block that is not all
    silence contributes, so both transforms deliver round-off of 4e-16 and less, and the oracle's happens to be 0.0 in both parts at 24 of
    those 2904 samples; an MI355X run had round-off at 23 of them (-8.2e-17 - 8.0e-17j at sample 9238).  tests/test_pre8400_cases.py shows
    the oracle's side of it."""
    O = oracle_mod
    sizes = PC.cycle_sizes([4096, 700, 3100], 22000)
    pcm = PC.fullscale_pcm(8, sum(sizes), 0x3500, zero_channel=2)
    pcm[5, 4096:12288] = 0
    pb = PreBank(8)
    try:
        models, gpu, _ = drive(O, pb, pcm, sizes, list(range(8)), what="zeros")
    finally:
        pb.close()
    for ch in range(8):
        assert not gpu[ch][:PC.L].any(), ch
    o5 = models[5].all_out()
    assert not o5[8192:14336].any() and o5[8191] != 0 and o5[14336] != 0  # input blocks 2 .. 5 are all silence
    assert not gpu[5][8192:14336].any() and gpu[5][8191] != 0 and gpu[5][14336] != 0 and not gpu[2].any()
    check_outputs(O, "zeros", models, gpu, [4, 5, 6, 7])


def test_restart(oracle_mod):
    """k_pre8400_restart on channels 1 and 66 of 67 at moments that are no multiples of 2048, channel 66 twice within 2048 samples: exact zeros for
    exactly 2048 samples, the ring columns of the neighbours bit-identical across the restart kernel, and the restarted channels on the oracle
    object's restart from there on.  Full-scale input throughout: under silence a one-channel restart leaves round-off where the reference,
    whose block grid restarts with the filter, has zeros (k_pre8400.h)."""
    O = oracle_mod
    sizes = [3000, 1111, 700, 3100, 4096, 2048, 2500]
    pcm = PC.fullscale_pcm(67, sum(sizes), 0x3600)
    chans = [0, 1, 2, 3, 64, 65, 66]
    pb = PreBank(67)

    def restart(chs):
        def go(models):
            n0 = pb.peek(0).n0
            first, n = max(0, n0 - 16384), min(n0, 16384)
            before = {c: pb.ring(c, first, n) for c in (0, 2, 3, 64, 65)}
            for ch in chs:
                pb.restart(ch)
                models[ch].restart()
                assert pb.peek(ch).hold == n0 + PC.L and not pb.ring(ch, first, n).any()
            for c, b in before.items():
                PC.check_bits(pb.ring(c, first, n), b, ("restart", chs, "ring column of channel", c))
                assert pb.peek(c).hold == 0
        return go

    try:
        models, gpu, _ = drive(O, pb, pcm, sizes, chans, fsums=lambda ch, k, nprev: (7990.0 + ch) * nprev,
                               events={1: restart([1]), 2: restart([66]), 3: restart([66]), 5: restart([1, 66])}, what="restart")
    finally:
        pb.close()
    assert models[66].restarts == [4111, 4811, 12007] and models[1].restarts == [3000, 12007] and all(r % PC.L for r in models[66].restarts)
    for ch in (1, 66):
        for r in models[ch].restarts:
            assert not gpu[ch][r:r + PC.L].any(), (ch, r)
            if not any(r < q <= r + PC.L for q in models[ch].restarts):
                assert gpu[ch][r + PC.L] != 0, (ch, r)
            if r - 1 >= PC.L and not any(q <= r - 1 < q + PC.L for q in models[ch].restarts):
                assert gpu[ch][r - 1] != 0, (ch, r)
    check_outputs(O, "restart", models, gpu, [1, 66, 0, 65])


def test_through_jaero_write(oracle_mod):
    """No write hook: a real 8400 bps signal on five channels through ordinary writes.  After every write the step the prefilter's oscillator
    ran at (peek) is the frequency the oracle's mixer_fir_pre had during the same write -- k_oqpsk_fb's S_PRE_FSUM over the write before and the
    division by its length -- to the 1e-6 Hz tests/test_gpu_parity.py::compare allows the status rows, and the prefiltered samples follow the
    captured cval_prefiltered."""
    from jaero_amd import signalgen as G

    O = oracle_mod
    nch, nsamp = 5, 30000
    pcm, _, _ = G.channel_bank("oqpsk", nch, nsamp, ebno_db=11.0, seed0=G.SEED_BASE + 8431, fb=8400.0)
    sizes = PC.cycle_sizes(PC.FILTER_CYCLE, nsamp)
    sizes[-1] -= sum(sizes) - nsamp
    refs = [O.run_demod(O.oqpsk_settings(fb=8400.0, lockingbw=8400.0), pcm[c], chunk=sizes, capture_prefiltered=True) for c in range(nch)]
    pb = PreBank(nch, softbit_capacity=nsamp)
    got = {c: [] for c in range(nch)}
    worst_hz = 0.0
    try:
        s = 0
        for k, n in enumerate(sizes):
            pb.bank.write(np.ascontiguousarray(pcm[:, s:s + n]))
            for c in range(nch):
                st = pb.peek(c)
                assert (st.n0, st.nprev) == (s + n, n)
                want = 8000.0 if k == 0 else refs[c]["pre_freq"][k - 1]
                d = abs(st.step * 48000.0 / PC.WT - want)
                worst_hz = max(worst_hz, d)
                assert d <= 1e-6, (k, c, st.step * 48000.0 / PC.WT, want)
                assert abs(st.fsum / n - refs[c]["pre_freq"][k]) <= 1e-6, (k, c, "the sum over this write")
                got[c].append(pb.out(c, n))
            s += n
        pb.bank.write(np.zeros((nch, 8), dtype=np.int16))  # peek and the readers left the bank usable
    finally:
        pb.close()
    print(f"\npre8400 through_jaero_write: largest |step * 48000 / 19999 - mixer_fir_pre frequency| = {worst_hz:.3g} Hz")
    assert np.ptp(np.concatenate([r["pre_freq"] for r in refs])) > 1.0
    # the exact sum needs the oracle's down-mixed samples: the stand-alone object fed the demodulator's sums gives them (and the same output bit
    # for bit, tests/test_pre8400_cases.py)
    models = {}
    for c in range(nch):
        m, s = PC.Model(O), 0
        for k, n in enumerate(sizes):
            m.write(pcm[c, s:s + n], None if k == 0 else refs[c]["pre_freq_sum"][k - 1])
            s += n
        PC.check_bits(m.all_out(), refs[c]["prefiltered"], ("stand-alone object against the demodulator's capture", c))
        models[c] = m
    check_outputs(O, "through_jaero_write", models, {c: np.concatenate(v) for c, v in got.items()}, [0, 1, 2, 3])


def test_hook_argument_checks():
    """What the hooks refuse on the host before any launch, and that write / poke / restart leave a bank that takes no more writes while peek
    and the two readers do not."""
    from jaero_amd import capi
    from jaero_amd import demodulator as D

    E = capi.E_INVAL
    pb = PreBank(5, max_write=2048)
    try:
        L, h = pb.L, pb.h
        st, buf = capi.Pre8400State(), np.zeros(8192, dtype=np.complex128)
        pcm = PC.fullscale_pcm(5, 2048, 1)
        pb.bank.write(pcm[:, :100])
        capi.check(L.jaero_debug_pre8400_peek(h, 4, C.byref(st)))
        assert (st.n0, st.nprev, st.ring, st.cap, st.hold) == (100, 100, 8192, 2048, 0)
        capi.check(L.jaero_debug_pre8400_read_ring(h, 0, 0, 100, buf.ctypes.data))
        capi.check(L.jaero_debug_read_prefiltered(h, 0, buf.ctypes.data, 100))
        pb.bank.write(pcm[:, :50])  # none of the three poisoned the bank
        for ch in (-1, 5):
            assert L.jaero_debug_pre8400_peek(h, ch, C.byref(st)) == E and L.jaero_debug_pre8400_poke(h, ch, C.byref(st)) == E
            assert L.jaero_debug_pre8400_restart(h, ch) == E and L.jaero_debug_pre8400_read_ring(h, ch, 0, 10, buf.ctypes.data) == E
        for first, n in ((0, 0), (0, -1), (-1, 10), (141, 10), (150, 1), (0, 151)):
            assert L.jaero_debug_pre8400_read_ring(h, 0, first, n, buf.ctypes.data) == E, (first, n)
        for n in (0, -1, 2049):
            assert L.jaero_debug_pre8400_write(h, pcm.ctypes.data, 0, n, 0) == E, n
        for stretches in (-1, 2, 7, 9, 64):
            assert L.jaero_debug_pre8400_write(h, pcm.ctypes.data, 0, 64, stretches) == E, stretches
        assert L.jaero_debug_pre8400_write(h, pcm.ctypes.data, 2, 64, 0) == E and L.jaero_debug_pre8400_write(h, None, 0, 64, 0) == E
        for bad in (dict(ptr=-1.0), dict(ptr=19999.0), dict(step=-1.0), dict(step=19999.0), dict(fsum=float("nan")), dict(fsum=float("inf")), dict(hold=-1)):
            s = capi.Pre8400State(ptr=1.0, step=2.0, fsum=3.0, hold=0)
            for k, v in bad.items():
                setattr(s, k, v)
            assert L.jaero_debug_pre8400_poke(h, 0, C.byref(s)) == E, bad
        assert L.jaero_debug_pre8400_poke(h, 0, None) == E and L.jaero_debug_pre8400_peek(h, 0, None) == E
        pb.bank.write(pcm[:, :50])  # and no refusal poisoned it either
        # five writes of 2048: the window must lie inside the last 8192 of the 10 440 samples
        for k in range(5):
            assert pb.write(pcm) == 0
        n0 = 200 + 5 * 2048
        assert L.jaero_debug_pre8400_read_ring(h, 0, n0 - 8193, 10, buf.ctypes.data) == E
        assert L.jaero_debug_pre8400_read_ring(h, 0, n0 - 8192, 8192, buf.ctypes.data) == 0
        assert L.jaero_debug_pre8400_read_ring(h, 0, n0 - 8192, 8193, buf.ctypes.data) == E
        with pytest.raises(capi.JaeroError) as e:
            pb.bank.write(pcm[:, :64])
        assert e.value.code == capi.E_HIP
    finally:
        pb.close()
    for poisoner in ("poke", "restart"):
        pb = PreBank(2)
        try:
            pb.poke(1, fsum=1.0) if poisoner == "poke" else pb.restart(1)
            with pytest.raises(capi.JaeroError) as e:
                pb.bank.write(np.zeros((2, 64), dtype=np.int16))
            assert e.value.code == capi.E_HIP
        finally:
            pb.close()
    pcm = np.zeros((1, 64), dtype=np.int16)
    buf = np.zeros(64, dtype=np.complex128)
    for bank in (D.DemodulatorBank([D.OqpskSettings()], max_write_samples=4096), D.DemodulatorBank([D.MskSettings()], max_write_samples=4096),
                 D.DemodulatorBank([D.BurstOqpskSettings()], max_write_samples=4096)):
        try:
            L, h, st = bank.L, bank.h, capi.Pre8400State(ptr=1.0, step=2.0)
            assert L.jaero_debug_pre8400_write(h, pcm.ctypes.data, 0, 64, 0) == E and L.jaero_debug_pre8400_poke(h, 0, C.byref(st)) == E
            assert L.jaero_debug_pre8400_peek(h, 0, C.byref(st)) == E and L.jaero_debug_pre8400_restart(h, 0) == E
            assert L.jaero_debug_pre8400_read_ring(h, 0, 0, 1, buf.ctypes.data) == E
            bank.write(pcm)  # refused before anything was marked
        finally:
            bank.close()
    assert capi.lib().jaero_debug_pre8400_peek(None, 0, C.byref(capi.Pre8400State())) == E
