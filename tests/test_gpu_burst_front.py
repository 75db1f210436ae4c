"""GPU (-m gpu): the burst banks' per-sample detector k_burst_front<false / true> with k_ev_compact behind it (jaero_amd/csrc/k_burst_front.h) on
its own, through jaero_debug_burst_front / _front_peek / _front_events / _front_poke / _poke_bt and jaero_debug_ev_compact: the launch lines of
jaero_write, not copies of them.  Against jo_peakdet_run, jo_burst_front_write and the long-double jo_burst_front_exact;
tests/burst_front_cases.py states what is asserted and why.  Every test prints its errors in units of 2^-52; DESIGN.md section 10 keeps the
table of an MI355X run."""
import ctypes as C

import numpy as np
import pytest

import burst_acq_cases as BC
import burst_front_cases as FC

pytestmark = pytest.mark.gpu
CHANNEL_MAJOR, FRAME_MAJOR = 0, 1


class FrontBank:
    """A burst bank driven through the front-end hooks."""

    def __init__(self, name, nch, max_write=4096, trace=False):
        from jaero_amd import capi
        from jaero_amd import demodulator as D

        self.capi, self.nch, self.cfg, self.D = capi, nch, FC.CONFIGS[name], D
        self.settings = D.BurstOqpskSettings() if self.cfg.oq else D.BurstMskSettings(fb=self.cfg.fb)
        self.bank = D.DemodulatorBank([self.settings] * nch, max_write_samples=max_write, trace=trace)
        self.L, self.h = self.bank.L, self.bank.h
        self.fg = capi.BurstFrontGeom()
        capi.check(self.L.jaero_debug_burst_front_geom(self.h, C.byref(self.fg)))
        g = FC.geometry(self.cfg)
        assert {k: getattr(self.fg, k) for k in ("PL", "bt_len", "bt_lag", "agc_len", "ma1_len", "mav1_len", "fa_len", "fa_lag", "pd_thr")} == \
            {k: getattr(g, k) for k in ("PL", "bt_len", "bt_lag", "agc_len", "ma1_len", "mav1_len", "fa_len", "fa_lag", "pd_thr")}
        assert self.fg.ngroups == (nch + 63) // 64 and self.fg.ev_cap == (4096 if trace else 256)
        self.g = g

    def close(self):
        self.bank.close()

    def nsamples(self):
        bg = self.capi.BurstGeom()
        self.capi.check(self.L.jaero_debug_burst_geom(self.h, C.byref(bg)))
        return bg.nsamples

    def front_rc(self, pcm, im, layout=CHANNEL_MAJOR):
        pcm = np.asarray(pcm, dtype=np.int16)
        a = np.ascontiguousarray(pcm if layout == CHANNEL_MAJOR else pcm.T)
        imc = None if im is None else np.ascontiguousarray(im, dtype=np.float64)
        evp, evl, cnt = np.full(self.nch, -7, dtype=np.int32), np.full(self.nch, -7, dtype=np.int32), C.c_int(-7)
        rc = self.L.jaero_debug_burst_front(self.h, a.ctypes.data, layout, pcm.shape[1], None if imc is None else imc.ctypes.data, evp.ctypes.data, evl.ctypes.data, C.byref(cnt))
        return rc, evp, evl, cnt.value

    def front(self, pcm, im, layout=CHANNEL_MAJOR):
        rc, evp, evl, cnt = self.front_rc(pcm, im, layout)
        self.capi.check(rc)
        assert np.all(evl[cnt:] == -7)
        return evp, evl, cnt

    def peek(self, ch, ring=None, first=0, n=0):
        st = self.capi.BurstFrontState()
        out = np.full(max(n, 1), np.nan)
        self.capi.check(self.L.jaero_debug_burst_front_peek(self.h, ch, C.byref(st), -1 if ring is None else self.capi.FRONT_RINGS[ring], first, n, out.ctypes.data))
        return st, out[:n]

    def events(self, ch):
        rows, n = np.zeros((4096, 3)), C.c_int(0)
        self.capi.check(self.L.jaero_debug_burst_front_events(self.h, ch, rows.ctypes.data, 4096, C.byref(n)))
        return rows[:n.value]

    def poke(self, ch, field, value):
        self.capi.check(self.L.jaero_debug_burst_front_poke(self.h, ch, field, float(value)))

    def poke_bt(self, ch, first, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        self.capi.check(self.L.jaero_debug_burst_poke_bt(self.h, ch, first, len(v), v.ctypes.data))

    def poke_case(self, ch, c):
        capi = self.capi
        self.poke_bt(ch, self.nsamples() - self.g.bt_len, c.hist)
        for f, v in ((capi.FRONT_CNTDOWN, c.cntdown), (capi.FRONT_LASTDY, c.lastdy), (capi.FRONT_MAXPOSCD, c.maxposcd), (capi.FRONT_TRI_PTR, c.tri_ptr)):
            if v is not None:
                self.poke(ch, f, v)


@pytest.mark.parametrize("name", list(FC.CONFIGS))
def test_peak_detector_on_poked_state(oracle_mod, name):
    """Part A: every scenario of burst_front_cases.scenarios on all-zero input -- event positions, the event list, the scalars of the observed and
    the poked channels behind every segment and the PEAK rows of the event log equal to jo_peakdet_run's, and the ring's new entries exactly 0."""
    for sc in FC.scenarios(name):
        exp = FC.expected(oracle_mod, sc)
        b = FrontBank(name, sc.nch, trace=True)
        try:
            watch = sorted(set(FC.chans(sc.nch)) | {ch for pokes, _ in sc.phases for ch in pokes})
            fires = {ch: [] for ch in watch}
            for (pokes, segs), phase in zip(sc.phases, exp):
                for ch, c in pokes.items():
                    b.poke_case(ch, c)
                for n, e in zip(segs, phase):
                    assert b.nsamples() == e.n0
                    z16, zim = np.zeros((sc.nch, n), dtype=np.int16), np.zeros((sc.nch, n))
                    evp, evl, cnt = b.front(z16, zim, FRAME_MAJOR if n % 2 else CHANNEL_MAJOR)
                    got = {ch: b.peek(ch)[0] for ch in watch}
                    FC.check_scenario_step(sc, e, got, evp, evl, cnt)
                    for ch in watch:
                        fires[ch] += e.fires[ch if ch in e.fires else -1]
                m = min(n, b.g.bt_len)
                for ch in watch:
                    assert not b.peek(ch, "bt", b.nsamples() - m, m)[1].any(), (name, sc.label, ch, "bt_sig of all-zero input must be exactly 0")
            for ch in watch:
                ev = b.events(ch)
                assert [int(s) for s, k, _ in ev if k == b.capi.EV_PEAK] == fires[ch], (name, sc.label, ch, "PEAK rows", ev, fires[ch])
        finally:
            b.close()
    print(f"burst_front {name}: {len(FC.scenarios(name))} scenarios equal to jo_peakdet_run")


def collect(b, sc, chs, segs, pcm, im, start=0, on_segment=None):
    """Feed the segments through the front hook; behind each, peek the last min(n, len) entries of every ring and the sums of the channels chs.
    Returns (series {ch: {column: [n] with NaN where never visible}}, per-segment (ev_pos, ev_list), states {ch: [state behind each segment]})."""
    total = sum(segs)
    cols = [FC.RING_COL[r] for r in FC.RINGS] + list(FC.SUMS)
    series = {ch: {c: np.full(total, np.nan) for c in cols} for ch in chs}
    evs, states, s = [], {ch: [] for ch in chs}, 0
    for k, n in enumerate(segs):
        evp, evl, cnt = b.front(pcm[:, s:s + n], None if im is None else im[:, s:s + n], FRAME_MAJOR if k % 2 else CHANNEL_MAJOR)
        evs.append((evp.copy(), list(evl[:cnt])))
        s += n
        for ch in chs:
            for r in FC.RINGS:
                m = min(n, FC.ring_len(b.g, r))
                st, v = b.peek(ch, r, start + s - m, m)
                series[ch][FC.RING_COL[r]][s - m:s] = v
            states[ch].append(st)
            for c in FC.SUMS:
                series[ch][c][s - 1] = getattr(st, c)
        if on_segment:
            on_segment(k, s)
    return series, evs, states


def report(name, what, E, worst):
    for c, ek in worst.items():
        bound = 4 * E[c] + 4 * FC.EPS
        print(f"burst_front {name} {what} {c}: kernel {ek / FC.EPS:.2f} eps, oracle {E[c] / FC.EPS:.2f} eps, kernel / bound {ek / bound:.3f}, oracle / bound {E[c] / bound:.3f}")


@pytest.mark.parametrize("name,draw,nch", [(n, d, (70, 67)[d]) for n in FC.CONFIGS for d in range(FC.NDRAWS)])
def test_values_streaming(oracle_mod, name, draw, nch):
    """Part B: one accepted draw of agc_len + 2 ma1_len samples from a fresh bank in segments of 1, 7, 1000, maxseg - 1, maxseg; every ring's
    entries and the running sums of the five observed channels behind every segment against the exact run at 4 E_o + 4 eps, the real-only channel
    against the oracle's bits; BI_EV_POS and the event list of every channel, tri_ptr behind every segment, the PEAK rows and the final cntdown /
    maxposcd equal to the oracle's.  (Burst MSK 600 needs 72 000 samples; nothing is shortened.)"""
    O = oracle_mod
    draws, E, _ = FC.population(O, name)
    sc = draws[draw] if nch == 70 else FC.run_oracle(O, FC.stream_case(name, nch, draws[draw].seed))
    b = FrontBank(name, nch, trace=True)
    try:
        series, evs, states = collect(b, sc, sc.obs, sc.segs, sc.pcm, sc.im)
        worst = {}
        for ch in sc.obs:
            for c, e in FC.check_stream(sc, E, ch, series[ch]).items():
                worst[c] = max(worst.get(c, 0.0), e)
        report(name, f"draw {draw}", E, worst)
        fire = {ch: sc.rows[ch][:, sc.cols["fire"]] for ch in sc.obs}
        filled = {ch: sc.rows[ch][:, sc.cols["filled"]] for ch in sc.obs}
        tri = {ch: FC.tri_ptr_series(sc.g, fire[ch]) for ch in sc.obs}
        s = 0
        for k, n in enumerate(sc.segs):
            want = np.array([int(np.flatnonzero(f)[0]) if f.any() else -1 for f in (filled[sc.obs[sc.kind[ch]]][s:s + n] for ch in range(nch))])
            assert np.array_equal(evs[k][0], want) and evs[k][1] == [int(c) for c in np.flatnonzero(want >= 0)], (name, draw, f"segment {k} from sample {s}", evs[k], want)
            s += n
            for ch in sc.obs:
                assert states[ch][k].tri_ptr == tri[ch][s - 1], (name, draw, ch, f"tri_ptr behind sample {s - 1}", states[ch][k].tri_ptr, tri[ch][s - 1])
        for ch in sc.obs:
            ev = b.events(ch)
            assert [int(x) for x, kd, _ in ev if kd == b.capi.EV_PEAK] == [int(i) for i in np.flatnonzero(fire[ch])], (name, draw, ch, "PEAK rows")
            st = states[ch][-1]
            assert (st.cntdown, st.maxposcd) == (sc.final[ch]["cntdown"], sc.final[ch]["maxposcd"]), (name, draw, ch)
    finally:
        b.close()


def pipeline_reference(O, cfg, pcm_ch, n_exact):
    """One channel through the oracle's Hilbert filter and front end, and the exact pipeline: the long-double Hilbert sum rounded to double into the
    long-double front end.  Returns (oracle rows, exact rows, oracle z, exact z)."""
    zo = O.hilbert_stream(pcm_ch, chunk=len(pcm_ch))[0]
    ze = zo.copy()
    ze.real[:] = -0.0
    ze.real[FC.HIL_SHIFT:] = -(pcm_ch[:len(pcm_ch) - FC.HIL_SHIFT].astype(np.float64) / 32768.0)  # the delayed copy itself, without the oracle's transform
    ze.imag[:n_exact] = BC.exact_hilbert(O, pcm_ch[:n_exact]).astype(np.float64)
    d = O.BurstDemod(FC.oracle_settings(O, cfg))
    return d.front_write(zo), d.front_exact(ze)[0], zo, ze


@pytest.mark.parametrize("name,nch", [("oqpsk", 67), ("msk1200", 70), ("msk600", 67)])
def test_hilbert_in_the_loop(oracle_mod, name, nch):
    """im = NULL: k_hilbert_fft feeds the detector as in jaero_write.  Against the exact pipeline (long-double Hilbert sum into the long-double
    front end); E_o = the oracle's pipeline (hilbert_stream into jo_burst_front_write) against it on the same channels.  The kernel must stay
    within 8 E_o + 4 eps: test_hilbert grants k_hilbert_fft 8 times the oracle's error at the transform's output (4 for another factorisation, 2 for
    the partner channel riding in the imaginary part), the detector behind it adds errors of the oracle's own size (part B), and both pipelines
    amplify what enters them alike.  k_hilbert_fft's error scales with the peak of the channel PAIR that shares a transform (burst_acq_cases), so
    every observed channel's partner carries a signal of the channel's own level: then the pair's peak is the scale the errors are measured in.  A
    him layout that differed from the kernel's would miss by the signal's size, not by eps."""
    O = oracle_mod
    cfg = FC.CONFIGS[name]
    g = FC.geometry(cfg)
    segs = [1000, g.maxseg - 1, g.maxseg, 7, 1]
    while sum(segs) < FC.HIL_SHIFT + 3500:
        segs.append(g.maxseg)
    n = sum(segs)
    assert FC.HIL_SHIFT + 3000 < n <= BC.MAX_EXACT_SAMPLES
    rng = np.random.default_rng(0x41B + nch)
    t = np.arange(n)
    obs = FC.chans(nch)
    pcm = np.rint(200.0 * rng.standard_normal((nch, n))).astype(np.int16)
    for k, ch in enumerate(obs):  # the two channels of a pair at one level (0 and 1 are a pair)
        for j, c in enumerate((ch, ch ^ 1)):
            if c < nch and not (j and c in obs):
                a = (20000.0, 20000.0, 300.0, 9000.0, 15000.0)[k]
                pcm[c] = np.rint(0.01 * a * rng.standard_normal(n) + a * np.cos(2 * np.pi * (0.05 + 0.03 * k + 0.011 * j) * t + k) * (t > 1500 * k)).astype(np.int16)
    sc = type("S", (), {})()
    sc.cfg, sc.g, sc.seed, sc.nch, sc.rows, sc.exact = cfg, g, 0, nch, {}, {}
    sc.cols = {c: i for i, c in enumerate(O.BurstDemod.FRONT_COLS)}
    for ch in obs:
        sc.rows[ch], sc.exact[ch], _, _ = pipeline_reference(O, cfg, pcm[ch], n)
    sc.z = {ch: None for ch in obs}
    E = FC.oracle_errors(sc)
    b = FrontBank(name, nch)
    try:
        series, _, _ = collect(b, sc, obs, segs, pcm, None)
        worst = {}
        for ch in obs:
            for c, v in series[ch].items():
                ex = sc.exact[ch][:, sc.cols[c]]
                seen, scale = ~np.isnan(v), float(np.abs(ex).max())
                e = float(np.abs(v[seen].astype(BC.LD) - ex[seen]).max()) / scale if scale else float(np.abs(v[seen]).max())
                worst[c] = max(worst.get(c, 0.0), e)
        for c, e in worst.items():
            bound = 8 * E[c] + 4 * FC.EPS
            print(f"burst_front {name} hilbert in the loop {c}: kernel {e / FC.EPS:.2f} eps, oracle {E[c] / FC.EPS:.2f} eps, kernel / bound {e / bound:.3f}")
        for c, e in worst.items():
            assert e <= 8 * E[c] + 4 * FC.EPS, (name, c, f"kernel {e / FC.EPS:.2f} eps, oracle {E[c] / FC.EPS:.2f} eps")
    finally:
        b.close()


def test_ev_compact_alone():
    """Part D: k_ev_compact on 1 .. 3000 groups (more than 1024: a thread takes a run of groups), against numpy's ascending enumeration of the set
    bits and their count; every entry behind the count keeps the sentinel."""
    from jaero_amd import capi

    L = capi.lib()
    rng = np.random.default_rng(0xE7C)
    for ng in FC.EV_NGROUPS:
        for label, m in FC.ev_masks(ng, rng):
            out, cnt = np.zeros(ng * 64, dtype=np.int32), C.c_int(0)
            capi.check(L.jaero_debug_ev_compact(0, m.ctypes.data, ng, out.ctypes.data, C.byref(cnt)))
            want = FC.ev_expected(m)
            assert cnt.value == len(want) and np.array_equal(out[:len(want)], want), (ng, label, cnt.value, len(want))
            assert np.all(out[len(want):].view(np.uint32) == 0xA5A5A5A5), (ng, label, "entries behind the count")
    for masks, ng in ((None, 1), (np.zeros(1, dtype=np.uint64), 0), (np.zeros(1, dtype=np.uint64), 65537)):
        out, cnt = np.zeros(64, dtype=np.int32), C.c_int(0)
        assert L.jaero_debug_ev_compact(0, None if masks is None else masks.ctypes.data, ng, out.ctypes.data, C.byref(cnt)) == capi.E_INVAL


def _errors(series, exact, cols, lo=0):
    out = {}
    for c, v in series.items():
        ex = exact[:, cols[c]]
        seen = ~np.isnan(v)
        seen[:lo] = False
        scale = float(np.abs(ex[lo:]).max())
        out[c] = (float(np.abs(v[seen].astype(BC.LD) - ex[seen]).max()) / scale if scale else float(np.abs(v[seen]).max())) if seen.any() else 0.0
    return out


@pytest.mark.parametrize("name", list(FC.CONFIGS))
def test_hold_behind_a_live_set_settings(oracle_mod, name):
    """Part C: k_burst_front<true> with lanes of one wavefront holding different counts.  Real jaero_write up to T - 3, the real jaero_set_settings on
    the pairs (62, 63) and (68, 69), a real write of 3 samples, jaero_set_settings on channels 1, 5 and 33 at T; then the front hook in segments of 1,
    bt_lag - 1, bt_lag, bt_lag + 1 and 64.  At T the lanes of both wavefronts hold bt_lag (set at T), bt_lag - 3 (set at T - 3) and 0 (never
    set); the counters end inside the second launch and at its end, the host's count is then 0 and the third launch is k_burst_front<false>.
    A setSettings zeroes the channel's PCM history (the Hilbert filter restarts), so a set channel sees re = -0 from then on; im comes from the test.
      set at T      everything behind the call depends on the samples behind it alone: the exact run of a fresh object on them, 4 E_o + 4 eps with
                    E_o = jo_burst_front_write behind jo_burst_set_settings against that run, on this stream
      set at T - 3  the same with three samples in front that are exactly 0 (both channels of the pair restarted: k_hilbert_fft gives a silent pair
                    exact zeros, burst_acq_cases), so bt_hold is bt_lag - 3 at T
      never set     their state comes from the real k_hilbert_fft: the pipeline bound of test_hilbert_in_the_loop, 8 E_o + 4 eps
    bt_hold from the peek behind every segment; cntdown = 2 PL - (samples behind the call) locks the detector for the whole test, so there is no
    decision to compare but tri_ptr, BI_EV_POS = -1 and an empty event list."""
    O = oracle_mod
    cfg = FC.CONFIGS[name]
    g = FC.geometry(cfg)
    nch, lag = 70, g.bt_lag
    T = FC.HIL_SHIFT + 3000 + 3
    post = [1, lag - 1, lag, lag + 1, 64]
    n = T + sum(post)
    X, Y = (62, 63, 68, 69), (1, 5, 33)
    obs = FC.chans(nch)
    rng = np.random.default_rng(0xC01D + lag)
    t = np.arange(n)
    pcm = np.rint(150.0 * rng.standard_normal((nch, n)) + 12000.0 * np.cos(2 * np.pi * 0.07 * t + np.arange(nch)[:, None])).astype(np.int16)
    im_post = np.zeros((nch, n - T))
    cols = {c: i for i, c in enumerate(O.BurstDemod.FRONT_COLS)}
    st_o = FC.oracle_settings(O, cfg)
    ref = {}
    for ch in obs:
        if ch in X or ch in Y:
            lead = 3 if ch in X else 0
            z = np.zeros(lead + n - T, dtype=complex)
            z.real[:] = -0.0
            z.imag[lead:] = 0.4 * np.cos(2 * np.pi * 0.13 * np.arange(n - T) + ch) + 0.01 * rng.standard_normal(n - T)
            im_post[ch] = z.imag[lead:]
            d = O.BurstDemod(st_o)
            d.front_write(O.hilbert_stream(pcm[ch, :T - lead], chunk=T)[0])
            d.set_settings(st_o)
            rows = d.front_write(z)
            ref[ch] = (rows[lead:], d.front_exact(z)[0][lead:], 4, lead)
        else:
            zo_pre = O.hilbert_stream(pcm[ch], chunk=n)[0]
            im_post[ch] = zo_pre.imag[T:]
            rows, exact, _, _ = pipeline_reference(O, cfg, pcm[ch], T)
            ref[ch] = (rows[T:], exact[T:], 8, None)
    for ch in range(nch):  # the channels nobody looks at: something of the right size
        if ch not in obs:
            im_post[ch] = 0.3 * np.sin(0.2 * np.arange(n - T) + ch)
    b = FrontBank(name, nch)
    try:
        for s in range(0, T - 3, 4096):
            b.bank.write(pcm[:, s:min(s + 4096, T - 3)])
        for ch in X:
            b.bank.set_settings(b.settings, channel=ch)
        b.bank.write(pcm[:, T - 3:T])
        for ch in Y:
            b.bank.set_settings(b.settings, channel=ch)
        assert b.nsamples() == T
        hold = {ch: (lag if ch in Y else lag - 3 if ch in X else 0) for ch in obs}
        assert {b.peek(ch)[0].bt_hold for ch in (1, 63)} == {lag, lag - 3}
        done = [0]

        def behind(k, s):
            for ch in obs:
                stt = b.peek(ch)[0]
                assert stt.bt_hold == max(0, hold[ch] - s), (name, ch, f"bt_hold behind {s} samples", stt.bt_hold)
                if ch in X or ch in Y:
                    assert (stt.cntdown, stt.maxposcd, stt.tri_ptr) == (2 * g.PL - s - ref[ch][3], -1, s + ref[ch][3]), (name, ch, s, stt.cntdown, stt.tri_ptr)
            done[0] = s

        sc = type("S", (), {})()
        series, evs, _ = collect(b, sc, obs, post, pcm[:, T:], im_post, start=T, on_segment=behind)
        assert done[0] == n - T and all(not l and np.all(p == -1) for p, l in evs)
        for ch in obs:
            rows, exact, factor, _ = ref[ch]
            eo = _errors({c: rows[:, cols[c]].copy() for c in series[ch]}, exact, cols)
            ek = _errors(series[ch], exact, cols)
            for c in ek:
                bound = factor * eo[c] + 4 * FC.EPS
                print(f"burst_front {name} hold channel {ch} (hold {hold[ch]}) {c}: kernel {ek[c] / FC.EPS:.2f} eps, oracle {eo[c] / FC.EPS:.2f} eps, kernel / bound {ek[c] / bound:.3f}")
            for c in ek:
                assert ek[c] <= factor * eo[c] + 4 * FC.EPS, (name, ch, c, f"kernel {ek[c] / FC.EPS:.2f} eps, oracle {eo[c] / FC.EPS:.2f} eps, factor {factor}")
    finally:
        b.close()


@pytest.mark.parametrize("name", list(FC.CONFIGS))
def test_hold_poked(oracle_mod, name):
    """bt_hold poked to 1 and 2 on two lanes of a running stream without a setSettings: the older tap of bt_d1 reads as zero for one sample, resp. both
    taps for one and the older for another.  Against jo_burst_front_exact with the same hold (the `hold` oldest of bt_d1's last bt_lag inputs
    zeroed) at 4 E_o + 4 eps, E_o from jo_burst_front_write with that hold on this stream; the lanes beside them (hold 0) against a plain run.  The
    launch behind the poke is k_burst_front<true> (the poke raises the host's count), the one after it <false>."""
    O = oracle_mod
    cfg = FC.CONFIGS[name]
    g = FC.geometry(cfg)
    nch = 67
    obs = FC.chans(nch)
    pre, post = [1000, 7, 1000], [9, 1000]
    n0, n = sum(pre), sum(pre) + sum(post)
    rng = np.random.default_rng(0x901D + g.bt_lag)
    z = {ch: 0.5 * np.exp(1j * (2 * np.pi * (0.03 + 0.01 * k) * np.arange(n) + k)) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) for k, ch in enumerate(obs)}
    for ch in obs:
        z[ch].real[:] = -0.0  # the PCM stays zero: re is -0, the imaginary part carries the signal
    im = np.stack([z[obs[obs.index(ch)] if ch in obs else obs[ch % 5]].imag for ch in range(nch)])
    pcm = np.zeros((nch, n), dtype=np.int16)
    hold = {obs[1]: 1, obs[2]: 2}
    cols = {c: i for i, c in enumerate(O.BurstDemod.FRONT_COLS)}
    b = FrontBank(name, nch)
    try:
        s1, _, _ = collect(b, None, obs, pre, pcm[:, :n0], im[:, :n0])
        for ch, h in hold.items():
            b.poke(ch, b.capi.FRONT_BT_HOLD, h)
        s2, _, states = collect(b, None, obs, post, pcm[:, n0:], im[:, n0:], start=n0)
        for ch in obs:
            h = hold.get(ch, 0)
            assert [st.bt_hold for st in states[ch]] == [0, 0], (name, ch)
            d = O.BurstDemod(FC.oracle_settings(O, cfg))
            rows = np.concatenate([d.front_write(z[ch][:n0]), d.front_write(z[ch][n0:], hold=h)])
            exact = d.front_exact(z[ch], hold_at=n0, hold=h)[0]
            if h:
                plain = d.front_exact(z[ch])[0]
                i = cols["ma1re"]
                assert np.any(exact[n0:n0 + h, i] != plain[n0:n0 + h, i]) and np.array_equal(exact[:n0, i], plain[:n0, i]), (name, ch, "the hold changes nothing")
            series = {c: np.concatenate([s1[ch][c], s2[ch][c]]) for c in s1[ch]}
            eo, ek = _errors({c: rows[:, cols[c]].copy() for c in series}, exact, cols), _errors(series, exact, cols)
            worst = max(ek, key=lambda c: ek[c] / (4 * eo[c] + 4 * FC.EPS))
            print(f"burst_front {name} poked hold {h} channel {ch}: worst column {worst}: kernel {ek[worst] / FC.EPS:.2f} eps, oracle {eo[worst] / FC.EPS:.2f} eps, "
                  f"kernel / bound {ek[worst] / (4 * eo[worst] + 4 * FC.EPS):.3f}")
            for c in ek:
                assert ek[c] <= 4 * eo[c] + 4 * FC.EPS, (name, ch, c, f"kernel {ek[c] / FC.EPS:.2f} eps, oracle {eo[c] / FC.EPS:.2f} eps")
    finally:
        b.close()


def test_front_hook_refusals():
    """Part E: JAERO_EINVAL before any launch for what the header lists, JAERO_EHIP from jaero_write and the setters behind front, front_poke and
    poke_bt; front_geom, front_peek and front_events leave a bank writable.  (Null contexts: tests/test_capi_host.py.)"""
    from jaero_amd import capi
    from jaero_amd import demodulator as D

    L = capi.lib()
    buf = np.zeros(70000)
    i16 = np.zeros(8 * 4096, dtype=np.int16)
    i32 = np.zeros(64, dtype=np.int32)
    n = C.c_int(0)
    cont = D.DemodulatorBank([D.OqpskSettings()] * 2, max_write_samples=4096)
    try:
        h = cont.h
        assert L.jaero_debug_burst_front_geom(h, C.byref(capi.BurstFrontGeom())) == capi.E_INVAL and b"not a burst bank" in L.jaero_last_error()
        assert L.jaero_debug_burst_front(h, i16.ctypes.data, 0, 16, None, i32.ctypes.data, i32.ctypes.data, C.byref(n)) == capi.E_INVAL
        assert L.jaero_debug_burst_front_peek(h, 0, C.byref(capi.BurstFrontState()), -1, 0, 0, None) == capi.E_INVAL
        assert L.jaero_debug_burst_front_events(h, 0, buf.ctypes.data, 4, C.byref(n)) == capi.E_INVAL
        assert L.jaero_debug_burst_front_poke(h, 0, capi.FRONT_CNTDOWN, 0.0) == capi.E_INVAL
        assert L.jaero_debug_burst_poke_bt(h, 0, 0, 1, buf.ctypes.data) == capi.E_INVAL
        cont.write(np.zeros((2, 64), dtype=np.int16))  # none of them marked it
    finally:
        cont.close()
    b = FrontBank("oqpsk", 5, max_write=1000)
    try:
        g, h = b.g, b.h
        pcm = np.zeros((5, 64), dtype=np.int16)
        st = capi.BurstFrontState()
        assert L.jaero_debug_burst_front_geom(h, None) == capi.E_INVAL
        out3 = (i32.ctypes.data, i32.ctypes.data, C.byref(n))
        for layout, ns in ((0, 0), (0, -1), (0, 1001), (0, 1008), (0, 1009), (2, 16), (-1, 16)):  # maxseg is 1008, max_write_samples 1000
            assert L.jaero_debug_burst_front(h, i16.ctypes.data, layout, ns, None, *out3) == capi.E_INVAL, (layout, ns)
        assert L.jaero_debug_burst_front(h, None, 0, 16, None, *out3) == capi.E_INVAL
        assert L.jaero_debug_burst_front(h, i16.ctypes.data, 0, 16, None, None, i32.ctypes.data, C.byref(n)) == capi.E_INVAL
        assert L.jaero_debug_burst_front(h, i16.ctypes.data, 0, 16, None, i32.ctypes.data, None, C.byref(n)) == capi.E_INVAL
        assert L.jaero_debug_burst_front(h, i16.ctypes.data, 0, 16, None, i32.ctypes.data, i32.ctypes.data, None) == capi.E_INVAL
        b.bank.write(pcm)  # refused before anything was marked
        for ch, ring, first, ns in ((64, -1, 0, 0), (-1, -1, 0, 0), (0, 8, 0, 1), (0, 7, 0, 0), (0, 7, 0, -1), (0, 7, 64 - g.bt_len - 1, 1), (0, 7, 64, 1), (0, 7, 0, 65),
                                    (0, 7, 64 - g.bt_len, g.bt_len + 1), (0, 0, 0, 65)):
            assert L.jaero_debug_burst_front_peek(h, ch, C.byref(st), ring, first, ns, buf.ctypes.data) == capi.E_INVAL, (ch, ring, first, ns)
        assert L.jaero_debug_burst_front_peek(h, 0, None, 7, 0, 1, None) == capi.E_INVAL
        for ch, ring, first, ns in ((63, -1, 0, 0), (0, 7, 64 - g.bt_len, g.bt_len), (4, 0, 0, 64), (0, 1, 63, 1)):  # padding lanes and the time before the stream included
            capi.check(L.jaero_debug_burst_front_peek(h, ch, C.byref(st), ring, first, ns, buf.ctypes.data))
        assert (st.cntdown, st.maxposcd, st.tri_ptr, st.bt_hold) == (2 * g.PL - 64, -1, 64, 0)
        for ch, cap in ((64, 4), (-1, 4), (0, -1)):
            assert L.jaero_debug_burst_front_events(h, ch, buf.ctypes.data, cap, C.byref(n)) == capi.E_INVAL
        assert L.jaero_debug_burst_front_events(h, 0, None, 4, C.byref(n)) == capi.E_INVAL
        capi.check(L.jaero_debug_burst_front_events(h, 0, buf.ctypes.data, 4, C.byref(n)))
        assert n.value == 1 and buf[1] == capi.EV_FREQ
        b.bank.write(pcm)  # the readers left the bank writable
        for ch, f, v in ((64, 0, 0.0), (-1, 0, 0.0), (0, 5, 0.0), (0, -1, 0.0), (0, capi.FRONT_CNTDOWN, 2 * g.PL + 1.0), (0, capi.FRONT_CNTDOWN, -1.0),
                         (0, capi.FRONT_CNTDOWN, 1.5), (0, capi.FRONT_MAXPOSCD, -2.0), (0, capi.FRONT_MAXPOSCD, 2 * g.PL + 1.0), (0, capi.FRONT_TRI_PTR, g.tri_sz + 2.0),
                         (0, capi.FRONT_TRI_PTR, -1.0), (0, capi.FRONT_BT_HOLD, g.bt_lag + 1.0), (0, capi.FRONT_BT_HOLD, -1.0), (0, capi.FRONT_LASTDY, float("nan")),
                         (0, capi.FRONT_LASTDY, float("inf")), (0, capi.FRONT_CNTDOWN, float("nan"))):
            assert L.jaero_debug_burst_front_poke(h, ch, f, v) == capi.E_INVAL, (ch, f, v)
        for ch, ns in ((64, 1), (-1, 1), (0, 0), (0, g.bt_len + 1)):
            assert L.jaero_debug_burst_poke_bt(h, ch, 0, ns, buf.ctypes.data) == capi.E_INVAL, (ch, ns)
        assert L.jaero_debug_burst_poke_bt(h, 0, 0, 1, None) == capi.E_INVAL
        b.bank.write(pcm)  # refused before anything was marked
    finally:
        b.close()
    for mark in ("front", "front_poke", "poke_bt"):
        b = FrontBank("msk1200", 3)
        try:
            pcm = np.zeros((3, 64), dtype=np.int16)
            if mark == "front":
                assert b.front(pcm, None)[2] == 0
            elif mark == "front_poke":
                b.poke(2, b.capi.FRONT_LASTDY, -1.0)
            else:
                b.poke_bt(63, -5, np.ones(10))
            assert L.jaero_write(b.h, pcm.ctypes.data, 64, 0, 0, None) == capi.E_HIP, mark
            assert L.jaero_set_settings(b.h, -1, C.byref(b.settings.to_c())) == capi.E_HIP, mark
            assert L.jaero_set_flags(b.h, -1, 1, 0, 0) == capi.E_HIP, mark
            assert b.peek(0)[0].bt_hold == 0 and len(b.events(0)) == 1  # the readers go on working
        finally:
            b.close()
