"""GPU (-m gpu): the burst banks' tracking kernels k_burst_oqpsk_demod<CAPSYM> and k_burst_msk_fb<CAPSYM, FIRN, LDSN> on their own, through
jaero_debug_burst_track / _track_peek / _track_fill / _track_read / _track_center_freq and jaero_debug_burst_poke_cv: the launch line of
jaero_write, not a copy of it, on input and verdicts the test supplies.  Against jo_burst_track_write; tests/burst_track_cases.py states what is
asserted and why, tests/test_burst_track_cases.py checks the cases themselves on the CPU.  Part B prints E_n and the kernel's deviation before it
asserts and, where JAERO_EVIDENCE_DIR names a directory, writes both to burst_track_direct.json there (committed copy: profiles/burst_track_direct.json)."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import burst_track_cases as TC

pytestmark = pytest.mark.gpu
NAMES = list(TC.CONFIGS)


class TrackBank:
    """A burst bank of a case, driven through the tracking hooks."""

    def __init__(self, c, afc=False, nch=TC.NCH):
        from jaero_amd import capi
        from jaero_amd import demodulator as D

        self.capi, self.c, self.nch = capi, c, nch
        settings = D.BurstOqpskSettings() if c.cfg.oq else D.BurstMskSettings(fb=c.cfg.fb)
        self.bank = D.DemodulatorBank([settings] * nch, max_write_samples=TC.MAX_WRITE, trace=c.trace, capture_symbols=c.capsym, softbit_capacity=c.softcap)
        self.L, self.h = self.bank.L, self.bank.h
        try:
            if c.sql or afc:
                self.bank.set_flags(afc=afc, sql=c.sql)  # before the first hook marks the bank
            self.bg, self.tg = capi.BurstGeom(), capi.BurstTrackGeom()
            capi.check(self.L.jaero_debug_burst_geom(self.h, C.byref(self.bg)))
            capi.check(self.L.jaero_debug_burst_track_geom(self.h, C.byref(self.tg)))
            g, cap = TC.geometry(c.cfg), TC.capacities(c)
            assert self.bg.maxseg == TC.MAXSEG and self.bg.cv_len == g.cv_len and self.bg.nchp == (nch + 63) // 64 * 64
            for k in ("D2", "msema_len", "win_ring", "agc2_len", "eb_len", "startstopstart", "firn", "ldsn", "ebno_tail"):
                assert getattr(self.tg, k) == getattr(g, k), (c.name, k, getattr(self.tg, k), getattr(g, k))
            assert (self.tg.soft_cap, self.tg.sym_cap, self.tg.ev_cap) == (cap.soft_cap, cap.sym_cap, cap.ev_cap)
            variant = C.create_string_buffer(256)
            capi.check(self.L.jaero_debug_kernel_variant(self.h, 0, variant, 256))
            want = f"k_burst_oqpsk_demod<{str(c.capsym).lower()}>" if c.cfg.oq else f"k_burst_msk_fb<{str(c.capsym).lower()}, {g.firn}, {g.ldsn}>"
            assert variant.value.decode() == want, (variant.value, want)
            self.lag = self.bg.D1 + self.tg.D2
            capi.check(self.L.jaero_debug_burst_track_fill(self.h, TC.SOFT_SENTINEL, TC.SYM_SENTINEL))
            self.poked = 0  # samples [0, poked) of every channel's input are in the ring
        except BaseException:
            self.bank.close()
            raise

    def close(self):
        self.bank.close()

    def nsamples(self):
        bg = self.capi.BurstGeom()
        self.capi.check(self.L.jaero_debug_burst_geom(self.h, C.byref(bg)))
        return bg.nsamples

    def feed(self, upto):
        """The kernel reads val of sample m at ring index m - D1 - D2: keep the ring filled up to sample `upto`, a chunk of cv_len - maxseg samples
        at a time (what it overwrites lies behind the samples consumed)."""
        c = self.c
        if not c.vals or upto <= self.poked:
            return
        s = self.nsamples()
        assert self.poked >= s or self.poked == 0
        n = min(self.bg.cv_len - TC.MAXSEG, c.total - s)
        for ch, v in c.vals.items():
            a = np.ascontiguousarray(v[s:s + n])
            self.capi.check(self.L.jaero_debug_burst_poke_cv(self.h, ch, s - self.lag, len(a), a.ctypes.data))
        self.poked = s + n
        assert upto <= self.poked

    def track_rc(self, n, first, ev):
        chans = np.array(sorted(ev), dtype=np.int32)
        pos = np.array([ev[ch][0] for ch in chans], dtype=np.int32)
        ver = (self.capi.TridentResult * max(len(chans), 1))(*[TC.to_struct(self.capi.TridentResult, ev[ch][1]) for ch in chans])
        return self.L.jaero_debug_burst_track(self.h, n, first, chans.ctypes.data, pos.ctypes.data, ver, len(chans))

    def peek(self, ch):
        st = self.capi.BurstTrackState()
        self.capi.check(self.L.jaero_debug_burst_track_peek(self.h, ch, C.byref(st)))
        return {k: getattr(st, k) for k in st.INTS + st.DBLS}

    def rows(self, ch):
        soft = np.zeros(self.tg.soft_cap, dtype=np.int16)
        self.capi.check(self.L.jaero_debug_burst_track_read(self.h, ch, 0, soft.ctypes.data, len(soft)))
        sym = np.zeros((max(self.tg.sym_cap, 1), 3))
        self.capi.check(self.L.jaero_debug_burst_track_read(self.h, ch, 1, sym.ctypes.data, self.tg.sym_cap))
        ev, n = np.zeros((self.tg.ev_cap, 3)), C.c_int(0)
        self.capi.check(self.L.jaero_debug_burst_front_events(self.h, ch, ev.ctypes.data, self.tg.ev_cap, C.byref(n)))
        return soft, sym[:self.tg.sym_cap], ev[:n.value].copy()

    def run(self, watch=None, between=None):
        """Every launch of the case; the peek of the watched channels behind every write (cases about a capacity: behind the last)"""
        c = self.c
        watch = c.watch if watch is None else watch
        states = {ch: [] for ch in watch}
        segs = list(TC.segments(c))
        for k, (s, n, first, ev) in enumerate(segs):
            assert self.nsamples() == s
            self.feed(s + n)
            if between:
                between(self, s)
            self.capi.check(self.track_rc(n, first, ev))
            last = k + 1 == len(segs)
            if last or (segs[k + 1][2] and not c.overflow):
                for ch in watch:
                    states[ch].append(self.peek(ch))
        got = {}
        for ch in watch:
            soft, sym, ev = self.rows(ch)
            got[ch] = SimpleNamespace(soft_row=soft, sym_rows=sym, events=ev, states=states[ch])
        return got


def run_exact(O, c):
    b = TrackBank(c)
    try:
        got = b.run()
        cap = TC.capacities(c)
        for ch in c.watch:
            TC.check_exact(c, ch, TC.expected(O, c, ch), got[ch], cap)
        return b
    except BaseException:
        b.close()
        raise


@pytest.mark.parametrize("capsym", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_edges_of_the_first_segment(oracle_mod, name, capsym):
    """Part A: the verdict on sample 0, 1, n - 2 and n - 1 of a first segment of n = 1, 2, 7, 35, 36, 37, 1000, maxseg - 1 and maxseg samples at
    n0 = 0 (below agc2_len and eb_len: s_agc2 and s_e start negative), a channel that never gets one, and what follows up to the marker."""
    for c in TC.edge_cases(name, capsym):
        run_exact(oracle_mod, c).close()


@pytest.mark.parametrize("capsym", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_whole_bursts_on_zero_input(oracle_mod, name, capsym):
    """Part A: bursts through marker, EbNo emission and time-out, past a wrap of win_ring, cv_len and the msema ring; second verdicts before the
    marker, between marker and EbNo emission, inside the last JD_EBNO_TAIL samples before it and behind the time-out; rejecting verdicts idle and in
    mid-burst, trace on and off; a channel without any verdict keeps its rows, its counters and its one event."""
    for c in TC.burst_cases(oracle_mod, name, capsym):
        b = run_exact(oracle_mod, c)
        try:
            st = b.peek(69)
            soft, sym, ev = b.rows(69)
            assert st["soft_cnt"] == 0 and st["sym_cnt"] == 0 and st["ev_cnt"] == 1 and st["startstop"] == -1 and st["cntr"] == 0 and st["overflow"] == 0
            assert np.all(soft == TC.SOFT_SENTINEL) and len(ev) == 1
        finally:
            b.close()


@pytest.mark.parametrize("capsym", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_segment_boundaries_at_the_landmarks(oracle_mod, name, capsym):
    """Part A: a segment boundary on, one before and one behind the marker, the EbNo emission, the time-out and the pair that completes the first
    group of soft bits; burst OQPSK also with the squelch on (the write whose lastmse was below the threshold, a first_of_write = 0 segment behind it)."""
    for c in TC.boundary_cases(oracle_mod, name, capsym) + TC.squelch_cases(oracle_mod, name, capsym):
        run_exact(oracle_mod, c).close()


@pytest.mark.parametrize("capsym", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_capacities(oracle_mod, name, capsym):
    """Part A: the soft row, the symbol log and the event log filled to their capacities: the prefix that fits equals the oracle's, the overflow bits
    say what did not, and nothing is stored behind the counts."""
    for c in TC.cap_cases(oracle_mod, name, capsym):
        run_exact(oracle_mod, c).close()


def test_the_hook_refuses_what_it_documents(oracle_mod):
    """jaero_debug_burst_track: a padding lane or a channel listed twice, an event position outside the segment, a segment longer than maxseg,
    first_of_write outside {0, 1}; the readers take channels up to nchp and no further; a bank that is not a burst bank.  Nothing launched: the sample
    count and the rows stay as they were."""
    from jaero_amd import capi
    from jaero_amd import demodulator as D

    c = TC.edge_cases("oqpsk", False)[2]
    b = TrackBank(c)
    try:
        A = TC.ACCEPT["oqpsk"]
        E = capi.E_INVAL
        assert b.track_rc(7, 1, {70: (0, A)}) == E and b"outside [0, 70)" in b.L.jaero_last_error()
        assert b.track_rc(7, 1, {0: (7, A)}) == E and b.track_rc(7, 1, {0: (-1, A)}) == E
        assert b.track_rc(0, 1, {}) == E and b.track_rc(TC.MAXSEG + 1, 1, {}) == E and b.track_rc(7, 2, {}) == E
        two = np.array([3, 3], dtype=np.int32)
        ver = (capi.TridentResult * 2)()
        assert b.L.jaero_debug_burst_track(b.h, 7, 1, two.ctypes.data, two.ctypes.data, ver, 2) == E and b"listed twice" in b.L.jaero_last_error()
        assert b.L.jaero_debug_burst_track(b.h, 7, 1, None, None, None, 1) == E and b.L.jaero_debug_burst_track(b.h, 7, 1, two.ctypes.data, two.ctypes.data, ver, 71) == E
        st = capi.BurstTrackState()
        assert b.L.jaero_debug_burst_track_peek(b.h, 128, C.byref(st)) == E and b.L.jaero_debug_burst_track_peek(b.h, -1, C.byref(st)) == E
        assert b.L.jaero_debug_burst_track_peek(b.h, 127, C.byref(st)) == 0
        buf = np.zeros(b.tg.soft_cap, dtype=np.int16)
        assert b.L.jaero_debug_burst_track_read(b.h, 0, 0, buf.ctypes.data, b.tg.soft_cap - 1) == E and b.L.jaero_debug_burst_track_read(b.h, 128, 0, buf.ctypes.data, b.tg.soft_cap) == E
        assert b.L.jaero_debug_burst_track_center_freq(b.h, 0, 1000.0) == E and b"burst MSK" in b.L.jaero_last_error()
        assert b.nsamples() == 0 and np.all(b.rows(0)[0] == TC.SOFT_SENTINEL)
        pcm = np.zeros((TC.NCH, 16), dtype=np.int16)
        assert b.L.jaero_write(b.h, pcm.ctypes.data, 16, 0, 0, None) == capi.E_HIP  # track_fill marked the bank
    finally:
        b.close()
    cont = D.DemodulatorBank([D.OqpskSettings()] * 2, max_write_samples=4096)
    try:
        assert cont.L.jaero_debug_burst_track(cont.h, 7, 1, None, None, None, 0) == capi.E_INVAL and b"not a burst bank" in cont.L.jaero_last_error()
        assert cont.L.jaero_debug_burst_track_geom(cont.h, C.byref(capi.BurstTrackGeom())) == capi.E_INVAL
    finally:
        cont.close()


RESULTS = {}


def record(key, rows):
    RESULTS[key] = rows
    out = os.environ.get("JAERO_EVIDENCE_DIR")
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "burst_track_direct.json"), "w") as f:
            json.dump(RESULTS, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.mark.parametrize("name,sql", [(n, False) for n in NAMES] + [("oqpsk", True)])
def test_values_on_recorded_bursts(oracle_mod, name, sql):
    """Part B: val_to_demod and the verdicts of the oracle's ordinary run on generated burst pairs (Eb/N0 18, 10 and 4 / 5 dB -- burst MSK 600: 18 and 10 --, carrier offsets
    to both ends of the range), segments rotating through 1, 7, 36, 1000, maxseg - 1 and maxseg.  Decisions exact, soft bytes within 1 in at most
    BURST_SOFT_ALLOW bytes, event values within 1e-6, symbols within min(SYM_TOL, E_n)."""
    O = oracle_mod
    c = TC.stream_case(O, name, sql=sql)
    b = TrackBank(c)
    try:
        got = b.run(watch=TC.OBS)
        cap = TC.capacities(c)
        rows, fails = {}, []
        for ch in TC.OBS:
            exp = TC.expected(O, c, ch)
            en, why = TC.noise_reference(O, c, ch, exp, 0)
            assert why is None, (name, ch, "the noise draw changes a decision of the oracle", why)
            tol = min(TC.SYM_TOL, en)
            dev = TC.symbol_deviation(got[ch].sym_rows[:len(exp.symbols)], exp.symbols) if got[ch].states[-1]["sym_cnt"] == len(exp.symbols) else float("nan")
            nd, mx = TC.soft_differences(got[ch].soft_row[:len(exp.soft)], exp.soft)
            print(f"burst_track {name} sql={int(sql)} channel {ch}: E_n {en:.3e}  kernel {dev:.3e}  bound {tol:.3e}  symbols {len(exp.symbols)}  soft bytes {len(exp.soft)} ({nd} differ)")
            rows[str(ch)] = {"E_n": en, "kernel": dev, "bound": tol, "symbols": len(exp.symbols), "soft": len(exp.soft), "soft_differ": nd}
            try:
                TC.check_values(c, ch, exp, got[ch], cap, tol)
            except AssertionError as e:
                fails.append(e)
        record(f"{name} sql={int(sql)}", rows)
        if fails:
            raise fails[0]
    finally:
        b.close()


@pytest.mark.parametrize("name", NAMES)
def test_ebno_emission_does_not_depend_on_the_segmentation(oracle_mod, name):
    """The EbNo meter is evaluated only in the last JD_EBNO_TAIL samples before an emission or a launch's end: the kernel's own emission on the recorded
    streams in two segmentations (the rotation; whole segments) agrees to EBNO_SEG_REL, the bound burst_track_cases derives from 0.8^192."""
    O = oracle_mod
    runs = []
    for sizes in (TC.ROTATION, (TC.MAXSEG,)):
        b = TrackBank(TC.ebno_case(O, name, sizes))
        try:
            runs.append(b.run(watch=TC.OBS))
        finally:
            b.close()
    worst = 0.0
    for ch in TC.OBS:
        ev = [r[ch].events[r[ch].events[:, 1] == TC.EV_EBNO] for r in runs]
        assert len(ev[0]) >= 1 and np.array_equal(ev[0][:, 0], ev[1][:, 0]), (name, ch, ev)
        for a, b2 in zip(ev[0][:, 2], ev[1][:, 2]):
            rel = abs(a - b2) / max(abs(a), abs(b2), 1e-300)
            worst = max(worst, rel)
            assert rel <= TC.EBNO_SEG_REL, (name, ch, a, b2, rel)
    print(f"burst_track {name}: EbNo emissions of two segmentations agree to {worst:.3e} relative")


@pytest.mark.parametrize("name", ["msk1200", "msk600"])
def test_center_freq_between_two_segments(oracle_mod, name):
    """Part C: k_burst_msk_center_freq on the middle one of three channels between two hook segments, afc on and off, the frequency inside the range
    and beyond both clamps: the FREQ row is stamped with the next segment's first sample and carries the oracle's value, mixer_center and mixer2
    follow, and the two neighbours equal their own runs."""
    O = oracle_mod
    A = TC.ACCEPT[name]
    for afc, hz in TC.center_cases():
        at = 700
        c = TC.case(name, f"center afc={int(afc)} {hz}", [[at], [900]], {0: [(10, A)], 1: [(20, A)], 2: [(30, A)]}, watch=(0, 1, 2))
        b = TrackBank(c, afc=afc, nch=3)
        try:
            def between(bank, s):
                if s == at:
                    bank.capi.check(bank.L.jaero_debug_burst_track_center_freq(bank.h, 1, hz))

            got = b.run(between=between)
            for ch in (0, 1, 2):
                d = O.BurstDemod(TC.oracle_settings(O, c.cfg), afc=afc)
                v = TC.to_struct(O.TridentResult, A)
                d.track_write(np.zeros(at), v, c.verdicts[ch][0][0])
                if ch == 1:
                    d.center_freq_changed(hz)
                d.track_write(np.zeros(900))
                st = d.track_state()
                ev = d.take_events()
                soft = np.concatenate([d.take_soft(), st["rx"]])
                g, last = got[ch], got[ch].states[-1]
                assert np.array_equal(g.events, ev), (name, afc, hz, ch, g.events, ev)
                assert ((ev[:, 0] == at) & (ev[:, 1] == TC.EV_FREQ)).sum() == (ch == 1)
                assert last["m2_freq"] == st["m2_freq"] and last["mc_freq"] == st["mc_freq"], (name, afc, hz, ch, last["m2_freq"], st["m2_freq"], last["mc_freq"], st["mc_freq"])
                assert last["soft_cnt"] == len(soft) and np.array_equal(g.soft_row[:len(soft)], soft) and np.all(g.soft_row[len(soft):] == TC.SOFT_SENTINEL)
                for f in TC.INTS_MSK:
                    assert last[f] == st[f], (name, afc, hz, ch, f)
        finally:
            b.close()
