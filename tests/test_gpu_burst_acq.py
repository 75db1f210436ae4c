"""GPU (-m gpu): the burst front end's two transform kernels on their own -- k_trident<true> / k_trident<false> behind k_ev_compact, and
k_hilbert_fft behind k_hist_push_frames / k_hist_push_chmajor (jaero_amd/csrc/k_burst_front.h) -- through jaero_debug_burst_geom / _hilbert /
_read_hist / _poke_cv / _trident: the launch lines of jaero_write, not copies of them.  Against the oracle's stand-alone trident check
(jo_trident), oracle.hilbert_stream and exact long-double sums; tests/burst_acq_cases.py states what is asserted and why.  Every test prints
its errors in units of 2^-52; DESIGN.md section 10 keeps the table of an MI355X run."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import burst_acq_cases as BC

pytestmark = pytest.mark.gpu
CHANNEL_MAJOR, FRAME_MAJOR = 0, 1
POISON = 1.0e6


class AcqBank:
    """A burst bank driven through the acquisition hooks."""

    def __init__(self, name, nch, max_write=4096):
        from jaero_amd import capi
        from jaero_amd import demodulator as D

        self.capi, self.nch, self.cfg = capi, nch, BC.CONFIGS[name]
        st = D.BurstOqpskSettings() if self.cfg.oq else D.BurstMskSettings(fb=self.cfg.fb)
        self.bank = D.DemodulatorBank([st] * nch, max_write_samples=max_write)
        self.L, self.h = self.bank.L, self.bank.h
        self.g = self.geom()
        want = BC.geometry(self.cfg, nch, max_write)
        assert {k: getattr(self.g, k) for k in want} == want and self.g.tri_grid >= 15 and self.g.nsamples == 0

    def close(self):
        self.bank.close()

    def geom(self):
        g = self.capi.BurstGeom()
        self.capi.check(self.L.jaero_debug_burst_geom(self.h, C.byref(g)))
        return g

    def hilbert(self, blk, layout):
        blk = np.asarray(blk, dtype=np.int16)
        a = np.ascontiguousarray(blk if layout == CHANNEL_MAJOR else blk.T)
        out = np.full(blk.shape, np.nan)
        self.capi.check(self.L.jaero_debug_burst_hilbert(self.h, a.ctypes.data, layout, blk.shape[1], out.ctypes.data))
        return out

    def read_hist(self, ch, first, n):
        out = np.empty(n, dtype=np.int16)
        self.capi.check(self.L.jaero_debug_burst_read_hist(self.h, ch, first, n, out.ctypes.data))
        return out

    def poke_cv(self, ch, first, re):
        re = np.ascontiguousarray(re, dtype=np.float64)
        self.capi.check(self.L.jaero_debug_burst_poke_cv(self.h, ch, first, len(re), re.ctypes.data))

    def trident_rc(self, channels, ev_pos, n0, grid):
        ch, ev = np.asarray(channels, dtype=np.int32), np.asarray(ev_pos, dtype=np.int32)
        res = (self.capi.TridentResult * max(1, len(ch)))()
        nchg = C.c_int(-1)
        rc = self.L.jaero_debug_burst_trident(self.h, ch.ctypes.data, ev.ctypes.data, len(ch), n0, grid, res, C.byref(nchg))
        return rc, [SimpleNamespace(ok=r.ok, freq=r.freq, phase_deg=r.phase_deg, vol_gain=r.vol_gain, metric=r.metric) for r in res[:len(ch)]], nchg.value

    def trident(self, channels, ev_pos, n0, grid):
        rc, res, nchg = self.trident_rc(channels, ev_pos, n0, grid)
        self.capi.check(rc)
        return res, nchg

    def place(self, ch, case, n0, ev_pos, rng, whole_ring):
        """The case's window where an event at sample n0 + ev_pos finds it (sample a of the AGC'd ring lives at slot a mod cv_len), every ring sample
        outside it (whole_ring) or the 64 on either side of it poisoned; burst OQPSK: the window's tail behind the two parts as well"""
        cfg, g = self.cfg, self.g
        w = case.window.copy()
        w[cfg.nb + cfg.nt:] = POISON
        pad = (lambda n: POISON * rng.choice([-1.0, 1.0], n))
        w0 = n0 + ev_pos - g.tri_sz - g.D1
        if whole_ring:
            self.poke_cv(ch, w0, np.concatenate([w, pad(g.cv_len - len(w))]))
        else:
            self.poke_cv(ch, w0 - 64, np.concatenate([pad(64), w, pad(64)]))
        return w0


def all_cases(O, name):
    cases, E, _ = BC.population(O, name, BC.NDRAWS)
    return cases, BC.deliberate_cases(O, name), E


def report(name, what, E, worst):
    for label, eo, ek in zip(("metric", "vol_gain", "phase"), E, worst):
        print(f"burst_acq trident {name} {what} {label}: kernel {ek / BC.EPS:.2f} eps, oracle {eo / BC.EPS:.2f} eps, kernel / bound {ek / (4 * eo + 4 * BC.EPS):.2f}, "
              f"oracle / bound {eo / (4 * eo + 4 * BC.EPS):.2f}")


@pytest.mark.parametrize("name", list(BC.CONFIGS))
def test_trident_values_and_placement(oracle_mod, name):
    """Draws and every deliberate case on channels 0, 1, 63, 64 and the last live one, five events per launch of ONE workgroup (per-event state
    must not leak from one to the next), the window placed so that it starts before sample 0, wraps the ring inside the base part, inside the
    top part, exactly at the part boundary, not at all and (burst MSK 600) between n and n + 8192 of the fold -- with every ring sample outside
    the window poisoned."""
    cfg = BC.CONFIGS[name]
    draws, delib, E = all_cases(oracle_mod, name)
    wraps = ["before", cfg.nb // 2, cfg.nb, cfg.nb + cfg.nt // 2, None] + ([8192, 8192 + 5, 8191] if cfg.nb > 8192 else [])
    cases = delib + draws[:5 * len(wraps) - len(delib)]  # five windows for every placement
    rng = np.random.default_rng(0x71D)
    b = AcqBank(name, 70)
    g = b.g
    chans = [0, 1, 63, 64, b.nch - 1]
    evs = [0, 1, g.maxseg - 1, 7, g.maxseg // 2]
    worst, seen = [0.0, 0.0, 0.0], set()
    try:
        for k in range(0, len(cases), 5):
            grp = cases[k:k + 5]
            x = wraps[(k // 5) % len(wraps)]
            if x == "before":
                n0 = 0
            elif x is None:
                n0 = 4 * g.cv_len + g.tri_sz + g.D1  # slot 0 for ev_pos 0
            else:
                n0 = 3 * g.cv_len + (g.tri_sz + g.D1 - x) % g.cv_len  # an event at ev_pos 0 finds its window's sample x at slot 0
            for ch, ev, c in zip(chans, evs, grp):
                w0 = b.place(ch, c, n0, ev, rng, True)
                wrap_at = (-w0) % g.cv_len  # the window index that lives at slot 0
                seen.add("before" if w0 < 0 and n0 == 0 else "base" if 0 < wrap_at < cfg.nb else "boundary" if wrap_at == cfg.nb else
                         "top" if cfg.nb < wrap_at < cfg.nb + cfg.nt else "none")
                if cfg.nb > 8192 and 8192 <= wrap_at < cfg.nb:
                    seen.add("fold")
            res, nchg = b.trident(chans[:len(grp)][::-1], evs[:len(grp)][::-1], n0, 1)
            assert nchg == len(grp), (name, k, nchg)
            for c, r in zip(grp[::-1], res):
                errs = BC.check_trident(c, r, E, f"n0 {n0}, wrap {x}")
                worst = [max(a, e or 0.0) for a, e in zip(worst, errs)]
        report(name, "placement", E, worst)
        assert seen >= {"before", "base", "boundary", "top", "none"} | ({"fold"} if cfg.nb > 8192 else set()), seen
    finally:
        b.close()


@pytest.mark.parametrize("name,nch", [("oqpsk", 70), ("msk1200", 67), ("msk600", 70)])
def test_trident_lists_and_grids(oracle_mod, name, nch):
    """A window of its own on every channel; one launch over all of them checked against the oracle, then lists of 0, 1, 7, 8, 9 and all
    channels in random order on grids of 1, 7, 8, 9, 15 workgroups and the default (the event list is split in eighths over the XCDs, unevenly
    unless grid and count are multiples of 8): every listed channel its own result bit for bit, nchanged == nlist, an empty list leaves every
    sentinel in place."""
    draws, delib, E = all_cases(oracle_mod, name)
    cases = (draws + delib)[:nch]
    assert len(cases) == nch
    rng = np.random.default_rng(0x615D)
    b = AcqBank(name, nch)
    g = b.g
    try:
        n0 = 5 * g.cv_len + 1234
        evs = [(0, 1, g.maxseg - 1)[c] if c < 3 else int(rng.integers(0, g.maxseg)) for c in range(nch)]
        for ch in range(nch):
            b.place(ch, cases[ch], n0, evs[ch], rng, False)
        res, nchg = b.trident(list(range(nch)), evs, n0, 0)
        assert nchg == nch
        worst = [0.0, 0.0, 0.0]
        for ch in range(nch):
            errs = BC.check_trident(cases[ch], res[ch], E, f"channel {ch} of all, default grid")
            worst = [max(a, e or 0.0) for a, e in zip(worst, errs)]
        report(name, "all channels", E, worst)
        expected = dict(enumerate(res))
        for grid in (1, 7, 8, 9, 15, 0):
            for nl in (0, 1, 7, 8, 9, nch):
                listed = [int(c) for c in rng.permutation(nch)[:nl]]
                if nl == 7:
                    listed = [nch - 1, 64, 63, 0] + [c for c in listed if c not in (0, 63, 64, nch - 1)][:3]
                r, nchg = b.trident(listed, [evs[c] for c in listed], n0, grid)
                BC.check_event_list(listed, r, nchg, expected, f"{name}: {nl} events on a grid of {grid}")
    finally:
        b.close()


@pytest.mark.parametrize("name,nch,max_write,layout", [("oqpsk", 67, 4096, CHANNEL_MAJOR), ("msk1200", 70, 4096, FRAME_MAJOR),
                                                       ("msk600", 67, 1000, FRAME_MAJOR), ("oqpsk", 70, 1000, CHANNEL_MAJOR)])
def test_hilbert(oracle_mod, name, nch, max_write, layout):
    """maxseg 2048 (burst OQPSK), 4096 (burst MSK) and 1008 (max_write_samples 1000); writes of 1, 7, 2047, 2048, 2049, 100, 3000 and the
    maximum, so that segments start off the 2048 grid, blocks are cut at both ends and the history ring wraps more than twice (read back by
    absolute index after every write); full-scale PCM with both extremes; one pair with a silent member, one pair silent on both sides, and with
    67 channels a last channel whose partner is padding.  A fresh bank: the first hil_lat + 2048 outputs see the zeros before the stream."""
    O = oracle_mod
    b = AcqBank(name, nch, max_write)
    g = b.g
    try:
        assert g.maxseg == {("oqpsk", 4096): 2048, ("msk1200", 4096): 4096}.get((name, max_write), 1008)
        sizes = BC.hilbert_sizes(max_write, 2 * g.hist_len + 3000)
        n = sum(sizes)
        pcm = BC.fullscale_pcm(nch, n, 0x41B + nch + max_write, silent=(4, 6, 7))
        peek = [0, 63, 64, nch - 1]
        out, s = [], 0
        for m in sizes:
            out.append(b.hilbert(pcm[:, s:s + m], layout))
            s += m
            assert b.geom().nsamples == s
            first = max(0, s - g.hist_len)
            for ch in peek:
                assert np.array_equal(b.read_hist(ch, first, s - first), pcm[ch, first:s]), (name, "history ring", ch, s)
        gpu = np.concatenate(out, axis=1)
        assert not np.isnan(gpu).any()
        orc = BC.oracle_hilbert(O, pcm, sizes)
        ncap = min(n, BC.MAX_EXACT_SAMPLES)
        assert ncap > BC.HIL_LAT + 2048 + 4096
        exact = {c: BC.exact_hilbert(O, pcm[c, :ncap]) for c in (0, 1, 4, nch - 1)}
        tag = f"{name} nch {nch} maxseg {g.maxseg} layout {layout}"
        _, worst = BC.check_hilbert(gpu[:, :ncap], orc[:, :ncap], exact, tag + " head")
        BC.check_hilbert(gpu, orc, {}, tag + " whole stream", e_oracle_worst=worst)
    finally:
        b.close()


def test_hook_refusals(oracle_mod):
    """JAERO_EINVAL before any launch for what the header lists, JAERO_EHIP from jaero_write and the setters after a hook that marks the bank;
    geom and read_hist leave a bank writable.  (Null contexts: tests/test_capi_host.py.)"""
    from jaero_amd import capi
    from jaero_amd import demodulator as D

    L = capi.lib()
    buf = np.zeros(8192)
    i16 = np.zeros(70 * 4096, dtype=np.int16)
    cont = D.DemodulatorBank([D.OqpskSettings()] * 2, max_write_samples=4096)
    try:
        h = cont.h
        assert L.jaero_debug_burst_geom(h, C.byref(capi.BurstGeom())) == capi.E_INVAL and b"not a burst bank" in L.jaero_last_error()
        assert L.jaero_debug_burst_hilbert(h, i16.ctypes.data, 0, 16, buf.ctypes.data) == capi.E_INVAL
        assert L.jaero_debug_burst_read_hist(h, 0, 0, 1, i16.ctypes.data) == capi.E_INVAL
        assert L.jaero_debug_burst_poke_cv(h, 0, 0, 1, buf.ctypes.data) == capi.E_INVAL
        assert L.jaero_debug_burst_trident(h, None, None, 0, 0, 0, None, None) == capi.E_INVAL
        cont.write(np.zeros((2, 64), dtype=np.int16))  # none of them marked it
    finally:
        cont.close()
    b = AcqBank("oqpsk", 5)
    try:
        g, h = b.g, b.h
        pcm = np.zeros((5, 64), dtype=np.int16)
        assert L.jaero_debug_burst_geom(h, None) == capi.E_INVAL
        assert L.jaero_debug_burst_read_hist(h, 0, 0, 1, i16.ctypes.data) == capi.E_INVAL  # nothing written yet
        b.bank.write(pcm)  # geom and the refused read_hist left the bank writable
        assert np.array_equal(b.read_hist(4, 0, 64), pcm[4])
        for ch, first, n in ((5, 0, 1), (-1, 0, 1), (0, 0, 0), (0, 1, 64), (0, -1, 2), (0, 0, 65)):
            assert L.jaero_debug_burst_read_hist(h, ch, first, n, i16.ctypes.data) == capi.E_INVAL, (ch, first, n)
        assert L.jaero_debug_burst_read_hist(h, 0, 0, 1, None) == capi.E_INVAL
        b.bank.write(pcm)
        for layout, n in ((0, 0), (0, 4097), (2, 16), (-1, 16)):
            assert L.jaero_debug_burst_hilbert(h, i16.ctypes.data, layout, n, buf.ctypes.data) == capi.E_INVAL, (layout, n)
        assert L.jaero_debug_burst_hilbert(h, None, 0, 16, buf.ctypes.data) == capi.E_INVAL
        assert L.jaero_debug_burst_hilbert(h, i16.ctypes.data, 0, 16, None) == capi.E_INVAL
        big = np.zeros(g.cv_len + 1)
        for ch, n in ((5, 1), (-1, 1), (0, 0), (0, g.cv_len + 1)):
            assert L.jaero_debug_burst_poke_cv(h, ch, 0, n, big.ctypes.data) == capi.E_INVAL, (ch, n)
        assert L.jaero_debug_burst_poke_cv(h, 0, 0, 1, None) == capi.E_INVAL
        b.bank.write(pcm)  # refused before anything was marked
        for chans, evs, n0, grid in (([0, 0], [0, 0], 0, 0), ([5], [0], 0, 0), ([-1], [0], 0, 0), ([0], [g.maxseg], 0, 0), ([0], [-1], 0, 0),
                                     ([0], [0], -1, 0), ([0], [0], 0, g.tri_grid + 1), ([0], [0], 0, -1), ([0, 1, 2, 3, 4, 0], [0] * 6, 0, 0)):
            assert b.trident_rc(chans, evs, n0, grid)[0] == capi.E_INVAL, (chans, evs, n0, grid)
        assert L.jaero_debug_burst_trident(h, None, None, 1, 0, 0, None, None) == capi.E_INVAL
        b.bank.write(pcm)  # refused before anything was marked
        assert b.trident([], [], 0, 0) == ([], 0)
        assert L.jaero_write(h, pcm.ctypes.data, 64, 0, 0, None) == capi.E_HIP
        assert L.jaero_set_flags(h, -1, 1, 0, 0) == capi.E_HIP
        assert b.geom().nsamples == 4 * 64 and np.array_equal(b.read_hist(0, 0, 256), np.zeros(256, dtype=np.int16))  # the readers go on working
    finally:
        b.close()
    for mark in ("hilbert", "poke_cv"):
        b = AcqBank("msk1200", 3)
        try:
            pcm = np.zeros((3, 64), dtype=np.int16)
            if mark == "hilbert":
                b.hilbert(pcm, CHANNEL_MAJOR)
            else:
                b.poke_cv(2, -5, np.ones(10))
            assert L.jaero_write(b.h, pcm.ctypes.data, 64, 0, 0, None) == capi.E_HIP, mark
            st = D.BurstMskSettings(fb=1200.0).to_c()
            assert L.jaero_set_settings(b.h, -1, C.byref(st)) == capi.E_HIP, mark
        finally:
            b.close()
