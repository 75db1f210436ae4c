"""Shared by tests/test_burst_front_cases.py (CPU) and tests/test_gpu_burst_front.py (GPU): configurations, cases, references and checkers for the
per-sample detector of the burst banks, k_burst_front<false / true> with k_ev_compact behind it (jaero_amd/csrc/k_burst_front.h;
JAERO/burstoqpskdemodulator.cpp:372-410,439-441 == JAERO/burstmskdemodulator.cpp:413-441, JAERO/DSP.h:491-576 PeakDetector).  No GPU code here.

Three things are compared.
  candidate  what is under test: the kernel's rings, scalars, event positions and lists; in the CPU test a numpy restatement of the detector
             (numpy_peakdet) or a deliberately wrong copy of it
  oracle     jo_burst_front_write (burst_front_end and the fire / tridentbuffer_ptr lines of boqpsk_write / bmsk_write on an ordinary jo_burst,
             the functions tests/test_oracle_vs_ref.py pins to the unmodified reference) and jo_peakdet_run (peakdet_update on given state)
  exact      jo_burst_front_exact: the same recurrence in long double, with every decision's clearance measured

A. The peak detector on poked state (scenarios, expected, check_scenario_step).  A fresh bank fed all-zero PCM and all-zero imaginary parts
   computes bt_sig = 0 exactly on every sample (a = hypot(-0, 0) = 0, the AGC gain is finite, every product and sum is 0, fastarm = 0 - 0), so the
   detector walks over what the test poked into its ring of the last 2 PL + 1 values and EVERY decision is exact: fire samples, cntdown, maxposcd,
   lastdy, tri_ptr, BI_EV_POS, the event list and its count and the PEAK rows of the event log must equal what jo_peakdet_run and the four
   tri_ptr lines (restated in expected()) give on the same history.  No tolerance anywhere.
   A history is indexed oldest first: entry j is sample N - (2 PL + 1) + j when poked at sample count N.  `t` samples later (sample index t behind
   the poke) the scan window's entry q is history[t + 1 + q] (zeros beyond the history), dy = 0 - history[t + 1] and vald = history[t + 1 + PL].  A
   trigger on sample t therefore needs history[t + 1] > 0 (dy < 0; this is the window's entry q = 0), history[t] == 0 for t > 0 (lastdy >= 0; on
   t = 0 the poked lastdy decides), history[t + 1 + PL] > pd_thr and cntdown == 0.  Consequences the case list lives with:
     - only samples t < PL behind a poke can trigger (vald has to come from the history), so of the issue's trigger positions 0, 7, 8, n - 1 for
       n = 1, 7, 9, 1001, maxseg those with index < PL are run: all for burst MSK 600 (PL 6000), all but 4095 for burst MSK 1200 (PL 2520), all but
       1000 and 2047 for burst OQPSK (PL 585).  A later peak needs a second poke (the lock-out case does that);
     - a maximum at q needs t + 1 + q <= 2 PL: q = 2 PL - 1 is reachable on t = 0 only, q = 2 PL never.  Nor can it be in a stream: a trigger has
       dy < 0, that is window[2 PL] < window[0], so the entry written on the trigger sample NEVER wins a search, and lastdy >= 0 says the value that
       entry's slot held before (sample k - 2 PL - 1) is <= window[2 PL - 1], so a stale read could at most tie.  What CAN show that the search reads
       the entry stored on this sample and not what the slot held before is the poked state: every case that triggers on t = 0 puts POISON = 1e6
       into history[0], the value the new entry overwrites.  A search that read the slot before its store would return maxpos = 2 PL there.  That
       replaces the streaming case with a maximum at 2 PL or 2 PL - 1 the issue asks to look for: there is none to find (test_burst_front_cases
       asserts that no trigger of the streaming draws has its maximum at q >= 2 PL - 1).

B. Values, streaming (stream_case, population, check_stream).  Per-channel analytic input: re = -pcm[m - hil_lat - 1024] / 32768 (int16 PCM pushed
   into the history ring), im through the hook's override.  The five observed channels carry: bursts of a full-scale complex tone in noise, the
   same at -40 dB, exact zeros followed by a tone, the two int16 extremes at random, and a REAL-ONLY signal (im = 0 exactly).  Other channels
   repeat them.  The stream passes agc_len + 2 ma1_len samples; segments are cut at 1, 7, 1000, maxseg - 1, maxseg in rotation.
   tolerance  E_o[column] = the oracle's double run against the exact run, largest over the configuration's NDRAWS accepted draws and the five
             channels, each relative to the column's largest magnitude in that channel's run.  The kernel's error in the same units must be
             <= 4 E_o + 4 * 2^-52 (the form of burst_acq_cases): it repeats the reference's operation order, so its error is of the oracle's size;
             hypot differs by an ulp in 14.5 % of the calls (jd_libm.h), and the two Delay<> weights are one constant each in the kernel where the
             oracle re-derives them from the buffer pointer on every sample (ulp(1172) on 0.71 for bt_ma_diff: the oracle's own error is the larger).
   bit-exact  the real-only channel: hypot(x, 0) = sqrt(x * x) = |x| exactly in binary floating point, and every other operation of the front end
             is one correctly rounded IEEE operation (-ffp-contract=off) in the reference's order.  So agc_ring, agc_sum, cvre and cvim must equal
             the oracle's bit for bit in every configuration, and with burst MSK's whole-sample delays (both weights exactly 0, the delayed value
             is a copy) every other ring and sum too.  This is the check a fused multiply-add, a reordered sum or `* (1 / len)` for `/ len` fails.
   decisions  fires, tri_ptr, BI_EV_POS, the event list: equal to the oracle's outright.  A draw counts only if the exact run's smallest
             clearance is above MARGIN = 1e-9 relative: the two clamps (fastarm < 0, bt_sig > 500) on every sample, the three trigger terms on
             every sample with cntdown == 0, every findmaxpos winner over its runner-up; terms whose operands are all exactly 0 or 500 are decided
             on both sides and do not enter (jaero_oracle_burst.c: jo_burst_front_exact).  At most 1 draw in 10 may be rejected.

D. k_ev_compact alone (ev_masks, ev_expected): numpy's ascending enumeration of the set bits and their count.
Every module prints its errors in units of 2^-52 before it asserts."""
import math
from types import SimpleNamespace

import numpy as np

import burst_acq_cases as BC

EPS = BC.EPS
MARGIN = 1e-9
POISON = 1.0e6
FS = BC.FS
CONFIGS = BC.CONFIGS
HIL_SHIFT = BC.HIL_LAT + 1024  # re of sample m is -pcm[m - HIL_SHIFT] / 32768
NDRAWS = 2  # accepted streaming draws per configuration
RINGS = ("agc_ring", "cvre", "cvim", "ma1re", "ma1im", "mav1", "fa", "bt")  # the peek's rings -> the oracle's columns
RING_COL = {"agc_ring": "agc_ring", "cvre": "cre", "cvim": "cim", "ma1re": "ma1re", "ma1im": "ma1im", "mav1": "mav1", "fa": "fa", "bt": "bt"}
SUMS = ("agc_sum", "ma1_re", "ma1_im", "mav1_sum")
EV_NGROUPS = [1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 3000]


def chans(nch):
    return [0, 1, 63, 64, nch - 1]


def geometry(cfg):
    """The detector's lengths as the two setSettings give them at 48 kHz, restated (burst_fill_geometry); jaero_debug_burst_front_geom and the
    oracle's jo_burst_front_geom must both agree"""
    mult = 128.0 if cfg.oq else (126.0 if cfg.fb >= 1200 else 150.0)
    sps = cfg.sps
    PL = int(sps * mult / 2.0)
    fa_lag = int(math.ceil(sps * mult))
    return SimpleNamespace(PL=PL, bt_len=2 * PL + 1, bt_lag=int(math.ceil(sps)), agc_len=48000, ma1_len=BC.qround(mult * sps), mav1_len=int(sps * mult),
                           fa_lag=fa_lag, fa_len=fa_lag + 1, pd_thr=0.1 if (not cfg.oq and cfg.fb >= 1200) else 0.2, tri_sz=cfg.tri_sz, maxseg=cfg.maxseg,
                           cv_len=cfg.D1 + max(cfg.D2, cfg.tri_sz) + cfg.maxseg + 64)


def oracle_settings(O, cfg):
    return O.burst_oqpsk_settings() if cfg.oq else O.burst_msk_settings(fb=cfg.fb)


def ring_len(g, ring):
    return {"agc_ring": g.agc_len, "cvre": g.cv_len, "cvim": g.cv_len, "ma1re": g.ma1_len, "ma1im": g.ma1_len, "mav1": g.mav1_len, "fa": g.fa_len, "bt": g.bt_len}[ring]


# ----------------------------------------------------------------------------------------------- A: the peak detector on poked state
def history(g, t, vals=(), vald=None, base=1.0e-3, poison=True):
    """A history that makes sample t behind the poke a trigger candidate: window entry q = 0 (history[t + 1]) = base > 0, vald (history[t + 1 + PL])
    = 1.5 pd_thr unless given, window entries {q: v} from vals, everything else 0; on t = 0 the slot the new entry overwrites is poisoned."""
    h = np.zeros(g.bt_len)
    h[t + 1] = base
    h[t + 1 + g.PL] = 1.5 * g.pd_thr if vald is None else vald
    for q, v in vals:
        assert 0 <= q and t + 1 + q <= 2 * g.PL, (t, q)
        h[t + 1 + q] = v
    if t == 0 and poison:
        h[0] = POISON
    return h


def plateau(q0, length, height=500.0):
    return [(q, height) for q in range(q0, q0 + length)]


def case(label, hist, trig=None, maxpos=None, cntdown=0, lastdy=0.0, maxposcd=-1, tri_ptr=None):
    """trig: the samples behind the poke on which the oracle must report a trigger (coverage, asserted on the CPU); maxpos: their winners"""
    return SimpleNamespace(label=label, hist=hist, cntdown=cntdown, lastdy=lastdy, maxposcd=maxposcd, tri_ptr=tri_ptr,
                           trig=None if trig is None else list(np.atleast_1d(trig)), maxpos=None if maxpos is None else list(np.atleast_1d(maxpos)))


def _segs(g, total):
    out = []
    while total > 0:
        out.append(min(total, g.maxseg))
        total -= out[-1]
    return out


def scenarios(name):
    """The launches of part A for one configuration: a list of namespaces (label, nch, phases); a phase = (pokes {channel: case}, segment lengths).
    Channels not poked in a phase keep their state.  Phase 0 of a scenario with n0 > 0 only advances the bank (zeros, no pokes)."""
    cfg = CONFIGS[name]
    g = geometry(cfg)
    PL, M, thr = g.PL, g.maxseg, g.pd_thr
    rng = np.random.default_rng(0xF407 + sum(map(ord, name)))
    out = []

    def scen(label, nch, phases, n0=0):
        ph = ([({}, _segs(g, n0))] if n0 else []) + phases
        out.append(SimpleNamespace(label=label, nch=nch, phases=ph, cfg=cfg, g=g))

    c5 = chans(70)
    # plateaus of 500s from q = 0, 1, 63, 64, 65 on a trigger on sample 0; the fire falls into a later segment for q >= 9 (maxposcd carried)
    starts = [0, 1, 63, 64, 65]
    scen("plateaus from q = 0, 1, 63, 64, 65", 70,
         [({ch: case(f"plateau from q = {q}", history(g, 0, plateau(q, 200)), 0, q) for ch, q in zip(c5, starts)}, [9, 1001, M])])
    # plateau from 2 PL - 1 (one entry: the newest of the history), two plateaus of equal height, unique maxima at q = 0, at a random q and at the last
    # reachable one; vald stays below the maxima
    qr = int(rng.integers(70, 2 * PL - 2))
    scen("plateau at 2 PL - 1, two plateaus, unique maxima", 67,
         [({0: case("plateau from q = 2 PL - 1", history(g, 0, plateau(2 * PL - 1, 1)), 0, 2 * PL - 1),
            1: case("two plateaus of 500 from q = 130 and q = 300", history(g, 0, plateau(130, 40) + plateau(300, 40)), 0, 130),
            63: case("unique maximum at q = 0 (fire on the trigger sample)", history(g, 0, [(5, 0.5), (77, 0.7)], base=0.9), 0, 0),
            64: case(f"unique maximum at q = {qr}", history(g, 0, [(qr, 7.25), (qr - 64, 7.0), (qr + 1, 7.0)]), 0, qr),
            66: case("unique maximum at q = 2 PL - 1", history(g, 0, [(2 * PL - 1, 3.0), (2 * PL - 2, 2.5)]), 0, 2 * PL - 1)}, [1, 7, M])])
    # threshold and slope
    up = float(np.nextafter(thr, 1.0))
    scen("threshold and slope", 70,
         [({0: case("vald == pd_thr exactly: no trigger", history(g, 0, [(9, 2.0)], vald=thr), []),
            1: case("vald one ulp above pd_thr: trigger", history(g, 0, [(9, 2.0)], vald=up), 0, 9),
            63: case("lastdy == 0 exactly and dy < 0: trigger (on sample 7)", history(g, 7, [(9, 2.0)]), 7, 9),
            64: case("dy == 0 exactly: no trigger", history(g, 0, [(9, 2.0)], base=0.0), []),
            69: case("lastdy < 0 on sample 0: no trigger", history(g, 0, [(9, 2.0)]), [], lastdy=-1.0e-300)}, [9, 1001])])
    # cntdown 1 and 0 on the sample the other terms first hold (sample 3: poked 4 and 3); cntdown 1 is 0 one sample later, when lastdy < 0 refuses; a second edge two samples on is taken
    two = history(g, 3, [(40, 2.0)])
    two[3 + 2] = 0.0; two[3 + 3] = 1.0e-3; two[3 + 3 + PL] = 1.5 * thr
    scen("cntdown", 67,
         [({0: case("cntdown == 1 where the terms first hold: ignored", history(g, 3, [(40, 2.0)]), [], cntdown=4),
            1: case("cntdown == 0 where the terms first hold", history(g, 3, [(40, 2.0)]), 3, 40, cntdown=3),
            63: case("cntdown == 1 on the first edge, 0 on a second edge two samples on", two.copy(), 5, 38, cntdown=4),
            64: case("cntdown == 2 PL: nothing in this history is taken", history(g, 3, [(40, 2.0)]), [], cntdown=2 * PL),
            66: case("maxposcd poked to 5 without a trigger: fire on sample 5", np.zeros(g.bt_len), [], maxposcd=5)}, [7, 9, 1001])])
    # a second peak inside the 2 PL lock-out is ignored, one just behind it is taken: a second poke of the ring 2 PL - 5 samples on, cntdown left alone
    h1 = history(g, 0, [(3, 2.0)])
    h1[100] = 0.0; h1[101] = 1.0e-3; h1[101 + PL] = 1.5 * thr  # an edge on sample 100, cntdown 2 PL - 100
    h2 = np.zeros(g.bt_len)
    for t in (3, 5):  # cntdown is 2 on sample 3 behind the second poke and 0 on sample 5
        h2[t] = 0.0; h2[t + 1] = 1.0e-3; h2[t + 1 + PL] = 1.5 * thr
    h2[5 + 1 + 20] = 4.0
    scen("lock-out", 70,
         [({c: case("peak on sample 0, another on sample 100 inside the lock-out", h1.copy(), 0, 3) for c in (1, 64)}, _segs(g, 2 * PL - 5)),
          ({c: SimpleNamespace(label="edges 2 samples before the lock-out ends and on its end", hist=h2.copy(), cntdown=None, lastdy=None, maxposcd=None, tri_ptr=None,
                               trig=[5], maxpos=[20]) for c in (1, 64)}, [9, 1001])])
    # the trigger's index in its segment: 0, 7, 8, n - 1 of n = 1, 7, 9, 1001, maxseg (those < PL), each in a segment of that length right behind the poke
    idx = sorted({i for n in (1, 7, 9, 1001, M) for i in (0, 7, 8, n - 1) if i < n and i < PL})
    for n in (1, 7, 9, 1001, M):
        mine = [i for i in idx if i < n][-5:] if n > 9 else [i for i in idx if i < n]
        mine = sorted(set(mine) | ({n - 1} if n - 1 < PL else set()))[-5:]
        pokes = {ch: case(f"trigger on sample {i} of a segment of {n}", history(g, i, [(11 + 3 * k, 2.0)]), i, 11 + 3 * k) for k, (ch, i) in enumerate(zip(c5, mine))}
        scen(f"trigger index in a segment of {n}", 70, [(pokes, [n, 9, M])])
    # all 64 lanes of group 0 on the same sample with 64 histories: lane r's plateau starts at a q with q mod 64 == r (the first 500 in every lane of the
    # strided scan, in strides 1 .. 8); lane 0 of group 1 triggers on that sample too, channel 69 two samples later
    t0 = 3
    pokes = {}
    for r in range(64):
        q = 64 * int(rng.integers(1, 9)) + r
        pokes[r] = case(f"lane {r}: plateau from q = {q}", history(g, t0, plateau(q, 130)), t0, q)
    pokes[64] = case("lane 0 of group 1 on the same sample", history(g, t0, plateau(77, 3)), t0, 77)
    pokes[69] = case("lane 5 of group 1 two samples later", history(g, t0 + 2, [(12, 9.0)]), t0 + 2, 12)
    scen("64 lanes on one sample", 70, [(pokes, [7, 9, 1001])])
    # 3 lanes of group 0 and 2 of group 1 on different samples of one block of 8 (samples 8 .. 15 of a segment of 1001), lane 63 and lane 0 of the next group
    # on the same one
    scen("several lanes in one block of 8", 67,
         [({0: case("sample 9", history(g, 9, [(30, 2.0)]), 9, 30), 1: case("sample 12", history(g, 12, plateau(64, 64)), 12, 64),
            63: case("sample 15", history(g, 15, [(2, 2.0)]), 15, 2), 64: case("sample 15, lane 0 of group 1", history(g, 15, [(127, 2.0)]), 15, 127),
            66: case("sample 10", history(g, 10, plateau(1, 500)), 10, 1)}, [1001, 9])])
    # tri_ptr reaches tri_sz on the first and on the last sample of a segment; a fire on the same segment's first sample restarts the fill; a padding
    # channel poked to fill never reaches the list
    n = 1001
    z = np.zeros(g.bt_len)
    scen("trident fill", 67,
         [({0: case("fills on the first sample", z, [], tri_ptr=g.tri_sz), 1: case("fills on the last sample", z, [], tri_ptr=g.tri_sz - (n - 1)),
            63: case("would fill on sample 3, fires on sample 0", z, [], tri_ptr=g.tri_sz - 3, maxposcd=0), 64: case("fills on sample 3", z, [], tri_ptr=g.tri_sz - 3),
            66: case("fills one sample behind the segment", z, [], tri_ptr=g.tri_sz - n),
            68: case("padding lane: fills on sample 0 and fires on sample 2", z, [], tri_ptr=g.tri_sz, maxposcd=2)}, [n, 1, 7])])
    # the ring's slot 0 at q = 0, in the middle and at q = 2 PL of the scan window (sample a lives at slot a mod bt_len; the trigger is on sample n0)
    for where, k in (("q = 0", 2 * PL), ("the middle", PL), ("q = 2 PL", 0)):
        n0 = g.bt_len + k
        assert (n0 - 2 * PL + {"q = 0": 0, "the middle": PL, "q = 2 PL": 2 * PL}[where]) % g.bt_len == 0
        scen(f"ring wrap: slot 0 at {where}", 70,
             [({ch: case(f"plateau from q = {q}", history(g, 0, plateau(q, min(3, 2 * PL - q))), 0, q) for ch, q in zip(c5, (1, PL - 1, PL + 1, 2 * PL - 2, 2 * PL - 1))}, [9, M])], n0=n0)
    return out


def fresh_state(g):
    return SimpleNamespace(hist=np.zeros(g.bt_len), cntdown=2 * g.PL, lastdy=0.0, maxposcd=-1, tri_ptr=0)


def expected(O, sc, detector=None):
    """What every channel of a scenario must show behind every segment: a list over phases of lists over segments of namespaces (n0, n, st {channel:
    state}, ev_pos [nchp], ev_list, fires {channel: absolute samples}, trig {channel: [(sample behind the phase's poke, maxpos)]}).  Channels without a
    poke anywhere share the fresh channel's track.  detector: jo_peakdet_run unless a candidate is given (CPU test)."""
    g = sc.g
    det = detector or (lambda h, cd, ldy, mp, n: O.peakdet_run(g.PL, g.pd_thr, h, cd, ldy, mp, np.zeros(n)))
    nchp = (sc.nch + 63) // 64 * 64
    poked = sorted({ch for pokes, _ in sc.phases for ch in pokes})
    st = {ch: fresh_state(g) for ch in poked + [-1]}  # -1: every other channel
    pos, out = 0, []
    for pokes, segs in sc.phases:
        for ch, c in pokes.items():
            s = st[ch]
            s.hist = c.hist.copy()
            for f in ("cntdown", "lastdy", "maxposcd", "tri_ptr"):
                if getattr(c, f) is not None:
                    setattr(s, f, getattr(c, f))
        rel, phase = 0, []
        for n in segs:
            e = SimpleNamespace(n0=pos, n=n, st={}, ev_pos=np.full(nchp, -1, dtype=np.int64), fires={}, trig={})
            for ch, s in st.items():
                fire, mp, (s.cntdown, s.lastdy, s.maxposcd) = det(s.hist, s.cntdown, s.lastdy, s.maxposcd, n)
                s.hist = np.concatenate([s.hist, np.zeros(n)])[-g.bt_len:]
                evp = -1
                for i in range(n):  # boqpsk_write :439-441 == bmsk_write :788-790
                    if fire[i]:
                        s.tri_ptr = 0
                    if s.tri_ptr < g.tri_sz:
                        s.tri_ptr += 1
                    elif s.tri_ptr == g.tri_sz:
                        s.tri_ptr += 1
                        evp = i
                who = [ch] if ch >= 0 else [c for c in range(nchp) if c not in st]
                for c in who:
                    e.ev_pos[c] = evp
                    e.st[c] = SimpleNamespace(cntdown=s.cntdown, lastdy=s.lastdy, maxposcd=s.maxposcd, tri_ptr=s.tri_ptr)
                e.fires[ch] = [pos + int(i) for i in np.flatnonzero(fire)]
                e.trig[ch] = [(rel + int(i), int(mp[i])) for i in np.flatnonzero(mp >= 0)]
            e.ev_list = [c for c in range(sc.nch) if e.ev_pos[c] >= 0]
            phase.append(e)
            pos += n
            rel += n
        out.append(phase)
    return out


def check_coverage(sc, exp):
    """The oracle reports the triggers and winners every case was built for (a case whose construction is wrong would still pass the comparison)"""
    for (pokes, _), phase in zip(sc.phases, exp):
        for ch, c in pokes.items():
            if c.trig is None:
                continue
            got = [tm for e in phase for tm in e.trig[ch]]
            want = list(zip(c.trig, c.maxpos)) if c.trig else []
            assert got == want, (sc.cfg.name, sc.label, ch, c.label, "oracle's (trigger, maxpos)", got, "built for", want)


def numpy_peakdet(g, wrong=None):
    """PeakDetector::update restated in numpy on an explicit window, as a candidate for expected(); wrong: "last_max" (ties go to the last entry),
    "lane_order" (ties go to the lowest lane of a 64-strided scan, then the lowest stride: the shuffle reduction without its `oq < bq` term),
    "stale" (the scan reads what the newest entry's slot held before the store), "ge_thr" (vald >= threshold)."""
    L2 = 2 * g.PL

    def det(h, cntdown, lastdy, maxposcd, n):
        buf = np.concatenate([h, np.zeros(n)])
        fire, mp = np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int32)
        for i in range(n):
            k = len(h) + i
            dy, vald = buf[k] - buf[k - L2], buf[k - g.PL]
            if cntdown == 0 and (vald >= g.pd_thr if wrong == "ge_thr" else vald > g.pd_thr) and lastdy >= 0 and dy < 0:
                w = buf[k - L2:k + 1].copy()
                if wrong == "stale":
                    w[L2] = buf[k - L2 - 1]
                eq = np.flatnonzero(w == w.max())
                q = int(eq[-1]) if wrong == "last_max" else int(min(eq, key=lambda x: (x % 64, x))) if wrong == "lane_order" else int(eq[0])
                cntdown, maxposcd, mp[i] = L2, q, q
            if cntdown > 0:
                cntdown -= 1
            lastdy = dy
            if maxposcd == 0:
                maxposcd, fire[i] = -1, 1
            elif maxposcd > 0:
                maxposcd -= 1
        return fire, mp, (cntdown, float(lastdy), maxposcd)
    return det


def check_scenario_step(sc, e, got_st, ev_pos, ev_list, ev_count, what=""):
    """One segment of a scenario: got_st {channel: the peek's scalars}, ev_pos [nch], ev_list, ev_count from the front hook.  Everything equal."""
    w = (sc.cfg.name, sc.label, f"segment of {e.n} from sample {e.n0}", what)
    assert ev_count == len(e.ev_list) and list(ev_list[:ev_count]) == e.ev_list, w + ("event list", list(ev_list[:ev_count]), "expected", e.ev_list)
    assert np.array_equal(np.asarray(ev_pos), e.ev_pos[:sc.nch]), w + ("BI_EV_POS", [(c, int(a), int(b)) for c, (a, b) in enumerate(zip(ev_pos, e.ev_pos)) if a != b][:8])
    for ch, s in got_st.items():
        x = e.st[ch]
        got = (s.cntdown, s.maxposcd, s.tri_ptr, np.float64(s.lastdy).view(np.uint64))
        want = (x.cntdown, x.maxposcd, x.tri_ptr, np.float64(x.lastdy).view(np.uint64))
        assert got == want, w + (f"channel {ch}: (cntdown, maxposcd, tri_ptr, lastdy bits)", got, "expected", want)
        assert s.ev_pos == e.ev_pos[ch], w + (f"channel {ch} BI_EV_POS", s.ev_pos, e.ev_pos[ch])


# ----------------------------------------------------------------------------------------------- B: streams
def seg_plan(g, total):
    cyc, out = [1, 7, 1000, g.maxseg - 1, g.maxseg], []
    while sum(out) < total:
        out.append(cyc[len(out) % len(cyc)])
    return out


def _bursts(rng, n, g, level, sigma):
    """A complex tone in bursts over a noise floor: one burst while the AGC window still fills, one behind agc_len"""
    t = np.arange(n)
    z = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    L = g.ma1_len
    for s in (int(rng.integers(8000, 12000)), g.agc_len + int(rng.integers(200, 600))):
        e = min(n, s + int(L * rng.uniform(1.2, 1.6)))
        f = rng.uniform(0.02, 0.2)
        z[s:e] += level * np.exp(1j * (2 * np.pi * f * t[s:e] + rng.uniform(0, 2 * np.pi)))
    return z


def stream_case(name, nch, seed):
    """One draw: (segment lengths, pcm int16 [nch][n], im [nch][n], z {observed channel: the analytic samples the kernel sees})"""
    cfg = CONFIGS[name]
    g = geometry(cfg)
    segs = seg_plan(g, g.agc_len + 2 * g.ma1_len + 64)
    n = sum(segs)
    rng = np.random.default_rng(seed)
    want = []
    want.append(_bursts(rng, n, g, 0.6, 0.02))
    want.append(_bursts(rng, n, g, 0.006, 0.0003))
    zt = np.zeros(n, dtype=complex)
    s0 = HIL_SHIFT + int(rng.integers(1500, 2500))
    zt[s0:] = 0.3 * np.exp(1j * (2 * np.pi * 0.11 * np.arange(n - s0)))
    want.append(zt)
    want.append(rng.choice([1.0, -32767.0 / 32768.0], n) + 1j * rng.choice([-32767.0 / 32768.0, 32767.0 / 32768.0], n))
    want.append(_bursts(rng, n, g, 0.5, 0.01).real.astype(complex))
    base_pcm, base_im = [], []
    for k, z in enumerate(want):
        r = np.clip(np.rint(z.real * 32768.0), -32767, 32768)  # re = -pcm / 32768: pcm = -r in [-32768, 32767]
        pcm = np.zeros(n, dtype=np.int16)
        pcm[:n - HIL_SHIFT] = (-r[HIL_SHIFT:]).astype(np.int16)
        base_pcm.append(pcm)
        base_im.append(np.ascontiguousarray(z.imag))
    assert base_pcm[3].min() == -32768 and base_pcm[3].max() == 32767
    obs = chans(nch)
    kind = lambda ch: obs.index(ch) if ch in obs else ch % 5
    pcm = np.stack([base_pcm[kind(ch)] for ch in range(nch)])
    im = np.stack([base_im[kind(ch)] for ch in range(nch)])
    z = {}
    for ch in obs:
        re = np.zeros(n)
        re[HIL_SHIFT:] = pcm[ch, :n - HIL_SHIFT].astype(np.float64) / 32768.0
        z[ch] = -re + 1j * im[ch]
    return SimpleNamespace(cfg=cfg, g=g, segs=segs, n=n, pcm=pcm, im=im, z=z, seed=seed, nch=nch, obs=obs, kind=[kind(ch) for ch in range(nch)])


def run_oracle(O, sc):
    """The oracle's double run and the exact run of the observed channels: rows {ch: [n][cols]}, exact {ch: long double}, margin, triggers"""
    sc.rows, sc.exact, sc.trig, sc.margin = {}, {}, {}, 1.0
    for ch, z in sc.z.items():
        d = O.BurstDemod(oracle_settings(O, sc.cfg))
        sc.rows[ch] = d.front_write(z)
        sc.final = getattr(sc, "final", {})
        sc.final[ch] = d.front_state()
        sc.exact[ch], m, sc.trig[ch], _ = d.front_exact(z)
        sc.margin = min(sc.margin, m)
    sc.cols = {c: i for i, c in enumerate(O.BurstDemod.FRONT_COLS)}
    return sc


def oracle_errors(sc):
    """{column: the oracle's largest error over the observed channels, relative to the column's largest exact magnitude in the channel's run}"""
    E = {}
    for c in [RING_COL[r] for r in RINGS] + list(SUMS):
        i, worst = sc.cols[c], 0.0
        for ch in sc.z:
            ex = sc.exact[ch][:, i]
            scale = float(np.abs(ex).max())
            if scale > 0:
                worst = max(worst, float(np.abs(sc.rows[ch][:, i].astype(BC.LD) - ex).max()) / scale)
        E[c] = worst
    return E


def tri_ptr_series(g, fire):
    """tridentbuffer_ptr behind every sample of a fresh channel's stream, from its fire column (boqpsk_write :439-441): samples since the last
    fire, that sample counted, capped at tri_sz + 1"""
    k = np.arange(len(fire))
    last = np.maximum.accumulate(np.where(fire != 0, k, -1))
    return np.minimum(np.where(last >= 0, k - last + 1, k + 1), g.tri_sz + 1)


_pop = {}


def population(O, name, nch=70, seed=0xB0B):
    """NDRAWS accepted draws of a configuration with the oracle's and the exact run: (draws, E_o per column, rejected).  At most 1 draw in 10
    may be rejected."""
    key = (name, nch, seed)
    if key not in _pop:
        draws, rejected, k = [], 0, 0
        while len(draws) < NDRAWS:
            sc = run_oracle(O, stream_case(name, nch, seed + 1000 * sum(map(ord, name)) + k))
            k += 1
            if sc.margin > MARGIN:
                draws.append(sc)
            else:
                rejected += 1
            assert rejected * 10 <= max(10, len(draws) + rejected), (name, f"{rejected} draws rejected among {len(draws) + rejected}")
        E = {}
        for sc in draws:
            for c, e in oracle_errors(sc).items():
                E[c] = max(E.get(c, 0.0), e)
        print(f"burst_front {name}: {NDRAWS} draws accepted, {rejected} rejected, smallest decision clearance {min(sc.margin for sc in draws):.2e}, "
              f"triggers per channel {[len(t) for sc in draws for t in sc.trig.values()]}; oracle's worst errors in eps: " + ", ".join(f"{c} {e / EPS:.2f}" for c, e in E.items()))
        _pop[key] = (draws, E, rejected)
    return _pop[key]


def bit_exact_columns(cfg):
    """The real-only channel's columns that must equal the oracle's bit for bit (module docstring)"""
    return ["agc_ring", "cre", "cim", "agc_sum"] + ([] if cfg.oq else ["ma1re", "ma1im", "mav1", "fa", "bt", "ma1_re", "ma1_im", "mav1_sum"])


def check_stream(sc, E, ch, series, what=""):
    """series {column: [n] values of the candidate, NaN where a ring entry was overwritten before it could be read}: the rules of part B for one
    observed channel.  Returns {column: the candidate's error}."""
    w = (sc.cfg.name, f"seed {sc.seed}", f"channel {ch}", what)
    errs = {}
    for c, v in series.items():
        i = sc.cols[c]
        ex, orc = sc.exact[ch][:, i], sc.rows[ch][:, i]
        seen = ~np.isnan(v)
        assert seen.any(), w + (c,)
        scale = float(np.abs(ex).max())
        if scale == 0.0:
            assert not v[seen].any(), w + (c, "must be exactly zero")
            errs[c] = 0.0
            continue
        e = float(np.abs(v[seen].astype(BC.LD) - ex[seen]).max()) / scale
        errs[c] = e
        assert e <= 4 * E[c] + 4 * EPS, w + (f"{c}: candidate {e / EPS:.2f} eps, oracle's worst {E[c] / EPS:.2f} eps, allowed {(4 * E[c] + 4 * EPS) / EPS:.2f}",)
        if ch == chans(sc.nch)[4] and c in bit_exact_columns(sc.cfg):
            bad = np.flatnonzero(seen & (v.view(np.uint64) != orc.view(np.uint64)) & ~((v == 0) & (orc == 0)))
            assert len(bad) == 0, w + (f"{c}: the real-only channel differs from the oracle's bits on {len(bad)} samples, first {bad[:3]}: {v[bad[:3]]} against {orc[bad[:3]]}",)
    return errs


# ----------------------------------------------------------------------------------------------- D: k_ev_compact alone
def ev_masks(ngroups, rng):
    def one(g, b):
        m = np.zeros(ngroups, dtype=np.uint64)
        m[g] = np.uint64(1) << np.uint64(b)
        return m

    return [("all zero", np.zeros(ngroups, dtype=np.uint64)), ("all ones", np.full(ngroups, ~np.uint64(0), dtype=np.uint64)),
            ("bit 0 only", np.full(ngroups, np.uint64(1), dtype=np.uint64)), ("bit 63 only", np.full(ngroups, np.uint64(1) << np.uint64(63), dtype=np.uint64)),
            ("a single bit in the last group", one(ngroups - 1, int(rng.integers(0, 64)))),
            ("random, density 1/64", np.packbits(rng.random((ngroups, 64)) < 1 / 64, axis=1, bitorder="little").view(np.uint64).ravel()),
            ("random, density 1/2", np.packbits(rng.random((ngroups, 64)) < 0.5, axis=1, bitorder="little").view(np.uint64).ravel())]


def ev_expected(mask):
    bits = np.unpackbits(mask.view(np.uint8), bitorder="little")  # bit l of mask[g] is channel 64 g + l (little-endian words)
    return np.flatnonzero(bits).astype(np.int32)
