"""Shared by tests/test_burst_track_cases.py (CPU) and tests/test_gpu_burst_track.py (GPU): configurations, cases, references and checkers for the
tracking chains of the burst banks, k_burst_oqpsk_demod<CAPSYM> (jaero_amd/csrc/k_burst_demod.h; JAERO/burstoqpskdemodulator.cpp:488-733) and
k_burst_msk_fb<CAPSYM, FIRN, LDSN> (jaero_amd/csrc/k_burst_msk_fb.h; JAERO/burstmskdemodulator.cpp:524-745).  No GPU code here.

  candidate  what is under test: the kernel behind jaero_debug_burst_track (one segment per launch, verdicts and input the test supplies); in the
             CPU test the oracle itself under another segmentation
  oracle     jo_burst_track_write: boqpsk_track_sample / bmsk_track_sample and the *_trident_apply functions, the very functions boqpsk_write /
             bmsk_write call (tests/test_oracle_vs_ref.py pins those to the unmodified reference; test_burst_track_cases pins the split once more
             by record and replay)

A case is a bank of NCH = 70 channels (two wavefronts, the second with 58 padding lanes) with max_write_samples = MAX_WRITE, so that maxseg is the
write size.  It lists WRITES (each a list of segment lengths: the first segment of a write runs with first_of_write = 1), per-channel verdicts by
absolute sample, and per-channel input (None: +0.0 everywhere).  The oracle runs one jo_burst_track_write per write (lastmse is taken once per
write), so a case never puts two verdicts of one channel into one write.

A. Bookkeeping on all-zero input: exact (check_exact).  Every product and sum of the chain is zero, symbol instants fall where the free-running
   symbol oscillator puts them, every soft byte behind an accepting verdict is 128 (burst MSK: what DiffDecode makes of zeros), the mean-square-error
   window fills with 2.0 and the time-out fires where the integers decide.  Event rows (sample, kind, value), the whole soft row with the sentinel
   behind its count, symbol rows, overflow and every integer of the peek must equal the oracle's, behind every write.
B. Values on real bursts (check_values): input and verdicts recorded from the oracle's ordinary run on signalgen bursts (stream_case).  Exact:
   markers, hard decisions, event kinds and stamps, counts and integers; soft bytes within 1 in at most BURST_SOFT_ALLOW bytes; event values within
   1e-6 relative; symbols within min(SYM_TOL, E_n), E_n being the oracle's own symbol deviation under additive white noise of 1e-9 of the stream's rms
   (noise_reference).
C. k_burst_msk_center_freq between two segments (center_cases)."""
import functools
from types import SimpleNamespace

import numpy as np

import burst_acq_cases as BC

CONFIGS = BC.CONFIGS
NCH = 70
OBS = (0, 1, 63, 64, 69)
MAX_WRITE = 1504  # a multiple of 16 below both kinds' maxseg (2048 / 4096): maxseg = MAX_WRITE
MAXSEG = MAX_WRITE
ROTATION = (1, 7, 36, 1000, MAXSEG - 1, MAXSEG)
EDGE_N = (1, 2, 7, 35, 36, 37, 1000, MAXSEG - 1, MAXSEG)
SOFT_SENTINEL, SYM_SENTINEL = -2, 1.25e300
SOFTCAP = 16384  # nothing drains a marked bank's rows between launches: room for a whole case unless the case is about the capacity
SYM_TOL = 1e-5
BURST_SOFT_ALLOW = 2
EV_REL = 1e-6
# The EbNo meter's value is a first-order average with weight 0.8 on its past; the kernels evaluate it only in the JD_EBNO_TAIL = 192 samples in front
# of an emission or of a launch's end, so what an emission carries differs between two segmentations of one stream by the term the average has
# forgotten, 0.8^192 = 2.5e-19 of a value of its own size -- below the rounding of the last steps (a few 2^-53).  Two kernel runs must agree to:
EBNO_SEG_REL = 1e-13
NOISE = 1e-9
EV_SIGNAL, EV_EBNO, EV_FREQ, EV_PEAK, EV_TRIDENT = 0, 1, 2, 3, 4
INTS_OQ = ("startstop", "cntr", "yui", "insertpre", "nrx", "msema_pos")
INTS_MSK = ("startstop", "cntr", "nrx", "msema_pos")
# a verdict: (ok, freq, phase_deg, vol_gain, metric)
ACCEPT = {"oqpsk": (1, 8012.5, 33.0, 1.25, 612.0), "msk1200": (1, 1911.0, -47.0, 0.75, 777.0), "msk600": (1, 1893.0, 101.0, 1.5, 901.0)}


def reject(v):
    return (0,) + tuple(v[1:])


def to_struct(cls, v):
    """a verdict as the oracle's or the library's trident result (the same five fields)"""
    return cls(int(v[0]), 0, float(v[1]), float(v[2]), float(v[3]), float(v[4]))


def oracle_settings(O, cfg):
    return O.burst_oqpsk_settings() if cfg.oq else O.burst_msk_settings(fb=cfg.fb)


def geometry(cfg):
    """What jaero_debug_burst_track_geom must report besides the capacities (burst_fill_geometry restated)"""
    sps = cfg.sps
    if cfg.oq:
        g = dict(D2=cfg.tri_sz, msema_len=128, agc2_len=int(round(sps * 64.0)), eb_len=int(sps * 256.0), startstopstart=int(sps * 1050), firn=55, ldsn=36)
    else:
        g = dict(D2=cfg.D2, msema_len=75, agc2_len=int(round(sps * 128.0)), eb_len=int(0.15 * BC.FS), startstopstart=int(sps * 500), firn=2 * int(sps),
                 ldsn=48 if int(sps) == 40 else 128)
    g["win_ring"] = max(g["agc2_len"], g["eb_len"])
    g["ebno_tail"] = 192
    g["cv_len"] = cfg.D1 + max(cfg.D2, cfg.tri_sz) + MAXSEG + 64
    return SimpleNamespace(**g)


def case(name, label, writes, verdicts, vals=None, capsym=False, sql=False, trace=False, softcap=SOFTCAP, watch=OBS, overflow=False):
    total = sum(sum(w) for w in writes)
    for w in writes:
        assert w and all(1 <= n <= MAXSEG for n in w), (label, w)
    for ch, vs in verdicts.items():
        assert 0 <= ch < NCH and all(0 <= a < total for a, _ in vs), (label, ch)
    return SimpleNamespace(name=name, cfg=CONFIGS[name], label=label, writes=writes, verdicts={ch: sorted(vs) for ch, vs in verdicts.items()}, vals=vals or {},
                           capsym=capsym, sql=sql, trace=trace, softcap=softcap, watch=tuple(watch), total=total, overflow=overflow)


def case_val(c, ch):
    v = c.vals.get(ch)
    return np.zeros(c.total) if v is None else v


def segments(c):
    """(start, n, first_of_write, {ch: (ev_pos, verdict)}) of every launch"""
    s = 0
    for w in c.writes:
        for k, n in enumerate(w):
            ev = {}
            for ch, vs in c.verdicts.items():
                hit = [(a - s, v) for a, v in vs if s <= a < s + n]
                assert len(hit) <= 1, (c.label, ch, "two verdicts in one segment")
                if hit:
                    ev[ch] = hit[0]
            yield s, n, int(k == 0), ev
            s += n


def plan_writes(total, sizes=ROTATION, cuts=(), group=1, keep_apart=()):
    """Writes that cover `total` samples: segment lengths rotate through `sizes`, a boundary falls on every sample of `cuts`, `group` segments make
    a write -- fewer where two samples of one list in keep_apart (a channel's verdicts) would share it."""
    cuts = sorted(set(int(c) for c in cuts if 0 < c < total))
    segs, s, k = [], 0, 0
    while s < total:
        n = min(sizes[k % len(sizes)], total - s)
        nxt = [c for c in cuts if s < c < s + n]
        if nxt:
            n = nxt[0] - s
        segs.append((s, n))
        s += n
        k += 1
    writes, cur, start = [], [], 0
    for s, n in segs:
        clash = any(sum(start <= a < s + n for a in lst) > 1 for lst in keep_apart)
        if cur and (len(cur) >= group or clash):
            writes.append(cur)
            cur, start = [], s
        cur.append(n)
    writes.append(cur)
    assert sum(sum(w) for w in writes) == total
    return writes


# ----------------------------------------------------------------------------------------------- the oracle's run of one channel
def expected(O, c, ch, val=None):
    """One jo_burst_track_write per write of the case: soft (emitted, then RxDataBits' pending tail: what the kernel's row holds), events, symbols,
    and behind every write the scalars with the counts so far"""
    d = O.BurstDemod(oracle_settings(O, c.cfg), sql=c.sql, capture_symbols=c.capsym, trace=c.trace)
    val = case_val(c, ch) if val is None else val
    vs = c.verdicts.get(ch, [])
    soft, ev, sym, states, s = [], [], [], [], 0
    nsoft = nev = nsym = 0
    for w in c.writes:
        n = sum(w)
        hit = [(a, v) for a, v in vs if s <= a < s + n]
        assert len(hit) <= 1, (c.label, ch, "two verdicts of one channel in one write")
        d.track_write(val[s:s + n], to_struct(O.TridentResult, hit[0][1]) if hit else None, hit[0][0] - s if hit else -1)
        s += n
        soft.append(d.take_soft()); ev.append(d.take_events())
        nsoft += len(soft[-1]); nev += len(ev[-1])
        if c.capsym:
            sym.append(d.take_symbols())
            nsym += len(sym[-1])
        st = d.track_state()
        st.update(soft_cnt=nsoft + st["nrx"], ev_cnt=nev, sym_cnt=nsym)
        states.append(st)
    soft.append(states[-1]["rx"])
    return SimpleNamespace(soft=np.concatenate(soft).astype(np.int16), events=np.concatenate(ev).reshape(-1, 3),
                           symbols=np.concatenate(sym).reshape(-1, 3) if sym else np.zeros((0, 3)), states=states, cov=d.coverage())


def cap_soft(soft, cap):
    """The kernels' capacity rule on a stream of one burst or of burst OQPSK (no entry is ever taken back): a marker is stored while there is room for
    one entry, a pair while there is room for two, whatever does not fit is dropped and sets overflow bit 1"""
    out, ovf, k = [], False, 0
    while k < len(soft):
        w = 1 if soft[k] < 0 else 2
        if len(out) + w <= cap:
            out.extend(soft[k:k + w])
        else:
            ovf = True
        k += w
    return np.asarray(out, dtype=np.int16), ovf


def ints_of(cfg):
    return INTS_OQ if cfg.oq else INTS_MSK


def capacities(c):
    """soft_cap, sym_cap and ev_cap of the case's bank (burst_create restated)"""
    soft_cap = (c.softcap + 7) & ~7
    return SimpleNamespace(soft_cap=soft_cap, sym_cap=soft_cap // 2 + 8 if c.capsym else 0, ev_cap=4096 if c.trace else 256)


def as_candidate(c, exp, geom):
    """An oracle run in the form the GPU test collects the kernel's: whole rows with the sentinel behind the counts (cases without overflow)"""
    soft_row = np.full(geom.soft_cap, SOFT_SENTINEL, dtype=np.int16)
    soft_row[:len(exp.soft)] = exp.soft
    sym_rows = np.full((geom.sym_cap, 3), SYM_SENTINEL)
    sym_rows[:len(exp.symbols)] = exp.symbols
    states = [dict(st, overflow=0) for st in exp.states]
    return SimpleNamespace(soft_row=soft_row, sym_rows=sym_rows, events=exp.events.copy(), states=states)


# ----------------------------------------------------------------------------------------------- checkers
def check_counts(c, ch, exp, got):
    """Behind every write: the integers of the peek (cases without overflow), overflow == 0"""
    assert len(got.states) == len(exp.states), (c.label, ch)
    for k, (e, g) in enumerate(zip(exp.states, got.states)):
        for f in ints_of(c.cfg) + ("soft_cnt", "sym_cnt"):
            assert g[f] == e[f], (c.name, c.label, ch, f"write {k}", f, g[f], e[f])
        assert g["ev_cnt"] == e["ev_cnt"], (c.name, c.label, ch, f"write {k}", "ev_cnt", g["ev_cnt"], e["ev_cnt"])
        assert g["overflow"] == 0, (c.name, c.label, ch, f"write {k}", "overflow", g["overflow"])


def check_rows_behind(c, ch, got, soft_cnt, sym_cnt):
    """Nothing is stored behind the counts.  With the squelch on the kernel stores a group where the oracle keeps it in RxDataBits and takes the count
    back when the group is dropped (soft_cnt -= nrx): the at most 33 entries of the last dropped group (31 and a pair) may stand behind the count."""
    slack = 33 if c.sql else 0
    stale = got.soft_row[soft_cnt:soft_cnt + slack]
    assert np.all((stale == SOFT_SENTINEL) | ((stale >= -1) & (stale <= 255))), (c.name, c.label, ch, "behind the soft count", stale)
    soft_cnt += slack
    assert np.all(got.soft_row[soft_cnt:] == SOFT_SENTINEL), (c.name, c.label, ch, "a store behind the soft count", np.nonzero(got.soft_row[soft_cnt:] != SOFT_SENTINEL)[0][:8] + soft_cnt)
    if c.capsym:
        assert np.all(got.sym_rows[sym_cnt:] == SYM_SENTINEL), (c.name, c.label, ch, "a store behind the symbol count")


def check_exact(c, ch, exp, got, geom):
    """Part A: everything equal outright.  got: soft_row [soft_cap], sym_rows [sym_cap, 3], events [ev_cnt, 3], states (the peek behind every
    write, as dicts).  geom: soft_cap, sym_cap, ev_cap."""
    tag = (c.name, c.label, ch)
    last = got.states[-1]
    if not c.overflow:
        check_counts(c, ch, exp, got)
        soft, ovf = exp.soft, 0
        assert len(soft) <= geom.soft_cap and len(exp.events) <= geom.ev_cap and (not c.capsym or len(exp.symbols) <= geom.sym_cap), tag + ("the case overflows",)
    else:
        soft, so = cap_soft(exp.soft, geom.soft_cap)
        ovf = (1 if so else 0) | (2 if c.capsym and len(exp.symbols) > geom.sym_cap else 0) | (4 if len(exp.events) > geom.ev_cap else 0)
        for f in [f for f in ints_of(c.cfg) if f != "nrx"]:
            assert last[f] == exp.states[-1][f], tag + (f, last[f], exp.states[-1][f])
    assert last["overflow"] == ovf, tag + ("overflow", last["overflow"], ovf)
    assert last["soft_cnt"] == len(soft), tag + ("soft_cnt", last["soft_cnt"], len(soft))
    assert np.array_equal(got.soft_row[:len(soft)], soft), tag + ("soft row", np.nonzero(got.soft_row[:len(soft)] != soft)[0][:8])
    ev = exp.events[:geom.ev_cap]
    assert last["ev_cnt"] == len(ev) == len(got.events), tag + ("ev_cnt", last["ev_cnt"], len(ev))
    assert np.array_equal(got.events, ev), tag + ("event rows", got.events[np.any(got.events != ev, axis=1)][:4], ev[np.any(got.events != ev, axis=1)][:4])
    nsym = 0
    if c.capsym:
        sym = exp.symbols[:geom.sym_cap]
        nsym = len(sym)
        assert last["sym_cnt"] == nsym, tag + ("sym_cnt", last["sym_cnt"], nsym)
        assert np.array_equal(got.sym_rows[:nsym], sym), tag + ("symbol rows", np.nonzero(np.any(got.sym_rows[:nsym] != sym, axis=1))[0][:8])
    check_rows_behind(c, ch, got, len(soft), nsym)


def soft_differences(got, ref):
    d = np.abs(np.asarray(got).astype(int) - np.asarray(ref).astype(int))
    return int((d != 0).sum()), int(d.max(initial=0))


def same_decisions(c, exp, other):
    """The decision part of the contract between two runs: markers, hard decisions, event kinds and stamps, counts and integers, soft bytes within 1
    in at most BURST_SOFT_ALLOW bytes.  Returns None or what differs."""
    if len(other.soft) != len(exp.soft) or not np.array_equal(other.soft < 0, exp.soft < 0):
        return "markers / soft count"
    if not np.array_equal(other.soft >= 128, exp.soft >= 128):
        return "hard decisions"
    nd, mx = soft_differences(other.soft, exp.soft)
    if mx > 1 or nd > BURST_SOFT_ALLOW:
        return f"{nd} soft bytes differ, by up to {mx}"
    if other.events.shape != exp.events.shape or not np.array_equal(other.events[:, :2], exp.events[:, :2]):
        return "event kinds / stamps"
    if other.symbols.shape != exp.symbols.shape:
        return "symbol count"
    for k, (e, g) in enumerate(zip(exp.states, other.states)):
        for f in ints_of(c.cfg) + ("soft_cnt", "sym_cnt", "ev_cnt"):
            if g[f] != e[f]:
                return f"write {k}: {f} {g[f]} != {e[f]}"
    return None


def symbol_deviation(a, b):
    return float(np.max(np.abs(a - b), initial=0.0))


def check_values(c, ch, exp, got, geom, sym_tol):
    """Part B.  Returns the kernel's largest symbol deviation (printed and recorded by the caller before this asserts on it: see measure_values)."""
    tag = (c.name, c.label, ch)
    check_counts(c, ch, exp, got)
    n = len(exp.soft)
    cand = SimpleNamespace(soft=got.soft_row[:n], events=got.events, symbols=got.sym_rows[:len(exp.symbols)], states=got.states)
    why = same_decisions(c, exp, cand)
    assert why is None, tag + (why,)
    ev = exp.events
    rel = np.abs(got.events[:, 2] - ev[:, 2]) / np.maximum(np.abs(ev[:, 2]), 1e-300)
    rel[got.events[:, 2] == ev[:, 2]] = 0.0
    assert np.all(rel <= EV_REL), tag + ("event values", got.events[rel > EV_REL][:4], ev[rel > EV_REL][:4])
    dev = symbol_deviation(cand.symbols, exp.symbols)
    assert dev <= sym_tol, tag + (f"symbols deviate by {dev:.3e}, allowed {sym_tol:.3e}",)
    check_rows_behind(c, ch, got, n, len(exp.symbols))
    return dev


# ----------------------------------------------------------------------------------------------- A: landmarks of a burst on zero input
@functools.lru_cache(maxsize=None)
def landmarks(O, name, v0=0):
    """Where a burst that an accepting verdict starts at sample v0 of an all-zero stream puts its marker, its EbNo emission, its time-out and its
    32nd soft entry (the sample of the pair that completes the first group), from the oracle run one sample at a time; and its length."""
    cfg = CONFIGS[name]
    d = O.BurstDemod(oracle_settings(O, cfg))
    v = to_struct(O.TridentResult, ACCEPT[name])
    z = np.zeros(1)
    lm, s = {"marker": None, "ebno": None, "timeout": None, "soft32": None}, 0
    if v0:
        d.track_write(np.zeros(v0))
        s = v0
    while lm["marker"] is None or lm["soft32"] is None:  # sample by sample until the marker is in RxDataBits and the first group is out
        d.track_write(z, v if s == v0 else None, 0 if s == v0 else -1)
        if lm["marker"] is None and -1 in d.track_state()["rx"]:
            lm["marker"] = s
        if lm["soft32"] is None and len(d.take_soft()):
            lm["soft32"] = s
        s += 1
        assert s < v0 + 4000
    d.track_write(np.zeros(16 * geometry(cfg).startstopstart))
    for smp, kind, val in d.take_events():
        if kind == EV_EBNO and lm["ebno"] is None:
            lm["ebno"] = int(smp)
        if kind == EV_SIGNAL and val == 0.0 and lm["timeout"] is None:
            lm["timeout"] = int(smp)
    assert all(x is not None for x in lm.values()), (name, lm)
    return SimpleNamespace(**lm)


def burst_len(O, name):
    return landmarks(O, name).timeout + 1


def spread(name, at):
    """the observed channels' verdicts at different samples, so that lanes of one wavefront are in different phases of a burst"""
    return {ch: [(a, ACCEPT[name])] for ch, a in zip(OBS, at) if a is not None}


def edge_cases(name, capsym):
    """Verdict on sample 0, 1, n - 2 and n - 1 of a first segment of n samples (n0 = 0: below agc2_len and eb_len), channel 69 never; then a few
    segments of the rotation, past the burst MSK marker (at the verdict) and, for burst OQPSK, past the marker 246 symbols later"""
    out = []
    tail = 2400 if CONFIGS[name].oq else 600
    for n in EDGE_N:
        at = [0, 1 if n > 1 else None, max(n - 2, 0), n - 1, None]
        rest = plan_writes(tail, sizes=(n, 7, 36, 1000, 1))
        out.append(case(name, f"edge n={n}", [[n]] + rest, spread(name, at), capsym=capsym))
    return out


def burst_cases(O, name, capsym):
    """Whole bursts, past one wrap of win_ring, of cv_len and of the msema ring, in the rotation's segmentation: second verdicts before the marker,
    between the marker and the EbNo emission, inside the last JD_EBNO_TAIL samples before it and after the time-out; rejecting verdicts with trace
    on and off, idle and in mid-burst; channel 69 never gets a verdict"""
    cfg, lm, A = CONFIGS[name], landmarks(O, name), ACCEPT[name]
    g = geometry(cfg)
    L = lm.timeout + 1
    total = max(2 * L + 700, g.cv_len + g.win_ring + 500)
    first = {0: 5, 1: 300, 63: 41, 64: 1000}
    second = {0: first[0] + L + 100,                                 # after the time-out
              1: first[1] + (lm.marker // 2 if cfg.oq else 900),     # before the marker (burst MSK: the marker is the verdict's; inside the preamble)
              63: first[63] + (lm.marker + lm.ebno) // 2,            # between the marker and the EbNo emission
              64: first[64] + lm.ebno - g.ebno_tail // 2}            # inside the last JD_EBNO_TAIL samples before the emission
    out = []
    for trace in (False, True):
        v = {ch: [(first[ch], A), (second[ch], A)] for ch in first}
        v[2] = [(77, reject(A))]                                # a rejecting verdict on an idle channel
        v[3] = [(10, A), (10 + lm.ebno // 2, reject(A))]        # and in mid-burst
        keep = [[a for a, _ in vs] for vs in v.values()]
        out.append(case(name, f"bursts trace={int(trace)}", plan_writes(total, group=2, keep_apart=keep), v, capsym=capsym, trace=trace, watch=OBS + (2, 3)))
    return out


def boundary_cases(O, name, capsym):
    """Segment boundaries on, one before and one behind the marker, the EbNo emission, the time-out and the 32nd soft entry of channel 0's burst"""
    lm, A = landmarks(O, name, 3), ACCEPT[name]
    L = lm.timeout + 40
    out = []
    for shift in (0, -1, 1):
        cuts = [x + shift for x in (lm.marker, lm.ebno, lm.timeout, lm.soft32)]
        v = {0: [(3, A)], 1: [(4, A)], 63: [(2, A)], 64: [(200, A)]}
        out.append(case(name, f"boundaries {shift:+d}", plan_writes(L, sizes=(MAXSEG, MAXSEG - 1), cuts=cuts), v, capsym=capsym))
    return out


def squelch_cases(O, name, capsym):
    """Burst OQPSK with the squelch on (burst MSK has none): with mse = 2 every group is dropped, except those of the write whose lastmse was taken
    while the window was still filling (below the threshold 0.6) -- that write has a second segment, first_of_write = 0, directly behind it."""
    if not CONFIGS[name].oq:
        return []
    lm, A = landmarks(O, name), ACCEPT[name]
    sps = CONFIGS[name].sps
    w0 = int(150 * sps)  # mse starts to rise at cntr > 138 symbols; 12 symbol pairs later it is 2 * 6 / 128
    v = {0: [(0, A)], 1: [(9, A)], 63: [(w0 - 40, A)], 64: [(w0 + 5, A)]}
    writes = [[w0]] + [[MAXSEG, MAXSEG - 1]] + plan_writes(lm.ebno + 2000 - w0 - 2 * MAXSEG + 1, sizes=(1000, 36, MAXSEG))
    return [case(name, "squelch", writes, v, capsym=capsym, sql=True)]


def _entries_before_marker(O, name, k):
    """soft entries in front of the marker of a burst OQPSK channel that gets a second accepting verdict k samples behind the first"""
    lm, A = landmarks(O, name), ACCEPT[name]
    c = case(name, "probe", [[k]] + plan_writes(lm.marker + 2, sizes=(MAXSEG,)), {0: [(0, A), (k, A)]})
    e = expected(O, c, 0)
    m = np.nonzero(e.soft < 0)[0]
    assert len(m) == 1
    return int(m[0])


def cap_cases(O, name, capsym):
    """Capacities.  A soft row of 512 entries: the pair that does not fit is dropped whole (the row's last entry keeps the sentinel: the count is
    odd behind a marker), and with captured symbols the symbol log (soft_cap / 2 + 8 rows) fills a few symbols later.  Burst OQPSK: a row that is
    exactly full when the marker comes (a second verdict k samples behind the first moves the number of entries in front of the marker to a
    multiple of 8).  Burst MSK stores its marker at the verdict, behind soft_cnt - nrx entries, a multiple of 12 below the count the row stopped
    at: its marker branch cannot overflow in a stream and is not run.  The event log: 4096 rows reached by the trace rows of rejecting verdicts,
    one per single-sample segment."""
    cfg, lm, A = CONFIGS[name], landmarks(O, name), ACCEPT[name]
    out = []
    n = lm.marker + int(285 * 2 * cfg.sps)  # 285 symbol pairs behind the marker: more than the 264 rows of the symbol log
    out.append(case(name, "soft row of 512", plan_writes(n, sizes=(MAXSEG, 1000)), {0: [(0, A)], 64: [(50, A)]}, capsym=capsym, softcap=512, watch=(0, 64, 69), overflow=True))
    if cfg.oq:
        for k in range(200, 2000, 3):
            e = _entries_before_marker(O, name, k)
            if e % 8 == 0:
                break
        assert e % 8 == 0
        out.append(case(name, f"marker overflows (second verdict at {k}, {e} entries)", [[k]] + plan_writes(lm.marker + 300, sizes=(MAXSEG, 7)),
                        {0: [(0, A), (k, A)]}, capsym=capsym, softcap=e, watch=(0, 69), overflow=True))
    if not capsym:
        nrows = 4096 + 5
        out.append(case(name, "event log full of trace rows", [[1]] * nrows, {0: [(s, reject(A)) for s in range(nrows)], 64: [(s, reject(A)) for s in range(0, nrows, 2)]},
                        trace=True, watch=(0, 64, 69), overflow=True))
    return out


def zero_cases(O, name, capsym):
    return edge_cases(name, capsym) + burst_cases(O, name, capsym) + boundary_cases(O, name, capsym) + squelch_cases(O, name, capsym) + cap_cases(O, name, capsym)


# ----------------------------------------------------------------------------------------------- B: values on real bursts
# per observed channel: Eb/N0 in dB, carrier offset from the configuration's centre in Hz.  18 dB, 10 dB and one low enough that the loop clips and
# ct_ec reaches its clamp (burst MSK 600: 10 dB, no burst below that is detected in a stream of this length); the last two offsets put the trident
# frequency near both ends of the range tests/burst_acq_cases.py searches (6000 .. 10 000 Hz, 1000 / 800 .. 3000 Hz).
STREAMS = {
    "oqpsk": dict(ebno=(18.0, 10.0, 4.0, 18.0, 10.0), off=(0.0, -90.0, 95.0, -1900.0, 1900.0), starts=(50000, 75000), ndata=330, total=91000, center=8000.0),
    "msk1200": dict(ebno=(18.0, 10.0, 5.0, 18.0, 10.0), off=(0.0, -40.0, 45.0, -850.0, 1050.0), starts=(30000, 72000), ndata=140, total=115000, center=1900.0),
    "msk600": dict(ebno=(18.0, 10.0, 10.0, 18.0, 10.0), off=(0.0, -40.0, 45.0, -1050.0, 1050.0), starts=(30000, 112000), ndata=140, total=200000, center=1900.0),
}
LEAD = 400  # samples of a recorded stream kept in front of its first accepting verdict (the generator's bursts start 30 000 samples in: the first AGC's
# window is a second long; the tracking chain meets what is left as a fresh object would)
STREAM_SEEDS = {"oqpsk": 100, "msk1200": 210, "msk600": 300}  # chosen so that none of ten noise draws changes a decision of the oracle (test_burst_track_cases)


@functools.lru_cache(maxsize=None)
def recorded(O, name, k, seed):
    """Observed channel k's stream: (val_to_demod of every sample, [(sample, verdict)], the ordinary run's outputs), recorded from jo_burst_write on a
    signalgen burst pair in 4096-sample writes with trace off"""
    from jaero_amd import signalgen as G

    cfg, S = CONFIGS[name], STREAMS[name]
    fc = S["center"] + S["off"][k]
    if cfg.oq:
        pcm, _ = G.burst_oqpsk(S["total"], burst_starts=list(S["starts"]), ndata_sym=S["ndata"], fc=fc, ebno_db=S["ebno"][k], seed=seed)
    else:
        pcm, _ = G.burst_msk(S["total"], burst_starts=list(S["starts"]), ndata=S["ndata"], fb=cfg.fb, fc=fc, ebno_db=S["ebno"][k], seed=seed)
    d = O.BurstDemod(oracle_settings(O, cfg), capture_symbols=True)
    d.record()
    for s in range(0, len(pcm), 4096):
        d.write(pcm[s:s + 4096])
    val, ver = d.take_recorded()
    st = d.track_state()
    run = SimpleNamespace(soft=np.concatenate([d.take_soft(), st["rx"]]).astype(np.int16), events=d.take_events(), symbols=d.take_symbols(), state=st, cov=d.coverage())
    verdicts = [(s, (t.ok, t.freq, t.phase_deg, t.vol_gain, t.metric)) for s, t in ver]
    return val, verdicts, run


def stream_case(O, name, capsym=True, sql=False, seed=None, sizes=ROTATION, limit=None, only_observed=False):
    """The five recorded streams on the observed channels; every other channel repeats the stream of observed channel (ch mod 5), 13 ch samples late
    (zeros in front), so that the lanes of a wavefront are at different points of their bursts.  limit: only the first `limit` samples;
    only_observed: every other channel gets zeros and no verdict."""
    seed = STREAM_SEEDS[name] if seed is None else seed
    vals, verdicts = {}, {}
    for k, ch in enumerate(OBS):
        val, ver, _ = recorded(O, name, k, seed + k)
        t0 = min(a for a, v in ver if v[0]) - LEAD
        vals[ch], verdicts[ch] = val[t0:], [(a - t0, v) for a, v in ver if a >= t0]
    total = min(len(v) for v in vals.values())
    total = total if limit is None else min(total, limit)
    for ch in range(NCH):
        if ch not in OBS and not only_observed:
            sh = 13 * ch
            vals[ch] = np.concatenate([np.zeros(sh), vals[OBS[ch % 5]]])
            verdicts[ch] = [(a + sh, v) for a, v in verdicts[OBS[ch % 5]]]
    vals = {ch: v[:total] for ch, v in vals.items()}
    verdicts = {ch: [(a, v) for a, v in vs if a < total] for ch, vs in verdicts.items()}
    keep = [[a for a, _ in vs] for vs in verdicts.values()]
    return case(name, f"streams seed {seed} sql={int(sql)}", plan_writes(total, sizes=sizes, group=2, keep_apart=keep), verdicts, vals=vals, capsym=capsym, sql=sql)


def noise_reference(O, c, ch, exp, draw):
    """The oracle once more on the same stream plus seeded white noise of NOISE x the stream's rms: (E_n = the largest symbol deviation between the
    two oracle runs, None or why the draw does not count: a decision differs)"""
    val = case_val(c, ch)
    rng = np.random.default_rng(7919 * draw + ch)
    noisy = val + NOISE * float(np.sqrt(np.mean(val * val))) * rng.standard_normal(len(val))
    other = expected(O, c, ch, noisy)
    why = same_decisions(c, exp, other)
    return (symbol_deviation(other.symbols, exp.symbols) if why is None else None), why


def ebno_case(O, name, sizes):
    """The recorded streams up to behind the first EbNo emission of every observed channel, in the given segmentation"""
    lm = landmarks(O, name)
    return stream_case(O, name, capsym=False, sizes=sizes, limit=LEAD + lm.ebno + 2 * MAXSEG, only_observed=True)


# ----------------------------------------------------------------------------------------------- C: CenterFreqChangedSlot between two segments
def center_cases():
    """(afc, frequency): inside the range and beyond both clamps (0.75 fb and Fs / 2 - 0.75 fb)"""
    return [(afc, hz) for afc in (False, True) for hz in (1500.0, 10.0, 23990.0)]
