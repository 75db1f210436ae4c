"""The cases of tests/test_aerol_branch_cases.py (CPU) and tests/test_gpu_aerol_branches.py (GPU): soft-bit streams, write schedules and
updateDCD tick schedules that take the three Aero-L bit pipelines (k_aerol.h, k_aerol_burst.h, aerolc.h) through the decisions no generated,
well-formed frame stream reaches, and the helpers that run a case through oracle/aerol_oracle.c with its branch counters
(jo_aerol_coverage) and its peeked state (jo_aerol_peek).

A case is one channel: a name, its family, the stream (int16), the per-write counts, the ticks behind each write, the oracle counters it is
there to hit, and -- where it aims at a kernel path the oracle has no counter for -- a predicate that proves the path from the stream and
the oracle's state in front of every write.  Noise has a fixed seed; everything else is sigma 0.

R/T channels: AeroL drops the rest of the demodulator's current GROUP of soft bits at the end of signal, so the oracle is fed group by
group (oracle.demod_groups, the bank's own rule) and a write may only end where a group ends; `writes` of an R/T case are targets that
`schedule` rounds up to the next group end."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from jaero_amd import aerol_frames as AF

FAMILIES = {"P10500": (10500, False), "P1200": (1200, False), "P600": (600, False), "RT10500": (10500, True), "RT1200": (1200, True),
            "RT600": (600, True), "C8400": (8400, False)}
# counter prefixes of a family's chain (oracle/aerol_oracle.c: AEROL_COV_LIST)
_P = ("tick_", "w_", "cn_", "hd_", "bl_", "sy_", "wr_", "bd_", "fe_")
_RT = ("tick_", "w_", "pi_", "inv_", "cn_", "hd_", "br_", "sy_", "wr_")
CHAINS = {"P10500": _P + ("oq_", "pi_", "gsl_", "inv_"), "P1200": _P + ("px_",), "P600": _P + ("px_",),
          "RT10500": _RT + ("oq_", "gsl_", "bm_", "rt_"), "RT1200": _RT + ("mk_", "mu_"), "RT600": _RT + ("mk_", "mu_"),
          "C8400": ("tick_", "c_", "gsl_", "inv_")}

# Counters of a family's chain that no input can reach, each with its derivation.
_U_SCR = "the scrambler position restarts at every unique word and at every frame-length wrap, and a frame decodes 576 / 2496 bits: never 5000"
_U_INFO = "ninfo restarts at cntr == 0 of every frame and a frame packs 72 / 312 bytes into a 4096-byte field"
_U_SAT = "a saturated cntr gives idx = (1e9 - BitsInHeader) % blocksz = 2366 / 48 / 240 (10500 / 1200 / 600), never blocksz - 1, on every bit"
_U_EOS = "`if (a->burstmode)` inside the wrap: a P object is not in burst mode"
_U_IDXNEG = "BitsInHeader is 16 and the block store needs cntr >= 16: cntr - BitsInHeader is never negative"
_U_HDR = "burst mode sets cntr = 16 in the same bit that made it 0: cntr is never 1 .. 15"
_U_SHORT = "`!a->burstmode &&` in front of the frame-length test: not evaluated in burst mode"
_U_TICKNEG = "the countdown is 12 (unique word), 0 (end of signal) or 12 - 3k (ticks): never negative; the frame end that subtracts from it is P's"
_U_ONEBLK = "a 10 500 bps frame is one interleaver block (blocksz = NumberOfBits = 4992): the only idx == blocksz - 1 below cntr = 5250 is the frame's last"
_U_P = {"bd_scr_clamp": _U_SCR, "bd_info_over": _U_INFO, "bl_done_sat": _U_SAT, "wr_end_of_signal": _U_EOS}
_U_RT = {"hd_shift": _U_HDR, "hd_done": _U_HDR, "sy_short": _U_SHORT, "sy_exact_len": _U_SHORT, "tick_neg": _U_TICKNEG}
_U_MSKLAST = "updateMSK leaves OK, BAD or nothing in lastpacketstate, never TEST_FAILED: resetblockptr has nothing to report"
_U_RTSCR = "the position restarts in front of every trial and a trial descrambles blockptr / 2 <= 3040 bits"
UNREACHABLE = {
    "P10500": dict(_U_P, fe_not_frame=_U_ONEBLK),
    "P1200": dict(_U_P, bl_idx_neg=_U_IDXNEG),
    "P600": dict(_U_P, bl_idx_neg=_U_IDXNEG),
    "RT10500": dict(_U_RT, rt_scr_clamp=_U_RTSCR),
    "RT1200": dict(_U_RT, mu_scr_clamp=_U_RTSCR, br_reset_bad=_U_MSKLAST),
    "RT600": dict(_U_RT, mu_scr_clamp=_U_RTSCR, br_reset_bad=_U_MSKLAST),
    "C8400": {"c_cdel_over": "ncdel restarts at every unique word and cntr counts 0 .. 4095 once behind it (no wrap in DecodeC): 16 blocks = 4096 <= 4352 bytes",
              "c_scr_clamp": "the position restarts at every unique word, which is followed by at most one frame end of 2714 bits",
              "c_first_short": "the codec always gets 4095 + 1365 = 5460 symbols: its first call returns (5460 + 24) / 2 - 25 = 2717 bits, every later one 2730, never fewer than 2714",
              "c_voice_over": "bits 1 .. 2713 minus 13 skipped behind every 96 are 25 x 96 = 2400 bits: exactly 300 bytes"},
}

UWB = np.array([(AF.UW >> (31 - k)) & 1 for k in range(32)], dtype=np.uint8)
C_W1 = np.array([(AF.C_UW1 >> (51 - k)) & 1 for k in range(52)], dtype=np.uint8)
C_W2 = np.array([(AF.C_UW2 >> (51 - k)) & 1 for k in range(52)], dtype=np.uint8)
WIDTH = 3000          # write width of the narrow banks (a multiple of 8: k_aerolb_bits takes its entries eight at a time)
WIDE = (40000, 65536)  # P 10500 only
SCAN_HI = 32768       # k_aerol_scan covers this many positions of a write
FRAME = {10500: 5250, 1200: 1200, 600: 1200, 8400: 4200}


@dataclass
class Case:
    name: str
    family: str
    stream: np.ndarray
    hits: tuple = ()
    writes: tuple = ()            # per-write counts, cycled until the stream is used up; () = WIDTH
    ticks: dict = field(default_factory=dict)  # {stream position: number of updateDCD ticks in front of that entry}; -1 = behind the last entry
    predicate: object = None      # f(case, run) raising AssertionError; run = run_oracle's result
    wide: bool = False            # P 10500: a case of the 40 000 / 65 536 wide bank only
    width: int = 3000             # the widest write of the case's own plan (= WIDTH but for the wide cases)

    @property
    def fb(self):
        return FAMILIES[self.family][0]

    @property
    def burst(self):
        return FAMILIES[self.family][1]


def noise(n, seed, sigma=40.0):
    rng = np.random.default_rng(seed)
    return np.clip(np.round(128 + rng.normal(0, sigma, n)), 0, 255).astype(np.int16)


def soft(bits):
    return AF.to_soft(np.asarray(bits, dtype=np.uint8))


def word(pattern=UWB, errors=0, invert=False, seed=0):
    """`pattern` (or its complement) with `errors` wrong bits at fixed places"""
    w = pattern.copy() ^ (1 if invert else 0)
    if errors:
        w[np.random.default_rng(1000 + seed).permutation(len(w))[:errors]] ^= 1
    return w


def two_arm(a, b):
    """bits a on the even positions, b on the odd ones"""
    out = np.empty(len(a) + len(b), dtype=np.uint8)
    out[0::2], out[1::2] = a, b
    return out


def schedule(case, width=None, final=True):
    """[(start, end, ticks)] of a case's writes: its counts in turn, cycled, a count above `width` (default: the case's own) in several writes, and a cut
    wherever the case ticks.  R/T: ends moved up to the next group end (at most 33 entries more).  final: the ticks behind the end of the stream are
    part of the plan (a bank adds them behind ITS last write instead)."""
    n = len(case.stream)
    width = width or case.width
    plan = list(case.writes) or [width]
    ends = None
    if case.burst:
        from oracle import oracle as O
        ends = np.array([e for _, e in O.demod_groups(case.stream)], dtype=np.int64)
    snap = (lambda q: int(ends[np.searchsorted(ends, q)])) if ends is not None else (lambda q: q)
    tick_at = {snap(q): t for q, t in case.ticks.items() if q >= 0}
    out, s, k, left = [], 0, 0, plan[0]
    while s < n:
        e = min(n, s + min(width, left))
        if e > s:
            e = snap(e)
        cut = [q for q in tick_at if s < q < e]
        if cut:
            e = min(cut)
        left -= e - s
        out.append([s, e, int(tick_at.get(e, 0)) if e > s or not out else 0])
        s = e
        if left <= 0:
            k += 1
            left = plan[k % len(plan)]
        if len(out) > 100000:
            raise RuntimeError("write plan makes no progress")
    if final:
        out[-1][2] += int(case.ticks.get(-1, 0))
    return [tuple(w) for w in out]


def run_oracle(O, case, plan=None):
    """The case through the oracle: rows, tick returns, counters, and the peeked state in front of every write."""
    a = O.AeroL(case.fb, burst=case.burst)
    plan = plan if plan is not None else schedule(case)
    peeks, dcd = [], []
    for s, e, t in plan:
        peeks.append(a.peek())
        seg = case.stream[s:e]
        if case.burst:
            for g0, g1 in O.demod_groups(seg):
                a.write(seg[g0:g1])
        elif len(seg):
            a.write(seg)
        dcd += [a.tick_dcd() for _ in range(t)]
    out = {"sus": a.take_sus(), "events": a.take_events(), "packets": a.take_packets(), "dcd": np.array(dcd, dtype=np.int32),
           "coverage": a.coverage(), "peeks": peeks, "final": a.peek(), "plan": plan}
    if case.fb == 8400:
        out["voice_frames"], out["voice"] = a.take_voice()
    return out


def cut_plans(case):
    """three other cuts of the same stream with the ticks at the same stream positions (test (c))"""
    base = schedule(case)
    marks = [(e, t) for _, e, t in base if t]
    n = len(case.stream)
    plans = []
    for step in (1 << 30, 997, 61):
        pts = sorted(set([e for e, _ in marks] + list(range(step, n, step)) + [n]))
        if case.burst:
            from oracle import oracle as O
            ends = np.array([e for _, e in O.demod_groups(case.stream)], dtype=np.int64)
            pts = sorted(set(int(ends[np.searchsorted(ends, q)]) for q in pts))
        tk = dict(marks)
        plan, s = [], 0
        for e in pts:
            plan.append((s, e, tk.get(e, 0)))
            s = e
        plans.append(plan)
    return plans


# ------------------------------------------------------------------------------------------------------------ predicates
def scan_positions(seg):
    """What k_aerol_scan reports for one write (the comment above it): positions q >= 62 of the first 32 768 at which the last 32 hard bits of
    q's parity are the unique word or its complement."""
    h = ((seg[:SCAN_HI].astype(np.int64) & 0xFF) >= 128).astype(np.uint8)
    out = []
    for par in (0, 1):
        s = h[par::2]
        if len(s) >= 32:
            win = np.lib.stride_tricks.sliding_window_view(s, 32)
            hit = (win == UWB).all(1) | (win == 1 - UWB).all(1)
            out += ((np.flatnonzero(hit) + 31) * 2 + par).tolist()
    return sorted(out)


def _p_scan_over_nmatch(case, run):
    assert any(len(scan_positions(case.stream[s:e])) >= 5 for s, e, _ in run["plan"]), "no write with more than AEROL_NMATCH positions"


def _p_straddle(case, run):
    """a unique word whose 64 soft bits lie on both sides of position 32 768 of a write, and that the oracle took as a sync"""
    syncs = run["events"][run["events"][:, 1] == 2][:, 0]
    assert any(s + SCAN_HI - 64 < q - 63 < s + SCAN_HI <= q < e for s, e, _ in run["plan"] for q in syncs), syncs


def _p_marker_behind_scan(case, run):
    ok = False
    for s, e, _ in run["plan"]:
        seg = case.stream[s:e]
        neg = np.flatnonzero(seg < 0)
        ok |= len(neg) > 0 and neg.min() >= SCAN_HI
    assert ok, "no write whose only markers lie at q >= 32768"


def _p_locked_in_body(case, run):
    assert any(p["datacd"] and 16 <= p["cntr"] <= 4924 for p in run["peeks"][1:]), "no write starts locked inside a frame body"


def _p_sync_behind_scan(case, run):
    """the channel is unlocked when a write starts and acquires lock at a position >= 32 768 of that write"""
    syncs = run["events"][run["events"][:, 1] == 2][:, 0]
    assert any((not p["datacd"]) and any(s + SCAN_HI <= q < e for q in syncs) for (s, e, _), p in zip(run["plan"], run["peeks"]))


def _final(**want):
    def f(case, run):
        for k, v in want.items():
            assert run["final"][k] == v, (k, run["final"][k], v)
    return f


def _short_values(*vals):
    def f(case, run):
        ev = run["events"]
        got = ev[ev[:, 1] == 1][:, 2].tolist()
        for v in vals:
            assert v in got, (v, got)
    return f


def _resume_next_write(case, run):
    """some one-bit write completes a block: the second half of that soft bit runs at the start of the next write"""
    geo = AF.geometry(case.fb)
    blk, hdr = 64 * geo["ncols"], geo["header"] + geo["dummy"]
    assert any(e - s == 1 and (p["cntr"] + 1 - hdr) % blk == blk - 1 and 16 <= p["cntr"] + 1 < 10 ** 9
               for (s, e, _), p in zip(run["plan"], run["peeks"]))


def _check(msg, fn):
    def f(case, run):
        assert fn(case, run), msg
    return f


_packet = _check("no packet came out", lambda c, r: len(r["packets"]) > 0)
_no_packet = _check("a packet came out", lambda c, r: len(r["packets"]) == 0)


def _all(*fs):
    def f(case, run):
        for g in fs:
            g(case, run)
    return f


# ------------------------------------------------------------------------------------------------------------ P channel
def _pframes(fb, nfr, seed, units=None, **kw):
    pay = AF.random_payloads(nfr, fb, seed=seed)
    for (f, k), u in (units or {}).items():
        pay[f][k] = bytes(u)
    bits, flen = AF.p_channel_bits(pay, fb, **kw)
    return bits, flen


def _bad(seed):
    u = bytearray(AF.make_su(bytes(np.random.default_rng(seed).integers(1, 256, 10, dtype=np.uint8))))
    u[10] ^= 0x55
    if u[10] == 0 and u[11] == 0:
        u[11] = 1
    return bytes(u)


def _weaken(x, lo, hi, step=4, junk=None):
    """soft bits [lo, hi) weak (130 / 125: 255 - v maps the one onto the other) and every `step`-th an exact 128.  junk = a seed: the weak values are random, so
    the decoder's output -- junk rows, but rows -- hangs on every single symbol and a 128 that an inverted arm turned into 127 changes them."""
    x = x.copy()
    hard = x[lo:hi] >= 128 if junk is None else np.random.default_rng(junk).integers(0, 2, hi - lo) > 0
    x[lo:hi] = np.where(hard, 130, 125)
    x[lo:hi:step] = 128
    return x


def _big(x, seed):
    """the same low bytes with 256 k added, k >= 1: values 256 .. 32767 (the ABI takes int16; the oracle keeps the low byte, the kernels mask)"""
    k = np.random.default_rng(seed).integers(1, 127, len(x))
    k[::97] = 127
    y = np.where(x >= 0, x.astype(np.int64) + 256 * k, x)
    assert y.max() <= 32767 and y.max() > 32700
    return y.astype(np.int16)


@functools.lru_cache(maxsize=None)
def p_cases(fam):
    fb = FAMILIES[fam][0]
    oq = fb == 10500
    T = FRAME[fb]
    dly = 2 if oq else 1          # frames between sending a unit and its CRC check
    nsu = 26 if oq else 6
    uwlen = 64 if oq else 32
    cases = []

    def add(name, stream, hits=(), **kw):
        cases.append(Case(f"{fam}.{name}", fam, np.asarray(stream, dtype=np.int16), tuple(hits), **kw))

    # --- signal-unit CRC at the end of a frame: the all-zero rule and its two neighbours
    zero_crc_payload = bytes([7, 0, 0, 0, 0, 0, 0, 0, 0, 1]) + bytes(2)       # zero CRC field over a non-zero payload: stays wrong
    true_crc0 = AF.payload_with_crc(bytes([3, 1, 4, 1, 5, 9, 2, 6]), 0) + bytes(2)  # a payload whose CRC IS 0x0000
    bits, _ = _pframes(fb, dly + 2, 11, {(1, 1): bytes(12), (1, 2): zero_crc_payload, (1, 3): _bad(1), (1, 4): true_crc0})
    add("crc_zero_rule", soft(bits), ("fe_zero_unit", "fe_zero_crc_payload", "fe_true_crc0", "fe_crc_field_nonzero"), ticks={-1: 7})
    # --- DCD countdown: 12 -> bad 9 -> good 11 -> good 13 (the guard is `< 12`), kept to the end of the stream; then ticks: 10 7 4 1 -2, 0 and the drop
    last = dly + 1   # the frame in which the units of frame 1 are checked is the stream's last
    bits, _ = _pframes(fb, last + 1, 12, {(1, 0): _bad(2)})
    add("dcd_9_11_13", soft(bits), ("fe_bad_dec", "fe_ok_inc", "fe_ok_cap", "tick_pos", "tick_neg", "tick_drop", "tick_zero", "tick_keep"), ticks={-1: 8},
        predicate=_final(datacdcountdown=0, datacd=0))
    bits, _ = _pframes(fb, last + 1, 13)
    add("dcd_all_good_then_ticks", soft(bits), ("fe_ok_cap", "tick_drop"), ticks={-1: 6})
    # --- a bad unit at a countdown of 2 drives it negative: 12 -> 9 6 3 (bad) 5 (good) 2 (bad) -1 (bad); the next tick makes it 0 and drops the carrier
    u = {(1, k): _bad(10 + k) for k in (0, 1, 2, 4, 5)}
    u.update({(1, k): _bad(20 + k) for k in range(6, nsu)})
    bits, _ = _pframes(fb, last + 1, 14, u)
    add("dcd_negative", soft(bits), ("fe_bad_dec", "fe_bad_floor", "tick_neg", "tick_drop"), ticks={-1: 2})
    # 12 -> 9 6 3 (bad) 5 (good) 2 (bad) 4 (good) 1 (bad) -2 (bad)
    u = {(1, k): _bad(30 + k) for k in (0, 1, 2, 4, 6, 7)} if nsu > 6 else {(1, k): _bad(30 + k) for k in (0, 1, 2, 3, 5)}
    bits, _ = _pframes(fb, last + 1, 15, u)
    add("dcd_bad_at_1_or_3", soft(bits), ("fe_bad_dec",), ticks={-1: 3})
    # --- ticks drop the carrier while a frame is being counted; the frame end raises it again (`!datacd && countdown > 2`)
    bits, _ = _pframes(fb, dly + 3, 16)
    cutpos = (dly + 1) * T + uwlen + 16 + (300 if oq else 100)
    add("dcd_rise_in_frame_end", soft(bits), ("fe_dcd_rise", "tick_drop") + (("oq_det_nodcd",) if oq else ()), ticks={cutpos: 5},
        predicate=_check("the ticks do not fall inside a frame", lambda c, r: any(t and 16 < p["cntr"] < 4000 for (_, _, t), p in zip(r["plan"], r["peeks"][1:]))))
    # --- frames early, late, missing
    b, _ = _pframes(fb, dly + 4 if oq else 7, 17)
    early = np.concatenate([b[:2 * T - 1], b[2 * T:]])
    add("word_one_bit_early", soft(early), ("sy_short",), predicate=_short_values(T - 1))
    late = np.concatenate([b[:2 * T], b[2 * T - 1:2 * T], b[2 * T:]])
    add("word_one_bit_late", soft(late), ("sy_short", "wr_wrap"), predicate=_short_values(1))
    gap = np.concatenate([b[:2 * T], np.zeros(2 * T + 7, np.uint8), b[2 * T:]])
    add("two_frames_without_word", soft(gap), ("wr_wrap", "sy_short"), ticks={-1: 1})
    # --- detector edges
    if oq:
        # tolerance 0: one wrong bit on one arm is no word; the exact complement on an arm is one (that arm inverted)
        x = b[:3 * T].copy()
        x[T + 10] ^= 1
        add("word_one_wrong_bit", soft(np.concatenate([x, b[3 * T:]])), ("pi_miss", "wr_wrap"))
        bi, _ = _pframes(fb, dly + 2, 18, invert_i=True)
        add("complement_on_one_arm", soft(bi), ("pi_inv_hit", "pi_up_hit", "inv_on", "inv_soft_gt", "inv_soft_lt"))
        # an exact 128 on an inverted arm stays 128
        x = soft(bi)
        for f in (1, 2):
            x = _weaken(x, f * T + 64 + 16 + 178, (f + 1) * T, junk=f)  # even positions: the inverted arm
        add("erasures_on_inverted_arm", x, ("inv_soft_128",))
        # gotsync_last in front of the first frame, where the detectors see every bit: hit / miss (a lone word on one arm), the word on the other arm one
        # arm-bit late (hit, miss, miss, hit, miss: no sync), then the frame's own hit / hit.  (A third hit in a row would need the word to equal itself
        # shifted by one bit: at tolerance 0 it cannot happen.)
        lone = two_arm(UWB, 1 - np.roll(UWB, 3))
        late_arm = np.concatenate([two_arm(UWB, np.concatenate([[0], UWB[:-1]])), [UWB[-1], 0]]).astype(np.uint8)
        x = np.concatenate([np.zeros(10, np.uint8), lone, np.zeros(40, np.uint8), late_arm, np.zeros(30, np.uint8), b[:(dly + 2) * T]])
        add("gotsync_last_patterns", soft(x), ("gsl_first_hit", "gsl_second_miss", "gsl_second_hit", "gsl_first_miss"),
            predicate=_check("one sync per frame", lambda c, r: int((r["events"][:, 1] == 2).sum()) == 4))
    else:
        # the exact detector clears its register on a hit: the word followed by its last 31 bits is a second hit exactly when the clear is missing
        x = np.concatenate([b[:2 * T], UWB, UWB[1:], np.zeros(9, np.uint8), b[2 * T:]])
        add("word_then_its_last_31_bits", soft(x), ("px_hit", "sy_short"),
            predicate=_check("the 31 bits made a second hit", lambda c, r: 31 not in r["events"][r["events"][:, 1] == 1][:, 2].tolist()))
        x = np.concatenate([b[:2 * T], UWB, UWB, b[2 * T:]])
        add("word_twice", soft(x), ("px_hit", "sy_short"), predicate=_short_values(32))
    # --- markers (a negative entry: muw = 0 and nothing else): inside a word, the header, a locked body; first and last entry of a write
    x = soft(b).astype(np.int16)
    f0 = 3 * T if not oq else 2 * T
    at = sorted([f0 + 20, f0 + uwlen + 5, f0 + uwlen + 16 + 400, WIDTH, 2 * WIDTH - 1])
    x = np.insert(x, [q - k for k, q in enumerate(at)], -1)  # entry q of the result is a marker
    x[f0 + 20] = -32768
    add("markers", x, ("w_marker",), writes=(WIDTH,),
        predicate=_check("no marker as first and as last entry of a write", lambda c, r: c.stream[WIDTH] < 0 and c.stream[2 * WIDTH - 1] < 0))
    # --- write shapes: one soft bit per write across the bit that completes a block; writes of 0 soft bits between full ones; a write exactly WIDTH long
    hdr = 16 + (178 if oq else 0)
    blk = 64 * AF.geometry(fb)["ncols"]
    done_at = 2 * T + uwlen + hdr + blk - 1     # the entry that completes the first block of frame 2
    add("one_bit_writes_across_a_block_end", soft(b[:(dly + 3) * T]), ("bl_done",), writes=(done_at - 2,) + (1,) * 5 + (0, WIDTH, 0, 0, WIDTH - 1, 1 << 30),
        predicate=_resume_next_write)
    # --- int16 values 256 .. 32767
    add("values_above_255", _big(soft(bi if oq else b[:(dly + 2) * T]), 5), ("fe_ok_cap",))
    # --- 100 000 soft bits and more without a marker: muw saturates
    add("muw_saturates", np.concatenate([soft(b[:(dly + 2) * T]), noise(100100 - (dly + 2) * T, 19, 30.0)]), ("w_muw_sat", "cn_sat" if not oq else "w_muw_sat"),
        writes=(1 << 30,) if oq else ())
    if oq:
        cases.extend(_p_wide_cases(fam))
    return tuple(cases)


def _plant(x, at, arm_word, sd):
    """a lone word on one arm (the positions at, at + 2, ..): what k_aerol_scan reports and the detector takes as a hit without a sync"""
    x[at:at + 64:2] = np.where(arm_word > 0, 203, 53)
    other = x[at + 1:at + 65:2]
    if (((other & 0xFF) >= 128).astype(np.uint8) == arm_word).all() or (((other & 0xFF) >= 128).astype(np.uint8) == 1 - arm_word).all():
        other[0] = 255 - other[0]
    return x


@functools.lru_cache(maxsize=None)
def _wide_bits():
    """38 frames = 199 500 channel bits, the Q arm inverted: more than three writes of 65 536"""
    return _pframes(10500, 38, 40, invert_q=True)[0]


def _p_wide_cases(fam):
    """10 500 bps writes of 40 000 and 65 536 soft bits: k_aerol_bits<true> with k_aerol_scan beyond one or two frames per write"""
    fb, T = 10500, 5250
    out = []

    def add(name, stream, hits=(), **kw):
        out.append(Case(f"{fam}.wide.{name}", fam, np.asarray(stream, dtype=np.int16), tuple(hits), wide=True, width=max(kw["writes"]), **kw))

    b = _wide_bits()
    # writes of 65 536: frame k's word ends at lead + k T + 63.  The word of frame 6 straddles 32 768 when lead + 6 T in (32704, 32768): lead = 1250
    x = np.concatenate([noise(1250, 41), soft(b)])
    x = x[:3 * 65536]
    add("locked_seven_frames", x, ("sy_sync", "oq_det_window"), writes=(65536,), predicate=_all(_p_straddle, _p_locked_in_body))
    add("locked_seven_frames_40000", x[:120000], ("sy_sync",), writes=(40000,), predicate=_p_locked_in_body)
    # locked, and the word on both arms inside the detector window of the sixth frame of the first write (behind the 64 bits that flush the registers): a
    # false sync at a position behind the four the scan recorded -- "no jumps past the last known one" -- then junk frames
    y = x.copy()
    at = 1250 + 6 * T - 261 + 70
    y[at:at + 64] = soft(two_arm(UWB, UWB))
    add("locked_false_sync_in_sixth_window", y, ("sy_sync", "sy_short"), writes=(65536,),
        predicate=_check("no sync at the planted place, behind the scan's fourth position",
                         lambda c, r, at=at: at + 63 in r["events"][r["events"][:, 1] == 2][:, 0].tolist() and scan_positions(c.stream[:65536])[3] < at))
    # noise only, six lone words planted in every write: more positions than AEROL_NMATCH
    for name, width in (("noise_six_words", 65536), ("noise_six_words_40000", 40000)):
        n = 3 * width
        x = noise(n, 42 + width, 45.0)
        for w in range(3):
            for k in range(6):
                _plant(x, w * width + 700 + 5003 * k + (k & 1), word(invert=bool(k & 2)), k)
        add(name, x, ("pi_miss", "gsl_second_miss"), writes=(width,), predicate=_p_scan_over_nmatch)
    # five lone words, then the word on both arms as the sixth position of the first write: a sync the scan did not record (then junk frames, carrier up)
    x = noise(3 * 65536, 47, 45.0)
    for k in range(5):
        _plant(x, 900 + 4001 * k + (k & 1), word(invert=bool(k & 1)), k)
    x[30011:30011 + 64] = soft(two_arm(UWB, UWB))
    add("noise_five_words_then_sync", x, ("sy_sync",), writes=(65536,),
        predicate=_check("the sync is not behind the scan's fourth position", lambda c, r: (lambda q: len(q) >= 6 and q[4] < r["events"][r["events"][:, 1] == 2][0, 0] <= q[-1] + 1)(
            scan_positions(c.stream[:65536]))))
    # a marker behind position 32 768 (seen only by the scan's q >= n loop) in a locked channel
    x = np.concatenate([noise(1250, 43), soft(b)])[:3 * 65536].copy()
    x = np.insert(x, [65536 + 40000, 2 * 65536 + 65000], -1)[:3 * 65536]
    add("marker_behind_32768", x, ("w_marker",), writes=(65536,), predicate=_p_marker_behind_scan)
    # unlocked (noise), the first unique word of the stream behind position 32 768 of the second write
    x = np.concatenate([noise(65536 + 40011, 44, 45.0), soft(b[:8 * T])])
    x = np.concatenate([x, noise(3 * 65536 - len(x), 45, 45.0)]) if len(x) < 3 * 65536 else x[:3 * 65536]
    add("acquires_behind_32768", x, ("sy_sync",), writes=(65536,), predicate=_p_sync_behind_scan)
    # a false sync (word on both arms) in noise, ending at 32 768 + 5 of the first write (the channel then counts junk frames with its carrier up), and three
    # lone words 150 soft bits apart in the second
    x = noise(3 * 65536, 46, 45.0)
    x[32768 + 5 - 63:32768 + 6] = soft(two_arm(UWB, UWB))
    for k in range(3):
        _plant(x, 65536 + 9000 + 150 * k, word(invert=bool(k & 1)), k)
    add("false_sync_at_32768", x, ("sy_sync", "sy_short"), writes=(65536,))
    return out


# ------------------------------------------------------------------------------------------------------------ R / T packets
def _rb(seed, n):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def _burst(fb, body, *, lead=80, wordbits=None, seed=0, inv=(False, False), gap=0, marker=True, gapsigma=40.0):
    """[marker] + lead noise + unique word + body bits + gap noise, the total number of soft bits even"""
    oq = fb == 10500
    w = wordbits if wordbits is not None else (two_arm(UWB, UWB) if oq else UWB)
    bits = np.concatenate([w, body]).astype(np.uint8)
    if oq:
        bits[0::2] ^= 1 if inv[0] else 0
        bits[1::2] ^= 1 if inv[1] else 0
    elif inv[0]:
        bits ^= 1
    n = lead + len(bits) + gap
    parts = [np.array([-1], np.int16)] if marker else []
    parts += [noise(lead, 7000 + seed), soft(bits), noise(gap + (n & 1), 7100 + seed, gapsigma)]
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def rt_cases(fam):
    fb = FAMILIES[fam][0]
    oq = fb == 10500
    total = fb if oq else 3 * fb
    cases = []

    def add(name, stream, hits=(), **kw):
        cases.append(Case(f"{fam}.{name}", fam, np.asarray(stream, dtype=np.int16), tuple(hits), **kw))

    pre = noise(64, 1)
    R = lambda s, **kw: (AF.rt_packet_bits if oq else AF.rt_packet_bits_msk)("R", _rb(s, 17), **kw)
    tail = max(total + 200, 3500)  # soft bits behind a word: past the end of signal and the dropped rest of its group, and past 50 blocks
    if oq:
        Tp = lambda s, n, **kw: AF.rt_packet_bits("T", (_rb(s, 4), [_rb(s + 1 + k, 10) for k in range(n)]), **kw)
        add("r_and_t", np.concatenate([pre, _burst(fb, R(1), seed=1, gap=tail), _burst(fb, Tp(2, 3), seed=2, inv=(True, False), gap=tail)]),
            ("rt_r_ok", "rt_t_ok", "rt_trial_128", "rt_full", "wr_end_of_signal", "pi_inv_hit", "inv_on"), ticks={-1: 6})
        # a good header CRC with a bad unit CRC: the trial fails at that length and at every longer one; the next word finds RT_TEST_FAILED.  (The next word has
        # to come more than 4924 soft bits behind the first: until then the detectors of a channel with carrier are off.)
        add("t_bad_unit_crc", np.concatenate([pre, _burst(fb, Tp(3, 3, bad_crc=(2,)), seed=3, gap=5000, gapsigma=2.0), _burst(fb, R(4), seed=4, gap=tail)]),
            ("rt_t_hdr_ok", "rt_t_su_bad", "rt_t_test_failed", "br_reset_bad", "rt_r_ok"))
        add("r_bad_crc_then_word", np.concatenate([pre, _burst(fb, R(5, bad_crc=(0,)), seed=5, gap=5200), _burst(fb, R(6), seed=6, lead=60, gap=tail)]),
            ("rt_r_fail", "br_reset_bad", "rt_r_ok"))
        # a word, then noise: the block fills to 6080 (the last trial says RT_BAD), then RT_FULL to the end of signal
        add("block_fills", np.concatenate([pre, _burst(fb, noise(0, 0), seed=7, gap=tail)]),
            ("rt_t_bad_full", "rt_full", "br_bad_event", "wr_end_of_signal", "rt_t_hdr_bad"))
        # |muw - 80| <= 150: the word's last bit is soft bit lead + 64 behind the marker
        add("muw_230", np.concatenate([pre, _burst(fb, R(8), lead=166, seed=8, gap=tail)]), ("bm_accept", "rt_r_ok"),
            predicate=_packet)
        add("muw_231", np.concatenate([pre, _burst(fb, R(9), lead=167, seed=9, gap=1500)]), ("bm_refuse",),
            predicate=_no_packet)
        # tolerance 4: 4 wrong bits on either arm is a word, 5 on one arm is none; 28 of 32 = the complement with 4 wrong, 27 is none
        add("word_4_errors", np.concatenate([pre, _burst(fb, R(10), wordbits=two_arm(word(errors=4, seed=1), word(errors=4, seed=2)), seed=10, gap=tail)]),
            ("pi_up_hit", "rt_r_ok"), predicate=_packet)
        add("word_5_errors", np.concatenate([pre, _burst(fb, R(11), wordbits=two_arm(word(errors=5, seed=3), UWB), seed=11, gap=1500)]), ("pi_miss",),
            predicate=_no_packet)
        add("complement_4_errors", np.concatenate([pre, _burst(fb, R(12), wordbits=two_arm(word(errors=4, seed=4), word(errors=4, seed=5)), inv=(True, True), seed=12, gap=tail)]),
            ("pi_inv_hit", "rt_r_ok", "inv_soft_gt", "inv_soft_lt"), predicate=_packet)
        add("complement_5_errors", np.concatenate([pre, _burst(fb, R(13), wordbits=two_arm(word(errors=5, seed=6), UWB), inv=(True, True), seed=13, gap=1500)]), ("pi_miss",),
            predicate=_no_packet)
        # ticks drop the carrier inside a packet: the detectors run again over the packet's bits (`!datacd`), with the arms' flags as they are
        x = np.concatenate([pre, _burst(fb, Tp(14, 20), seed=14, inv=(False, True), gap=tail)])
        add("ticks_inside_packet", x, ("oq_det_nodcd", "tick_drop", "tick_pos", "tick_zero", "tick_keep"), ticks={64 + 1 + 80 + 64 + 700: 5})
        x = _weaken(_burst(fb, Tp(15, 4), seed=15, inv=(True, True), gap=tail), 1 + 80 + 64, 1 + 80 + 64 + 64 * 14, 3)
        add("erasures_on_inverted_arms", np.concatenate([pre, x]), ("inv_soft_128",))
        # markers inside a word, inside a packet that is being collected, as first and last entry of a write
        x = np.concatenate([pre, _burst(fb, Tp(16, 6), seed=16, gap=tail), _burst(fb, R(17), seed=17, gap=tail)])
        m = [64 + 1 + 80 + 21, 64 + 1 + 80 + 64 + 501, WIDTH, 2 * WIDTH - 1]
        for q in m:
            x[q:q + 2] = -1      # two markers in place of a pair of soft bits: the pairs behind stay pairs
        add("markers", x, ("w_marker",), writes=(WIDTH,))
        add("values_above_255", _big(np.concatenate([pre, _burst(fb, Tp(18, 5), seed=18, inv=(True, False), gap=tail)]), 6), ("rt_t_ok",))
        add("muw_saturates", np.concatenate([pre, _burst(fb, R(19), seed=19, gap=tail), noise(100200, 20)]), ("w_muw_sat", "cn_sat"), writes=(WIDTH, 1 << 30))
    else:
        Tm = lambda s, n, **kw: AF.rt_packet_bits_msk("T", (_rb(s, 4), [_rb(s + 1 + k, 10) for k in range(n)]), **kw)
        add("r_and_t", np.concatenate([pre, _burst(fb, R(1), seed=1, gap=tail), _burst(fb, Tm(2, 5), seed=2, inv=(True, False), gap=tail)]),
            ("mu_r_ok", "mu_t_ok", "mu_trial_5", "mu_trial_11", "mu_trial_target", "mu_11_plain", "mu_full", "wr_end_of_signal", "pi_inv_hit", "inv_on"), ticks={-1: 6})
        # the announced count: 0 -> 11 blocks (announced at 11 and never looked at again); 14 -> 16 halved to 9 units, 32 blocks; 60 -> 62 halved to 32 units, 101 blocks, above the block's 95
        add("target_11", np.concatenate([pre, _burst(fb, Tm(3, 3, count=0), seed=3, gap=tail, gapsigma=2.0)]),
            ("mu_trial_11", "mu_11_plain", "mu_trial_50", "mu_hdr_ok_no_match"),
            predicate=_all(_final(rt_targetBlocks=11), _no_packet))
        add("target_halved", np.concatenate([pre, _burst(fb, Tm(4, 10, count=14), seed=4, gap=tail)]), ("mu_11_halved", "mu_t_ok"),
            predicate=_final(rt_targetBlocks=32, rt_targetSUSize=9))
        add("target_above_95", np.concatenate([pre, _burst(fb, Tm(5, 4, count=60), seed=5, gap=tail, gapsigma=2.0)]), ("mu_11_halved",),
            predicate=_final(rt_targetBlocks=101))
        # (the collector goes on behind the end of signal -- cntr stays saturated at >= 16 -- so 50 blocks are within reach at 600 bps' 1800-bit countdown too)
        add("target_50", np.concatenate([pre, _burst(fb, Tm(6, 16), seed=6, gap=tail)]), ("mu_trial_target", "mu_t_ok"), predicate=_final(rt_targetBlocks=50))
        add("bad_header_at_11", np.concatenate([pre, _burst(fb, Tm(7, 5, bad_crc=(0,)), seed=7, gap=tail)]), ("mu_hdr_bad", "br_bad_event"))
        add("r_bad_crc", np.concatenate([pre, _burst(fb, R(8, bad_crc=(0,)), seed=8, gap=300), _burst(fb, R(9), seed=9, gap=tail)]), ("mu_r_fail", "mu_r_ok"))
        # muw > 250 refuses a word and puts the inversion flag back: an inverted packet with the upright word (weak soft values: erasures to the Viterbi decoder)
        # written over 32 of its channel bits more than 250 soft bits behind the marker
        x = _burst(fb, Tm(10, 6), seed=10, inv=(True, False), gap=tail)
        at = 1 + 80 + 32 + 16 * 64 + 7
        x[at:at + 32] = np.where(UWB > 0, 131, 124)
        add("late_word_restores_inversion", np.concatenate([pre, x]), ("mk_refuse", "mu_t_ok"))
        add("muw_250", np.concatenate([pre, _burst(fb, R(11), lead=218, seed=11, gap=tail)]), ("mk_accept", "mu_r_ok"))
        add("muw_251", np.concatenate([pre, _burst(fb, R(12), lead=219, seed=12, gap=tail)]), ("mk_refuse",),
            predicate=_no_packet)
        add("word_4_errors", np.concatenate([pre, _burst(fb, R(13), wordbits=word(errors=4, seed=1), seed=13, gap=tail)]), ("pi_up_hit", "mu_r_ok"))
        add("word_5_errors", np.concatenate([pre, _burst(fb, R(14), wordbits=word(errors=5, seed=2), seed=14, gap=900)]), ("pi_miss",),
            predicate=_no_packet)
        add("complement_4_errors", np.concatenate([pre, _burst(fb, R(15), wordbits=word(errors=4, seed=3), inv=(True, False), seed=15, gap=tail)]),
            ("pi_inv_hit", "mu_r_ok", "inv_soft_gt", "inv_soft_lt"))
        add("complement_5_errors", np.concatenate([pre, _burst(fb, R(16), wordbits=word(errors=5, seed=4), inv=(True, False), seed=16, gap=900)]), ("pi_miss",),
            predicate=_no_packet)
        x = np.concatenate([pre, _burst(fb, Tm(17, 8), seed=17, gap=tail)])
        add("ticks_inside_packet", x, ("tick_drop", "tick_pos", "tick_zero", "tick_keep"), ticks={64 + 1 + 80 + 32 + 500: 5})
        x = _weaken(_burst(fb, Tm(18, 5), seed=18, inv=(True, False), gap=tail), 1 + 80 + 32, 1 + 80 + 32 + 64 * 20, 3)
        add("erasures_on_inverted_stream", np.concatenate([pre, x]), ("inv_soft_128",))
        x = np.concatenate([pre, _burst(fb, Tm(19, 6), seed=19, gap=tail), _burst(fb, R(20), seed=20, gap=tail)])
        for q in (64 + 1 + 80 + 11, 64 + 1 + 80 + 32 + 301, WIDTH, 2 * WIDTH - 1):
            if q + 2 <= len(x):
                x[q:q + 2] = -1
        add("markers", x, ("w_marker",), writes=(WIDTH,))
        add("values_above_255", _big(np.concatenate([pre, _burst(fb, Tm(21, 5), seed=21, inv=(True, False), gap=tail)]), 7), ("mu_t_ok",))
        add("muw_saturates", np.concatenate([pre, _burst(fb, R(22), seed=22, gap=tail), noise(100200, 23)]), ("w_muw_sat", "cn_sat"), writes=(WIDTH, 1 << 30))
    return tuple(cases)


# ------------------------------------------------------------------------------------------------------------ C channel
def _cframes(nfr, seed, units=None):
    rng = np.random.default_rng(seed)
    fr = [(rng.integers(0, 256, 300, dtype=np.uint8), [bytes(rng.integers(1, 256, 10, dtype=np.uint8)) for _ in range(3)]) for _ in range(nfr)]
    for (f, k), u in (units or {}).items():
        fr[f][1][k] = bytes(u)
    return fr


@functools.lru_cache(maxsize=None)
def c_cases(fam="C8400"):
    cases = []

    def add(name, stream, hits=(), **kw):
        cases.append(Case(f"{fam}.{name}", fam, np.asarray(stream, dtype=np.int16), tuple(hits), **kw))

    lead = np.random.default_rng(3).integers(0, 2, 74, dtype=np.uint8)
    end = np.zeros(300, np.uint8)
    base = AF.c_channel_bits(_cframes(4, 50))

    def with_words(bits, frame, wr, wi):
        x = bits.copy()
        x[4200 * frame:4200 * frame + 104] = two_arm(wr, wi)
        return x

    # tolerance 6 on 52 bits: 6 wrong is a word, 7 is none; 46 = the complement with 6 wrong, 45 is none; on the first pattern (real arm) and the second (imag)
    for pat, pname in ((0, "first"), (1, "second")):
        for inv in (False, True):
            for k in (6, 7):
                wr = word(C_W1, k if pat == 0 else 0, inv, seed=10 + k)
                wi = word(C_W2, k if pat == 1 else 0, inv, seed=20 + k)
                bits = AF.c_channel_bits(_cframes(4, 51 + k + 2 * pat), invert_real=inv, invert_imag=inv)
                x = with_words(bits, 2, wr, wi)
                hit = ("c_p1_inv" if inv else "c_p1_up") if pat == 0 else ("c_p2_inv" if inv else "c_p2_up")
                add(f"{pname}_pattern_{'complement_' if inv else ''}{k}_errors", soft(np.concatenate([lead, x, end])), (hit,) if k == 6 else ("c_miss", "gsl_second_miss"),
                    predicate=_check("6 errors are a word, 7 are none", lambda c, r, k=k: int((r["events"][:, 1] == 2).sum()) == (4 if k == 6 else 3)))
    # a unique word before the frame's end: the frame is abandoned, ncdel restarts.  The detectors are off (and their registers stand still) up to cntr 3984, so the
    # word's 104 bits have to lie in cntr 3985 .. 4094: frame 1 loses the last 108 of its 4096 bits
    x = np.concatenate([base[:4200 + 104 + 3988], base[2 * 4200:]])
    add("sync_mid_frame", soft(np.concatenate([lead, x, end])), ("c_sync", "c_det_off"), writes=(WIDTH,),
        predicate=_check("no frame was abandoned", lambda c, r: int((r["events"][:, 1] == 2).sum()) == 4 and len(r["voice"]) == 3))
    # a stream that starts with its first frame (the codec's first call; that frame's units are lost).  DecodeC's unique word leaves the countdown alone: six good
    # units take it to 12, then bad ones 7, 2, -3; the next tick makes it 0 and drops the carrier
    fr = _cframes(5, 60, {(3, 0): _bad(60), (3, 1): _bad(61), (3, 2): _bad(62)})
    add("first_frame_and_negative_countdown", soft(AF.c_channel_bits(fr)), ("c_bad_dec", "c_ok_inc", "c_dcd_rise", "tick_neg", "tick_drop"),
        ticks={-1: 2}, predicate=_all(_final(datacd=0, datacdcountdown=0), _check("the countdown was not -3", lambda c, r: r["dcd"].tolist() == [0, 0])))
    # a bad unit costs 5 here (3 on the P channel): 12 -> 7 -> 9 -> 11, and the fifth tick drops the carrier (8 5 2 -1 0); at 3 it would be the sixth
    fr = _cframes(5, 66, {(3, 0): _bad(66)})
    add("one_bad_unit_then_ticks", soft(AF.c_channel_bits(fr)), ("c_bad_dec", "tick_neg", "tick_drop"), ticks={-1: 7},
        predicate=_check("the carrier did not drop at the fifth tick", lambda c, r: r["dcd"].tolist() == [1, 1, 1, 1, 0, 0, 0]))
    # a long stretch without a word: cntr runs on past the frame, nothing is stored; then frames again
    x = np.concatenate([base[:2 * 4200], np.zeros(9000, np.uint8), AF.c_channel_bits(_cframes(3, 61))])
    add("long_stretch_without_sync", soft(np.concatenate([lead, x, end])), ("c_nostore", "c_cntr_sat", "c_det_window"))
    # ticks until the carrier is lost (12 9 6 3 0), then frames again: good units 2, 4: the frame end raises the carrier
    x = np.concatenate([lead, base, end])
    more = AF.c_channel_bits(_cframes(3, 62))
    add("carrier_loss_and_reacquisition", soft(np.concatenate([x, more, end])), ("tick_pos", "tick_zero", "tick_drop", "tick_keep", "c_dcd_rise", "c_ok_inc", "c_ok_cap"),
        ticks={len(x) + 104 + 1500: 6})
    # all units bad: the countdown never leaves 0
    fr = _cframes(4, 63, {(f, k): _bad(70 + 3 * f + k) for f in range(4) for k in range(3)})
    add("all_units_bad", soft(np.concatenate([lead, AF.c_channel_bits(fr), end])), ("c_bad_floor", "tick_zero"), ticks={-1: 1})
    # exact 128 on inverted arms; values 256 .. 32767
    bits = AF.c_channel_bits(_cframes(3, 64), invert_real=True, invert_imag=True)
    x = soft(np.concatenate([lead, bits, end]))
    for f in (1, 2):
        x = _weaken(x, 74 + 4200 * f + 104, 74 + 4200 * (f + 1), 3, junk=f)
    add("erasures_on_inverted_arms", x, ("inv_soft_128", "inv_soft_gt", "inv_soft_lt", "c_p1_inv", "c_p2_inv"))
    bits = AF.c_channel_bits(_cframes(3, 65), invert_real=True)
    add("values_above_255", _big(soft(np.concatenate([lead, bits, end])), 8), ("c_ok_inc",))
    # one soft bit per write across the end of a frame, empty writes, a write exactly WIDTH long
    fe = 74 + 4200 + 104 + 4096 - 1
    add("one_bit_writes_across_a_frame_end", soft(np.concatenate([lead, base, end])), ("c_frame_end",), writes=(fe - 2,) + (1,) * 5 + (0, WIDTH, 0, 1 << 30))
    return tuple(cases)


def cases(fam):
    return p_cases(fam) if fam.startswith("P") else rt_cases(fam) if fam.startswith("RT") else c_cases(fam)


def all_cases():
    return [c for fam in FAMILIES for c in cases(fam)]


def chain_counters(O, fam):
    return [n for n in O.AeroL.coverage_names() if n.startswith(CHAINS[fam]) and not (fam.startswith("P") and n.startswith("pi_") and fam != "P10500")]


# ------------------------------------------------------------------------------------------------------------ banks
NCH = 70  # two wave groups, the second with six live lanes
_SLOTS = [0, 1, 31, 63, 64, 69] + [c for c in range(2, 69, 3) if c not in (31, 63, 64)] + [c for c in range(3, 69, 3) if c not in (63,)]


@functools.lru_cache(maxsize=None)
def filler(fam, c):
    """an ordinary generated channel of the family (what the existing bank tests feed), for the lanes between the cases"""
    fb, burst = FAMILIES[fam]
    rng = np.random.default_rng(9000 + c)
    if fam == "C8400":
        _, x = AF.c_channel_case(9100 + c, 3, 10.0 + 5.0 * (c % 5), inv=(bool(c & 1), bool(c & 2)), lead=int(rng.integers(0, 900)))
    elif not burst:
        bits, _ = AF.p_channel_bits(AF.random_payloads(4, fb, seed=9200 + c), fb, invert_i=bool(c & 1), invert_q=bool(c & 2))
        x = AF.to_soft(np.concatenate([rng.integers(0, 2, int(rng.integers(0, 900)), dtype=np.uint8), bits]), sigma=float(rng.uniform(0, 40)), seed=c)
    elif fb == 10500:
        pk = [("R", _rb(9300 + c, 17)), ("T", (_rb(9400 + c, 4), [_rb(9500 + 7 * c + k, 10) for k in range(2 + c % 4)]))]
        x = AF.rt_burst_stream(pk, sigma=float(rng.uniform(8, 40)), seed=c, invert_i=bool(c & 1), invert_q=bool(c & 2), gap=1500 + 2 * c)
    else:
        pk = [("R", _rb(9300 + c, 17)), ("T", (_rb(9400 + c, 4), [_rb(9500 + 7 * c + k, 10) for k in range(4 + c % 4)]))]
        x = AF.rt_burst_stream_msk(pk, sigma=float(rng.uniform(8, 35)), seed=c, invert=bool(c & 1), gap=1200 + 2 * c)
    return Case(f"{fam}.filler{c}", fam, x, writes=tuple(int(v) for v in rng.integers(1, WIDTH + 1, 5)))


@functools.lru_cache(maxsize=None)
def filler_wide(c):
    """a locked 10 500 bps channel three writes of 65 536 long: the same frames on every channel, its own lead, noise and arm polarities"""
    rng = np.random.default_rng(9600 + c)
    b = _wide_bits().copy()
    b[0::2] ^= c & 1
    b[1::2] ^= (c >> 1) & 1
    x = np.concatenate([noise(int(rng.integers(0, 5250)), 9700 + c, 45.0), AF.to_soft(b, sigma=float(rng.uniform(0, 30)), seed=c)])[:3 * 65536]
    return Case(f"P10500.filler_wide{c}", "P10500", x, writes=(65536,), wide=True, width=65536)


def bank(fam, which, width=None):
    """One bank's worth: (per-channel cases, per-channel plans, ticks behind each bank write, ticks behind the last, stride).  which: "quiet" = the cases
    without ticks inside their stream, "ticked" = the others (every channel of the bank gets their ticks), "wide" = the 40 000 / 65 536 wide cases."""
    width = width or (65536 if which == "wide" else WIDTH)
    sel = [c for c in cases(fam) if c.wide == (which == "wide") and (which == "wide" or (any(k >= 0 for k in c.ticks) == (which == "ticked")))]
    assert len(sel) <= len(_SLOTS)
    chan = {_SLOTS[i]: c for i, c in enumerate(sel)}
    per = [chan.get(c) or (filler_wide(c) if which == "wide" else filler(fam, c)) for c in range(NCH)]
    plans = [schedule(c, None if which == "wide" else width, final=False) for c in per]
    nw = max(len(p) for p in plans)
    ticks = [max((p[k][2] if k < len(p) else 0) for p in plans) for k in range(nw)]
    last = max([int(c.ticks.get(-1, 0)) for c in per])
    stride = width + (64 if FAMILIES[fam][1] else 0)
    assert all(e - s <= stride for p in plans for s, e, _ in p)
    return per, plans, ticks, last, stride


def bank_writes(per, plans, ticks, last, stride):
    """the bank's writes in order: (buf int16 [NCH, stride], counts int32 [NCH], per-channel segments, ticks behind this write)"""
    nw = len(ticks)
    for k in range(nw):
        buf = np.zeros((len(per), stride), np.int16)
        cnt = np.zeros(len(per), np.int32)
        segs = []
        for c, (case, plan) in enumerate(zip(per, plans)):
            s, e = plan[k][:2] if k < len(plan) else (0, 0)
            buf[c, :e - s] = case.stream[s:e]
            cnt[c] = e - s
            segs.append(case.stream[s:e])
        yield buf, cnt, segs, ticks[k] + (last if k == nw - 1 else 0)


def oracle_write(O, a, case, seg):
    if case.burst:
        for g0, g1 in O.demod_groups(seg):
            a.write(seg[g0:g1])
    elif len(seg):
        a.write(seg)
