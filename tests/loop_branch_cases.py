"""The cases of tests/test_gpu_loop_branches.py: streams, pokes and write plans that take the continuous sample loops (k_oqpsk_fb, k_msk_fb,
k_msk_samples) through the branches ordinary test signals never reach, and the oracle's result for each.  tests/test_loop_branch_cases.py
checks on the CPU that every case takes the branch it exists for.

A GROUP is one bank's worth: at most five cases, one stream length and ONE write plan (a bank writes all its channels together).  The plan
cycles WRITES, is cut wherever a case pokes, and carries one-sample writes at the samples a meter case needs (SINGLES) and at the end
([..., 1, 1, 1]): the device evaluates the EbNo formula only over the last JD_EBNO_TAIL samples of a launch, a one-sample write puts a chosen
sample there.

Streams.  An OQPSK stream starts HEAD samples RATIO times louder than it goes on (the same signal, a level step of 24 dB): the AGC's
window is 4 s long and starts empty, so a 1 s stream at one level is clipped to |sig2| = 2.84 from end to end, the symbol-timing detector --
which works on the envelope -- sees nothing and st_osc free-runs.  Behind the loud head the window holds what a full one would, the clip
stops (sample ~18 000) and the timing loop runs: only then does st_osc's frequency move by more than the sign of a zero decides.
A meter group is longer than 48 000 samples because the EbNo window is 2 Fs long and starts empty: mvr's floor / tebno > 50 (OQPSK) and
the NaN / > 50 lines (MSK) need var <= 0.0247 mean^2 resp. 2 var / mean^2 <= 0.0085, which a window that still holds initial zeros cannot
give; the silence cases need the whole window silent behind a signal."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np

import kernel_variants as KV

FAMILIES = ("oqpsk_10500", "oqpsk_8400", "msk_1200", "msk_600", "msk_1200_24k", "msk_1200_12k")
WRITES = [4096, 3000, 1, 777, 4095, 2048]  # cycled; 4096 = max_write_samples
MAX_WRITE = 4096
NCH = 70  # two channel groups, the second with six live lanes
SPECIAL = (0, 1, 63, 64, 69)  # the channels that carry the cases; every other channel carries the neighbour of SPECIAL[c % 5]
N_LOOP = 48000
MID = 21114  # a boundary of the plain write cycle (one cycle + 4096 + 3000 + 1), in lock: where the mid-stream pokes go
LATE = 35131  # another (two cycles + 4096 + 3000 + 1)
HEAD, RATIO = 12000, 16.0
THRESH = {"oqpsk": 0.65, "msk": 0.5}

# Branches a family's chain does not have, with the oracle line that says so (oracle/jaero_oracle.c).
_NO_OQ_METER = {k: "msk_write calls msk_ebno_update: oqpsk_ebno_update's lines are not in the MSK chain" for k in
                ("oq_mvr_floor", "oq_tebno_hi", "oq_tebno_lo", "oq_nan")}
_MSK_ONLY = dict(_NO_OQ_METER, **{
    "st_low": "msk_write moves st_osc by AdvanceFractionOfWave alone: no frequency term, no clamp against st_osc_ref",
    "st_high": "msk_write moves st_osc by AdvanceFractionOfWave alone: no frequency term, no clamp against st_osc_ref",
    "sym_gated": "msk_write pushes both soft bits of every symbol: no `if (d->mse < d->signalthreshold)` around them",
    "mu_floor": "msk_write forms mse with its own moving average (msema): msecalc_update and its mu floor are OQPSK's",
    "m2_countdown2": "jo__msk_slot has no countdown2: mixer2 is only set by its `mse > signalthreshold && fabs(...) > 0.0` rule",
})
_OQ_ONLY = {"msk_nan": "oqpsk_write calls oqpsk_ebno_update: msk_ebno_update's lines are not in the OQPSK chain",
            "msk_tebno_hi": "oqpsk_write calls oqpsk_ebno_update: msk_ebno_update's lines are not in the OQPSK chain"}
NOT_IN_CHAIN = {
    "oqpsk_10500": dict(_OQ_ONLY),
    "oqpsk_8400": dict(_OQ_ONLY, lf_pi2_pos="oqpsk_write: the +-pi/2 clamp is inside `if (d->fb > 8400)`; the 8400 branch moves the phase by the raw error",
                       lf_pi2_neg="oqpsk_write: the +-pi/2 clamp is inside `if (d->fb > 8400)`; the 8400 branch moves the phase by the raw error"),
    "msk_1200": _MSK_ONLY, "msk_600": _MSK_ONLY, "msk_1200_24k": _MSK_ONLY, "msk_1200_12k": _MSK_ONLY,
}
# The AFC recentre and its two clamps run in the estimate kernel's slot, not in a sample loop: credited to the test that drives all three
# (m2 inside, below the lower clamp, above the upper) through that kernel.  k_coarse6_13 and its slot serve every MSK family.
AFC_COUNTERS = ("afc_recentre", "afc_clamp_lo", "afc_clamp_hi")
AFC_CREDIT = {
    "oqpsk_10500": ("tests/test_gpu_coarse.py", "test_recentre_inside_a_persistent_list", "oqpsk_10500"),
    "oqpsk_8400": ("tests/test_gpu_coarse.py", "test_recentre_inside_a_persistent_list", "oqpsk_8400"),
    "msk_1200": ("tests/test_gpu_coarse.py", "test_recentre_inside_a_persistent_list", "msk_1200"),
    "msk_600": ("tests/test_gpu_coarse.py", "test_recentre_inside_a_persistent_list", "msk_1200"),
    "msk_1200_24k": ("tests/test_gpu_coarse.py", "test_recentre_inside_a_persistent_list", "msk_1200"),
    "msk_1200_12k": ("tests/test_gpu_coarse.py", "test_recentre_inside_a_persistent_list", "msk_1200_12k"),
}


@dataclass(frozen=True)
class Case:
    name: str
    stream: tuple  # argument of stream(): (builder, family, ...)
    pokes: tuple = ()  # ((sample, (("field", value), ...)), ...): jo_loop_state fields set in front of the write that starts at `sample`
    branch: tuple = ()  # counters this case exists for: each taken at least once
    crossing: bool = False  # ... and not taken in every sample: 0 < count < samples
    on_clamp: bool = False  # T1: every peek of st_freq is compared bit for bit
    singles: tuple = ()  # ((offset from the group's first single, counter), ...): taken INSIDE that one-sample write
    at_end: tuple = ()  # counters taken inside the last one-sample write of the plan
    at_start: tuple = ()  # counters taken inside the first write of the plan, which is one sample long in a meter group
    locked: bool = True  # mse below the threshold at the end
    noise: bool = True  # False: the stream is digital silence or a tone built on exact samples; noise draws leave exact zeros alone


@dataclass(frozen=True)
class Group:
    family: str
    name: str
    n: int
    cases: tuple
    single_from: tuple = ()  # (case index, counter): the plan's one-sample writes start at the first sample where that case takes the counter

    @property
    def id(self):
        return f"{self.family}-{self.name}"


def fam(family):
    return KV.FAMILIES[family]


def oracle_settings(O, family):
    f = fam(family)
    if f["kind"] == "oqpsk":
        return O.oqpsk_settings(freq_center=8000.0, lockingbw=f["fb"], fb=f["fb"], Fs=f["Fs"], power=f["power"], threshold=0.65)
    return O.msk_settings(freq_center=1000.0, lockingbw=1.5 * f["fb"], fb=f["fb"], Fs=f["Fs"], power=f["power"], threshold=0.5)


def bank_settings(family):
    from jaero_amd import demodulator as D

    f = fam(family)
    if f["kind"] == "oqpsk":
        return D.OqpskSettings(freq_center=8000.0, lockingbw=f["fb"], fb=f["fb"], Fs=f["Fs"], coarsefreqest_fft_power=f["power"], signalthreshold=0.65)
    return D.MskSettings(freq_center=1000.0, lockingbw=1.5 * f["fb"], fb=f["fb"], Fs=f["Fs"], coarsefreqest_fft_power=f["power"], signalthreshold=0.5)


def stref(family):
    """st_osc's frequency as setSettings leaves it: fb (OQPSK), fb / 2 (MSK)"""
    f = fam(family)
    return f["fb"] if f["kind"] == "oqpsk" else f["fb"] / 2


# ---- streams ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream(key):
    """int16 samples of a case's stream.  key = (builder, family, n, ...)"""
    from jaero_amd import signalgen as G

    kind, family, n = key[:3]
    f = fam(family)
    fb, Fs = f["fb"], f["Fs"]
    seed0 = G.SEED_BASE + 7700 + 100 * FAMILIES.index(family)
    if kind == "oq":  # (ppm, ebno_db or None, seed): the loud head, then RATIO times quieter
        ppm, ebno, seed = key[3:]
        loud = G.oqpsk(n, fb=fb * (1.0 + ppm * 1e-6), Fs=Fs, ebno_db=ebno, seed=seed0 + seed, peak=0.9)[0]
        quiet = G.oqpsk(n, fb=fb * (1.0 + ppm * 1e-6), Fs=Fs, ebno_db=ebno, seed=seed0 + seed, peak=0.9 / RATIO)[0]
        return np.concatenate([loud[:HEAD], quiet[HEAD:]])
    if kind == "oq_flat":  # (ebno_db or None, seed): one level from end to end (the meter cases: the EbNo window must not hold a level step)
        ebno, seed = key[3:]
        return G.oqpsk(n, fb=fb, Fs=Fs, ebno_db=ebno, seed=seed0 + seed)[0]
    if kind == "msk":  # (ebno_db or None, seed)
        ebno, seed = key[3:]
        return G.msk(n, fb=fb, Fs=Fs, ebno_db=ebno, seed=seed0 + seed)[0]
    if kind == "tone":  # (Hz, amplitude): a noiseless tone of constant envelope
        hz, amp = key[3:]
        return np.round(amp * 32768.0 * np.cos(2.0 * np.pi * hz * np.arange(n) / Fs)).astype(np.int16)
    if kind == "narrow":  # (bit rate, seed): a noiseless MSK carrier far narrower than the channel, at the channel's centre: constant envelope
        fbm, seed = key[3:]
        return np.round(G.msk(n, fb=fbm, Fs=Fs, fc=8000.0, ebno_db=None, seed=G.SEED_BASE + 5000 + seed)[0] * (0.2 / 0.3)).astype(np.int16)
    if kind == "then_silence":  # (inner key, nsignal): a stream, then digital silence to the end
        inner, nsig = key[3:]
        x = np.zeros(n, dtype=np.int16)
        x[:nsig] = stream(inner)[:nsig]
        return x
    raise KeyError(key)


# ---- write plans -----------------------------------------------------------------------------------------------------------------------
def plan_writes(n, cuts=(), singles=()):
    """Write sizes summing to n: WRITES cycled, a boundary at every cut, a one-sample write at every entry of `singles` and at n - 3 .. n - 1."""
    singles = sorted(set(singles) | {n - 3, n - 2, n - 1})  # (a meter group passes sample 0 as well: the plan then starts with a one-sample write)
    stops = sorted(set(cuts) | set(singles) | {s + 1 for s in singles} | {n})
    out, pos, k = [], 0, 0
    while pos < n:
        nxt = min(s for s in stops if s > pos)
        m = min(WRITES[k % len(WRITES)], nxt - pos)
        out.append(m)
        pos += m
        k += 1
    assert sum(out) == n and out[-3:] == [1, 1, 1] and max(out) <= MAX_WRITE
    return out


def poke_dict(case):
    return {s: dict(fields) for s, fields in case.pokes}


# ---- the oracle on a case ---------------------------------------------------------------------------------------------------------------
def run(O, family, x, writes, pokes=None, capture=True):
    """The oracle on stream x (int16, or float64 on the same scale) under the write plan, jo_loop_state fields set in front of the writes that
    start at the samples of `pokes`.  Returns what the bank is compared with, the branch counters in total and per write, and the loop state
    behind every write."""
    pokes = pokes or {}
    d = O.Demod(oracle_settings(O, family), capture_symbols=capture)
    names = O.Demod.COVERAGE
    per_write, states, meter = np.zeros((len(writes), len(names)), dtype=np.int64), [], []
    prev = np.zeros(len(names), dtype=np.int64)
    s = 0
    left = set(pokes)
    for k, m in enumerate(writes):
        if s in pokes:
            d.set_loop_state(**pokes[s])
            left.discard(s)
        d.write(x[s:s + m])
        s += m
        cov = d.coverage()
        now = np.array([cov[k_] for k_ in names], dtype=np.int64)
        per_write[k] = now - prev
        prev = now
        states.append(d.loop_state)
        meter.append((d.ebno, d.tebno_raw))  # the meter's value behind the write; tebno of its last sample in front of the limits
    assert not left, ("a poke is not on a write boundary", sorted(left))
    ref = {"soft": d.take_soft(), "status": d.take_status(), "pending": d.pending, "mse": d.mse, "freq_est": d.freq_est,
           "freq_center": d.freq_center, "ebno": d.ebno}
    if capture:
        ref["symbols"] = d.take_symbols()
    return SimpleNamespace(ref=ref, cov=dict(zip(names, prev.tolist())), per_write=per_write, states=states, meter=meter, writes=list(writes),
                           starts=np.concatenate([[0], np.cumsum(writes)[:-1]]).tolist())


def first_taken(O, family, x, counter, start, writes):
    """First sample >= start in which the oracle takes `counter` on stream x: the write of the plan that holds it is found first, then the
    plan is repeated up to that write and the stream goes on sample by sample (at 8400 bps every write retunes the prefilter's mixer, so a
    long run of one-sample writes is another signal path)."""
    e = run(O, family, x, writes, capture=False)
    col = list(e.cov).index(counter)
    hit = [k for k, s in enumerate(e.starts) if s + e.writes[k] > start and e.per_write[k, col] > 0]
    if not hit:
        return -1
    d = O.Demod(oracle_settings(O, family))
    s = 0
    for m in writes[:hit[0]]:
        d.write(x[s:s + m])
        s += m
    base = d.coverage()[counter]
    while s < len(x):
        d.write(x[s:s + 1])
        s += 1
        if s > start and d.coverage()[counter] != base:
            return s - 1
        base = d.coverage()[counter]
    return -1


@functools.lru_cache(maxsize=None)
def group_plan(O, gid):
    """(write sizes, first single or -1) of a group."""
    g = GROUPS[gid]
    cuts = sorted({s for c in g.cases for s, _ in c.pokes})
    if not g.single_from:
        return tuple(plan_writes(g.n, cuts)), -1
    ci, counter = g.single_from
    c = g.cases[ci]
    x = stream(c.stream)
    # where the leading zeros leave the EbNo window (2 Fs): search from a little in front of it
    near = first_taken(O, g.family, x, counter, int(1.9 * fam(g.family)["Fs"]), plan_writes(g.n, cuts, [0]))
    assert near > 0, (gid, "the stream never takes", counter)
    offs = sorted({o for cc in g.cases for o, _ in cc.singles})
    # the write sizes in front of a sample change the 8400 bps prefilter's rounding, and with it the sample where a line is crossed: the
    # sample found under sample-by-sample writes is confirmed under the plan itself, its neighbours tried if it moved
    for p0 in (near, near - 1, near + 1, near - 2, near + 2):
        writes = plan_writes(g.n, cuts, [0] + [p0 + o for o in range(min(offs), max(offs) + 1)])
        if all(verdicts(g, c, run(O, g.family, x, writes, poke_dict(c), capture=False), p0).values()):
            return tuple(writes), p0
    raise AssertionError((gid, "no plan puts the lines of", c.name, "on one-sample writes near", near))


@functools.lru_cache(maxsize=None)
def expected(O, gid, ci, poked=True):
    """The oracle's run of case ci of a group (poked=False: its ordinary neighbour, the same stream without the pokes)."""
    g = GROUPS[gid]
    c = g.cases[ci]
    writes, _ = group_plan(O, gid)
    return run(O, g.family, stream(c.stream), writes, poke_dict(c) if poked else None)


def noisy(x, draw, seed=0):
    """x as float64 with additive noise at 1e-9 of its rms; exact zeros stay exact (digital silence is silence, not a quiet signal)."""
    xf = x.astype(np.float64)
    rms = float(np.sqrt(np.mean(xf[xf != 0.0] ** 2))) if np.any(xf) else 0.0
    rng = np.random.default_rng([0x10B, seed, draw])
    return xf + (xf != 0.0) * rng.normal(0.0, 1e-9 * rms, size=xf.shape)


def verdicts(g, c, e, p0):
    """Every taken / not-taken verdict the CPU test makes of a case, as a dict: what a noise draw must not change."""
    nsamp = sum(e.writes)
    v = {("taken", k): e.cov[k] > 0 for k in c.branch}
    if c.crossing:
        v.update({("not always", k): e.cov[k] < nsamp for k in c.branch})
    names = list(e.cov)
    for off, k in c.singles:
        w = e.starts.index(p0 + off)
        assert e.writes[w] == 1
        v[("single", off, k)] = bool(e.per_write[w, names.index(k)] == 1)
        if k.endswith("tebno_hi"):
            # ... and the line changes the meter's value behind that write by more than the 1e-6 it is compared to: 0.2 (tebno - 50)
            v[("observable", off, k)] = bool(0.2 * (e.meter[w][1] - 50.0) > 1e-3)
    for k in c.at_end:
        v[("end", k)] = bool(e.per_write[-1, names.index(k)] == 1)
    for k in c.at_start:
        assert e.writes[0] == 1
        v[("start", k)] = bool(e.per_write[0, names.index(k)] == 1)
    return v


# ---- the case list ---------------------------------------------------------------------------------------------------------------------
def _P(sample, **fields):
    return (sample, tuple(sorted(fields.items())))


def _oqpsk_groups(family):
    fb = fam(family)["fb"]
    lbw = fb
    lock = ("oq", family, N_LOOP, 0, 11.0, 1)
    # seeds and the place of the mid-stream poke from the CPU search: at 10.5 kbps the frequency term carries st_osc DOWN from the upper clamp
    # in every stream tried, so the "+" cases reach it in a handful of samples only, and only on some seeds
    ten = family == "oqpsk_10500"
    up, dn = ("oq", family, N_LOOP, +50, 11.0, 3 if ten else 0), ("oq", family, N_LOOP, -50, 11.0, 0 if ten else 1)
    mid_up = LATE if ten else MID
    quiet = ("oq", family, N_LOOP, 0, None, 2)
    # T1: st_osc on its clamp, symbol clock 50 ppm off; before the first write and in lock
    t1 = [Case("T1+", up, (_P(0, st_freq=fb + 0.1),), ("st_high",), on_clamp=True),
          Case("T1-", dn, (_P(0, st_freq=fb - 0.1),), ("st_low",), on_clamp=True),
          Case("T1+mid", up, (_P(mid_up, st_freq=fb + 0.1),), ("st_high",), on_clamp=True),
          Case("T1-mid", dn, (_P(MID, st_freq=fb - 0.1),), ("st_low",), on_clamp=True)]
    # T2: d short of the clamp at the nominal clock; d and the place of the poke from the CPU search
    if family == "oqpsk_10500":
        t2 = [Case("T2+", ("oq", family, N_LOOP, 0, 11.0, 3), (_P(0, st_freq=fb + (0.1 - 1e-8)),), ("st_high",), crossing=True),
              Case("T2-", lock, (_P(0, st_freq=fb - (0.1 - 1e-6)),), ("st_low",), crossing=True),
              Case("T2-mid", lock, (_P(MID, st_freq=fb - (0.1 - 1e-8)),), ("st_low",), crossing=True)]
    else:
        t2 = [Case("T2+mid", lock, (_P(MID, st_freq=fb + (0.1 - 1e-6)),), ("st_high",), crossing=True),
              Case("T2-", lock, (_P(0, st_freq=fb - (0.1 - 1e-6)),), ("st_low",), crossing=True),
              Case("T2-mid", lock, (_P(MID, st_freq=fb - (0.1 - 1e-7)),), ("st_low",), crossing=True)]
    # C2: mixer2 off by a part of lockingbw / 2 on a noiseless stream (the unlocked rule of the slot pulls it back)
    c2 = [Case("C2+", quiet, (_P(0, m2_freq=8000.0 + 0.45 * lbw),), ("m2_rule",)),
          Case("C2-", quiet, (_P(0, m2_freq=8000.0 - 0.45 * lbw),), ("m2_rule", "lf_pi2_pos") if ten else ("m2_rule",))]
    groups = [Group(family, "t1", N_LOOP, tuple(t1 + [Case("plain", lock)]))]
    if family == "oqpsk_10500":
        # C1: the loop filter's two last outputs at +-3: the next symbol's output passes pi / 2
        c1 = [Case("C1+", lock, (_P(0, lf_y1=3.0, lf_y2=3.0),), ("lf_pi2_pos",)),
              Case("C1-", lock, (_P(0, lf_y1=-3.0, lf_y2=-3.0),), ("lf_pi2_neg",)),
              Case("C1+mid", lock, (_P(MID, lf_y1=3.0, lf_y2=3.0),), ("lf_pi2_pos",)),
              Case("C1-mid", lock, (_P(MID, lf_y1=-3.0, lf_y2=-3.0),), ("lf_pi2_neg",))]
        groups += [Group(family, "t2c2", N_LOOP, tuple(t2 + c2)), Group(family, "c1", N_LOOP, tuple(c1 + [Case("plain", up)]))]
    else:
        groups += [Group(family, "t2c2", N_LOOP, tuple(t2 + c2))]
    # meters: E1 on a stream of constant level from end to end, E2 silence behind a locked stream, three ordinary seeds beside them
    nm = 14000 + 96000 + 200
    if family == "oqpsk_10500":
        e1 = Case("E1", ("oq_flat", family, nm, None, 16), singles=((0, "oq_tebno_hi"), (1, "oq_mvr_floor"), (2, "oq_mvr_floor")), locked=False)
    else:
        # the 8400 bps chain never reaches either line on a noiseless OQPSK stream (its envelope behind the alpha 0.6 filter varies by more
        # than 0.0247 mean^2); a signal of constant envelope does.  A bare tone does too, but the loops on an unmodulated carrier amplify a
        # 1e-9 change of the input to 1e-1 in the symbols (a modulated stream: 1e-3), and the FFT prefilter's own rounding, which is not the
        # reference's, then shows as 5e-5 (measured on the device): a 1200 bps MSK carrier in the channel is as well conditioned as data
        e1 = Case("E1", ("narrow", family, nm, 1200.0, 2), singles=((0, "oq_tebno_hi"), (1, "oq_mvr_floor"), (2, "oq_mvr_floor")), locked=False)
    # E2: the window sums do not return to exact zeros behind the signal (10.5 kbps: rounding residue of the running sums; 8400 bps: the FFT
    # prefilter's output on silence is 1e-20, not 0), so the silent window ends in the lines below, not in the NaN line; that one is taken
    # by the very first sample of every stream (0 / 0 on the empty window), which the plan makes a write of its own
    e2 = Case("E2", ("then_silence", family, nm, ("oq", family, N_LOOP, 0, 11.0, 3), 14000), at_start=("oq_nan",),
              at_end=("oq_mvr_floor", "oq_tebno_lo") if ten else ("oq_tebno_lo",), branch=("oq_nan", "mu_floor", "sym_gated"), locked=False)
    rest = [Case(f"seed{k}", ("oq_flat", family, nm, 11.0 + k, ((30, 32, 34) if ten else (30, 32, 33))[k]), branch=("oq_tebno_lo",), locked=False) for k in range(3)]
    groups.append(Group(family, "meter", nm, tuple([e1, e2] + rest), single_from=(0, "oq_tebno_hi")))
    return groups


# the tone that crosses both lines of the MSK meter in neighbouring samples, per family: 1000 + fb / 4 + 0.5 k Hz, k from the CPU search
_MSK_TONE_K = {"msk_1200": 0, "msk_600": 1, "msk_1200_24k": 2, "msk_1200_12k": 15}


def _msk_groups(family):
    f = fam(family)
    fb, Fs = f["fb"], f["Fs"]
    mid = MID
    a, b = ("msk", family, N_LOOP, 11.0, 0), ("msk", family, N_LOOP, 11.0, 1)
    loop = [Case("M+", a, (_P(0, m2_freq=1000.0 + 0.3 * fb),), ("m2_rule",)),
            Case("M-", a, (_P(0, m2_freq=1000.0 - 0.3 * fb),), ("m2_rule",)),
            Case("S+mid", b, (_P(mid, st_freq=0.5 * fb * (1.0 + 2e-4), lf_x1=1.0, lf_x2=-2.0, lf_y1=3.0, lf_y2=-4.0),), ("lf_pi2_pos", "lf_pi2_neg")),
            Case("S-mid", b, (_P(mid, st_freq=0.5 * fb * (1.0 - 2e-4)),), ("ec_pi",)),
            Case("plain", b, (), ("clip", "soft_255", "soft_0"))]
    nm = int(0.3 * Fs) + int(2 * Fs) + 200
    hz = 1000.0 + fb / 4 + 0.5 * _MSK_TONE_K[family]
    e3 = Case("E3tone", ("tone", family, nm, hz, 0.2), singles=((0, "msk_tebno_hi"), (1, "msk_nan"), (2, "msk_nan")), locked=False, noise=False)
    # at 48 kHz the running sums keep a rounding residue behind the signal and the silent window gives tebno = -157, neither line; at 24 and
    # 12 kHz they return to exact zeros and 0 * inf takes the NaN line -- a verdict that noise at 1e-9 of the signal in front changes, so it is
    # no verdict of this case (the bank is still compared with the oracle there).  The first sample of every stream takes the line robustly
    # (sqrt(2) / 0 * 0 on the empty window): the plan makes it a write of its own.
    e3s = Case("E3silence", ("then_silence", family, nm, ("msk", family, N_LOOP, 11.0, 3), int(0.3 * Fs)), at_start=("msk_nan",),
               branch=("msk_nan",), locked=False)
    rest = [Case(f"seed{k}", ("msk", family, nm, 11.0 + k, 20 + k), locked=False) for k in range(3)]
    return [Group(family, "loop", N_LOOP, tuple(loop)), Group(family, "meter", nm, tuple([e3, e3s] + rest), single_from=(0, "msk_tebno_hi"))]


GROUPS = {}
for _f in FAMILIES:
    for _g in (_oqpsk_groups(_f) if fam(_f)["kind"] == "oqpsk" else _msk_groups(_f)):
        assert len(_g.cases) <= len(SPECIAL)
        GROUPS[_g.id] = _g
GROUP_IDS = list(GROUPS)


def layouts(family):
    """jaero_debug_sample_loop_layout values a family's groups run with: both for the kernels chosen by size, 0 for the others"""
    return sorted({v.layout for v in KV.VARIANTS if v.family == family})
