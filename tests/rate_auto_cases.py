"""What the one-pass gates' tests share (tests/test_gpu_rate_auto.py on the GPU, tests/test_rate_auto_host.py on the CPU): rows of +-1 whose
segment energies are any integers one likes, with what the rule must make of them; the 7 x 8 segments whose channels join and restart
differently inside one workgroup; and the burst rows of tests/rate_gate_cases.py in three arrangements, with the oracle's results on
them.  Each is built once per process and left unchanged.  Nothing here touches a GPU."""
import functools

import numpy as np

import rate_auto_oracle as AO
import rate_cases as RC
import rate_gate_cases as GC
import rate_gate_oracle as GO
import rate_oracle as RO
from jaero_amd import ratemeter as RM

L, BINS = RO.L, RO.BINS
NONE = AO.U64_MAX  # `start` of a channel that never restarted

# ---------------------------------------------------------------------------------------------- rows of +-1: E is what one likes
# (energy sequence, the gate after every segment or None where it is not pinned, the segments in R at the end, start)
ONES = [
    ([200, 300, 300, 250, 249, 300], [0, 0, 250, 250, 250, 250], [2, 3, 5], 2),  # 2 * 300 == 3 * 200 exactly; 250 joins, 249 does not
    ([200, 299, 299, 250], [0, 0, 0, 0], [0, 1, 2, 3], NONE),                    # 598 < 600: gate 0 throughout
    ([300, 300, 200, 250, 249], None, [0, 1, 3], NONE),                          # loud first: no restart
    ([200, 3000, 200, 300, 300], None, [3, 4], 3),                               # the click is ignored
    ([0, 0, 5, 5, 2, 3], [0, 0, 0, 2, 2, 2], [3, 4, 5], 3),
]


def ones_row(energies):
    """int16 [len(energies) L]: segment j holds energies[j] samples of +1, -1, +1, ... and zeros behind them"""
    row = np.zeros(len(energies) * L, dtype=np.int16)
    for j, e in enumerate(energies):
        assert 0 <= e <= L
        row[j * L:j * L + e] = 1 - 2 * (np.arange(e) % 2)
    return row


@functools.lru_cache(maxsize=None)
def ones_groups():
    """The ONES rows grouped by their number of segments, a meter taking rows of one length: [(indices into ONES, pcm int16 [k, nseg L])]"""
    out = []
    for nseg in sorted({len(t[0]) for t in ONES}):
        idx = [i for i, t in enumerate(ONES) if len(t[0]) == nseg]
        pcm = np.stack([ones_row(ONES[i][0]) for i in idx])
        pcm.flags.writeable = False
        out.append((idx, pcm))
    return out


def joined_only(pcm, c, joins):
    """int16 [1, len(joins) L]: channel c's segments `joins`, in order (GC.joined_only)"""
    return GC.joined_only(pcm, c, joins)


# ---------------------------------------------------------------------------------------------- joining and restarting inside a workgroup
AMIX_NCH, AMIX_NSEG, AMIX_TAIL = 7, 8, 100
# 1 = loud (the case row as it is), 0 = quiet (a quarter of its amplitude: a sixteenth of the energy)
AMIX_LOUD = [
    [0, 0, 1, 1, 0, 1, 1, 0],  # quiet first: restarts at its second loud segment; shares a workgroup with
    [1, 1, 0, 0, 1, 0, 0, 1],  # loud first, quiet later: never restarts
    None,                      # zeros, beside
    [1, 1, 1, 1, 1, 1, 1, 1],  # a level row
    [0, 0, 0, 1, 0, 0, 0, 0],  # one loud segment, a click: gate 0, everything joins; beside
    [0, 1, 1, 1, 1, 1, 1, 1],  # quiet, then loud for good
    [1, 0, 1, 0, 1, 0, 1, 0],  # alone in the last workgroup
]
AMIX_JOINS = [[3, 5, 6], [0, 1, 4, 7], list(range(8)), list(range(8)), list(range(8)), [2, 3, 4, 5, 6, 7], [2, 4, 6]]
AMIX_START = [3, NONE, NONE, NONE, NONE, 2, 2]
AMIX_CUTS = [1, 4095, 4097, 1, 8197, AMIX_NSEG * L + AMIX_TAIL - 16391]  # RC.CUTS with the rest of these rows


@functools.lru_cache(maxsize=None)
def auto_mixed():
    """pcm int16 [7, 8 L + 100]: segments of the case rows (the two OQPSK and the two MSK rows, the clipped sine, white noise) at full and
    at a quarter amplitude, and a row of zeros, as GC.mixed() builds its own.  The oracle says here that each channel joins and restarts
    where AMIX_JOINS and AMIX_START say."""
    n = AMIX_NSEG * L + AMIX_TAIL
    base = RC.base_rows(n).astype(np.int64)
    src = [0, 2, None, 1, 3, 7, 4]  # case row of each channel, as in GC.mixed()
    pcm = np.zeros((AMIX_NCH, n), dtype=np.int64)
    for c, s in enumerate(src):
        if s is None:
            continue
        pcm[c] = base[s]
        for j in range(AMIX_NSEG):
            if not AMIX_LOUD[c][j]:
                pcm[c, j * L:(j + 1) * L] //= 4
    pcm = pcm.astype(np.int16)
    o = AO.AutoRateOracle(AMIX_NCH)
    o.write(pcm)
    assert o.n == AMIX_NSEG and o.joined == AMIX_JOINS and o.start == AMIX_START, (o.joined, o.start)  # the construction does what it says
    assert o.gate[2] == o.gate[3] == o.gate[4] == 0 and all(o.gate[c] > 0 for c in (0, 1, 5, 6))
    pcm.flags.writeable = False
    return pcm


# ---------------------------------------------------------------------------------------------- the burst rows, three ways
CLICK_AT = (10 * L + 100, 10 * L + 400)
ARRANGEMENTS = ("plain", "click", "burst_first")
AUTO_RATES = GC.BURST_RATES  # [1200, 600, 10500, 1200, 0] in one pass, every arrangement
AUTO_JOINED = {"plain": [25, 27, 7, 256, 256], "click": [26, 28, 8, 256, 256], "burst_first": [26, 28, 8, 256, 256]}
AUTO_START = {"plain": [41, 41, 41, NONE, NONE], "click": [40, 40, 40, NONE, NONE], "burst_first": [NONE] * 5}
CLICK_RATES_TODAY = [1200, 600, 0, 1200, 0]  # the two-pass flow with suggest_gate(emax, emin) on the click rows: the failure
CLICK_HIST_GATES = [266287972352, 274877906944, 34896609280, 0, 0]  # suggest_gate(*hist_extremes(hist)) on the click rows


@functools.lru_cache(maxsize=None)
def burst_rows(arrangement):
    """GC.burst_rows() as they are ("plain"), with one 300-sample click of clipped Gaussian noise at sigma = 30 000 in segment 10 of all
    five rows, before the bursts ("click"), or rolled left by 40 L, so that the burst comes first ("burst_first")"""
    pcm = GC.burst_rows()
    if arrangement == "plain":
        return pcm
    if arrangement == "click":
        out = pcm.copy()
        click = np.random.default_rng(5).normal(0.0, 30000.0, (5, 300))
        out[:, CLICK_AT[0]:CLICK_AT[1]] = np.clip(np.rint(click), -32768, 32767).astype(np.int16)
    else:
        assert arrangement == "burst_first"
        out = np.roll(pcm, -40 * L, axis=1)
    out.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def burst_auto(arrangement):
    """The AUTO oracle after one pass over burst_rows(arrangement) (its R, numbers, gates, joined, start and histogram)"""
    o = AO.AutoRateOracle(5, AO.AUTO | AO.HIST)
    o.write(burst_rows(arrangement))
    o.R.flags.writeable = False
    return o


@functools.lru_cache(maxsize=None)
def click_two_pass():
    """The two two-pass flows on the click rows, on the oracles alone.  A dict: `today` = (gates, R) of measure -> suggest_gate(emax,
    emin) -> reset -> measure; `hist` = (gates, R, (emax, emin, njoin, ejoin)) of measure with the histogram -> suggest_gate(*hist_extremes(hist)) ->
    reset -> measure."""
    pcm = burst_rows("click")
    first = burst_auto("click")  # emax, emin and the histogram do not depend on the gates
    out = {}
    for name, gates in (("today", RM.suggest_gate(first.emax, first.emin)), ("hist", RM.suggest_gate(*RM.hist_extremes(first.hist_array())))):
        o = GO.GatedRateOracle(5)
        o.set_gate(gates)
        o.write(pcm)
        o.R.flags.writeable = False
        out[name] = (gates, o.R, o.stats())
    return out
