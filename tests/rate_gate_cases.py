"""What the gated rate lines' tests share (tests/test_gpu_rate_gate.py on the GPU, tests/test_rate_gate_host.py on the CPU): the 7 x 6
segments whose channels join differently inside one workgroup, and the five long rows (three bursts, one continuous carrier, noise) with
the oracle's results of the documented flow on them.  Each is built once per process and left unchanged.  Nothing here touches a GPU."""
import functools

import numpy as np

import rate_cases as RC
import rate_gate_oracle as GO
import rate_oracle as RO
from jaero_amd import ratemeter as RM
from jaero_amd import signalgen as G

L, BINS = RO.L, RO.BINS

# ---------------------------------------------------------------------------------------------- mixed joining inside a workgroup
MIX_NCH, MIX_NSEG, MIX_TAIL = 7, 6, 100
# the segments each channel joins: 0 / 1 and 4 / 5 share a workgroup and differ, 2 / 3 join nothing and everything, 6 is alone in the last
MIX_JOINS = [[0, 2, 5], [1], [], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [], [3]]
MIX_CUTS = [1, 4095, 4097, 1, 8197, MIX_NSEG * L + MIX_TAIL - 16391]  # RC.CUTS with the rest of these rows


@functools.lru_cache(maxsize=None)
def mixed():
    """(pcm int16 [7, 6 L + 100], gates): segments of the case rows (the two OQPSK and the two MSK rows, the clipped sine, white noise) at
    full and at a quarter amplitude, and a row of zeros.  A channel's loud segments are the ones it joins; its gate lies exactly at the
    weakest of them (E_j >= gate: joins).  Channel 1's segment 4 is its segment 1 with one sample zeroed, and its gate is that segment's
    E_4 + 1 (does not join) <= E_1 (joins); channel 5 is loud throughout under the gate max E_j + 1; channel 2 is zeros under gate 1;
    channel 3 mixes both amplitudes under the gate min E_j; channel 4 runs under gate 0."""
    n = MIX_NSEG * L + MIX_TAIL
    base = RC.base_rows(n).astype(np.int64)
    src = [0, 2, None, 1, 3, 7, 4]  # case row of each channel
    pcm = np.zeros((MIX_NCH, n), dtype=np.int64)
    for c, s in enumerate(src):
        if s is None:
            continue
        pcm[c] = base[s]
        for j in range(MIX_NSEG):
            quiet = j not in MIX_JOINS[c] if c in (0, 1, 6) else (c == 3 and j % 2 == 1)
            if quiet:
                pcm[c, j * L:(j + 1) * L] //= 4
    pcm[1, 4 * L:5 * L] = pcm[1, L:2 * L]
    k = 4 * L + int(np.argmax(np.abs(pcm[1, 4 * L:5 * L]) > 100))
    pcm[1, k] = 0
    E = np.array([GO.segment_energy(pcm[:, j * L:(j + 1) * L]) for j in range(MIX_NSEG)], dtype=object).T  # [7][6] Python ints
    gates = [min(E[0][j] for j in MIX_JOINS[0]), E[1][4] + 1, 1, min(E[3]), 0, max(E[5]) + 1, E[6][3]]
    for c in range(MIX_NCH):  # the construction does what it says
        assert [j for j in range(MIX_NSEG) if E[c][j] >= gates[c]] == MIX_JOINS[c], (c, E[c], gates[c])
    assert E[1][4] < E[1][1] and gates[0] in E[0] and gates[3] in E[3] and gates[6] in E[6]
    pcm = pcm.astype(np.int16)
    pcm.flags.writeable = False
    return pcm, gates


def joined_only(pcm, c, joins):
    """int16 [1, len(joins) L]: channel c's joined segments, in order"""
    return np.concatenate([pcm[c:c + 1, j * L:(j + 1) * L] for j in joins], axis=1)


# ---------------------------------------------------------------------------------------------- the burst rows
BURST_NSEG, BURST_FS = 256, 48000.0
BURST_START = 40 * L + 777
BURST_WRITE = 4 * L                                   # the GPU test's write size
BURST_RATES = [1200, 600, 10500, 1200, 0]             # gated, by the flow of jaero_amd/ratemeter.py's docstring
BURST_RATES_UNGATED = [0, 0, 0, 1200, 0]
BURST_FC = [1900.0, 1900.0, 8000.0]
BURST_JOINED = [26, 28, 8, BURST_NSEG, BURST_NSEG]    # segments that join, on record in the issue for the three bursts


@functools.lru_cache(maxsize=None)
def burst_rows():
    """int16 [5, 256 L] at 48 kHz: one 1200 bps and one 600 bps MSK burst, one 10 500 bps OQPSK burst, each starting at sample 40 L + 777 in
    noise; continuous 1200 bps MSK; white noise."""
    n = BURST_NSEG * L
    rng = np.random.default_rng(29)
    rows = [
        G.burst_msk(n, burst_starts=[BURST_START], ndata=2400, fb=1200.0, fc=1900.0, ebno_db=13.5, seed=G.SEED_BASE + 7)[0],
        G.burst_msk(n, burst_starts=[BURST_START], ndata=1200, fb=600.0, fc=1900.0, ebno_db=16.0, seed=G.SEED_BASE + 8)[0],
        G.burst_oqpsk(n, burst_starts=[BURST_START], ndata_sym=3040, ebno_db=8.0, seed=G.SEED_BASE + 9)[0],
        G.msk(n, fb=1200.0, fc=2000.0, ebno_db=13.0, seed=G.SEED_BASE + 3)[0],
        np.rint(rng.normal(0.0, 3000.0, n)),
    ]
    out = np.stack([np.asarray(r).astype(np.int16) for r in rows])
    out.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def burst_flow():
    """The oracle's results of the flow on burst_rows(): measure under gate 0 -> suggest_gate -> reset -> measure.  A dict: `first` and
    `second` = (R, (emax, emin, njoin, ejoin), nseg) of the two passes, `gates` = what suggest_gate gave.  The first pass, every gate
    being 0, is also what an ungated meter gives."""
    pcm = burst_rows()
    o = GO.GatedRateOracle(pcm.shape[0])
    o.write(pcm)
    first = (o.R.copy(), o.stats(), o.n)
    gates = RM.suggest_gate(o.emax, o.emin)
    o.set_gate(gates)
    o.reset()
    o.write(pcm)
    second = (o.R.copy(), o.stats(), o.n)
    for a in (first[0], second[0]):
        a.flags.writeable = False
    return {"first": first, "gates": gates, "second": second}
