"""What the tests of the rate lines read on the device share (tests/test_gpu_rate_lines.py on the GPU, tests/test_rate_lines_host.py on the
CPU): the ten made rows no signal produces, the sample rates and kmin every comparison runs over, and the comparison itself.  Each is
built once per process and left unchanged.  Nothing here touches a GPU."""
import functools

import numpy as np

import rate_lines_oracle as LO
from jaero_amd import ratemeter as RM

BINS = LO.BINS
FS = (48000.0, 12000.0)  # at 12 kHz the distances of 8400 and 10 500 bps (2867, 3584) are skipped
KMIN = (8, 7, 1)         # 2041, 2042 and 2048 values under the median: both parities
D48 = (51, 102, 717, 896)
NMADE = 10
AT_KMIN = 8              # made row 9's best pair for d = 51 sits at a = 8 = kmin


@functools.lru_cache(maxsize=None)
def made_rows():
    """float64 [10, 2049], in the order of the list in the module's tests:
    0 all ones; 1 ones with 50.0 at bins 100, 202, 300, 402 (two equal pairs for d = 102: the first wins); 2 a descending ramp; 3 zeros but
    one bin; 4 values of 1e-300 scale with 1e300 at two bins 896 apart (score / floor overflows to inf); 5 integers 1 .. 3 at random (many
    equal values at the median); 6 all 5e-324, the smallest denormal; 7 uniform noise with 100.0 at bins 2048 and 1997 (a line at the
    clipped upper end); 8 uniform noise whose best pair for d = 51 sits at a = kmin = 8, lines at bins 7 and 58 -- bin 7 itself lies below
    kmin and reaches a = 8 through the three-bin maximum; 9 zeros."""
    assert RM.rate_distances(48000.0) == list(D48)
    rng = np.random.default_rng(41)
    rows = np.empty((NMADE, BINS), dtype=np.float64)
    rows[0] = 1.0
    rows[1] = 1.0
    rows[1, [100, 202, 300, 402]] = 50.0
    rows[2] = np.arange(BINS, 0, -1, dtype=np.float64)
    rows[3] = 0.0
    rows[3, 1000] = 7.0
    rows[4] = rng.uniform(1.0, 2.0, BINS) * 1e-300
    rows[4, [600, 600 + 896]] = 1e300
    rows[5] = rng.integers(1, 4, BINS).astype(np.float64)
    rows[6] = 5e-324
    rows[7] = rng.uniform(0.5, 1.5, BINS)
    rows[7, [2048, 1997]] = 100.0
    rows[8] = rng.uniform(0.5, 1.5, BINS)
    rows[8, [7, 58]] = 80.0
    rows[9] = 0.0
    assert rows[6, 0] > 0.0 and rows[6, 0] / 2 == 0.0
    rows.flags.writeable = False
    return rows


def cycled(rows, nch):
    """[nch, 2049]: row i is rows[i mod len(rows)]"""
    return np.ascontiguousarray(rows[np.arange(nch) % len(rows)])


def assert_lines_equal(got, want, where=""):
    """(floor, score, where) twice, compared with np.array_equal: the device only selects, so there is no tolerance"""
    for name, g, w in zip(("floor", "score", "where"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (where, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError((where, name, f"{len(bad)} of {g.size} differ; first at {bad[0].tolist()}: {g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}"))


def assert_decisions_equal(got, want, where=""):
    """(rate, audio, score_db) twice: np.array_equal, audio with equal_nan"""
    (r0, a0, s0), (r1, a1, s1) = got, want
    assert np.array_equal(r0, r1), (where, "rate", r0, r1)
    assert np.array_equal(a0, a1, equal_nan=True), (where, "audio", a0, a1)
    assert np.array_equal(s0, s1), (where, "score_db", s0, s1)


def decide_from_oracle(R, fs, kmin):
    """rate_lines_oracle.lines followed by decide_rates: the new path with the oracle in the device's place"""
    d = RM.rate_distances(fs)
    floor, score, where = LO.lines(R, kmin, d)
    with np.errstate(all="ignore"):
        return RM.decide_rates(floor, score, where, d, fs)


def classify_reference(R, fs, kmin):
    with np.errstate(all="ignore"):
        return RM.classify_rates(R, fs, kmin=kmin)
