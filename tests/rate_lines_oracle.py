"""The definition of the rate lines read on the device (include/jaero_hip.h, "rate lines, read on the device"), literally: per row a sort
for the median, a Python loop over the bins for the three-bin maximum and over every pair for the search.  No vectorised shortcut shares
code with jaero_amd.ratemeter.classify_rates, which is the other side of the comparison.  Nothing here touches a GPU."""
import numpy as np

BINS = 2049


def lines_row(R, kmin, d):
    """(floor, score [nd], where [nd]) of one row R [2049]"""
    R = np.asarray(R, dtype=np.float64)
    assert R.shape == (BINS,) and 1 <= kmin <= BINS - 2
    s = np.sort(R[kmin:])
    n = len(s)
    if n % 2:
        floor = s[n // 2]
    else:
        with np.errstate(over="ignore"):
            floor = (s[n // 2 - 1] + s[n // 2]) / 2
    r = R.tolist()  # Python floats: the same doubles, quicker to compare
    P = [max(r[max(k - 1, 0)], r[k], r[min(k + 1, BINS - 1)]) for k in range(BINS)]
    score = np.zeros(len(d), dtype=np.float64)
    where = np.full(len(d), -1, dtype=np.int32)
    for i, di in enumerate(d):
        di = int(di)
        assert di >= 1
        if kmin + di >= BINS:
            continue
        best, at = None, -1
        for a in range(kmin, BINS - di):
            m = min(P[a], P[a + di])
            if best is None or m > best:  # the smallest a among equals
                best, at = m, a
        score[i], where[i] = best, at
    return floor, score, where


def lines(R, kmin, d):
    """(floor [nch], score [nch, nd], where [nch, nd] int32) of R [nch, 2049]"""
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    out = [lines_row(row, kmin, d) for row in R]
    return np.array([o[0] for o in out], dtype=np.float64), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def ties(R, kmin, d):
    """[nch, nd] bool: the maximum is attained at more than one a (False where the distance is skipped)"""
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    out = np.zeros((R.shape[0], len(d)), dtype=bool)
    for c, row in enumerate(R.tolist()):
        P = [max(row[max(k - 1, 0)], row[k], row[min(k + 1, BINS - 1)]) for k in range(BINS)]
        for i, di in enumerate(d):
            if kmin + di >= BINS:
                continue
            m = [min(P[a], P[a + di]) for a in range(kmin, BINS - di)]
            out[c, i] = m.count(max(m)) > 1
    return out
