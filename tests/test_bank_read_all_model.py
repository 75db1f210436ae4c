"""CPU: a numpy restatement of k_sweep_gather_i16's ownership map (jaero_amd/csrc/k_aerol_sweep.h) -- which output elements each 256-channel
workgroup stores as whole 16-byte words (8 int16) and which singly, and from which channel each element comes -- checked for what the
kernel relies on: every output element is written exactly once, by exactly one workgroup; no whole-word store covers an element of another
workgroup; the packed output is the concatenation of the channels' rows."""
import numpy as np
import pytest

W = 256  # SWEEP_W: channels per workgroup
E = 8    # int16 per 16-byte output word


def owner(s_off, tk, e):
    """sweep_owner: the last i < tk with s_off[i] <= e (channels without rows share their offset with the next one and are passed over)."""
    lo, hi = 0, tk
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if s_off[mid] <= e:
            lo = mid
        else:
            hi = mid
    return lo


def gather_map(v, taken=None):
    """v[c]: rows channel c hands over; taken: channels taken (a prefix; default all).  Returns (total, stores) with stores a list of
    (workgroup, first element, number of elements, whole-word?, [source channel per element], [source row per element])."""
    v = np.asarray(v, dtype=np.int64)
    nch = len(v)
    taken = nch if taken is None else taken
    off = np.concatenate([[0], np.cumsum(v)])
    stores = []
    for b in range((nch + W - 1) // W):
        ch0 = b * W
        tk = min(max(taken - ch0, 0), W)
        if tk <= 0:
            continue
        s_off = off[ch0:ch0 + tk + 1]
        e0, e1 = int(s_off[0]), int(s_off[tk])
        w0, w1 = e0 >> 3, ((e1 - 1) >> 3) + 1
        for w in range(w0, w1):
            lo, hi = max(w * E, e0), w * E + min(E, e1 - w * E)
            if lo >= hi:
                continue
            i = owner(s_off, tk, lo)
            chs, rows = [], []
            for e in range(lo, hi):
                if e >= s_off[i + 1]:
                    i = owner(s_off, tk, e)
                chs.append(ch0 + i)
                rows.append(e - int(s_off[i]))
            stores.append((b, lo, hi - lo, hi - lo == E, chs, rows))
    return int(off[taken]), stores


def check(v, taken=None):
    v = np.asarray(v, dtype=np.int64)
    total, stores = gather_map(v, taken)
    off = np.concatenate([[0], np.cumsum(v)])
    times = np.zeros(total + E, dtype=np.int64)  # (+ E: a store past the end would show)
    by = np.full(total + E, -1, dtype=np.int64)
    src = np.full((total + E, 2), -1, dtype=np.int64)
    for b, lo, n, whole, chs, rows in stores:
        if whole:
            assert lo % E == 0 and n == E  # a vector store is a whole aligned word
        times[lo:lo + n] += 1
        by[lo:lo + n] = b
        src[lo:lo + n, 0] = chs
        src[lo:lo + n, 1] = rows
    assert np.all(times[:total] == 1) and np.all(times[total:] == 0)
    # each element's writer is the workgroup of the channel that owns it, so a whole-word store never covers another workgroup's element
    want_ch = np.repeat(np.arange(len(v)), v)[:total]
    want_row = np.concatenate([np.arange(n) for n in v] + [np.zeros(0, np.int64)])[:total]
    assert np.array_equal(src[:total, 0], want_ch) and np.array_equal(src[:total, 1], want_row)
    assert np.array_equal(by[:total], want_ch // W)
    assert np.all(want_row < v[want_ch]) and np.array_equal(off[want_ch] + want_row, np.arange(total))
    return stores


def counts(rng, nch, kind):
    if kind == "dense":
        return rng.integers(0, 40, nch)
    if kind == "sparse":  # runs of channels without rows between the others
        v = rng.integers(1, 30, nch)
        v[rng.random(nch) < 0.8] = 0
        return v
    if kind == "tiny":  # several channels inside one word
        return rng.integers(0, 3, nch)
    raise ValueError(kind)


@pytest.mark.parametrize("nch", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("kind", ["dense", "sparse", "tiny"])
def test_every_element_written_once(nch, kind):
    rng = np.random.default_rng(1000 + nch)
    seen_unaligned = False
    for _ in range(6):
        v = counts(rng, nch, kind)
        check(v)
        seen_unaligned |= nch > W and int(v[:W].sum()) % E != 0
    if nch > W:
        assert seen_unaligned  # a workgroup boundary inside a word was among the cases


def test_boundary_word_is_shared_singly():
    """Workgroup 0 ends in the middle of a word, workgroup 1 starts there: both store their part of it singly, neither as a word."""
    v = np.zeros(513, dtype=np.int64)
    v[:W] = 1
    v[5] = 20           # workgroup 0: 275 rows, 275 % 8 = 3
    v[W:2 * W] = 2      # workgroup 1: 512 rows -> ends at 787, 787 % 8 = 3
    v[512] = 9
    stores = check(v)
    shared = [(b, lo, n, whole) for b, lo, n, whole, _, _ in stores if lo // E == 275 // E]
    assert sorted(shared) == [(0, 272, 3, False), (1, 275, 5, False)]
    shared = [(b, lo, n, whole) for b, lo, n, whole, _, _ in stores if lo // E == 787 // E]
    assert sorted(shared) == [(1, 784, 3, False), (2, 787, 5, False)]
    assert any(whole for _, _, _, whole, _, _ in stores)


def test_workgroup_without_rows_and_zero_runs():
    v = np.zeros(3 * W, dtype=np.int64)
    v[3], v[200] = 5, 13          # workgroup 0: a long run of empty channels between two others
    v[2 * W + 255] = 11           # workgroup 1 holds nothing; workgroup 2 only in its last channel
    stores = check(v)
    assert {b for b, *_ in stores} == {0, 2}
    # one word with three owners: rows 5..7 of the word [0, 8) come from channel 200
    first = [s for s in stores if s[1] == 0][0]
    assert first[3] and first[4] == [3] * 5 + [200] * 3
    check(np.zeros(W + 1, dtype=np.int64))  # nothing anywhere


@pytest.mark.parametrize("taken", [0, 1, 100, 256, 257, 400])
def test_prefix_taken(taken):
    """Only the taken prefix is moved; the workgroup that holds the first channel not taken stops in front of it."""
    rng = np.random.default_rng(7)
    v = rng.integers(0, 25, 513)
    total, stores = gather_map(v, taken)
    assert total == int(v[:taken].sum())
    check(v, taken)
    assert all(max(chs) < taken for *_, chs, _ in stores)
