"""Shared by tests/test_pre8400_cases.py (CPU) and tests/test_gpu_pre8400.py (GPU): case generators, the exact reference and the checker for
the 8400 bps prefilter (k_pre8400_mix / _commit / _fft / _restart of jaero_amd/csrc/k_pre8400.h; JAERO/oqpskdemodulator.cpp:343-381).

Three things are compared.
  candidate  what is under test (the kernels' output; in the CPU test the oracle's own output, or a deliberately wrong copy of it)
  oracle     oracle.Pre8400: mixer_fir_pre and fir_pre of the reference's demodulator on their own, bit-identical to what the oracle's
             demodulator computes (tests/test_pre8400_cases.py::test_stand_alone_object_is_the_demodulators_prefilter)
  exact      out[m] = sum_k h[k] x[m - 2048 - k] as a direct-form sum in long double on the ORACLE'S down-mixed samples x (the mix is compared bit
             for bit, so they are the candidate's as well), taps h from jo_rrc_design, then the up-mix in long double with the table entries of an
             fp64 restatement of the up-mix oscillator (up_indices).  Behind a restart at sample r the sum runs over x[j >= r] only and
             out[r .. r + 2047] = 0 (JFastFir::SetKernel: empty history, L queued zeros).

What is asserted (check_filtered):
  exact given    e_cand = max|cand - exact| / max|exact| <= 4 * e_oracle.  Both are a forward transform, a pointwise product and an inverse
                 transform of 4096 points in fp64: each error a small multiple of log2(4096) * 2^-53 of the peak; 4 covers the other
                 factorisation (16 x 16 x 16) and the kernel's fused twiddles, nothing else.
  oracle only    |cand - oracle| <= 5 * e_oracle_worst * max|oracle| (at most the two errors added), e_oracle_worst = the largest e_oracle of
                 the exact-sum channels of the same test.
  exact zeros    cand == 0 at every sample where the oracle's output is 0 (both parts); no sample exempt.  A single part that is 0.0 beside a
                 part of order one is no zero of the filter: while the oscillator stands at 0 Hz the up-mix forms im = yr * (-sin) + yi * cos
                 from yr ~ cos * v, yi ~ sin * v, two rounded products that cancel to 0.0 or to 1e-16 depending on the last bit of yr and yi
                 (11 and 16 such parts in the oracle's output of two channels of the `frequencies` case, all in writes at 0 Hz; an MI355X run
                 had 1e-16 at the first 11).  They fall under the error bound like every other value.
The mix (ring contents, pointer, step) is compared as bit patterns (check_bits)."""
import math

import numpy as np

LD = np.longdouble
WT = 19999
L = 2048          # JFastFir latency nfft - K + 1
EPS = 2.0 ** -52
MAX_EXACT_CHANNELS, MAX_EXACT_SAMPLES = 4, 40000  # the exact sum is 2049 long-double multiply-adds per output

SEQ_SMALL = [1, 7, 8, 9, 511]                      # below 512: one stretch by the product's own choice
SEQ_LARGE = [512, 513, 519, 520, 4095, 4096]       # eight stretches; tails of 0, 1, 7 and 0 samples behind the groups of eight
FILTER_CYCLE = [700, 3100, 4096, 50, 2048]         # writes inside one transform block and writes spanning three
CHECK67 = [0, 1, 2, 3, 63, 64, 66]                 # a whole LDS group, the last lane of a wavefront, the second wavefront's first and last live lane
FREQS = ["zero", "negative", 7985.3, 23999.9, "integer_step"]


def check_channels(nch):
    return list(range(nch)) if nch <= 5 else CHECK67


def fullscale_pcm(nch, n, seed, zero_channel=None):
    """Full-scale random int16 (peaks of the filtered signal near 1), with -32768 and 32767 in every channel's first write and optionally one
    channel of digital silence."""
    rng = np.random.default_rng(seed)
    pcm = rng.integers(-32768, 32768, size=(nch, n), dtype=np.int64).astype(np.int16)
    pcm[:, 0] = -32768
    if n > 3:
        pcm[:, 3] = 32767
    if zero_channel is not None:
        pcm[zero_channel] = 0
    return pcm


def cycle_sizes(cycle, total):
    out, s = [], 0
    while s < total:
        out.append(cycle[len(out) % len(cycle)])
        s += out[-1]
    return out


def freq_sum(kind, ch, k, nprev):
    """fsum such that fsum / nprev is the wanted frequency of FREQS (as nearly as fp64 has it; oracle and kernel get the same fsum)"""
    if kind == "zero":
        return 0.0
    if kind == "negative":
        return -123.456 * nprev
    if kind == "integer_step":
        return (3000 + 17 * ch + k) * 48000.0 / 19999.0 * nprev  # step = an integer up to the division's rounding: the pointer lands on table boundaries
    return float(kind) * nprev


def up_indices(ptr0, step, n):
    """fp64 restatement of the up-mix oscillator of one write (oqpskdemodulator.cpp:371-379: SetPhaseDeg(GetPhaseDeg before the write),
    DSP.cpp:175-180,192-195; WTCISValue_conj's index, DSP.cpp:79-93; WTnextFrame, DSP.cpp:70-77): (table indices, pointer after the write)"""
    phase = math.fmod(360.0 * ptr0 / float(WT), 360.0)
    while phase < 0:
        phase += 360.0
    p = (phase / 360.0) * float(WT)
    s = step if step >= 0 else 0.0
    idx = np.empty(n, dtype=np.int64)
    for i in range(n):
        t = int(p)
        idx[i] = 0 if t >= WT else t
        p += s
        while int(p) >= WT:
            p -= WT
    return idx, p


class Model:
    """One channel's oracle object with what the tests need recorded: per write the down-mixed samples, the output, the state after it and the
    up-mix table indices; the restarts."""

    def __init__(self, O):
        self.o = O.Pre8400()
        self.down, self.out, self.upidx, self.restarts = [], [], [], []
        self.n, self.nprev = 0, 0

    def write(self, pcm, fsum=None):
        """fsum: the sum the kernel finds in S_PRE_FSUM at this write (0 behind k_pre8400_commit unless poked); applied as the reference applies
        it at the end of the write before (oqpskdemodulator.cpp:607-608)"""
        if self.nprev > 0:
            self.o.end_of_write(0.0 if fsum is None else fsum, self.nprev)
        ptr0, step = self.o.state
        down, out = self.o.write(pcm)
        idx, p = up_indices(ptr0, step, len(pcm))
        assert p == self.o.state[0], "the restated up-mix oscillator left the oracle's"
        self.down.append(down); self.out.append(out); self.upidx.append(idx)
        self.n += len(pcm); self.nprev = len(pcm)
        return down, out

    def restart(self):
        self.o.restart()
        self.restarts.append(self.n)

    @property
    def state(self):
        return self.o.state

    def all_down(self):
        return np.concatenate(self.down)

    def all_out(self):
        return np.concatenate(self.out)


_taps = {}


def taps_ld(O):
    if "h" not in _taps:
        h = O.rrc_taps(0.6, 2048, 48000.0, 4200.0)
        assert h.shape == (2049,)
        _taps["h"] = h.astype(LD)
        cis = np.empty(2 * WT)
        O.lib().jo_cis_table(cis.ctypes.data)
        _taps["cis"] = cis.reshape(WT, 2)
    return _taps["h"], _taps["cis"]


def exact_prefilter(O, model):
    """The exact reference of a Model's whole stream (module docstring): (re, im) as long double arrays"""
    h, cis = taps_ld(O)
    x = model.all_down()
    n = len(x)
    assert n <= MAX_EXACT_SAMPLES
    yr, yi = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    cuts = [0] + list(model.restarts) + [n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b - a <= L:
            continue
        seg = x[a:b - L]  # out[a + L + i] = sum_k h[k] x[a + i - k], the terms with a + i - k >= a
        yr[a + L:b] = np.convolve(seg.real.astype(LD), h)[:b - a - L]
        yi[a + L:b] = np.convolve(seg.imag.astype(LD), h)[:b - a - L]
    idx = np.concatenate(model.upidx)
    bre, bim = cis[idx, 0].astype(LD), -cis[idx, 1].astype(LD)  # WTCISValue_conj
    return yr * bre - yi * bim, yr * bim + yi * bre


def err_vs_exact(z, exact):
    """max |z - exact| / max |exact|"""
    er, ei = exact
    d = np.sqrt((z.real.astype(LD) - er) ** 2 + (z.imag.astype(LD) - ei) ** 2)
    return float(d.max() / np.sqrt(er * er + ei * ei).max())


def check_bits(cand, oracle, what=""):
    """bit patterns, complex or real"""
    a, b = np.ascontiguousarray(cand).view(np.uint64), np.ascontiguousarray(oracle).view(np.uint64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        raise AssertionError((what, f"{len(bad)} of {a.size} words differ, first at word {bad[0]}",
                              np.ascontiguousarray(cand).view(np.float64)[bad[0]], np.ascontiguousarray(oracle).view(np.float64)[bad[0]]))


def check_zeros(cand, oracle, what=""):
    """cand == 0 at every sample where the oracle's output is 0 (module docstring: both parts)"""
    c, o = np.ascontiguousarray(cand), np.ascontiguousarray(oracle)
    bad = np.flatnonzero((o.real == 0.0) & (o.imag == 0.0) & ((c.real != 0.0) | (c.imag != 0.0)))
    assert len(bad) == 0, (what, f"{len(bad)} samples where the oracle has an exact zero, first at sample {bad[0]}: {c[bad[0]]!r}")


def check_filtered(cand, oracle, exact=None, e_oracle_worst=None, what=""):
    """The rules of the module docstring; returns (e_cand, e_oracle) against the exact sum, or (largest |cand - oracle| / peak, None)."""
    assert cand.shape == oracle.shape, (what, cand.shape, oracle.shape)
    check_zeros(cand, oracle, what)
    if exact is not None:
        e_c, e_o = err_vs_exact(cand, exact), err_vs_exact(oracle, exact)
        assert e_c <= 4 * e_o, (what, f"candidate {e_c / EPS:.2f} eps, oracle {e_o / EPS:.2f} eps of the peak: ratio {e_c / e_o:.2f} > 4")
        return e_c, e_o
    assert e_oracle_worst is not None
    peak = float(np.abs(oracle).max())
    d = float(np.abs(cand - oracle).max())
    assert d <= 5 * e_oracle_worst * peak, (what, f"|cand - oracle| = {d / peak / EPS:.2f} eps of the peak {peak:.3g}; allowed {5 * e_oracle_worst / EPS:.2f}")
    return (d / peak if peak else 0.0), None


def report(name, rows):
    """rows of (label, e_cand, e_oracle): the table DESIGN.md section 14 keeps, in units of 2^-52"""
    for label, ec, eo in rows:
        if eo is None:
            print(f"pre8400 {name} {label}: |kernel - oracle| / peak = {ec / EPS:.2f} eps")
        else:
            print(f"pre8400 {name} {label}: kernel {ec / EPS:.2f} eps, oracle {eo / EPS:.2f} eps, ratio {ec / eo:.2f}")
