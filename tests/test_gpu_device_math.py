"""GPU: the device primitives the sample kernels are built from, each against an independent high-precision or libm reference.

The functions run are the product headers' own (jaero_amd/libjaero_prims.so, jaero_amd/csrc/prims_check.hip, compiled with the product's flags),
one element per lane.  References: glibc's hypot / tanh / expm1 and __float128's atan2q (tests/device_math_ref.c, compiled here), IEEE division
(numpy and the device's own `/`), Qt's qRound and JAERO's WaveTable restated in Python floats, and the matched filter summed term by term.
Bit identity with libm is defined against glibc 2.35: on another glibc only those assertions skip, with the version in the reason.
"""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import device_prims as DP

pytestmark = pytest.mark.gpu

W = 19999.0  # JD_WTSIZE
INT_MAX, INT_MIN = 2**31 - 1, -(2**31)


@pytest.fixture(scope="module")
def L():
    return DP.prims()


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return DP.build_ref(tmp_path_factory.mktemp("device_math_ref"))


def glibc_235(R):
    v = R.ref_libc_version().decode()
    if v != "2.35":
        pytest.skip(f"bit identity with libm is defined against glibc 2.35; this host has glibc {v}")


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def call(L, name, *args):
    rc = getattr(L, name)(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args])
    assert rc == 0, f"{name}: hipError {rc}"


def bits(a):
    return f64(a).view(np.int64)


def same(a, b):
    a, b = f64(a), f64(b)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def ulps(x, k):
    """x moved by k units in the last place (x > 0 finite, no exponent crossing below 0)."""
    return (f64(x).view(np.int64) + np.asarray(k, np.int64)).view(np.float64)


def assert_same(what, got, want, *ops):
    bad = np.flatnonzero(~same(got, want))
    if len(bad):
        i = bad[:5]
        rows = [" ".join(float(o[j]).hex() for o in ops) + f" -> {float(got[j]).hex()} want {float(want[j]).hex()}" for j in i]
        pytest.fail(f"{what}: {len(bad)} of {len(got)} differ, e.g.\n  " + "\n  ".join(rows))


def one_ulp_apart(a, b):
    """|a - b| in ulps for doubles of the same sign."""
    return np.abs(bits(a) - bits(b))


def rsign(rng, x):
    return np.where(rng.integers(0, 2, len(x)) == 1, -x, x)


# ---- hypot ----------------------------------------------------------------------------------------------------------------------
def hypot_families(rng, n=1 << 18):
    u = lambda m=n: rng.random(m)  # noqa: E731
    fam = {}
    ph, sc = 2 * np.pi * u(), np.exp2(80 * u() - 60)
    mre, mim = sc * (2 * u() - 1), sc * (2 * u() - 1) * np.exp2(-6 * u())
    fam["oscillator x resonator pair"] = (np.cos(ph) * mre - np.sin(ph) * mim, np.cos(ph) * mim + np.sin(ph) * mre)
    ph, r = 2 * np.pi * u(), np.exp2(80 * u() - 40)
    fam["uniform angle, radius 2^[-40,40]"] = (r * np.cos(ph), r * np.sin(ph))
    ay = np.exp2(200 * u() - 100) * (1 + u())
    fam["ax = ay 2^54 +- 4 ulp"] = (ulps(ay * 2.0**54, rng.integers(-4, 5, n)), ay)
    fam["ax / ay in 2^[50,58]"] = (ay * np.exp2(50 + 8 * u()), ay)
    ax = ulps(np.full(n, 2.0**511), rng.integers(-300, 300, n))
    fam["ax near 2^511"] = (ax, ax * np.exp2(-60 * u()))
    ay = ulps(np.full(n, 2.0**-459), rng.integers(-300, 300, n))
    fam["ay near 2^-459"] = (ay * np.exp2(60 * u()), ay)
    for e in (200, -200):
        r = u()
        ax = ulps(2.0**e / np.sqrt(1 + r * r), rng.integers(-8, 9, n))
        fam[f"h near 2^{e}"] = (ax, ax * r)
    sp = [0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.0**-1022, 2.0**-459, 2.0**-460, 1.0, -3.0, 2.0**511, 2.0**512, 2.0**1023, 1.7976931348623157e308,
          np.inf, -np.inf, np.nan, -np.nan]
    a, b = np.meshgrid(np.array(sp), np.array(sp))
    fam["zeros, subnormals, inf, NaN"] = (a.ravel(), b.ravel())
    return {k: (f64(rsign(rng, x)), f64(rsign(rng, y))) for k, (x, y) in fam.items()}


def test_hypot_is_glibcs_bit_for_bit(L, R):
    rng = np.random.default_rng(11)
    fams = hypot_families(rng)
    got = {}
    for name, (x, y) in fams.items():
        o = np.zeros(len(x))
        call(L, "jp_hypot", x, y, o, len(x))
        got[name] = o
    # C99 F.9.4.3, independent of the libm version: hypot(+-inf, y) = +inf even for a NaN y
    x, y = f64([np.inf, -np.inf, np.nan, np.nan, np.inf]), f64([np.nan, np.nan, np.inf, -np.inf, -np.inf])
    o = np.zeros(5)
    call(L, "jp_hypot", x, y, o, 5)
    assert np.all(o == np.inf), o
    glibc_235(R)
    outside = 0
    for name, (x, y) in fams.items():
        want = np.zeros(len(x))
        R.ref_hypot(x.ctypes.data, y.ctypes.data, want.ctypes.data, len(x))
        # glibc's unscaled range (2^-459 < min, max < 2^511) and everything jd_hypot settles itself (infinities, NaN, a zero min):
        # bit for bit.  Beyond it jd_hypot takes the device library's hypot (jd_libm.h), which glibc's scaled branches do not match bit for
        # bit (measured: 4 % of the operands next to 2^511 differ by one ulp); no call site gets there (the operands are AGC'd samples).
        ax, ay = np.maximum(np.abs(x), np.abs(y)), np.minimum(np.abs(x), np.abs(y))
        scaled = np.isfinite(ax) & (ay != 0) & ((ax >= 2.0**511) | (ay <= 2.0**-459))
        assert_same(f"jd_hypot, {name}", got[name][~scaled], want[~scaled], x[~scaled], y[~scaled])
        assert one_ulp_apart(got[name][scaled], want[scaled]).max(initial=0) <= 1, name
        outside += int(scaled.sum())
    assert outside > 0  # the boundary families straddle the switch


# ---- atan2 ----------------------------------------------------------------------------------------------------------------------
# the operand families of scripts/atan2_check.c, 2^22 calls
def atan2_families(rng):
    fam = {}
    n = 1 << 21
    u = lambda m: rng.random(m)  # noqa: E731
    ph, sc = 2 * np.pi * u(n), np.exp2(80 * u(n) - 60)
    mre, mim = sc * (2 * u(n) - 1), sc * (2 * u(n) - 1) * np.exp2(-6 * u(n))
    fam["oscillator x resonator pair"] = (np.cos(ph) * mim + np.sin(ph) * mre, np.cos(ph) * mre - np.sin(ph) * mim)
    n = 1 << 19
    ph, r = 2 * np.pi * u(n), np.exp2(80 * u(n) - 40)
    fam["uniform angle, radius 2^[-40,40]"] = (r * np.sin(ph), r * np.cos(ph))
    base, d, r = rng.integers(0, 8, n) * (np.pi / 4), np.exp2(-60 * u(n)) * (u(n) - 0.5), np.exp2(20 * u(n) - 10)
    fam["near axes and diagonals"] = (r * np.sin(base + d), r * np.cos(base + d))
    i, q = rng.integers(0, 65, n), rng.integers(0, 8, n)
    mx = 1.0 + u(n)
    mn = mx * (i / 64.0 + np.where(i & 1, 1.0, -1.0) * (1.0 / 128.0) * rng.integers(0, 2, n))
    mn = mn * (1.0 + (rng.integers(0, 16, n) - 8) * 2.0**-52)
    mn = np.where(mn <= 0, 2.0**-30 * u(n) + 2.0**-200, mn)
    x, y = np.where(q & 1, mn, mx), np.where(q & 1, mx, mn)
    fam["table points +- few ulp"] = (np.where(q & 4, -y, y), np.where(q & 2, -x, x))
    # exponents in [-299, 299]: outside [2^-300, 2^300) the device library's atan2 takes over (jd_libm.h), which is not what is measured here
    a, b = np.exp2(598 * u(n) - 299) * (1 + u(n)), np.exp2(598 * u(n) - 299) * (1 + u(n))
    fam["wide exponent gap"] = (rsign(rng, b), rsign(rng, a))
    return {k: (f64(y), f64(x)) for k, (y, x) in fam.items()}


ATAN2_NOT_CR_BUDGET = 8  # of 2^22 calls not correctly rounded (jd_libm.h: ~2e-7 of the calls, i.e. about one)


def atan2_dev(L, y, x, mask=~0 & 0xFFFFFFFFFFFFFFFF, n=None, fill=np.nan):
    n = len(x) if n is None else n
    o = np.full(len(x), fill)
    call(L, "jp_atan2", y, x, o, n, mask)
    return o


def test_atan2_is_within_one_ulp_and_nearly_always_correctly_rounded(L, R):
    rng = np.random.default_rng(12)
    not_cr, total, report = 0, 0, []
    for name, (y, x) in atan2_families(rng).items():
        got = atan2_dev(L, y, x)
        cr = np.zeros(len(x))
        R.ref_atan2q(y.ctypes.data, x.ctypes.data, cr.ctypes.data, len(x))
        assert np.all(np.sign(got) == np.sign(cr)), name
        d = one_ulp_apart(got, cr)
        assert d.max() <= 1, (name, int(d.max()), float(y[d.argmax()]).hex(), float(x[d.argmax()]).hex())
        not_cr += int((d != 0).sum())
        total += len(x)
        report.append(f"{name}: {int((d != 0).sum())}")
    assert total == 1 << 22
    assert not_cr <= ATAN2_NOT_CR_BUDGET, f"{not_cr} of 2^22 results not correctly rounded ({', '.join(report)})"


def test_atan2_special_operands_are_glibcs(L, R):
    sp = f64([0.0, -0.0, 1.0, -1.0, 3.0, -0.5, np.inf, -np.inf, np.nan])
    a, b = np.meshgrid(sp, sp)
    y, x = f64(a.ravel()), f64(b.ravel())
    special = ~np.isfinite(y) | ~np.isfinite(x) | (y == 0) | (x == 0)
    y, x = f64(y[special]), f64(x[special])
    got = atan2_dev(L, y, x)
    # C99 F.9.1.4 signs, independent of the libm version
    assert math.copysign(1, got[(y == 0) & (x == 0) & (np.signbit(y)) & ~np.signbit(x)][0]) == -1.0
    assert got[(y == 0) & np.signbit(x) & (x == 0) & ~np.signbit(y)][0] == math.pi
    glibc_235(R)
    want = np.zeros(len(x))
    R.ref_atan2(y.ctypes.data, x.ctypes.data, want.ctypes.data, len(x))
    assert_same("jd_atan2 on +-0 / +-inf / NaN", got, want, y, x)


def test_atan2_gives_the_full_wave_result_under_every_lane_mask(L):
    """jda_fetch reads the table from other lanes (ds_bpermute) while the whole wavefront runs, and from memory when part of it is
    switched off: odd lanes only, a single lane, a ragged last wavefront must all give the full-wave bits."""
    rng = np.random.default_rng(13)
    fams = atan2_families(rng)
    y = f64(np.concatenate([v[0][:1 << 14] for v in fams.values()]))
    x = f64(np.concatenate([v[1][:1 << 14] for v in fams.values()]))
    full = atan2_dev(L, y, x)
    lane = (np.arange(len(x)) % 64).astype(np.uint64)
    for what, mask in (("odd lanes", 0xAAAAAAAAAAAAAAAA), ("even lanes", 0x5555555555555555), ("lane 0", 1), ("lane 37", 1 << 37),
                       ("lane 63", 1 << 63), ("lanes 0-31", 0xFFFFFFFF)):
        got = atan2_dev(L, y, x, mask, fill=-7.0)
        on = (np.uint64(mask) >> lane) & np.uint64(1) == 1
        assert_same(f"jd_atan2 with {what} active", got[on], full[on], y[on], x[on])
        assert np.all(got[~on] == -7.0), what
    for n in (len(x) - 41, len(x) - 63, 1):  # last wavefront with 23, 1 active lane(s); a lone lane
        got = atan2_dev(L, y, x, n=n, fill=-7.0)
        assert_same(f"jd_atan2, {n} elements", got[:n], full[:n], y[:n], x[:n])
        assert np.all(got[n:] == -7.0)


# ---- tanh / expm1 ---------------------------------------------------------------------------------------------------------------
LN2 = math.log(2)
# glibc's branch points: high words (s_expm1.c: 56 ln2, o_threshold, 0.5 ln2, 1.5 ln2, 2^-54; s_tanh.c: 2^-55, 1, 22) and jd_tanh's 6.5
EXPM1_HI = (0x4043687A, 0x40862E42, 0x3FD62E42, 0x3FF0A2B2, 0x3C900000)
TANH_HI = (0x3C800000, 0x3FF00000, 0x40360000, 0x401A0000)


def words(his, rng):
    out = []
    for h in his:
        for hh in (h - 1, h, h + 1):
            lo = np.concatenate([np.array([0, 1, 0xFFFFFFFE, 0xFFFFFFFF], np.uint64), rng.integers(0, 2**32, 60, dtype=np.uint64)])
            out.append(((np.uint64(hh) << np.uint64(32)) | lo).view(np.float64))
    v = np.concatenate(out)
    return np.concatenate([v, -v])


def near(points, k=64):
    p = np.abs(f64(points))
    v = np.concatenate([ulps(p, j) for j in range(-k, k + 1)])
    return np.concatenate([v, -v])


def tanh_expm1_operands(rng):
    n = 1 << 19
    parts = [rsign(rng, np.exp2(rng.uniform(-60, 7, n)))]
    # every reduction index k of expm1 (x = k ln2 + r, |r| <= ln2 / 2) from -60 to 60, and tanh's arguments, which are half of expm1's
    k = np.repeat(np.arange(-60, 61), 1 << 12)
    x = (k + rng.uniform(-0.5, 0.5, len(k))) * LN2
    parts += [x, x / 2]
    pts = [2.0**-55, 2.0**-54, 0.5 * LN2, 1.5 * LN2, 1.0, 6.5, 22.0, 56 * LN2, 7.09782712893383973096e02]
    parts += [near(pts), near(np.array(pts) / 2), words(EXPM1_HI + TANH_HI, rng)]
    hw = words(EXPM1_HI, rng)
    parts.append(hw / 2)  # tanh's expm1(+-2|x|) at expm1's branch points
    parts.append(f64([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1e-310, -1e-310, 1e300, -1e300, 800.0, -800.0, 710.0, -710.0,
                      -40.0, -38.0, 19.0 * LN2, 20.0 * LN2, 21.0 * LN2]))
    return f64(np.concatenate(parts))


def test_tanh_and_expm1_are_glibcs_bit_for_bit(L, R):
    x = tanh_expm1_operands(np.random.default_rng(14))
    got = {}
    for name in ("jp_tanh", "jp_tanh_full", "jp_expm1"):
        o = np.zeros(len(x))
        call(L, name, x, o, len(x))
        got[name] = o
    # what does not depend on the libm version
    for name in ("jp_tanh", "jp_tanh_full"):
        g = got[name]
        assert np.all(np.abs(g[np.isfinite(x)]) <= 1.0) and np.all(np.isnan(g[np.isnan(x)]))
        assert np.all(g[x == np.inf] == 1.0) and np.all(g[x == -np.inf] == -1.0)
        z = got[name][x == 0]
        assert np.array_equal(np.signbit(z), np.signbit(x[x == 0]))
    assert np.all(got["jp_expm1"][x == -np.inf] == -1.0) and np.all(got["jp_expm1"][x == np.inf] == np.inf)
    glibc_235(R)
    want_t, want_e = np.zeros(len(x)), np.zeros(len(x))
    R.ref_tanh(x.ctypes.data, want_t.ctypes.data, len(x))
    R.ref_expm1(x.ctypes.data, want_e.ctypes.data, len(x))
    assert_same("jd_tanh", got["jp_tanh"], want_t, x)
    assert_same("jd_tanh_full", got["jp_tanh_full"], want_t, x)
    assert_same("jd_expm1", got["jp_expm1"], want_e, x)


# ---- jd_log10 -------------------------------------------------------------------------------------------------------------------
def log10_families(rng):
    """The coarse estimate's arguments are max(|Z|^2, 1) with |Z|^2 up to 4e21: [1, 1e24] log-spaced, the first doubles above 1, powers of
    two and ten, and both sides of the point m = sqrt(1/2) where the reduction x = m 2^e changes e."""
    fam = {"log-spaced in [1, 1e24]": np.power(10.0, rng.uniform(0.0, 24.0, 1 << 22))}
    fam["1 + k eps, k < 4096"] = 1.0 + np.arange(4096) * 2.0**-52
    fam["powers of two"] = np.exp2(np.arange(0, 81))
    fam["powers of ten"] = np.array([float(f"1e{k}") for k in range(25)])
    s = math.sqrt(0.5)
    fam["around m = sqrt(1/2)"] = np.concatenate([ulps(np.full(4001, s * 2.0**e), np.arange(-2000, 2001)) for e in (1, 2, 11, 40, 72)])
    fam["[2, 1e24]"] = np.power(10.0, rng.uniform(math.log10(2.0), 24.0, 1 << 20))
    return {k: f64(v) for k, v in fam.items()}


def test_log10_within_two_ulp_of_the_correctly_rounded_value(L):
    """jd_log10 (the estimate kernels' 0.5 * log10(|Z|^2)) against log10 in long double: the header's bound of 2 ulp.  The error is measured
    against the unrounded long-double value in ulps of the correctly rounded double; every family's maximum is printed.
    Measured on an MI355X: 1.47 ulp (log-spaced, at 0x1.048e8e69e6a11p+0), 1.46 (1 + k eps), 1.16 (around m = sqrt(1/2)), 1.03 from 2 on,
    0.49 at powers of two.  The form this test first met (quotient, series and both constants in single doubles) gave 3.43 ulp below
    x = 2.83: 3.43 log-spaced, 2.42 at 1 + k eps, 2.32 around sqrt(1/2), 1.53 from 2 on."""
    fams = log10_families(np.random.default_rng(16))
    worst = {}
    for name, x in fams.items():
        assert np.all(x >= 1.0)
        o = np.full(len(x), np.nan)
        call(L, "jp_log10", x, o, len(x))
        ref = np.log10(x.astype(np.longdouble))
        cr = ref.astype(np.float64)
        assert np.all(o[x == 1.0] == 0.0) and np.all(np.isfinite(o)) and np.all(o >= 0.0)
        nz = cr != 0
        err = np.abs(o[nz].astype(np.longdouble) - ref[nz]) / np.spacing(cr[nz]).astype(np.longdouble)
        i = int(np.argmax(err))
        worst[name] = (float(err[i]), float(x[nz][i]).hex())
        print(f"jd_log10 {name}: max {worst[name][0]:.3f} ulp at {worst[name][1]}")
    # exact where the result is an integer the format holds: log10(10^k)
    o = np.zeros(25)
    call(L, "jp_log10", fams["powers of ten"], o, 25)
    assert np.max(np.abs(o - np.arange(25))) <= 2 * np.spacing(24.0)
    bad = {k: v for k, v in worst.items() if not v[0] <= 2.0}
    assert not bad, f"jd_log10 is more than 2 ulp from log10: {bad}"


# ---- jd_div ---------------------------------------------------------------------------------------------------------------------
def test_div_is_the_ieee_quotient_in_its_documented_range(L):
    rng = np.random.default_rng(15)
    n = 1 << 20
    a = rsign(rng, np.exp2(rng.uniform(-500, 499, n)) * (1 + rng.random(n)))
    b = rsign(rng, np.exp2(rng.uniform(-500, 499, n)) * (1 + rng.random(n)))
    # quotients next to a rounding boundary: a = RN(b (q + ulp(q) / 2)) +- a few ulps, and near-exact multiples
    m = 1 << 19
    bb = np.exp2(rng.uniform(-100, 100, m)) * (1 + rng.random(m))
    q = np.exp2(rng.uniform(-100, 100, m)) * (1 + rng.random(m))
    qm = (q.astype(np.longdouble) + np.nextafter(q, np.inf).astype(np.longdouble)) / 2
    a_mid = ulps((qm * bb.astype(np.longdouble)).astype(np.float64), rng.integers(-3, 4, m))
    a_mul = ulps(q * bb, rng.integers(-3, 4, m))
    a = f64(np.concatenate([a, rsign(rng, a_mid), rsign(rng, a_mul), np.zeros(64)]))
    b = f64(np.concatenate([b, rsign(rng, bb), rsign(rng, bb), rsign(rng, np.exp2(rng.uniform(-500, 499, 64)))]))
    assert np.all((np.abs(b) >= 2.0**-500) & (np.abs(b) <= 2.0**500))
    assert np.all((a == 0) | ((np.abs(a) >= 2.0**-500) & (np.abs(a) <= 2.0**500)))
    o, o_ieee = np.zeros(len(a)), np.zeros(len(a))
    call(L, "jp_div", a, b, o, o_ieee, len(a))
    assert_same("device `/` against IEEE division", o_ieee, a / b, a, b)
    assert_same("jd_div against the device's `/`", o, o_ieee, a, b)
    # the documented exception (jd_libm.h): -0 / b for b > 0 gives +0 where IEEE gives -0; the other zero quotients keep IEEE's sign
    a0, b0 = f64([-0.0, -0.0, 0.0, 0.0]), f64([3.0, -3.0, -3.0, 3.0])
    o, o_ieee = np.zeros(4), np.zeros(4)
    call(L, "jp_div", a0, b0, o, o_ieee, 4)
    assert list(np.signbit(o_ieee)) == [True, False, True, False]
    assert list(np.signbit(o)) == [False, False, True, False] and np.all(o == 0)


# ---- jd_div_const ---------------------------------------------------------------------------------------------------------------
def div_const_operands(rng, d, n=1 << 22):
    """The families of scripts/div_const_check.c, n of each: random mantissa and exponent, near-multiples, near-midpoints, moderate values."""
    mant = lambda m: 1 + rng.integers(0, 2**52, m) * 2.0**-52  # noqa: E731
    x0 = mant(n) * np.exp2(rng.integers(-60, 61, n))
    q = mant(n) * np.exp2(rng.integers(-30, 31, n))
    x1 = ulps(d * q, rng.integers(-3, 4, n))
    q = mant(n) * np.exp2(rng.integers(-20, 21, n))
    qm = (q.astype(np.longdouble) + np.nextafter(q, np.inf).astype(np.longdouble)) / 2
    x2 = ulps((qm * np.longdouble(d)).astype(np.float64), rng.integers(-3, 4, n))
    x3 = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64) * 2.0**-40
    return f64(np.concatenate([rsign(rng, x0), rsign(rng, x1), rsign(rng, x2), x3, [0.0, -0.0]]))


@pytest.mark.parametrize("dc", DP.DIV_CONSTS, ids=lambda dc: f"{dc.d:g} {dc.site}")
def test_div_const_is_the_ieee_quotient(L, dc):
    x = div_const_operands(np.random.default_rng(int(dc.d)), dc.d)
    assert len(x) >= 1 << 24
    o, o_ieee = np.zeros(len(x)), np.zeros(len(x))
    call(L, "jp_div_const", x, o, o_ieee, len(x), dc.d, 1.0 / dc.d)
    want = x / dc.d
    assert_same(f"jd_div_const(x, {dc.d:g}) ({dc.what})", o, want, x)
    assert_same("device `/`", o_ieee, want, x)
    assert np.signbit(o[-1]) and not np.signbit(o[-2]) and o[-1] == 0  # x = -0 keeps its sign


# ---- qRound and soft bits -------------------------------------------------------------------------------------------------------
def qround(d):
    """Qt 5.9 qRound (qglobal.h:525-526; oracle/jaero_oracle.c:46) in Python floats: int() truncates as the C cast does in range."""
    if d >= 0.0:
        return int(d + 0.5)
    t = int(d - 1)
    return int(d - float(t) + 0.5) + t


def test_qround_and_softbit_are_qts(L):
    halves = np.arange(-2048, 2049) / 2.0
    h = np.arange(-2, 258) + 0.5
    nb = np.concatenate([np.nextafter(h, np.inf), np.nextafter(h, -np.inf), np.nextafter(np.nextafter(h, np.inf), np.inf),
                         np.nextafter(np.nextafter(h, -np.inf), -np.inf), h])
    rng = np.random.default_rng(16)
    v = f64(np.concatenate([halves, nb, [0.49999999999999994, -0.49999999999999994, 2.0**30, -(2.0**30), 2.0**30 + 0.5, -0.0],
                            rng.uniform(-300, 300, 1 << 16)]))
    qr, sb = np.zeros(len(v), np.int32), np.zeros(len(v), np.int32)
    call(L, "jp_qround", v, qr, len(v))
    call(L, "jp_softbit", v, sb, len(v))
    want = np.array([qround(float(d)) for d in v])
    bad = np.flatnonzero(qr != want)
    assert not len(bad), [(float(v[i]).hex(), int(qr[i]), int(want[i])) for i in bad[:5]]
    assert np.array_equal(sb, np.clip(want, 0, 255))
    assert qr[np.flatnonzero(v == 0.49999999999999994)[0]] == 1


# Outside int's range the C casts of qRound are undefined; what each machine gives (x86-64 cvttsd2si: 0x80000000 for NaN and out of range;
# gfx950 v_cvt_i32_f64: 0 for NaN, saturated otherwise).  Only +inf and v >= 2^31 differ, and no call site reaches them: every jd_softbit
# argument is 128 + 127 k s (k = 1 or 0.75) with s a symbol formed from AGC'd samples clipped to magnitude 2.84 (demod_stages.h:161 and its
# counterparts in the OQPSK and burst kernels), i.e. finite and small -- or NaN, where both give 0.  jd_qround's other call (k_burst_front.h:384-385) rounds
# constants of the bank's geometry.
#            v:        (device qRound, x86 qRound, device soft bit, x86 soft bit)
QROUND_OUTSIDE = {
    "nan": (0, 0, 0, 0),
    "+inf": (INT_MAX, INT_MIN, 255, 0),
    "2^31": (INT_MAX, INT_MIN, 255, 0),
    "1e300": (INT_MAX, INT_MIN, 255, 0),
    "-inf": (0, 0, 0, 0),
    "-2^31": (INT_MIN, INT_MIN, 0, 0),
    "-1e300": (0, 0, 0, 0),
}


def test_qround_outside_int_range_is_as_documented(L):
    vals = {"nan": np.nan, "+inf": np.inf, "2^31": 2.0**31, "1e300": 1e300, "-inf": -np.inf, "-2^31": -(2.0**31), "-1e300": -1e300}
    v = f64(list(vals.values()))
    qr, sb = np.zeros(len(v), np.int32), np.zeros(len(v), np.int32)
    call(L, "jp_qround", v, qr, len(v))
    call(L, "jp_softbit", v, sb, len(v))
    got = {k: (int(qr[i]), int(sb[i])) for i, k in enumerate(vals)}
    assert got == {k: (t[0], t[2]) for k, t in QROUND_OUTSIDE.items()}, got


# ---- WaveTable ------------------------------------------------------------------------------------------------------------------
def wt_next(ptr, step):  # WaveTable::WTnextFrame (JAERO/DSP.cpp:70-77)
    if step < 0:
        step = 0.0
    ptr += step
    while int(ptr) >= W:
        ptr -= W
    return ptr, step


def wt_setfreq(f, sr):  # WaveTable::SetFreq (DSP.cpp:151-156)
    freq = f
    if freq < 0:
        freq = 0.0
    return freq, freq * W / sr


def wt_inc_phase_deg(ptr, phase_deg):  # WaveTable::IncresePhaseDeg -> SetPhaseDeg (DSP.cpp:169-180)
    phase_deg += 360.0 * ptr / W
    phase_deg = math.fmod(phase_deg, 360.0)
    while phase_deg < 0:
        phase_deg += 360.0
    return (phase_deg / 360.0) * W


def set_phase_deg(phase_deg):  # WaveTable::SetPhaseDeg (DSP.cpp:175-180)
    phase_deg = math.fmod(phase_deg, 360.0)
    while phase_deg < 0:
        phase_deg += 360.0
    return (phase_deg / 360.0) * W


def advance_fraction(ptr, f):  # WaveTable::AdvanceFractionOfWave (DSP.h:56)
    ptr += f * W
    while ptr >= W:
        ptr -= W
    while ptr < 0:
        ptr += W
    return ptr


def passed(last_ptr, ptr, step, fow, frac):  # WaveTable::IfHavePassedPoint (DSP.cpp:222-238)
    pt = fow * W
    tl, tp = last_ptr - pt, ptr - pt
    if tl < 0.0:
        tl += W
    if tp < 0.0:
        tp += W
    if tl > (3.0 * W / 4.0) and tp < (1.0 * W / 4.0):
        return 1, tp / step
    return 0, frac


def cisidx(p):
    t = int(p)
    if t >= W:
        t = 0
    if t < 0:
        t = int(W) - 1
    return t


def check_elementwise(what, got, want, *ops):
    assert_same(what, f64(got), f64(want), *[f64(o) for o in ops])


def edge_ptrs(rng, n):
    e = [W, np.nextafter(W, 0), np.nextafter(W, 2 * W), W - 1, W - 0.5, 0.0, -0.0, -1e-300, -0.5, -1.0, -W + 0.5, 1e-12, 2 * W - 1]
    return f64(np.concatenate([e, rng.uniform(-W, W, n), rng.uniform(W - 2, W + 2, n)]))


def test_wt_next_and_fb_wt_next_are_wavetables(L):
    rng = np.random.default_rng(17)
    p = edge_ptrs(rng, 1 << 14)
    p = np.concatenate([p, np.repeat(f64([np.nextafter(W, 0), W - 1e-9, 0.0, -3.5]), 64)])
    m = len(p)
    steps = f64(np.concatenate([[0.0, -0.0, -1.0, -1e-300, W - 1e-9, np.nextafter(W, 0), W, 1.0, 1e-300], rng.uniform(-100, W, m - 9)]))
    steps[len(steps) - 256:] = np.tile(f64([np.nextafter(W, 0), 0.5, -5.0, W - 1]), 64)
    steps = np.concatenate([steps, rng.uniform(W, 2.5 * W, 4096)])
    p = np.concatenate([p, rng.uniform(0, W, 4096)])
    want = [wt_next(float(a), float(b)) for a, b in zip(p, steps)]
    for name in ("jp_wt_next", "jp_fb_wt_next"):
        pp, ss = p.copy(), steps.copy()
        call(L, name, pp, ss, len(pp))
        check_elementwise(f"{name} ptr", pp, [w[0] for w in want], p, steps)
        check_elementwise(f"{name} step", ss, [w[1] for w in want], p, steps)


def test_setfreq_forms_agree_with_wavetable_at_every_sample_rate(L):
    rng = np.random.default_rng(18)
    f = f64(np.concatenate([[0.0, -0.0, -1.0, -1e-300, 1e-300, 10500.0, 5250.0, 600.0, 1200.0, 8400.0], rng.uniform(-100, 24000, 1 << 16),
                            rng.uniform(-1, 1, 4096) * 0.1 + 10500.0]))
    for sr in DP.SAMPLE_RATES:
        want = [wt_setfreq(float(v), sr) for v in f]
        fr, st = np.zeros(len(f)), np.zeros(len(f))
        call(L, "jp_wt_setfreq", f, fr, st, len(f), sr)
        check_elementwise(f"jd_wt_setfreq freq at {sr:g}", fr, [w[0] for w in want], f)
        check_elementwise(f"jd_wt_setfreq step at {sr:g}", st, [w[1] for w in want], f)
        fr2, st2 = np.zeros(len(f)), np.zeros(len(f))
        call(L, "jp_fb_wt_setfreq", f, fr2, st2, len(f), sr, 1.0 / sr)
        check_elementwise(f"fb_wt_setfreq freq at {sr:g}", fr2, fr, f)
        check_elementwise(f"fb_wt_setfreq step at {sr:g}", st2, st, f)


def test_phase_helpers_are_wavetables(L):
    rng = np.random.default_rng(19)
    deg_edges = np.array([0.0, -0.0, 360.0, -360.0, 720.0, -720.0, 1080.0, -1080.0, 359.99999999999994, -359.99999999999994])
    degs = f64(np.concatenate([deg_edges, np.nextafter(deg_edges, np.inf), np.nextafter(deg_edges, -np.inf), rng.uniform(-2000, 2000, 1 << 15),
                               rng.uniform(-730, 730, 1 << 15)]))
    o = np.zeros(len(degs))
    call(L, "jp_fb_fmod360", degs, o, len(degs))
    check_elementwise("fb_fmod360", o, [math.fmod(float(v), 360.0) for v in degs], degs)
    ptr = np.full(len(degs), -5.0)
    call(L, "jp_bd_set_phase_deg", degs, ptr, len(degs))
    check_elementwise("bd_set_phase_deg", ptr, [set_phase_deg(float(v)) for v in degs], degs)
    p = edge_ptrs(rng, len(degs))[:len(degs)]
    pp = p.copy()
    call(L, "jp_wt_inc_phase_deg", pp, degs, len(degs))
    check_elementwise("jd_wt_inc_phase_deg", pp, [wt_inc_phase_deg(float(a), float(b)) for a, b in zip(p, degs)], p, degs)
    p = f64(np.concatenate([[0.0, np.nextafter(W, 0), W - 1, 1e-9], rng.uniform(0, W, 1 << 15)]))
    fr = f64(np.concatenate([[-1e-20, 1e-20, 0.0, -1e-12], rng.uniform(-3, 3, 1 << 15)]))
    pp = p.copy()
    call(L, "jp_wt_advance_fraction", pp, fr, len(p))
    check_elementwise("jd_wt_advance_fraction", pp, [advance_fraction(float(a), float(b)) for a, b in zip(p, fr)], p, fr)


def test_passed_point_and_table_index_are_wavetables(L):
    rng = np.random.default_rng(20)
    n = 1 << 16
    fow = f64(np.concatenate([np.tile([0.0, 0.25, 0.5, 0.75], n // 8), rng.random(n // 2)]))
    step = f64(rng.uniform(1e-3, 2000, n))
    ptr = f64(np.mod(fow * W + rng.uniform(-3000, 3000, n), W))
    last = f64(np.where(rng.random(n) < 0.7, np.mod(ptr - step, W), rng.uniform(-10, W, n)))
    frac = np.full(n, -3.0)
    hit = np.zeros(n, np.int32)
    call(L, "jp_wt_passed", last, ptr, step, fow, frac, hit, n)
    want = [passed(float(a), float(b), float(c), float(d), -3.0) for a, b, c, d in zip(last, ptr, step, fow)]
    assert np.array_equal(hit, [w[0] for w in want])
    assert 0.05 < hit.mean() < 0.95
    check_elementwise("jd_wt_passed frac", frac, [w[1] for w in want], last, ptr, step, fow)
    p = f64(np.concatenate([[W, np.nextafter(W, 0), np.nextafter(W, 2 * W), W + 1, -0.5, -1.0, -1e-300, -0.0, 0.0, -W], rng.uniform(-3, W + 3, n)]))
    idx = np.zeros(len(p), np.int32)
    call(L, "jp_cisidx", p, idx, len(p))
    assert np.array_equal(idx, [cisidx(float(v)) for v in p])


# ---- the stages' primitives: IIR::update, DiffDecode::UpdateSoft, the symbol oscillator's step --------------------------------------
@pytest.mark.parametrize("bq", DP.BIQUADS, ids=lambda bq: bq.what)
def test_biquad_is_iir_update_term_by_term(L, bq):
    """jd_biquad against IIR::update restated operation by operation in numpy (which does not fuse), 64 consecutive steps per lane."""
    src, ln = bq.site.split(":")
    with open(os.path.join(DP.CSRC, src)) as fh:
        text = " ".join(fh.read().splitlines()[int(ln) - 2:int(ln) + 1])  # the a's are set on the line before or after the b's
    coef = {k: float(v) for k, v in re.findall(r"g\.(?:res|lf)_([ab][012]) = (-?[0-9.e+-]+);", text)}
    assert coef == dict(zip(("b0", "b1", "b2", "a1", "a2"), bq.b + bq.a)), (bq.site, coef)
    n, steps = 4096, 64
    rng = np.random.default_rng(31)
    special = f64([0.0, -0.0, 1e-300, -1e-300, 1e300, -1e300])
    draw = lambda *shape: f64(rng.standard_normal(shape) * np.exp2(rng.uniform(-8, 8, shape)))  # noqa: E731
    x, st = draw(steps, n), draw(4, n)
    mix = rng.random((steps, n)) < 0.05
    x[mix] = rng.choice(special, int(mix.sum()))
    st[:, :len(special)] = special  # each special value in every state slot of some lane ...
    st[:, len(special):2 * len(special)] = special[::-1]
    x[0, :2 * len(special)] = np.tile(special, 2)  # ... and as the first input of a lane
    (b0, b1, b2), (a1, a2) = bq.b, bq.a
    x1, x2, y1, y2 = (v.copy() for v in st)
    want = np.zeros((steps, n))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for k in range(steps):
            y = np.zeros(n)
            y = y + x2 * b2
            y = y + x1 * b1
            y = y + x[k] * b0
            y = y - y2 * a2
            y = y - y1 * a1
            x2, x1, y2, y1 = x1, x[k].copy(), y1, y
            want[k] = y
    got_st, got = f64(st.copy()), np.full((steps, n), np.nan)
    call(L, "jp_biquad", f64(x), got_st, got, n, steps, b0, b1, b2, a1, a2)
    assert_same(f"jd_biquad y ({bq.what})", got.ravel(), want.ravel(), x.ravel())
    assert_same(f"jd_biquad state ({bq.what})", got_st.ravel(), np.concatenate([x1, x2, y1, y2]), st.ravel())


def test_diff_soft_is_diffdecodes_updatesoft(L):
    """jd_diff_soft against DiffDecode::UpdateSoft (DSP.cpp:531-563): every sign combination with +-0 on either side, then random pairs."""
    rng = np.random.default_rng(32)
    signs = f64([-2.5, -0.0, 0.0, 3.5, -1e-300, 1e-300])
    si = f64(np.concatenate([np.repeat(signs, len(signs)), rng.standard_normal(4096)]))
    dl = f64(np.concatenate([np.tile(signs, len(signs)), rng.standard_normal(4096)]))
    want = np.where((si < 0) & (dl < 0), dl, np.where((si > 0) & (dl > 0), -dl, np.fabs(dl)))
    got, got_dl = np.full(len(si), np.nan), dl.copy()
    call(L, "jp_diff_soft", si, got_dl, got, len(si))
    assert_same("jd_diff_soft value", got, want, si, dl)
    assert_same("jd_diff_soft diff_last", got_dl, si, si, dl)


def wt_next_symbol(ptr, step):  # WTnextFrame with last_WTptr (DSP.cpp:70-77)
    if step < 0:
        step = 0.0
    last = ptr
    ptr += step
    while int(ptr) >= W:
        ptr -= W
    return ptr, step, last


def test_symbol_oscillator_step_is_wavetables(L):
    """jd_wt_next_symbol: step negative, zero, just below / at / just above JD_WTSIZE - ptr, and beyond two table lengths (the `while`)."""
    rng = np.random.default_rng(33)
    ptrs = f64(np.concatenate([[0.0, 0.5, 1234.56789, W - 1, W - 0.5, np.nextafter(W, 0)], rng.uniform(0, W, 250)]))
    p, s = [], []
    for q in ptrs:
        gap = W - q
        for st in (-1.0, -1e-300, -0.0, 0.0, np.nextafter(gap, 0), gap, np.nextafter(gap, 2 * W), gap - 1e-9, gap + 1e-9, 2 * W + 0.25, 2.5 * W,
                   3 * W + gap, 761.9, 2187.4):
            p.append(q)
            s.append(st)
    p, s = f64(p), f64(s)
    want = [wt_next_symbol(float(a), float(b)) for a, b in zip(p, s)]
    assert sum(1 for a, b in zip(p, s) if a + max(b, 0.0) >= 2 * W) > 500  # the loop behind the first subtraction runs
    pp, ss, ll = p.copy(), s.copy(), np.full(len(p), -7.0)
    call(L, "jp_wt_next_symbol", pp, ss, ll, len(p))
    for k, what, got in ((0, "ptr", pp), (1, "step", ss), (2, "last", ll)):
        check_elementwise(f"jd_wt_next_symbol {what}", got, [w[k] for w in want], p, s)


# ---- matched-filter evaluators --------------------------------------------------------------------------------------------------
def fma_exact(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # one rounding (int / int true division is correctly rounded)


@pytest.mark.parametrize("row", DP.FIR_ROWS, ids=lambda r: r.export)
def test_fir_evaluator_sums_in_the_reference_order_at_every_ring_position(L, row):
    rng = np.random.default_rng(21 + row.firn + row.ldsn + 7 * row.fused)
    firn, ldsn = row.firn, row.ldsn
    tailn = firn - row.t0 - ldsn  # block rows sum taps t0 .. firn-1 on top of per-lane start sums
    data = lambda *shape: f64(rng.standard_normal(shape) * np.exp2(rng.uniform(-6, 6, shape)))  # noqa: E731
    taps = data(firn)
    if firn == 55:
        taps[28:] = taps[:27][::-1]
        assert np.array_equal(taps, taps[::-1])
    tre, tim, rre, rim = data(max(tailn, 1), 64), data(max(tailn, 1), 64), data(ldsn, 64), data(ldsn, 64)
    ore, oim = np.full((ldsn, 64), np.nan), np.full((ldsn, 64), np.nan)
    start = (data(64), data(64)) if row.bs else (np.zeros(64), np.zeros(64))
    if row.bs:
        assert ldsn % row.bs == 0 and np.all(start[0] != 0) and np.all(start[1] != 0)
        call(L, row.export, taps, tre, tim, rre, rim, start[0], start[1], ore, oim)
    else:
        call(L, row.export, taps, tre, tim, rre, rim, ore, oim)
    last = row.func == "jd_fir_eval_sym_static_but_last"
    for slot in range(ldsn):
        # oldest first: the register tail (tre[j] = x[n-LDSN-1-j]), then the ring from fir_slot (but_last: from the slot after slot_old,
        # whose entry the caller has moved into tre[0], and without the newest term)
        order = [(tre[tailn - 1 - s], tim[tailn - 1 - s]) for s in range(tailn)]
        first = slot + 1 if last else slot
        order += [(rre[(first + q) % ldsn], rim[(first + q) % ldsn]) for q in range(ldsn - 1 if last else ldsn)]
        if row.fused:
            for arm, out in ((0, ore), (1, oim)):
                acc = [float(v) for v in start[arm]]
                for k, xs in enumerate(order):
                    acc = [fma_exact(float(taps[row.t0 + k]), float(xs[arm][ln]), acc[ln]) for ln in range(64)]
                check_elementwise(f"{row.export} fir_slot {slot} arm {arm}", out[slot], acc)
            continue
        are, aim = start[0].copy(), start[1].copy()
        for k, (xr, xi) in enumerate(order):
            are = are + taps[row.t0 + k] * xr
            aim = aim + taps[row.t0 + k] * xi
        check_elementwise(f"{row.export} fir_slot {slot} re", ore[slot], are)
        check_elementwise(f"{row.export} fir_slot {slot} im", oim[slot], aim)
