"""GPU (-m gpu): the estimate kernels' transforms with absorbed twiddles (jaero_amd/csrc/wg_fft.h, C6_ABSORB) on inputs whose transform
is known in closed form, through jaero_debug_coarse_poke / _launch / _peek on banks of 3 channels, one estimate each: 10.5 kbps and 8400 bps
(2^14 points), 1200 bps MSK (2^13 points).

  impulse at ring position 0, 1, NT - 1 = 511 (2^14), NT = 512, N - 1 (pointer 0: ring position = time index; 511 / 512 are the last thread
      of one slot and the first of the next; every bin of the first transform has the impulse's modulus),
  one complex tone exactly on a bin inside the band limit (the third transform is N^3 a^2 on one bin, nothing elsewhere) and one outside
      it (nothing passes: y_out = 0.9 y_in),
  all zeros (y_out = 0.9 y_in bit for bit).

y is compared with the long-double restatement of tests/coarse_cases.py by the rule of tests/test_gpu_coarse.py: kernel error <= 8 x oracle
error + 4 eps max|Z| on L = 10^(y_out - 0.9 y_in); the peak bin must be the oracle's wherever coarse_cases.margin_ok calls it binding (and
there oracle and restatement agree, checked before anything is launched)."""
import numpy as np
import pytest

import coarse_cases as CC
from test_gpu_coarse import Bank, bin_from_state, check_visible_after, oracle_estimate, visible_state

pytestmark = pytest.mark.gpu
LD = np.longdouble
NAMES = ["oqpsk_10500", "oqpsk_8400", "msk_1200"]


def tone(N, k, amp):
    """amp exp(2 pi i k n / N) with the phase reduced exactly"""
    ph = (k * np.arange(N)) % N
    return amp * np.exp(2j * np.pi * ph / N)


def inputs(cfg):
    """[(name, x in time order, ring pointer, y_in)]: eight of them, y_in zeros / all 20 / a ramp in turn"""
    N, NT, sb = cfg.N, cfg.NT, cfg.startbin(cfg.lbw0)
    ptrs = cfg.pointers()
    out = []
    for pos in (0, 1, 511, 512, N - 1):
        x = np.zeros(N, dtype=np.complex128)
        x[pos] = 0.75 - 0.5j
        out.append((f"impulse_{pos}", x, 0))
    assert 2 <= sb // 2 < sb and sb + 100 < N // 2 and NT in (256, 512)
    out.append(("tone_inside", tone(N, sb // 2, 0.25 + 0.125j), ptrs[3]))
    out.append(("tone_outside", tone(N, sb + 100, 0.25 + 0.125j), ptrs[6]))
    out.append(("zeros", np.zeros(N, dtype=np.complex128), ptrs[4]))
    ys = [np.zeros(N), np.full(N, 20.0), np.linspace(0.0, 30.0, N)]
    return [(n, x, p, ys[i % 3]) for i, (n, x, p) in enumerate(out)]


def cpu_side(O, cfg):
    """per input: (oracle bin, oracle y, restatement's L, binding?) -- and what the inputs were chosen for, checked on the CPU"""
    lbw = cfg.lbw0
    out = []
    for name, x, ptr, y_in in inputs(cfg):
        bin_o, y_o = oracle_estimate(O, cfg, lbw, x, y_in)
        L_ref, y_ld = CC.restate(cfg, lbw, x, y_in)
        ok, ratio = CC.margin_ok(cfg, lbw, y_ld, y_o)
        if ok:
            assert bin_o == CC.peak_bin(cfg, lbw, y_ld), (cfg.name, name, "oracle and restatement disagree on a binding peak")
        if name in ("zeros", "tone_outside"):
            assert float(L_ref.max()) == 1.0 and np.array_equal(y_o, y_in * 0.9), (cfg.name, name)
        if name == "tone_inside":
            k2 = (2 * (cfg.startbin(lbw) // 2) + cfg.N // 2) % cfg.N   # the squared tone's bin, shifted
            assert int(np.argmax(L_ref)) == k2 and float(np.sort(L_ref)[-2]) == 1.0, (cfg.name, name)
        out.append((bin_o, y_o, L_ref, ok, ratio))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_inputs(oracle_mod, name):
    O, cfg = oracle_mod, CC.CONFIGS[name]
    lbw = cfg.lbw0
    cases = inputs(cfg)
    cpu = cpu_side(O, cfg)
    bank = Bank(cfg, [lbw] * 3)
    try:
        for first in range(0, len(cases), 3):
            group = list(range(first, min(first + 3, len(cases))))
            for ch, i in enumerate(group):
                _, x, ptr, y_in = cases[i]
                bank.poke(ch, ring=np.roll(x, ptr), y=y_in, **visible_state(cfg, ptr))  # ring[(ptr + j) % N] = x[j]
            before = bank.peek_all()
            assert bank.launch(list(range(len(group))), 0) == 0, bank.L.jaero_last_error()
            after = bank.peek_all()
            for ch, i in enumerate(group):
                cname, x, ptr, y_in = cases[i]
                bin_o, y_o, L_ref, ok, ratio = cpu[i]
                what = (name, cname)
                check_visible_after(cfg, before[ch], after[ch], what)
                y_k = after[ch][1]
                if cname in ("zeros", "tone_outside"):
                    assert np.array_equal(y_k.view(np.uint64), (y_in * 0.9).view(np.uint64)), (what, "y_out != 0.9 * y_in")
                zmax = float(L_ref.max())
                lin = lambda y: np.power(LD(10), np.asarray(y, dtype=LD) - LD(0.9) * np.asarray(y_in, dtype=LD))
                err_o = float(np.max(np.abs(lin(y_o) - L_ref)))
                err_k = float(np.max(np.abs(lin(y_k) - L_ref)))
                print(f"\ncoarse absorbed {name} {cname}: max|L - ref| / max|Z|: oracle {err_o / zmax / CC.EPS:.2f} eps, kernel {err_k / zmax / CC.EPS:.2f} eps "
                      f"(max|Z| {zmax:.3g}); peak {'binding' if ok else 'not binding'} (margin ratio {ratio:.3g})")
                assert err_k <= 8 * err_o + 4 * CC.EPS * zmax, (what, f"y: kernel {err_k / zmax / CC.EPS:.1f} eps, oracle {err_o / zmax / CC.EPS:.1f} eps of max|Z| = {zmax:.3g}")
                if ok:
                    assert bin_from_state(cfg, after[ch][2]) == bin_o, (what, f"peak bin (margin ratio {ratio:.3g})")
    finally:
        bank.close()
