"""GPU (-m gpu): the addresses the coarse-frequency estimate kernels form themselves (coarse6_body of jaero_amd/csrc/k_coarse6.h, DESIGN 9
item 34): the ring entries of the first estimate and of the prefetch for the next one, read at a 32-bit byte offset that wraps in bytes, the
rows of the exchange buffer above 64 KiB, and the band limit's single range test.

Every configuration of coarse_cases.CONFIGS runs lists with more entries than workgroups, so that every workgroup prefetches the ring of its
next entry under its epilogue, the last entry's dummy prefetch included.  The ring pointers are the quarter points 0, N / 4, N / 2, 3 N / 4
(where a slot's row starts on a row of the ring) and the unaligned ones of Cfg.pointers(); the locking bandwidths give startbin 1, a startbin
that is no multiple of the thread count, and one from which the fold leaves the spectrum.  y, the estimate's bin and the slot state are held
to what tests/test_gpu_coarse.py::test_parity_matrix holds them to, with its harness."""
import numpy as np
import pytest

import coarse_cases as CC
from test_gpu_coarse import (Bank, bin_from_state, check_untouched, check_visible_after, oracle_estimate, visible_state, y_after_three)

pytestmark = pytest.mark.gpu
LD = np.longdouble


def bandwidths(cfg):
    """[startbin == 1, startbin not a multiple of NT with the fold inside, fold_inside false, the default]"""
    one = next(b for b in cfg.lbws if cfg.startbin(b) == 1)
    odd = next(b for b in cfg.lbws if cfg.startbin(b) > 1 and cfg.startbin(b) % cfg.NT and cfg.fold_inside(b))
    wide = next(b for b in cfg.lbws if not cfg.fold_inside(b) and b < cfg.Fs / 2)
    assert cfg.startbin(wide) % cfg.NT  # (the default's startbin is a whole number of rows for 10.5 kbps, 7 x 512, and not for the others)
    return [one, odd, wide, cfg.lbw0]


def ring_pointers(cfg):
    N = cfg.N
    p = [0, N // 4, N // 2, 3 * N // 4] + cfg.pointers()[1:]
    assert len(set(p)) == len(p) and all(0 <= q < N for q in p) and {1, cfg.NT - 1, 4097} <= set(p)
    return p


@pytest.mark.parametrize("name", list(CC.CONFIGS))
def test_lists_longer_than_the_grid(oracle_mod, name):
    O, cfg = oracle_mod, CC.CONFIGS[name]
    N = cfg.N
    rng = np.random.default_rng(0xADD2 + list(CC.CONFIGS).index(name))
    bws, ptrs = bandwidths(cfg), ring_pointers(cfg)
    nch = len(ptrs) + 1                                       # 12: one channel stays outside every list
    lbws = [bws[ch % len(bws)] for ch in range(nch)]
    bank = Bank(cfg, lbws)
    try:
        perm = [int(c) for c in rng.permutation(nch - 1)]
        # (list, grid): 11 entries on 5 workgroups (3 + 2 + 2 + 2 + 2), then 5 entries on 2 (3 + 2) with every pointer moved on by three,
        # which gives each bandwidth other pointers
        for case, (chans, grid) in enumerate([(perm, 5), (perm[::-1][:5], 2)]):
            inputs = []
            for ch, lbw in enumerate(lbws):
                x = CC.draw(cfg, lbw, rng, signal=(ch + case) % 2 == 0)
                ptr = ptrs[(ch + 3 * case) % len(ptrs)]
                ykind = (ch + case) % 3
                y_in = np.zeros(N) if ykind == 0 else np.full(N, 20.0) if ykind == 1 else y_after_three(O, cfg, lbw, rng)
                bank.poke(ch, ring=np.roll(x, ptr), y=y_in, **visible_state(cfg, ptr))  # ring[(ptr + j) % N] = x[j]
                inputs.append((x, y_in, ptr))
            before = bank.peek_all()
            cpu = {}
            for ch in chans:
                x, y_in, _ = inputs[ch]
                bin_o, y_o = oracle_estimate(O, cfg, lbws[ch], x, y_in)
                L_ref, y_ld = CC.restate(cfg, lbws[ch], x, y_in)
                ok, ratio = CC.margin_ok(cfg, lbws[ch], y_ld, y_o)
                cpu[ch] = (bin_o, y_o, L_ref, ok, ratio)
            assert bank.launch(chans, grid) == 0, bank.L.jaero_last_error()
            after = bank.peek_all()
            check_untouched(before, after, [c for c in range(nch) if c not in chans], (name, case))
            nbound = 0
            for ch in chans:
                what = (name, case, f"channel {ch} lockingbw {lbws[ch]:g} startbin {cfg.startbin(lbws[ch])} ptr {inputs[ch][2]}")
                bin_o, y_o, L_ref, ok, ratio = cpu[ch]
                y_in = inputs[ch][1]
                check_visible_after(cfg, before[ch], after[ch], what)
                if ok:
                    nbound += 1
                    assert bin_from_state(cfg, after[ch][2]) == bin_o, (what, f"peak bin (margin ratio {ratio:.3g})")
                zmax = float(L_ref.max())
                lin = lambda y: np.power(LD(10), np.asarray(y, dtype=LD) - LD(0.9) * np.asarray(y_in, dtype=LD))
                err_o = float(np.max(np.abs(lin(y_o) - L_ref)))
                err_k = float(np.max(np.abs(lin(after[ch][1]) - L_ref)))
                print(f"{what}: y kernel {err_k / zmax / CC.EPS:.1f} eps, oracle {err_o / zmax / CC.EPS:.1f} eps of max|Z|")
                assert err_k <= 8 * err_o + 4 * CC.EPS * zmax, (what, f"y: kernel {err_k / zmax / CC.EPS:.1f} eps, oracle {err_o / zmax / CC.EPS:.1f} eps of max|Z| = {zmax:.3g}")
            assert nbound * 2 >= len(chans), (name, case, f"only {nbound} of {len(chans)} draws bind the peak bin")
    finally:
        bank.close()
