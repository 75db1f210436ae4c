"""GPU (-m gpu): every launch mode of the Viterbi decoders against the oracle, through jaero_debug_viterbi (the library's own viterbi_launch
with all of its parameters in the test's hands, the output buffer not cleared).  Cases and the expected bytes: tests/viterbi_cases.py.
Integer arithmetic: every comparison is np.array_equal on the WHOLE output buffer (and the whole overlap buffer), poison included."""
import ctypes as C

import numpy as np
import pytest

import viterbi_cases as V

pytestmark = pytest.mark.gpu


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def run(c, layout, soft_buf=None, tiled=None, out=None):
    """One launch of case c in `layout`; returns (out, overlap) as the device left them."""
    from jaero_amd import capi

    soft = c.soft_buffer() if soft_buf is None else soft_buf
    out = c.poisoned_out() if out is None else out
    ov = None if c.overlap is None else c.overlap.copy()
    valid, lens = _i32(c.valid), _i32(c.lens)
    q = capi.ViterbiProbe(soft=soft.ctypes.data, nblocks=c.nblocks, nsoft=c.nsoft, pitch=c.pitch, tiled=c.tiled if tiled is None else tiled,
                          soft_misalign=c.misalign, pad=c.pad, overlap=None if ov is None else ov.ctypes.data, out=out.ctypes.data,
                          out_rows=out.shape[0], out_stride=out.shape[1], out_start=c.out_start, out_want=c.out_want, packed=c.packed,
                          layout=V.LAYOUTS[layout], update_overlap=c.update_overlap, valid=None if valid is None else valid.ctypes.data,
                          lens=None if lens is None else lens.ctypes.data)
    capi.check(capi.lib().jaero_debug_viterbi(0, C.byref(q)))
    return out, ov


def check(O, c):
    want_out, want_ov = V.expected(O, c)
    assert (want_out != V.POISON).any() or c.valid is not None and not c.valid.any()
    for layout in c.layouts:
        out, ov = run(c, layout)
        assert np.array_equal(out, want_out), (c.name, layout, "first differing rows", np.unique(np.nonzero(out != want_out)[0])[:8])
        if ov is not None:
            assert np.array_equal(ov, want_ov), (c.name, layout, "overlap rows", np.unique(np.nonzero(ov != want_ov)[0])[:8])
    print(f"{c.name}: layouts {'/'.join(c.layouts)}, {c.nblocks} blocks, {c.bits_compared()} bits in {want_out.size} output bytes compared per layout")
    return want_out, want_ov


def _params(group):
    return pytest.mark.parametrize("c", V.by_group(group), ids=lambda c: c.name)


@_params("lengths")
def test_lengths(oracle_mod, c):
    check(oracle_mod, c)


@_params("long")
def test_renormalise_and_traceback_on_one_step(oracle_mod, c):
    check(oracle_mod, c)


@_params("overlap")
def test_overlap_passes_and_continuation(oracle_mod, c):
    """Mixed overlap lengths in one wavefront; then the next call of the same streams from the overlap the device left."""
    _, ov = check(oracle_mod, c)
    if c.update_overlap:
        check(oracle_mod, V.continuation(c, ov))


@_params("window")
def test_window(oracle_mod, c):
    check(oracle_mod, c)


@_params("pitch")
def test_pitch_and_alignment(oracle_mod, c):
    check(oracle_mod, c)


@_params("tiled")
def test_tiled_input(oracle_mod, c):
    """Tiled rows against the oracle, and against the same rows given row-major."""
    want_out, want_ov = check(oracle_mod, c)
    for layout in c.layouts:
        out, ov = run(c, layout, soft_buf=np.ascontiguousarray(c.soft), tiled=0)
        assert np.array_equal(out, want_out) and np.array_equal(ov, want_ov), (c.name, layout, "row-major")


@_params("lens")
def test_lens(oracle_mod, c):
    check(oracle_mod, c)


@_params("valid")
def test_valid(oracle_mod, c):
    check(oracle_mod, c)


@pytest.mark.parametrize("name", ["len300_pad24_x130", "len1210_pad0_x65", "ovmix292", "win662_s25_w351_by", "pitch116_in128_mis0", "lens_ov_pad", "valid_alternating"])
def test_entry_points_agree(name):
    """k_viterbi, k_viterbi_lanes and k_viterbi_lanes_x2 leave the same bytes for the same probe (no oracle involved)."""
    c = V.case(name)
    assert c.layouts == ("wave", "lanes", "x2")
    res = {layout: run(c, layout) for layout in c.layouts}
    for layout in ("lanes", "x2"):
        assert np.array_equal(res[layout][0], res["wave"][0]), (name, layout)
        if c.overlap is not None:
            assert np.array_equal(res[layout][1], res["wave"][1]), (name, layout)
    print(f"{name}: {c.nblocks} blocks, {res['wave'][0].size} output bytes x 3 entry points")


@pytest.mark.parametrize("layout", ["wave", "lanes"])
def test_public_entry_points_give_the_hooks_bytes(force_viterbi_layout, layout):
    """jaero_viterbi_decode_soft and jaero_viterbi_continuous against the hook with the probe they amount to (they clear the output first,
    so the probe's buffer starts as zeros): ties the hook to the production launch."""
    from jaero_amd import capi

    L = capi.lib()
    force_viterbi_layout(layout)
    nb, ns = 65, 662
    soft = np.ascontiguousarray(V.rows(ns)[:nb])
    out = np.full((nb, ns // 2), V.POISON, np.uint8)
    capi.check(L.jaero_viterbi_decode_soft(0, soft.ctypes.data, nb, ns, out.ctypes.data, 0, None))
    c = V.Case("public_soft", "public", soft)
    got, _ = run(c, layout, out=np.zeros((nb, ns // 2), np.uint8))
    assert np.array_equal(out, got)
    ov0 = V.overlaps(nb, (62, 0), 5)
    ov0[:, 63] = 0  # the host path of jaero_viterbi_continuous rewrites all 64 bytes
    ov0[ov0[:, 62] == 0] = 0
    ov = ov0.copy()
    out = np.full((nb, ns // 2), V.POISON, np.uint8)
    nbits = np.zeros(nb, np.int32)
    capi.check(L.jaero_viterbi_continuous(0, soft.ctypes.data, nb, ns, 24, ov.ctypes.data, out.ctypes.data, nbits.ctypes.data, 0, None))
    c = V.Case("public_cont", "public", soft, pad=24, overlap=ov0, update_overlap=1, out_start=25)
    got, gov = run(c, layout, out=np.zeros((nb, ns // 2), np.uint8))
    assert np.array_equal(out, got) and np.array_equal(ov, gov)
    assert np.array_equal(nbits, np.where(ov0[:, 62] == 0, (ns + 24) // 2 - 25, ns // 2))
    print(f"public entry points, {layout}: {nb} blocks, 2 x {out.size} output bytes and {ov.size} overlap bytes compared")
