"""Host only: tests/kernel_variants.py lists exactly the kernel instantiations the library holds, and every row is consistent with its recipe.

A new or renamed instantiation (a re-tuned FB_LDSN / MFB4_TB / ..., a new rate) without a row fails here with its name, and so does a row
the library no longer builds; the GPU side (tests/test_gpu_variants.py) then runs every row against the oracle."""
import ctypes as C
import re
import shutil
import subprocess

import pytest

import kernel_variants as KV
from jaero_amd import capi

# the kernel-handle symbols (`V void k_msk_fb<...>(...)`, `D k_coarse6(...)`), not the host stubs (`T __device_stub__k_msk_fb<...>(...)`)
_HANDLE = re.compile(r"^[0-9a-fA-F]+\s+[A-Za-z]\s+(?:void\s+)?(k_[A-Za-z0-9_]+(?:<[^<>()]*>)?)\(")


def library_kernels():
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm on PATH")
    out = subprocess.run([nm, "-C", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    found = set()
    for line in out.splitlines():
        m = _HANDLE.match(line)
        if m and m.group(1).split("<")[0] in KV.KERNEL_FAMILIES:
            found.add(m.group(1))
    return found


def test_table_lists_every_instantiation_of_the_library():
    have = library_kernels()
    want = KV.expected_symbols()
    assert have, "no kernel of the chosen families found in the library"
    missing = sorted(have - want)
    stale = sorted(want - have)
    assert not missing, f"instantiations in the library without a row in tests/kernel_variants.py: {missing}"
    assert not stale, f"rows of tests/kernel_variants.py the library does not build: {stale}"


def _targs(name):
    return [a.strip() for a in name[name.index("<") + 1:-1].split(",")] if "<" in name else []


def test_rows_agree_with_their_recipes():
    ids = [v.id for v in KV.VARIANTS]
    assert len(ids) == len(set(ids)), "two rows with the same recipe"
    assert len({v.kernel0 for v in KV.VARIANTS}) == len(KV.VARIANTS), "two rows expect the same sample-loop / demodulator instantiation"
    tf = {"true": True, "false": False}
    for v in KV.VARIANTS:
        fam = KV.FAMILIES[v.family]
        base, args = v.kernel0.split("<")[0], _targs(v.kernel0)
        assert v.layout in (0, 1, 2), v
        if v.burst:
            assert not v.ebno and v.layout == 0, v
            cs = args[0]
            assert tf[cs] == v.capture, v
            assert v.kernel1 == f"k_trident<{'true' if fam['kind'] == 'burst_oqpsk' else 'false'}>", v
            if fam["kind"] == "burst_msk":
                assert base == "k_burst_msk_fb" and int(args[1]) == round(2 * fam["Fs"] / fam["fb"]), v
            else:
                assert base == "k_burst_oqpsk_demod", v
            continue
        assert (tf[args[2]], tf[args[3]]) == (v.ebno, v.capture), v
        taps = 55 if fam["kind"] == "oqpsk" else round(2 * fam["Fs"] / fam["fb"])
        assert int(args[0]) == taps, v
        if base == "k_oqpsk_fb":
            assert tf[args[5]] == (fam["fb"] == 8400.0), v
        if base == "k_oqpsk_fb" or (base == "k_msk_fb" and taps == 80):
            assert v.layout in (1, 2) and int(args[4]) == (4 if v.layout == 2 else 1), v  # chosen by size: every row forces its layout
        else:
            assert v.layout == 0, v
        coarse = "k_coarse6_13" if fam["power"] == 13 else ("k_coarse6_w8400" if fam["fb"] == 8400.0 else "k_coarse6")
        assert v.kernel1 == coarse, v


def test_layout_hook_validates_its_argument():
    L = capi.lib()
    try:
        for mode in (0, 1, 2):
            assert L.jaero_debug_sample_loop_layout(mode) == 0
        assert L.jaero_debug_sample_loop_layout(3) == capi.E_INVAL
        assert L.jaero_debug_sample_loop_layout(-1) == capi.E_INVAL
    finally:
        L.jaero_debug_sample_loop_layout(0)
    buf = C.create_string_buffer(64)
    assert L.jaero_debug_kernel_variant(None, 0, buf, 64) == capi.E_INVAL
