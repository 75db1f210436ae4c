"""CPU: the C restatement (oracle/) must reproduce, bit for bit, what the UNMODIFIED reference emitted for the
committed golden inputs (tests/golden/*.npz, produced by oracle/_ref via tests/golden/make_golden.py)."""

import numpy as np
import pytest

from conftest import load_golden, oracle_settings

CASES = ["oqpsk_10k5_default", "oqpsk_10k5_afc_chunk1000_dcd", "msk_1200_default", "msk_600_chunk777_dcd",
         "oqpsk_10k5_cpureduce", "oqpsk_8400_default", "oqpsk_8400_afc_chunk1500_dcd"]


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference_golden(oracle_mod, name):
    O = oracle_mod
    g = load_golden(name)
    opts = g["opts"]
    r = O.run_demod(oracle_settings(O, g["kind"], opts), g["pcm"], chunk=opts.get("chunk", 4096), afc=bool(opts.get("afc", 0)),
                    cpu_reduce=bool(opts.get("cpureduce", 0)), dcd_at=opts.get("dcd_at", -1))
    assert np.array_equal(r["soft"], g["soft"])
    assert r["status"].shape == g["status"].shape
    # columns: n, freq_est, freq_center, mse, (ebno), signal -- EbNo starts from an uninitialised member in the
    # reference (DSP.cpp:715-721) so it is compared separately with NaN tolerance
    assert np.array_equal(r["status"][:, [0, 1, 2, 3, 5]], g["status"][:, [0, 1, 2, 3, 5]])
    eb_ref = g["status"][:, 4]
    ok = np.isfinite(eb_ref)
    assert np.array_equal(r["status"][ok, 4], eb_ref[ok])


@pytest.mark.parametrize("name", ["1200bps_burst_sample1", "1200bps_burst_sample2"])
def test_oracle_on_bundled_recordings(oracle_mod, name):
    """The reference's own sample recordings (continuous MSK demod over burst audio); their PCM is tests/golden/<name>_pcm.npz."""
    O = oracle_mod
    g = load_golden(name + "_contmsk")
    x = load_golden(name + "_pcm")["pcm"]
    assert len(x) == int(g["nsamples"])
    r = O.run_demod(O.msk_settings(), x)
    assert np.array_equal(r["soft"], g["soft"])
    assert np.array_equal(r["status"][:, [0, 1, 2, 3, 5]], g["status"][:, [0, 1, 2, 3, 5]])


def test_chunking_invariance(oracle_mod):
    """Reference property: the soft-bit stream does not depend on how writeData is chunked."""
    O = oracle_mod
    g = load_golden("oqpsk_10k5_default")
    a = O.run_demod(O.oqpsk_settings(), g["pcm"], chunk=4096)["soft"]
    b = O.run_demod(O.oqpsk_settings(), g["pcm"], chunk=777)["soft"]
    c = O.run_demod(O.oqpsk_settings(), g["pcm"], chunk=len(g["pcm"]))["soft"]
    assert np.array_equal(a, b) and np.array_equal(a, c)


def test_empty_and_tiny_writes(oracle_mod):
    O = oracle_mod
    d = O.Demod(O.oqpsk_settings())
    d.write(np.zeros(0, np.int16))
    d.write(np.zeros(1, np.int16))
    assert d.take_soft().size == 0 and d.pending == 0
    d = O.Demod(O.msk_settings())
    d.write(np.full(3, 32767, np.int16))
    assert d.take_soft().size == 0


def test_full_scale_input_is_finite(oracle_mod):
    """int16 extremes: the AGC/clip path must keep everything finite."""
    O = oracle_mod
    x = np.tile(np.array([32767, -32768], np.int16), 24000)
    r = O.run_demod(O.oqpsk_settings(), x, capture_symbols=True)
    assert np.all(np.isfinite(r["symbols"]))
    assert np.all((r["soft"] >= 0) & (r["soft"] <= 255))
