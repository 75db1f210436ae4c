"""CPU: the burst bank's reassembly code (jaero_amd/csrc/k_aerolb_isu.h, compiled for the host) under the address and undefined-behaviour
sanitizers, as a program of its own: tests/host_emul/aerolb_isu_main.cpp is built with g++ -fsanitize=address,undefined and run over every
case stream.  The R slots and the input rows are allocated exactly, so a read behind a slot (the emit's sixteen-byte loads) or behind a row
is an error, not luck.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import rt_isu_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(oracle_mod):
    oracle_mod.lib()
    td = tempfile.mkdtemp(prefix="aerolb_isu_san_")
    exe = os.path.join(td, "aerolb_isu_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "tests", "host_emul", "stub"), "-o", exe, os.path.join(ROOT, "tests", "host_emul", "aerolb_isu_main.cpp"),
           "-L" + os.path.join(ROOT, "oracle"), "-l:liboracle.so", "-Wl,-rpath," + os.path.join(ROOT, "oracle")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode and "sanitizer" in r.stderr.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("this g++ has no sanitizer runtimes")
    assert r.returncode == 0, r.stderr
    return exe, td


@pytest.mark.parametrize("fb,width,cap", [(10500, 3000, 64), (1200, 2996, 3)])
def test_every_case_runs_clean_under_the_sanitizers(prog, oracle_mod, fb, width, cap):
    """cap 3: the log overflows on most channels (the refused rows must not be written anywhere)."""
    exe, td = prog
    plan = RC.channel_plan(len(RC.NAMES) + 1, fb, noise_every=len(RC.NAMES) + 1)
    path = os.path.join(td, f"streams_{fb}.bin")
    with open(path, "wb") as f:
        f.write(np.int32(len(plan)).tobytes())
        for name, inv in plan:
            s = RC.stream(name, fb, inv)
            f.write(np.int32(len(s)).tobytes())
            f.write(np.ascontiguousarray(s, np.int16).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(fb), str(cap), str(width), path], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    rows = [[int(v) for v in ln.split()] for ln in r.stdout.strip().split("\n")]
    assert len(rows) == len(plan)
    for (name, inv), row in zip(plan, rows):
        msgs, stats, _, _, _, _ = RC.expected(oracle_mod, name, fb, inv)
        assert row[1] == min(len(msgs), cap) and row[2] == (8 if len(msgs) > cap else 0) and row[3:] == list(stats), (name, row)
