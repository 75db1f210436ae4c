"""Which decisions of the Aero-L oracle (oracle/aerol_oracle.c, jo_aerol_coverage) do the streams of the existing Aero-L GPU tests take?

Feeds, on the CPU, the tests/golden/aerol_* fixtures and the generator calls of tests/test_gpu_aerol.py, test_gpu_aerol_burst.py and
test_gpu_aerol_c.py (their parameters; the tick schedule of the carrier-loss test) through the counting oracle, then every case of
tests/aerol_branch_cases.py, and writes profiles/aerol_branches.json: {"survey": {family: {counter: total}}, "cases": {case: {counter: count}}}
(cases: the counters of the family's chain that are not zero).  tests/test_aerol_branch_cases.py reads the survey.

    python scripts/aerol_branch_survey.py
"""
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import aerol_branch_cases as ABC  # noqa: E402
from jaero_amd import aerol_frames as AF  # noqa: E402
from oracle import oracle as O  # noqa: E402


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"), allow_pickle=False)


def feed(fam, stream, total, group=32, ticks=None):
    """one channel: the stream in groups (R/T: the demodulator's), ticks = {stream position: count}"""
    fb, burst = ABC.FAMILIES[fam]
    a = O.AeroL(fb, burst=burst)
    cuts = [(s, e) for s, e in O.demod_groups(stream)] if burst else [(s, min(len(stream), s + group)) for s in range(0, len(stream), group)]
    for s, e in cuts:
        a.write(stream[s:e])
        for _ in range((ticks or {}).get(e, 0)):
            a.tick_dcd()
    for k, v in a.coverage().items():
        total[k] = total.get(k, 0) + v


def noise(rng, n, sigma=45):
    return np.clip(np.round(128 + rng.normal(0, sigma, n)), 0, 255).astype(np.int16)


def survey():
    out = {fam: {n: 0 for n in O.AeroL.coverage_names()} for fam in ABC.FAMILIES}
    spec = importlib.util.spec_from_file_location("mk", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    # ---- test_gpu_aerol.py
    for fb in (10500, 1200, 600):
        fam = f"P{fb}"
        feed(fam, golden(f"aerol_{fb}")["soft"], out[fam])
    for fb in (10500, 1200, 600):  # test_bank_vs_oracle (1200 and 10500 in the wave layout, 10500 and 600 in the lane layout: the streams are the same)
        rng = np.random.default_rng(fb)
        for c in range(70):
            bits, _ = AF.p_channel_bits(AF.random_payloads(5, fb, seed=1000 + c), fb, invert_i=bool(c & 1), invert_q=bool(c & 2))
            pre = rng.integers(0, 2, size=int(rng.integers(0, 900)), dtype=np.uint8)
            feed(f"P{fb}", AF.to_soft(np.concatenate([pre, bits]), sigma=float(rng.uniform(0, 45)), seed=c), out[f"P{fb}"])
    rng = np.random.default_rng(66)  # test_unique_words_planted_in_the_detector_window
    uw = ABC.UWB
    for c in range(66):
        bits, _ = AF.p_channel_bits(AF.random_payloads(6, 10500, seed=3000 + c), 10500, invert_i=bool(c & 1), invert_q=bool(c & 2))
        bits = bits.copy()
        pre = rng.integers(0, 2, size=int(rng.integers(0, 700)), dtype=np.uint8)
        for f in range(1, 5):
            body_end = 5250 * (f + 1)
            win0 = body_end - 261
            kind = (c + f) % 6
            if kind == 0:
                continue
            start = {1: win0 + 70, 2: win0 + 71, 3: win0 + 10, 4: win0 + 40, 5: win0 + 150}[kind] + int(rng.integers(0, 8)) * 2
            word = uw if (c + f) & 1 else 1 - uw
            if len(bits[start:start + 64:2]) == 32 and start + 64 < body_end - 2:
                bits[start:start + 64:2] = word
                if kind in (2, 5):
                    bits[start + 1:start + 65:2] = word if kind == 2 else 1 - word
        feed("P10500", AF.to_soft(np.concatenate([pre, bits]), sigma=float(rng.uniform(0, 20)), seed=c), out["P10500"])
    rng = np.random.default_rng(5)  # test_start_of_burst_markers
    for c in range(12):
        bits, _ = AF.p_channel_bits(AF.random_payloads(5, 10500, seed=300 + c), 10500, invert_i=bool(c & 1), invert_q=bool(c & 2))
        x = AF.to_soft(bits, sigma=20.0, seed=c)
        if c % 3 == 0:
            x = np.insert(x, np.sort(rng.integers(0, len(x), size=4)), -1)
        feed("P10500", x, out["P10500"])
    rng, W = np.random.default_rng(11), 5250  # test_carrier_loss_noise_and_reacquisition: two ticks behind every write from the fourth on
    for c in range(9):
        if c % 3 == 2:
            x = noise(rng, 11 * W)
            if c == 5:
                x[20011:20011 + 64] = np.where(np.repeat(uw, 2) > 0, 200, 55)
        else:
            a, _ = AF.p_channel_bits(AF.random_payloads(3, 10500, seed=500 + c), 10500, invert_i=bool(c & 1), invert_q=bool(c & 2))
            b, _ = AF.p_channel_bits(AF.random_payloads(3, 10500, seed=600 + c), 10500, first_counter=7)
            x = np.concatenate([noise(rng, int(rng.integers(0, 700))), AF.to_soft(a, sigma=25.0, seed=c), noise(rng, 4 * W + int(rng.integers(0, 999))),
                                AF.to_soft(b, sigma=25.0, seed=c + 50)])
        ends = [min(len(x), s + W) for s in range(0, len(x), W)]
        feed("P10500", x, out["P10500"], ticks={e: 2 for k, e in enumerate(ends) if k >= 3})
    g = golden("aerol_1200")  # test_tick_dcd: six ticks behind the golden stream
    feed("P1200", g["soft"], out["P1200"], ticks={len(g["soft"]): 6})
    # ---- test_gpu_aerol_burst.py
    for name in ("10500_a", "10500_b", "1200_a", "600_a"):
        feed("RT" + name.split("_")[0], golden(f"aerol_burst_{name}")["soft"], out["RT" + name.split("_")[0]])
    rng = np.random.default_rng(3)  # test_bank_vs_oracle
    for c in range(70):
        x = noise(rng, 30000, 40) if c % 7 == 6 else mk.rt_case(100 + c, float(rng.uniform(8, 45)), (bool(c & 1), bool(c & 2)), cut=(c % 3 == 0))[1]
        feed("RT10500", x, out["RT10500"])
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_aerolb_emul import short_gap_streams  # test_bank_short_gaps
    for x in short_gap_streams(16):
        feed("RT10500", x, out["RT10500"])
    for fb in (1200, 600):  # test_msk_bank_vs_oracle
        rng = np.random.default_rng(fb)
        for c in range(66):
            x = noise(rng, 20000, 40) if c % 11 == 10 else mk.rt_case_msk(200 + c, float(rng.uniform(8, 40)), invert=bool(c & 1), cut=(c % 3 == 0))[1]
            feed(f"RT{fb}", x, out[f"RT{fb}"])
    # ---- test_gpu_aerol_c.py
    feed("C8400", golden("aerol_c_8400_a")["soft"], out["C8400"])
    for nch in (5, 70):  # test_bank_vs_oracle
        rng = np.random.default_rng(nch)
        for c in range(nch):
            _, x = AF.c_channel_case(5000 + c, 4 + c % 3, 10.0 + 5.0 * (c % 7), inv=(bool(c & 1), bool(c & 2)), lead=int(rng.integers(0, 4200)))
            feed("C8400", x, out["C8400"])
    feed("C8400", AF.c_channel_case(6001, 4, 30.0, inv=(False, False), lead=100)[1], out["C8400"])  # test_overflow_is_reported
    return out


def main():
    O.build()
    sv = survey()
    cases = {}
    for c in ABC.all_cases():
        cov = ABC.run_oracle(O, c)["coverage"]
        cases[c.name] = {n: cov[n] for n in ABC.chain_counters(O, c.family) if cov[n]}
    path = os.path.join(ROOT, "profiles", "aerol_branches.json")
    with open(path, "w") as f:  # one family / case per line
        f.write('{\n "survey": {\n' + ",\n".join(f'  "{k}": {json.dumps(v)}' for k, v in sv.items()) + '\n },\n "cases": {\n')
        f.write(",\n".join(f'  "{k}": {json.dumps(v)}' for k, v in cases.items()) + "\n }\n}\n")
    for fam in ABC.FAMILIES:
        zero = [n for n in ABC.chain_counters(O, fam) if not sv[fam][n]]
        print(fam, "not reached by the existing tests' streams:", zero)


if __name__ == "__main__":
    main()
