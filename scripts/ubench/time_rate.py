"""Timing of the rate meter's line kernels: RateMeter.write_device of 4096 samples per channel (one segment, one launch) per step, from
device tensors.  Prints one JSON line and writes it to --out.  A recording: there is no pass mark.

Default: k_rate_lines on uniform int16 noise -- HIP-event time per write, the same per transform, the wall time per step, the engine clock
over the timed steps, and beside them the figures on record for the same step of 4096 samples per channel on 65 536 channels (DESIGN 18:
k_chan_synth 1.40 ms, the OQPSK bank's kernels 23.07 ms).

--gated (default --out profiles/rate_gate_timing.json): three measurements in one process, each `steps` timed writes after `warmup`:
  ungated    k_rate_lines on the noise above: this build's reference for the other two;
  gate_zero  k_rate_lines_gated on the same noise with every gate 0 (every segment joins): what the decision and the statistics cost;
  burst_bank k_rate_lines_gated on a bank in which channel c is on in the writes w with w mod 16 == c mod 16 (Gaussian noise, rms 0.1 of
             full scale on and 0.02 off), the gates at the midpoint of the two levels' segment energies: a workgroup holds channels 2 b and
             2 b + 1, so in 14 writes of 16 neither joins and it skips the transform.  The share of workgroups that skipped is counted from
             njoin (a workgroup skips a write iff none of its channels joins) and recorded beside the time.

--auto (default --out profiles/rate_auto_timing.json): k_rate_lines_auto, three meters in one process, each beside k_rate_lines_gated of
the same build on the same input (the reference: the two kernels do the same work but for the decision and the histogram):
  level       noise at one level under JAERO_GATE_AUTO: no channel leaves gate 0 (asserted), R bit-identical to the gated kernel's under
              gate 0 (asserted);
  burst_bank  the burst bank above under JAERO_GATE_AUTO, beside k_rate_lines_gated with the gates at the midpoint.  A channel runs under
              gate 0 until its second loud write, so fewer workgroups skip than under gates known in advance; the share is counted
              from where the rule makes each channel join, which start and njoin must confirm (asserted);
  manual_hist JAERO_GATE_MANUAL | JAERO_GATE_HIST with every gate 0 on the level noise: what the histogram costs, R bit-identical again.

--classify (default --out profiles/rate_classify_timing.json): the rate lines read on the device, k_rate_classify, after 8 written
segments of the noise above.  RateMeter.classify_lines `steps` times (default 20) after `warmup` (default 3): the HIP-event time of the
launch and the wall time per call (launch, synchronise, copy out 56 bytes a channel).  Then once, in the same process, the host path it
replaces, its wall time split into read() (16 392 bytes a channel over PCIe) and classify_rates (numpy); the two decisions are asserted
equal.  Beside them what one read of R costs at the rate on record for k_rate_lines (2.5 TB/s), and the two ratios.
usage: python scripts/ubench/time_rate.py [channels] [steps] [warmup] [--gated | --auto | --classify] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bench_state import GpuStateSampler  # noqa: E402
from jaero_amd.ratemeter import BINS, L, RATES, RateMeter, classify_rates, decide_rates, rate_distances  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("channels", nargs="?", type=int, default=65536)
ap.add_argument("steps", nargs="?", type=int, default=None)
ap.add_argument("warmup", nargs="?", type=int, default=None)
ap.add_argument("--gated", action="store_true")
ap.add_argument("--auto", action="store_true")
ap.add_argument("--classify", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
nch = args.channels
K = args.steps if args.steps is not None else (20 if args.classify else 50)
W = args.warmup if args.warmup is not None else (3 if args.classify else 5)
out = args.out or os.path.join(ROOT, "profiles", "rate_classify_timing.json" if args.classify else "rate_auto_timing.json" if args.auto
                               else "rate_gate_timing.json" if args.gated else "rate_timing.json")
g = torch.Generator(device="cuda")
g.manual_seed(1)
pcm = torch.randint(-8000, 8000, (nch, L), device="cuda", dtype=torch.int32, generator=g).to(torch.int16)
st = torch.cuda.current_stream().cuda_stream


def timed(m, src):
    """W warm-up and K timed writes of src(w) (a device tensor [nch, L]); (kernel ms per write, wall ms per write, box state)"""
    for w in range(W):
        m.write_device(src(w).data_ptr(), L, stream=st)
    torch.cuda.synchronize()
    m.profile_enable(True)
    state = GpuStateSampler().start("timed")
    t0 = time.perf_counter()
    for w in range(W, W + K):
        assert m.write_device(src(w).data_ptr(), L, stream=st) == 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    state.stop()
    ms, launches = m.profile_read()
    assert launches == K
    return ms / K, 1e3 * dt / K, state.summary()


def burst_bank():
    """16 tensors, channel c loud in tensor c mod 16; the midpoint of the two levels' expected segment energies"""
    on, off = 0.1 * 32768.0, 0.02 * 32768.0
    phase = torch.arange(nch, device="cuda") % 16
    bank = []
    for p in range(16):
        amp = torch.where(phase == p, on, off).to(torch.float32)[:, None]
        bank.append((torch.randn((nch, L), device="cuda", generator=g) * amp).round().clamp(-32768, 32767).to(torch.int16))
    return bank, int(L * (on * on + off * off) / 2.0)


def auto_legs():
    line = dict(shape)
    # level noise: the gated kernel under gate 0, then the new kernel under AUTO and under MANUAL | HIST
    m = RateMeter(nch, 48000.0, max_write_samples=L)
    m.gate_enable()
    ms_g, wall_g, box = timed(m, lambda w: pcm)
    Rg, _ = m.read()
    m.close()
    line["level_gated_reference"] = {"k_rate_lines_gated_ms_per_step": round(ms_g, 4), "wall_ms_per_step": round(wall_g, 3), "gpu_state": box}
    for name, kw in (("level_auto", {"auto": True}), ("manual_hist", {"hist": True})):
        m = RateMeter(nch, 48000.0, max_write_samples=L)
        m.gate_enable(**kw)
        ms1, wall1, box = timed(m, lambda w: pcm)
        R1, nseg = m.read()
        assert nseg == W + K and np.array_equal(R1, Rg), name + ": R is not the gated kernel's under gate 0"
        del R1
        if "auto" in kw:
            *_, start, gate, _ = m.read_gate_auto()
            assert not gate.any() and (start == np.uint64(2 ** 64 - 1)).all(), "a level channel left gate 0"
        else:
            hist, _ = m.read_gate_hist()
            assert (hist.sum(axis=1) == W + K).all()
        m.close()
        line[name] = {"k_rate_lines_auto_ms_per_step": round(ms1, 4), "wall_ms_per_step": round(wall1, 3),
                      "over_gated": round(ms1 / ms_g, 4), "gpu_state": box}
    del Rg
    # the burst bank: the gated kernel under the midpoint gates, then the new kernel choosing its own
    bank, gate = burst_bank()
    m = RateMeter(nch, 48000.0, max_write_samples=L)
    m.gate_enable()
    m.set_gate([gate] * nch)
    ms_b, wall_b, box = timed(m, lambda w: bank[w % 16])
    m.close()
    line["burst_bank_gated_reference"] = {"k_rate_lines_gated_ms_per_step": round(ms_b, 4), "wall_ms_per_step": round(wall_b, 3),
                                          "workgroups_skipped_share": 0.875, "gate": gate, "gpu_state": box}
    m = RateMeter(nch, 48000.0, max_write_samples=L)
    m.gate_enable(auto=True)
    ms2, wall2, box = timed(m, lambda w: bank[w % 16])
    _, _, njoin, _, _, start, gates, nseg = m.read_gate_auto()
    m.close()
    # by the rule channel c, loud in the writes w with w mod 16 == p = c mod 16, joins every write below p + 16 (gate 0) and restarts there
    p = np.arange(nch) % 16
    w = np.arange(W + K)[:, None]
    joins = (w < p + 16) | (w % 16 == p)                                  # [writes][channels]
    assert nseg == W + K and np.array_equal(start, (p + 16).astype(np.uint64)) and gates.all()
    assert np.array_equal(njoin, ((w >= p + 16) & (w % 16 == p)).sum(axis=0).astype(np.uint64)), "the bank's channels did not restart where the rule says"
    pad = np.concatenate([joins, np.zeros((W + K, nch % 2), dtype=bool)], axis=1)
    ran = pad.reshape(W + K, -1, 2).any(axis=2)[W:]                       # [timed writes][workgroups]
    line["burst_bank_auto"] = {"k_rate_lines_auto_ms_per_step": round(ms2, 4), "wall_ms_per_step": round(wall2, 3),
                               "over_gated": round(ms2 / ms_b, 4), "workgroups_skipped_share": round(1.0 - float(ran.mean()), 4),
                               "gpu_state": box}
    return line


def classify_legs():
    segs = 8
    m = RateMeter(nch, 48000.0, max_write_samples=L)
    for _ in range(segs):
        assert m.write_device(pcm.data_ptr(), L, stream=st) == 1
    d = rate_distances(m.fs)
    for _ in range(W):
        m.classify_lines(d)
    kernel, wall = [], []
    state = GpuStateSampler().start("timed")
    for _ in range(K):
        t0 = time.perf_counter()
        floor, score, where, nseg = m.classify_lines(d)
        wall.append(1e3 * (time.perf_counter() - t0))
        kernel.append(m.kernel_ms)
    state.stop()
    assert nseg == segs
    got = decide_rates(floor, score, where, d, m.fs)
    t0 = time.perf_counter()
    R, _ = m.read()
    t1 = time.perf_counter()
    want = classify_rates(R, m.fs)
    t2 = time.perf_counter()
    m.close()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True) and np.array_equal(got[2], want[2]), \
        "the two paths decide differently"
    k_ms, w_ms = float(np.mean(kernel)), float(np.mean(wall))
    read_ms, host_ms = 1e3 * (t1 - t0), 1e3 * (t2 - t1)
    r_bytes = nch * BINS * 8
    one_read_ms = 1e3 * r_bytes / 2.5e12  # what one read of R costs at the rate on record for k_rate_lines
    return {"channels": nch, "calls": K, "warmup": W, "segments_written": segs, "distances": d, "rates": list(RATES),
            "R_bytes": r_bytes, "result_bytes_per_channel": 8 + 12 * len(d),
            "k_rate_classify_ms_per_call": round(k_ms, 4), "k_rate_classify_ms_min_max": [round(min(kernel), 4), round(max(kernel), 4)],
            "classify_lines_wall_ms_per_call": round(w_ms, 3),
            "one_read_of_R_at_2p5_TBps_ms": round(one_read_ms, 4), "kernel_over_one_read": round(k_ms / one_read_ms, 3),
            "host_path_once": {"read_wall_ms": round(read_ms, 1), "classify_rates_wall_ms": round(host_ms, 1),
                               "wall_ms": round(read_ms + host_ms, 1)},
            "host_wall_over_device_wall": round((read_ms + host_ms) / w_ms, 1), "decisions_equal": True, "gpu_state": state.summary()}


shape = {"channels": nch, "steps": K, "warmup": W, "samples_per_channel_per_step": L}
if args.auto or args.classify:
    line = classify_legs() if args.classify else auto_legs()
    print(json.dumps(line))
    with open(out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
    sys.exit(0)
m = RateMeter(nch, 48000.0, max_write_samples=L)
ms, wall, box = timed(m, lambda w: pcm)
R, nseg = m.read()
assert nseg == W + K and (R > 0.0).any(axis=1).all()
m.close()
if not args.gated:
    line = dict(shape)
    line.update({
        "k_rate_lines_ms_per_step": round(ms, 4), "k_rate_lines_launches": K,
        "k_rate_lines_ns_per_transform": round(1e6 * ms / nch, 3),
        "wall_ms_per_step": round(wall, 3),
        "on_record_same_step": {"k_chan_synth_ms": 1.40, "oqpsk_bank_kernels_ms": 23.07},
        "k_rate_lines_over_bank": round(ms / 23.07, 4),
        "gpu_state": box})
else:
    line = dict(shape)
    line["ungated"] = {"k_rate_lines_ms_per_step": round(ms, 4), "wall_ms_per_step": round(wall, 3), "gpu_state": box}
    # every gate 0: R must come out as the ungated kernel's, bit for bit
    m = RateMeter(nch, 48000.0, max_write_samples=L)
    m.gate_enable()
    ms0, wall0, box = timed(m, lambda w: pcm)
    R0, _ = m.read()
    njoin = m.read_gate()[2]
    assert np.array_equal(R0, R) and (njoin == W + K).all()
    del R0, R
    m.close()
    line["gate_zero"] = {"k_rate_lines_gated_ms_per_step": round(ms0, 4), "wall_ms_per_step": round(wall0, 3),
                         "over_ungated": round(ms0 / ms, 4), "gpu_state": box}
    # the burst bank: 16 tensors, channel c loud in tensor c mod 16
    bank, gate = burst_bank()
    m = RateMeter(nch, 48000.0, max_write_samples=L)
    m.gate_enable()
    m.set_gate([gate] * nch)
    ms1, wall1, box = timed(m, lambda w: bank[w % 16])
    emax, emin, njoin, _, _, nseg = m.read_gate()
    m.close()
    assert nseg == W + K
    want = np.array([sum(1 for w in range(W + K) if w % 16 == c % 16) for c in range(nch)], dtype=np.uint64)
    assert np.array_equal(njoin, want), "the bank's channels did not join where they are on"
    # a workgroup (channels 2 b, 2 b + 1) ran the transform in the writes in which one of them was on: its channels' phases differ, so
    # these are the sum of their joins
    pairs = njoin[:nch // 2 * 2].reshape(-1, 2).sum(axis=1).astype(np.int64)
    ran = int(pairs.sum()) + (int(njoin[-1]) if nch % 2 else 0)
    total = ((nch + 1) // 2) * (W + K)
    line["burst_bank"] = {"k_rate_lines_gated_ms_per_step": round(ms1, 4), "wall_ms_per_step": round(wall1, 3),
                          "over_ungated": round(ms1 / ms, 4), "workgroups_skipped_share": round(1.0 - ran / total, 4),
                          "gate": gate, "emax_max": int(emax.max()), "emin_min": int(emin.min()), "gpu_state": box}
print(json.dumps(line))
with open(out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
