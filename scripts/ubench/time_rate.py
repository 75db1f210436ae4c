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
usage: python scripts/ubench/time_rate.py [channels] [steps] [warmup] [--gated] [--out FILE]"""
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
from jaero_amd.ratemeter import L, RateMeter  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("channels", nargs="?", type=int, default=65536)
ap.add_argument("steps", nargs="?", type=int, default=50)
ap.add_argument("warmup", nargs="?", type=int, default=5)
ap.add_argument("--gated", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
nch, K, W = args.channels, args.steps, args.warmup
out = args.out or os.path.join(ROOT, "profiles", "rate_gate_timing.json" if args.gated else "rate_timing.json")
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


shape = {"channels": nch, "steps": K, "warmup": W, "samples_per_channel_per_step": L}
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
    on, off = 0.1 * 32768.0, 0.02 * 32768.0
    phase = torch.arange(nch, device="cuda") % 16
    bank = []
    for p in range(16):
        amp = torch.where(phase == p, on, off).to(torch.float32)[:, None]
        bank.append((torch.randn((nch, L), device="cuda", generator=g) * amp).round().clamp(-32768, 32767).to(torch.int16))
    gate = int(L * (on * on + off * off) / 2.0)  # the midpoint of the two levels' expected segment energies
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
