"""Timing of the rate meter's line kernel: RateMeter.write_device of 4096 samples per channel (one segment, one launch of k_rate_lines) per
step, from a device tensor of uniform int16 noise.  Prints one JSON line and writes it to --out: HIP-event time per write of k_rate_lines,
the same per transform, the wall time per step, the engine clock over the timed steps, and beside them the figures on record for the same
step of 4096 samples per channel on 65 536 channels (k_chan_synth 1.40 ms, the OQPSK bank's kernels 23.07 ms).  A recording:
there is no pass mark.
usage: python scripts/ubench/time_rate.py [channels] [steps] [warmup] [--out profiles/rate_timing.json]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bench_state import GpuStateSampler  # noqa: E402
from jaero_amd.ratemeter import L, RateMeter  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("channels", nargs="?", type=int, default=65536)
ap.add_argument("steps", nargs="?", type=int, default=50)
ap.add_argument("warmup", nargs="?", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_timing.json"))
args = ap.parse_args()
nch, K, W = args.channels, args.steps, args.warmup
g = torch.Generator(device="cuda")
g.manual_seed(1)
pcm = torch.randint(-8000, 8000, (nch, L), device="cuda", dtype=torch.int32, generator=g).to(torch.int16)
m = RateMeter(nch, 48000.0, max_write_samples=L)
st = torch.cuda.current_stream().cuda_stream
for _ in range(W):
    m.write_device(pcm.data_ptr(), L, stream=st)
torch.cuda.synchronize()
m.profile_enable(True)
state = GpuStateSampler().start("timed")
t0 = time.perf_counter()
for _ in range(K):
    assert m.write_device(pcm.data_ptr(), L, stream=st) == 1
torch.cuda.synchronize()
dt = time.perf_counter() - t0
state.stop()
ms, launches = m.profile_read()
R, nseg = m.read()
assert nseg == W + K and launches == K and (R > 0.0).any(axis=1).all()
line = {
    "channels": nch, "steps": K, "warmup": W, "samples_per_channel_per_step": L,
    "k_rate_lines_ms_per_step": round(ms / K, 4), "k_rate_lines_launches": launches,
    "k_rate_lines_ns_per_transform": round(1e6 * ms / K / nch, 3),
    "wall_ms_per_step": round(1e3 * dt / K, 3),
    "on_record_same_step": {"k_chan_synth_ms": 1.40, "oqpsk_bank_kernels_ms": 23.07},
    "k_rate_lines_over_bank": round(ms / K / 23.07, 4),
    "gpu_state": state.summary()}
print(json.dumps(line))
with open(args.out, "w") as f:
    json.dump(line, f, indent=1)
    f.write("\n")
