"""Timing of the Aero-L bank's one-call reads and dcd link: a 10.5 kbps bank fed one frame per step as bench.py's aerol workload feeds it
(64 distinct streams at their own frame phases, the step's input resident in HBM), linked to a demodulator bank of the same size, and after
every step read_sus_all + read_events_all.  Prints one JSON line: host wall clock of the two reads per step, the HIP-event time of the sweep's
kernels (slot 3) and of the link kernel (slot 4) per step, the bank's own three kernel classes from the same steps, and -- timed over one
or two more steps, it is slow -- the per-channel loop (jaero_aerol_read_sus + jaero_aerol_read_events for every channel) with the ratio.
usage: python scripts/ubench/time_aerol_read.py [channels] [steps] [warmup] [--loops N] [--out profiles/aerol_read_timing.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jaero_amd import aerol_frames as AF  # noqa: E402
from jaero_amd import capi  # noqa: E402
from jaero_amd.demodulator import AeroLBank, DemodulatorBank, OqpskSettings  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("channels", nargs="?", type=int, default=65536)
ap.add_argument("steps", nargs="?", type=int, default=20)
ap.add_argument("warmup", nargs="?", type=int, default=5)
ap.add_argument("--loops", type=int, default=1, help="steps read channel by channel at the end (each takes seconds at 65 536 channels)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
nch, K, W, NL = args.channels, args.steps, args.warmup, args.loops
fb, flen, nuniq = 10500, 5250, 64
dev = torch.device("cuda", 0)
nsteps = K + W + NL
prng = np.random.default_rng(77)
streams = []
for u in range(nuniq):
    bits, _ = AF.p_channel_bits(AF.random_payloads(nsteps + 1, fb, seed=900 + u), fb, invert_i=bool(u & 1), invert_q=bool(u & 2))
    pre = prng.integers(0, 2, size=int(prng.integers(0, flen)), dtype=np.uint8)
    streams.append(AF.to_soft(np.concatenate([pre, bits])[: nsteps * flen], sigma=25.0, seed=u))
soft = torch.from_numpy(np.stack(streams)).to(dev)
idx = torch.arange(nch, device=dev) % nuniq
counts = torch.full((nch,), flen, dtype=torch.int32, device=dev)
pitch = (flen + 7) // 8 * 8
frame = torch.zeros((nch, pitch), dtype=torch.int16, device=dev)
bank = AeroLBank(nch, fb, max_softbits_per_write=flen + 8, su_capacity=26 * 3)
demod = DemodulatorBank(OqpskSettings(), nch, ebno=False, max_write_samples=64, softbit_capacity=64)
bank.link_dcd(demod)
stream = torch.cuda.current_stream().cuda_stream


def step(i):
    frame[:, :flen].copy_(soft[idx, i * flen:(i + 1) * flen])
    bank.write_device(frame.data_ptr(), counts.data_ptr(), pitch, flen, stream)


rows = 0
for i in range(W):
    step(i)
    bank.read_sus_all(); bank.read_events_all()
torch.cuda.synchronize()
bank.profile_enable(True)
wall = []
for i in range(W, W + K):
    step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, sus, _ = bank.read_sus_all()
    _, ev, _ = bank.read_events_all()
    wall.append(time.perf_counter() - t0)
    rows += len(sus) + len(ev)
prof = {name: bank.profile2_read(k) for k, name in enumerate(("bits", "viterbi", "post", "sweep", "link"))}
bank.profile_enable(False)
L = bank.L
loop = []
sbuf, ebuf, n = np.empty((26 * 3, 16), np.int32), np.empty((256, 3), np.int64), C.c_int(0)
for i in range(W + K, W + K + NL):
    step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = 0
    for c in range(nch):
        assert L.jaero_aerol_read_sus(bank.h, c, sbuf.ctypes.data, len(sbuf), C.byref(n)) == capi.E_OK
        got += n.value
        assert L.jaero_aerol_read_events(bank.h, c, ebuf.ctypes.data, len(ebuf), C.byref(n)) == capi.E_OK
        got += n.value
    loop.append(time.perf_counter() - t0)
line = {
    "what": "aerol_read_timing", "channels": nch, "steps": K, "warmup": W, "fb": fb, "rows_per_step": round(rows / K, 1),
    "read_all_wall_ms_per_step": round(1e3 * float(np.mean(wall)), 4), "read_all_wall_ms_min": round(1e3 * float(np.min(wall)), 4),
    "read_all_wall_ms_max": round(1e3 * float(np.max(wall)), 4),
    "sweep_kernels_ms_per_step": round(prof["sweep"][0] / K, 5), "sweep_timed_regions": prof["sweep"][1],
    "link_kernel_ms_per_step": round(prof["link"][0] / K, 5), "link_launches": prof["link"][1],
    "bank_kernels_ms_per_step": {k: round(prof[k][0] / K, 4) for k in ("bits", "viterbi", "post")},
    "per_channel_loop_s": [round(x, 3) for x in loop], "per_channel_loop_rows": got,
    "ratio_loop_over_read_all": round(float(np.mean(loop)) / float(np.mean(wall)), 1) if loop else None,
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(line))
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
bank.close()
demod.close()
