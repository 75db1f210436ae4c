"""Timing of the splitter against the stand-alone handles it replaces: one write of 16 hops per step into (a) one Splitter and (b) one
Channeliser per output, fed the same input from a device tensor.  Prints one JSON line: HIP-event time per step of every kernel class on both
sides (front end: k_chan_fwd, or k_capture_stage + k_capture_fwd with --capture; per output: k_chan_synth), their totals, and the wall time
per step of each side (the input copy included), alternated `--rounds` times in one process.  Default shape: the four outputs of
tests/test_gpu_chan_split.py's twin test at fs_c = 3 072 000 (48 kHz x 9, 24 kHz x 5, 12 kHz x 33, 48 kHz x 1 with other taps);
--capture cu8:2400000: the two outputs of its capture test (48 kHz x 3, 12 kHz x 7).  --scale N multiplies every channel count.
usage: python scripts/ubench/time_chan_split.py [steps] [warmup] [--capture FMT:FS_IN] [--scale N] [--rounds R]"""
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
from jaero_amd.channeliser import HP, Capture, Channeliser, Splitter, design_taps, resample_ratio  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("steps", nargs="?", type=int, default=50)
ap.add_argument("warmup", nargs="?", type=int, default=5)
ap.add_argument("--capture", default=None, metavar="FMT:FS_IN")
ap.add_argument("--scale", type=int, default=1)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
K, W, hops, fs_c = args.steps, args.warmup, 16, 3072000
rng = np.random.default_rng(1)
shape = [(48000.0, 3, None), (12000.0, 7, None)] if args.capture else [(48000.0, 9, None), (24000.0, 5, None), (12000.0, 33, None), (48000.0, 1, 20000.0)]
outs = []
for fs_out, nch, cutoff in shape:
    chans = [(int(t), 715827883, 1.0) for t in rng.integers(0, 1 << 32, size=nch * args.scale, dtype=np.uint64)]
    outs.append((fs_out, chans, design_taps(int(fs_c // fs_out), cutoff_hz=cutoff, ntaps=2049, beta=10.0, fs_out=fs_out)))
capture = None
if args.capture:
    fmt, fs_in = args.capture.split(":")
    capture = Capture(fs_in=int(fs_in), fmt=fmt)
    L, Mr = resample_ratio(int(fs_in), fs_c)
    nin = hops * HP * Mr // L
    assert -(-nin * L // Mr) == hops * HP, "choose a rate whose 16 hops are a whole number of capture samples"
    lo, hi, dt = {"cs16": (-8000, 8000, np.int16), "cu8": (64, 192, np.uint8), "cs8": (-64, 64, np.int8)}[fmt]
    raw = rng.integers(lo, hi, size=(nin, 2), dtype=dt)
else:
    nin = hops * HP
    raw = rng.integers(-8000, 8000, size=(nin, 2), dtype=np.int16)
iq = torch.from_numpy(raw).cuda()
sp = Splitter(fs_c, outs, capture=capture, max_write_iq=nin)
alone = [Channeliser(int(fs_c // fs_out), chans, taps=taps, max_write_iq=nin, fs_out=fs_out, capture=capture) for fs_out, chans, taps in outs]
st = torch.cuda.current_stream().cuda_stream
want = [hops * o.Mo for o in sp.outputs]


def step_split():
    assert sp.write(iq, stream=st) == want


def step_alone():
    for c, n in zip(alone, want):
        assert c.write(iq, stream=st) == n


for _ in range(W):
    step_split()
    step_alone()
torch.cuda.synchronize()
sp.profile_enable(True)
for c in alone:
    c.profile_enable(True)
state = GpuStateSampler().start("timed")
wall = {"split": [], "alone": []}
for _ in range(args.rounds):
    for name, step in (("split", step_split), ("alone", step_alone)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            step()
        torch.cuda.synchronize()
        wall[name].append(1e3 * (time.perf_counter() - t0) / K)
state.stop()
n = K * args.rounds
per = lambda ms: round(ms / n, 4)
split = {"fwd": per(sp.profile_read(0)[0]), "stage": per(sp.profile_read(1)[0]), "synth": [per(o.profile_read(1)[0]) for o in sp.outputs],
         "fwd_launches": sp.profile_read(0)[1], "stage_launches": sp.profile_read(1)[1]}
if capture is None:
    al = {"fwd": [per(c.profile_read(0)[0]) for c in alone], "stage": [0.0] * len(alone)}
else:
    al = {"fwd": [per(c.capture_profile_read(1)[0]) for c in alone], "stage": [per(c.capture_profile_read(0)[0]) for c in alone]}
al["synth"] = [per(c.profile_read(1)[0]) for c in alone]
split["total"] = round(split["fwd"] + split["stage"] + sum(split["synth"]), 4)
al["total"] = round(sum(al["fwd"]) + sum(al["stage"]) + sum(al["synth"]), 4)
print(json.dumps({
    "fs_c": fs_c, "capture": args.capture, "outputs": [[o[0], len(o[1])] for o in outs], "input_pairs_per_step": nin, "hops_per_step": hops,
    "steps": K, "warmup": W, "rounds": args.rounds, "kernel_ms_per_step": {"splitter": split, "stand_alone": al},
    "kernel_total_ratio": round(split["total"] / al["total"], 4),
    "wall_ms_per_step": {k: [round(v, 4) for v in vs] for k, vs in wall.items()},
    "wall_ratio_of_means": round(float(np.mean(wall["split"]) / np.mean(wall["alone"])), 4), "gpu_state": state.summary()}))
