"""Timing of the Aero-L bank's ISU reassembly (jaero_aerol_isu_enable): two 10.5 kbps banks fed the same frame per step as time_aerol_read.py
feeds it (64 distinct streams at their own frame phases, the step's input resident in HBM), one with the reassembly off -- the kernels a bank
launched before the feature existed -- and one with it on.  Payload: per channel one ACARS block of 220 characters (an ISU and 30 SSUs)
every second frame, fill-in units otherwise.  Prints one JSON line: the HIP-event time per step of the bank's three kernel classes with the
feature off and on and of the reassembly kernel (slot 5), and on the same steps the host wall clock and the bytes of read_msgs_all against
read_sus_all.  The host reassembly a caller of read_sus_all would still have to run on those rows is NOT timed.
usage: python scripts/ubench/time_aerol_msgs.py [channels] [steps] [warmup] [--out profiles/aerol_isu_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jaero_amd import acars  # noqa: E402
from jaero_amd import aerol_frames as AF  # noqa: E402
from jaero_amd.demodulator import AeroLBank  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("channels", nargs="?", type=int, default=65536)
ap.add_argument("steps", nargs="?", type=int, default=20)
ap.add_argument("warmup", nargs="?", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
nch, K, W = args.channels, args.steps, args.warmup
fb, flen, nuniq, per_frame = 10500, 5250, 64, 26
FILL = bytes([0x01] + [0] * 9)
dev = torch.device("cuda", 0)
nsteps = K + W
prng = np.random.default_rng(78)
streams = []
for u in range(nuniq):
    frames = []
    for pair in range((nsteps + 3) // 2):
        text = "".join(chr(32 + int(v)) for v in prng.integers(0, 95, 220))
        block = acars.acars_userdata(".A6-E%02d" % (u % 100), "2", "\x15", "H1", "ABCDEFGHIJ"[pair % 10], text)
        units = acars.isu_payloads(0x890000 + u, 0x90, u % 16, pair % 16, block)
        units += [FILL] * (2 * per_frame - len(units))
        frames += [units[:per_frame], units[per_frame:]]
    bits, _ = AF.p_channel_bits(frames, fb, invert_i=bool(u & 1), invert_q=bool(u & 2))
    pre = prng.integers(0, 2, size=int(prng.integers(0, flen)), dtype=np.uint8)
    streams.append(AF.to_soft(np.concatenate([pre, bits])[: nsteps * flen], sigma=25.0, seed=u))
soft = torch.from_numpy(np.stack(streams)).to(dev)
idx = torch.arange(nch, device=dev) % nuniq
counts = torch.full((nch,), flen, dtype=torch.int32, device=dev)
pitch = (flen + 7) // 8 * 8
frame = torch.zeros((nch, pitch), dtype=torch.int16, device=dev)
off = AeroLBank(nch, fb, max_softbits_per_write=flen + 8, su_capacity=26 * 3)
on = AeroLBank(nch, fb, max_softbits_per_write=flen + 8, su_capacity=26 * 3)
on.isu_enable(4)
stream = torch.cuda.current_stream().cuda_stream


def step(i):
    frame[:, :flen].copy_(soft[idx, i * flen:(i + 1) * flen])
    off.write_device(frame.data_ptr(), counts.data_ptr(), pitch, flen, stream)
    on.write_device(frame.data_ptr(), counts.data_ptr(), pitch, flen, stream)


for i in range(W):
    step(i)
    off.read_sus_all(); on.read_sus_all(); on.read_msgs_all()
torch.cuda.synchronize()
off.profile_enable(True); on.profile_enable(True)
wall_m, wall_s, nmsg, nsus = [], [], 0, 0
for i in range(W, W + K):
    step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, msgs, ovm = on.read_msgs_all()
    t1 = time.perf_counter()
    _, sus, _ = on.read_sus_all()
    t2 = time.perf_counter()
    off.read_sus_all()
    assert not ovm.any()
    wall_m.append(t1 - t0); wall_s.append(t2 - t1)
    nmsg += len(msgs); nsus += len(sus)
names = ("bits", "viterbi", "post", "sweep", "link", "isu")
p_off = {name: off.profile2_read(k) for k, name in enumerate(names)}
p_on = {name: on.profile2_read(k) for k, name in enumerate(names)}
stats = on.isu_stats().sum(axis=0)
ms = lambda x: round(1e3 * float(x), 4)
line = {
    "what": "aerol_isu_timing", "channels": nch, "steps": K, "warmup": W, "fb": fb,
    "payload": "per channel one 220-character ACARS block (ISU + 30 SSUs) every second frame, fill-in units otherwise",
    "kernels_ms_per_step_off": {k: round(p_off[k][0] / K, 4) for k in ("bits", "viterbi", "post")},
    "kernels_ms_per_step_on": {k: round(p_on[k][0] / K, 4) for k in ("bits", "viterbi", "post", "isu")},
    "isu_launches": p_on["isu"][1], "isu_launches_off": p_off["isu"][1],
    "messages_per_step": round(nmsg / K, 1), "su_rows_per_step": round(nsus / K, 1),
    "read_msgs_all_wall_ms_per_step": ms(np.mean(wall_m)), "read_msgs_all_wall_ms_min": ms(np.min(wall_m)), "read_msgs_all_wall_ms_max": ms(np.max(wall_m)),
    "read_sus_all_wall_ms_per_step": ms(np.mean(wall_s)), "read_sus_all_wall_ms_min": ms(np.min(wall_s)), "read_sus_all_wall_ms_max": ms(np.max(wall_s)),
    "read_msgs_all_bytes_per_step": round(544 * nmsg / K), "read_sus_all_bytes_per_step": round(64 * nsus / K),
    "not_timed": "the host reassembly (ISUData::update, ParserISU::parse) a caller of read_sus_all would run on those rows",
    "isu_stats_total": {"isu": int(stats[0]), "ssu": int(stats[1]), "missing": int(stats[2]), "completed": int(stats[3])},
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(line))
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
off.close()
on.close()
