"""Timing of the demodulator bank's one-call reads against the readers they stand beside, on the same bank in the same run: after every
4096-sample write (PCM resident in HBM) of
  - a continuous 10.5 kbps bank: read_all(SOFTBITS); the dense jaero_read_softbits_all at the smallest cap_per_channel that fits; 1024
    per-channel jaero_read_softbits calls, scaled to the bank;
  - a burst OQPSK bank with a burst on one channel in sixteen, the others noise: read_all(SOFTBITS) and 1024 per-channel calls, scaled (there
    is no dense form for a burst bank);
  - read_status_all against 1024 jaero_read_status calls, scaled (the continuous bank);
and the HIP-event time of the calls' own kernels (jaero_profile2_read(5)) beside the host wall clock, whose rest is copies and synchronisation.
Prints one JSON line.
usage: python scripts/ubench/time_read_all.py [channels] [steps] [--out profiles/read_all_timing.json]"""
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
from bench_state import GpuStateSampler  # noqa: E402
from jaero_amd import capi  # noqa: E402
from jaero_amd import signalgen as G  # noqa: E402
from jaero_amd.demodulator import BurstOqpskSettings, DemodulatorBank, OqpskSettings  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("channels", nargs="?", type=int, default=65536)
ap.add_argument("steps", nargs="?", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
nch, K, CH, NP = args.channels, args.steps, 4096, min(1024, args.channels)
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
idx = torch.arange(nch, device=dev)


def ms(xs):
    return round(1e3 * float(np.mean(xs)), 4)


def run(bank, table, first, dense):
    """Writes table[:, k CH : (k + 1) CH] for k = 0 ..; steps `first` .. are measured.  Returns the figures of one bank."""
    src = torch.from_numpy(table).to(dev)
    sel = idx % len(table)

    def write(k):
        bank.write(src[sel, k * CH:(k + 1) * CH].contiguous(), stream=stream)
        torch.cuda.synchronize()

    for k in range(first):
        write(k)
        bank.read_all(capi.BANK_SOFTBITS, overflowed=True)
    bank.profile_enable(True)
    k, wall, rows, held = first, [], [], []
    for _ in range(K):
        write(k); k += 1
        cnt, pend = bank.softbit_counts()
        held.append(int((cnt > pend).sum()))
        t0 = time.perf_counter()
        flat, off, taken = bank.read_all(capi.BANK_SOFTBITS)
        wall.append(time.perf_counter() - t0)
        assert taken == nch
        rows.append(len(flat))
    kern_ms, regions = bank.profile2_read(5, reset=True)
    out = {"rows_per_step": round(float(np.mean(rows)), 1), "channels_with_rows_per_step": round(float(np.mean(held)), 1),
           "read_all_wall_ms": ms(wall), "read_all_wall_ms_min": round(1e3 * min(wall), 4), "read_all_wall_ms_max": round(1e3 * max(wall), 4),
           "read_all_kernels_ms": round(kern_ms / K, 4), "read_all_timed_regions": regions}
    out["read_all_copies_and_sync_ms"] = round(out["read_all_wall_ms"] - out["read_all_kernels_ms"], 4)
    if dense:
        dw = []
        for _ in range(K):
            write(k); k += 1
            cap = int(bank.softbit_counts()[0].max())
            t0 = time.perf_counter()
            _, counts = bank.read_softbits_all(cap)
            dw.append(time.perf_counter() - t0)
        out.update({"dense_cap_per_channel": cap, "dense_wall_ms": ms(dw), "dense_rows": int(counts.sum()),
                    "dense_over_read_all": round(ms(dw) / out["read_all_wall_ms"], 3)})
    write(k); k += 1
    buf, n = np.empty(1 << 16, np.int16), C.c_int(0)
    t0 = time.perf_counter()
    for c in range(NP):
        assert bank.L.jaero_read_softbits(bank.h, c, buf.ctypes.data, len(buf), C.byref(n)) == capi.E_OK
    per = time.perf_counter() - t0
    out.update({"per_channel_calls": NP, "per_channel_wall_ms": round(1e3 * per, 3), "per_channel_scaled_to_bank_ms": round(1e3 * per * nch / NP, 1),
                "per_channel_scaled_over_read_all": round(1e3 * per * nch / NP / out["read_all_wall_ms"], 1)})
    return out


state = GpuStateSampler().start("timed")
nsamp = (4 + 2 * K + 2) * CH
cont_table = np.stack([G.oqpsk(nsamp, fc=8000.0 + 3.0 * u, seed=G.SEED_BASE + 2000 + u)[0] for u in range(16)])
cont = DemodulatorBank(OqpskSettings(), nch, max_write_samples=CH)
line = {"what": "read_all_timing", "channels": nch, "steps": K, "samples_per_write": CH, "continuous_10k5": run(cont, cont_table, 4, True)}
# read_status_all on the same bank
sw = []
for _ in range(K):
    t0 = time.perf_counter()
    st = cont.read_status_all()
    sw.append(time.perf_counter() - t0)
skern, sreg = cont.profile2_read(5, reset=True)
one = capi.Status()
t0 = time.perf_counter()
for c in range(NP):
    assert cont.L.jaero_read_status(cont.h, c, C.byref(one)) == capi.E_OK
sper = time.perf_counter() - t0
line["status"] = {"read_status_all_wall_ms": ms(sw), "read_status_all_kernel_ms": round(skern / K, 4), "per_channel_calls": NP,
                  "per_channel_wall_ms": round(1e3 * sper, 3), "per_channel_scaled_to_bank_ms": round(1e3 * sper * nch / NP, 1),
                  "per_channel_scaled_over_read_status_all": round(1e3 * sper * nch / NP / ms(sw), 1)}
cont.close()
# burst bank: one channel in sixteen carries a long burst whose data is in flight during the measured writes, the others noise
first = 14  # the demodulator hands over a burst's first bits about 12 000 samples after its start (40 000)
nb = (first + K + 1) * CH
ndata = int((nb - 40000) / (48000 / 5250)) - 256 - 64
rows = []
for u in range(32):
    if u % 16 == 0:
        rows.append(G.burst_oqpsk(nb, burst_starts=[40000 + 300 * (u // 16)], ndata_sym=ndata, ebno_db=16.0, seed=G.SEED_BASE + 2100 + u)[0])
    else:
        rows.append(G.burst_oqpsk(nb, burst_starts=[], ebno_db=16.0, seed=G.SEED_BASE + 2100 + u)[0])
burst = DemodulatorBank(BurstOqpskSettings(), nch, max_write_samples=CH)
line["burst_oqpsk_one_in_16"] = run(burst, np.stack(rows), first, False)
burst.close()
state.stop()
line["device"] = torch.cuda.get_device_name(0)
line["gpu_state"] = state.summary()
print(json.dumps(line))
if args.out:
    with open(os.path.join(ROOT, args.out), "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
