"""Timing of the channeliser in front of a demodulator bank: Channeliser.feed of 16 hops (131 072 I/Q pairs; at D = 32 -> 4096 samples per
channel) per step.  Prints one JSON line: HIP-event time per step of k_chan_fwd and k_chan_synth, of the bank's sample loop and coarse estimate
from the same steps, their ratio (the yardstick: the two channeliser kernels together against the demodulator bank's own step time), the
same per second of signal and per output sample, the engine clock over the timed steps.  Defaults: the headline OQPSK bank behind D = 32.
--survey: the survey (spectrum and levels) is on during the same steps; k_chan_psd and k_chan_level per step are printed beside the rest.
--activity: the activity (peak-hold spectrum and block statistics) is on during the same steps.  Alone it launches the peak-only k_chan_psd and
the statistics-only k_chan_level; with --survey every launch is the fused one (spectrum + peak, levels + statistics), timed once, under
the activity's slots, so the survey's own slots then read zero.
--capture FMT:FS_IN: the channeliser takes a capture of that format (cs16, cu8, cs8, cf32) at that rate through its capture front end; a step
is then the capture samples that stage 16 hops, and k_capture_stage and k_capture_fwd are timed beside k_chan_synth (k_chan_fwd does not run).
usage: python scripts/ubench/time_chan.py [channels] [steps] [warmup] [--decim D] [--fs-out 48000|24000|12000] [--bank oqpsk|msk600|msk1200] [--survey]
       [--activity] [--capture FMT:FS_IN]"""
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
from jaero_amd.channeliser import HP, Capture, Channeliser, resample_ratio  # noqa: E402
from jaero_amd.demodulator import DemodulatorBank, MskSettings, OqpskSettings  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("channels", nargs="?", type=int, default=65536)
ap.add_argument("steps", nargs="?", type=int, default=50)
ap.add_argument("warmup", nargs="?", type=int, default=5)
ap.add_argument("--decim", type=int, default=32, help="total decimation, capture to output")
ap.add_argument("--fs-out", type=float, default=48000.0, help="the channeliser's output rate = the bank's Fs")
ap.add_argument("--bank", choices=("oqpsk", "msk600", "msk1200"), default="oqpsk")
ap.add_argument("--survey", action="store_true", help="survey the capture (spectrum and levels) in every step and time its two kernels")
ap.add_argument("--activity", action="store_true", help="keep the peak-hold spectrum and the block statistics in every step and time their launches")
ap.add_argument("--capture", default=None, metavar="FMT:FS_IN", help="feed a capture of this format and rate through the capture front end")
args = ap.parse_args()
nch, K, W, decim, fs_out, hops = args.channels, args.steps, args.warmup, args.decim, args.fs_out, 16
rng = np.random.default_rng(1)
chans = [(int(t), 715827883, 1.0) for t in rng.integers(0, 1 << 32, size=nch, dtype=np.uint64)]
capture = None
if args.capture:
    fmt, fs_in = args.capture.split(":")
    capture = Capture(fs_in=int(fs_in), fmt=fmt)
    L, Mr = resample_ratio(int(fs_in), int(fs_out * decim))
    nin = hops * HP * Mr // L  # the largest count of capture samples that stages no more than 16 hops; exactly 16 when L divides it
    assert -(-nin * L // Mr) == hops * HP, "choose a rate whose 16 hops are a whole number of capture samples"
    if fmt == "cf32":
        raw = (0.25 * rng.normal(size=(nin, 2))).astype(np.float32)
    else:
        lo, hi, dt = {"cs16": (-8000, 8000, np.int16), "cu8": (64, 192, np.uint8), "cs8": (-64, 64, np.int8)}[fmt]
        raw = rng.integers(lo, hi, size=(nin, 2), dtype=dt)
    iq = torch.from_numpy(raw).cuda()
    chan = Channeliser(decim, chans, max_write_iq=nin, fs_out=fs_out, capture=capture)
else:
    iq = torch.from_numpy(rng.integers(-8000, 8000, size=(hops * HP, 2), dtype=np.int16)).cuda()
    chan = Channeliser(decim, chans, max_write_iq=hops * HP, fs_out=fs_out)
if args.bank == "oqpsk":
    settings = OqpskSettings(Fs=fs_out)
else:
    fb = 600.0 if args.bank == "msk600" else 1200.0
    settings = MskSettings(fb=fb, lockingbw=1.5 * fb, Fs=fs_out)
if args.survey:
    chan.survey_enable(psd=True, levels=True)
if args.activity:
    chan.activity_enable(peak=True, blocks=True)
bank = DemodulatorBank(settings, nch, ebno=True, max_write_samples=(hops + 1) * chan.Mo, softbit_capacity=4096)
st = torch.cuda.current_stream().cuda_stream
for _ in range(W):
    chan.feed(bank, iq, stream=st)
    bank.discard_softbits(st)
torch.cuda.synchronize()
chan.profile_enable(True)
bank.profile_enable(True)
state = GpuStateSampler().start("timed")
t0 = time.perf_counter()
for _ in range(K):
    assert chan.feed(bank, iq, stream=st) == hops * chan.Mo
    bank.discard_softbits(st)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
state.stop()
fwd, nf = chan.profile_read(0)
syn, ns = chan.profile_read(1)
loop, nl = bank.profile_read(0)
coarse, nc = bank.profile_read(1)
survey = {}
if args.survey:
    (psd, npsd), (lvl, nlvl) = chan.survey_profile_read(0), chan.survey_profile_read(1)
    survey = {"k_chan_psd_ms_per_step": round(psd / K, 4), "k_chan_psd_launches": npsd,
              "k_chan_level_ms_per_step": round(lvl / K, 4), "k_chan_level_launches": nlvl,
              "k_chan_level_over_synth": round(lvl / syn, 4), "survey_blocks": int(chan.read_psd()[1])}
if args.activity:
    (pk, npk), (blk, nblk) = chan.activity_profile_read(0), chan.activity_profile_read(1)
    fused = bool(args.survey)
    survey.update({"activity_fused_with_survey": fused,
                   "k_chan_psd_peak_ms_per_step": round(pk / K, 4), "k_chan_psd_peak_launches": npk,
                   "k_chan_level_act_ms_per_step": round(blk / K, 4), "k_chan_level_act_launches": nblk,
                   "k_chan_level_act_over_synth": round(blk / syn, 4), "activity_blocks": int(chan.read_peak_sums()[1])})
cap = {}
if capture is not None:
    (stg, nstg), (cfwd, ncf) = chan.capture_profile_read(0), chan.capture_profile_read(1)
    cap = {"capture": args.capture, "capture_samples_per_step": int(iq.shape[0]),
           "k_capture_stage_ms_per_step": round(stg / K, 4), "k_capture_stage_launches": nstg,
           "k_capture_fwd_ms_per_step": round(cfwd / K, 4), "k_capture_fwd_launches": ncf}
front = fwd  # what stands in front of the synthesis: k_chan_fwd, or on a capture handle (where it never runs) the two capture kernels
if capture is not None:
    front = stg + cfwd
chan_ms, bank_ms = (front + syn) / K, (loop + coarse) / K
signal_s = hops * HP / (fs_out * decim)  # seconds of signal per step
print(json.dumps({
    "channels": nch, "decim": decim, "fs_out": fs_out, "bank": args.bank, "bank_kernels": [bank.profile_kernel(0), bank.profile_kernel(1)],
    "steps": K, "warmup": W, "samples_per_channel_per_step": hops * chan.Mo, "signal_ms_per_step": round(1e3 * signal_s, 4),
    "k_chan_fwd_ms_per_signal_s": round(fwd / K / signal_s, 3), "k_chan_synth_ms_per_signal_s": round(syn / K / signal_s, 3),
    "bank_ms_per_signal_s": round(bank_ms / signal_s, 3),
    "k_chan_synth_ps_per_output_sample": round(1e9 * syn / K / (nch * hops * chan.Mo), 3),
    "k_chan_fwd_ms_per_step": round(fwd / K, 4), "k_chan_fwd_launches": nf,
    "k_chan_synth_ms_per_step": round(syn / K, 4), "k_chan_synth_launches": ns, **survey, **cap,
    "bank_sample_loop_ms_per_step": round(loop / K, 4), "bank_sample_loop_launches": nl,
    "bank_coarse_ms_per_step": round(coarse / K, 4), "bank_coarse_launches": nc,
    "chan_ms_per_step": round(chan_ms, 4), "bank_ms_per_step": round(bank_ms, 4), "chan_over_bank": round(chan_ms / bank_ms, 4),
    "wall_ms_per_step": round(1e3 * dt / K, 3), "gpu_state": state.summary()}))
