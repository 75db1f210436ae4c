"""Timing of the burst Aero-L bank's R / T reassembly (jaero_aerol_rt_enable): two 10.5 kbps burst banks fed the same bursts per step (64
distinct streams, the step's input resident in HBM), one with the reassembly off -- the kernels a bank launched before the feature existed --
and one with it on.  Payload: per channel one burst per step of STEP soft entries (the start-of-burst marker, 80 entries of noise, the unique
word, the packet, noise to the end of the step); even steps carry a T packet with one 100-character ACARS block (an ISU and 15 SSUs), odd
steps an R packet with a one-unit message, so every step completes one message per channel.  Prints one JSON line: the HIP-event time per
step of the bank's three kernel classes with the feature off and on and of the reassembly kernel (slot 5), and on the same steps the host
wall clock and the bytes of read_msgs_all against read_packets_all.  The host reassembly a caller of read_packets_all would still have to
run on those rows is NOT timed.
usage: python scripts/ubench/time_aerol_rt_msgs.py [channels] [steps] [warmup] [--out profiles/aerol_rt_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jaero_amd import acars  # noqa: E402
from jaero_amd import aerol_frames as AF  # noqa: E402

FB, STEP, NUNIQ, LEAD = 10500, 12000, 64, 80  # a step is longer than the one-second frame countdown (10 500 bits behind the unique word)


def build_streams(nsteps: int, nuniq: int = NUNIQ) -> np.ndarray:
    """int16 [nuniq, nsteps * STEP]: stream u's burst of step i starts at entry i * STEP."""
    prng = np.random.default_rng(79)
    uw = np.repeat(np.array([(AF.UW >> (31 - k)) & 1 for k in range(32)], dtype=np.uint8), 2)
    noise = lambda n: np.clip(np.round(128 + prng.normal(0, 40, n)), 0, 255).astype(np.int16)
    out = np.zeros((nuniq, nsteps * STEP), np.int16)
    for u in range(nuniq):
        aes = 0x890000 + u
        for i in range(nsteps):
            if i % 2 == 0:
                text = "".join(chr(32 + int(v)) for v in prng.integers(0, 95, 100))
                block = acars.acars_userdata(".A6-E%02d" % (u % 100), "2", "\x15", "H1", "ABCDEFGHIJ"[(i // 2) % 10], text)
                units = acars.isu_payloads(aes, 0x90, u % 16, (i // 2) % 16, block)
                kind, payload = "T", acars.t_packets(aes, 0x90, units, len(units))[0]
            else:
                kind, payload = "R", acars.r_isu_payloads(aes, 0x90, u % 16, i % 8, bytes(prng.integers(0, 256, 11, dtype=np.uint8)))[0]
            bits = np.concatenate([uw, AF.rt_packet_bits(kind, payload)])
            if u & 1:
                bits[0::2] ^= 1
            if u & 2:
                bits[1::2] ^= 1
            body = AF.to_soft(bits, sigma=20.0, seed=1000 * u + i)
            row = np.concatenate([np.array([-1], np.int16), noise(LEAD), body])
            out[u, i * STEP:(i + 1) * STEP] = np.concatenate([row, noise(STEP - len(row))])
    return out


def main():
    import torch

    from jaero_amd.demodulator import AeroLBank

    ap = argparse.ArgumentParser()
    ap.add_argument("channels", nargs="?", type=int, default=65536)
    ap.add_argument("steps", nargs="?", type=int, default=20)
    ap.add_argument("warmup", nargs="?", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--off-only", action="store_true", help="time the bank without the reassembly alone (runs on a library from before the feature)")
    args = ap.parse_args()
    nch, K, W = args.channels, args.steps, args.warmup
    dev = torch.device("cuda", 0)
    soft = torch.from_numpy(build_streams(K + W)).to(dev)
    idx = torch.arange(nch, device=dev) % NUNIQ
    counts = torch.full((nch,), STEP, dtype=torch.int32, device=dev)
    frame = torch.zeros((nch, STEP), dtype=torch.int16, device=dev)
    off = AeroLBank(nch, FB, max_softbits_per_write=STEP, su_capacity=32, burst=True)
    if args.off_only:
        off.profile_enable(True)
        for i in range(W + K):
            if i == W:
                torch.cuda.synchronize()
                for k in range(3):
                    off.profile_read(k, reset=True)
            frame.copy_(soft[idx, i * STEP:(i + 1) * STEP])
            off.write_device(frame.data_ptr(), counts.data_ptr(), STEP, STEP, torch.cuda.current_stream().cuda_stream)
            off.read_packets_all()
        print(json.dumps({"what": "aerol_rt_timing_off_only", "channels": nch, "steps": K, "warmup": W,
                          "kernels_ms_per_step_off": {name: round(off.profile_read(k)[0] / K, 4) for k, name in enumerate(("bits", "viterbi", "post"))}}))
        off.close()
        return
    on = AeroLBank(nch, FB, max_softbits_per_write=STEP, su_capacity=32, burst=True)
    on.rt_enable(4)
    stream = torch.cuda.current_stream().cuda_stream

    def step(i):
        frame.copy_(soft[idx, i * STEP:(i + 1) * STEP])
        off.write_device(frame.data_ptr(), counts.data_ptr(), STEP, STEP, stream)
        on.write_device(frame.data_ptr(), counts.data_ptr(), STEP, STEP, stream)

    for i in range(W):
        step(i)
        off.read_packets_all(); on.read_packets_all(); on.read_msgs_all()
    torch.cuda.synchronize()
    off.profile_enable(True); on.profile_enable(True)
    wall_m, wall_p, nmsg, npk = [], [], 0, 0
    for i in range(W, W + K):
        step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, msgs, ovm = on.read_msgs_all()
        t1 = time.perf_counter()
        _, pk, ovp = on.read_packets_all()
        t2 = time.perf_counter()
        off.read_packets_all()
        assert not ovm.any() and not ovp.any()
        wall_m.append(t1 - t0); wall_p.append(t2 - t1)
        nmsg += len(msgs); npk += len(pk)
    names = ("bits", "viterbi", "post", "sweep", "link", "isu")
    p_off = {name: off.profile2_read(k) for k, name in enumerate(names)}
    p_on = {name: on.profile2_read(k) for k, name in enumerate(names)}
    stats = on.rt_stats().sum(axis=0)
    ms = lambda x: round(1e3 * float(x), 4)
    line = {
        "what": "aerol_rt_timing", "channels": nch, "steps": K, "warmup": W, "fb": FB, "softbits_per_step": STEP,
        "payload": "per channel one burst per step: a T packet with a 100-character ACARS block (ISU + 15 SSUs) on even steps, an R packet with a one-unit message on odd steps",
        "kernels_ms_per_step_off": {k: round(p_off[k][0] / K, 4) for k in ("bits", "viterbi", "post")},
        "kernels_ms_per_step_on": {k: round(p_on[k][0] / K, 4) for k in ("bits", "viterbi", "post", "isu")},
        "isu_launches": p_on["isu"][1], "isu_launches_off": p_off["isu"][1],
        "messages_per_step": round(nmsg / K, 1), "packet_rows_per_step": round(npk / K, 1),
        "read_msgs_all_wall_ms_per_step": ms(np.mean(wall_m)), "read_msgs_all_wall_ms_min": ms(np.min(wall_m)), "read_msgs_all_wall_ms_max": ms(np.max(wall_m)),
        "read_packets_all_wall_ms_per_step": ms(np.mean(wall_p)), "read_packets_all_wall_ms_min": ms(np.min(wall_p)), "read_packets_all_wall_ms_max": ms(np.max(wall_p)),
        "read_msgs_all_bytes_per_step": round(544 * nmsg / K), "read_packets_all_bytes_per_step": round(64 * npk / K),
        "not_timed": "the host reassembly (RISUData::update, ISUData::update, ParserISU::parse) a caller of read_packets_all would run on those rows",
        "rt_stats_total": {k: int(v) for k, v in zip(("t_isu", "t_ssu", "t_missing", "t_completed", "r_fed", "r_new", "r_completed", "r_signal"), stats)},
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(line))
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")
    off.close()
    on.close()


if __name__ == "__main__":
    main()
