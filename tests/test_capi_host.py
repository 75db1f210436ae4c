"""CPU: the C-ABI library loads, exports every symbol include/jaero_hip.h declares, fails loudly without a GPU, and
its host-side scheduling (where the coarse estimate fires) matches the reference's counters."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from jaero_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "jaero_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(jaero_[a-z_0-9]+)\s*\(", hdr))
    assert len(declared) >= 20
    L = capi.lib()
    for name in sorted(declared):
        assert hasattr(L, name), f"{name} declared in include/jaero_hip.h but not exported"
    assert declared == set(capi.EXPORTS)
    assert L.jaero_abi_version() == 1


def test_struct_layout_matches_header():
    assert C.sizeof(capi.Settings) == 48  # 2 ints + 5 doubles
    assert C.sizeof(capi.Status) == 40


def test_no_cpu_fallback():
    """Without a HIP device jaero_create must fail with ENODEV (never silently compute on the host)."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    L = capi.lib()
    s = capi.Settings(capi.KIND_OQPSK, 14, 8000.0, 10500.0, 10500.0, 48000.0, 0.65)
    h = C.c_void_p()
    rc = L.jaero_create(0, 4, C.byref(s), 0, 0, 4096, 0, C.byref(h))
    assert rc == capi.E_NODEV and not h.value
    assert b"fallback" in L.jaero_last_error() or b"device" in L.jaero_last_error()
    assert L.jaero_strerror(rc) == b"no usable HIP device"


def test_ingest_and_aerol_argument_checks_need_no_device():
    """Null / out-of-range arguments are refused before any HIP call (codes and messages as the header documents)."""
    L = capi.lib()
    h = C.c_void_p()
    assert L.jaero_ingest_create(None, 4096, 0, C.byref(h)) == capi.E_INVAL and not h.value
    assert L.jaero_ingest_push(None, 0, b"", 0, 48000) == capi.E_INVAL
    assert L.jaero_ingest_queued(None, 0) == capi.E_INVAL
    assert L.jaero_ingest_pump(None, 0, None, None) == capi.E_INVAL
    assert L.jaero_ingest_stats(None, None) == capi.E_INVAL
    assert b"jaero_ingest" in L.jaero_last_error()
    assert L.jaero_write(None, None, 0, 0, 0, None) == capi.E_INVAL
    n = C.c_int(0)
    buf = (C.c_double * 64)()
    for name in ("jaero_read_softbits", "jaero_read_status_log", "jaero_read_symbols", "jaero_read_events", "jaero_aerol_read_sus",
                 "jaero_aerol_read_packets", "jaero_aerol_read_events", "jaero_aerol_read_voice"):
        assert getattr(L, name)(None, 0, buf, 4, C.byref(n)) == capi.E_INVAL, name


def test_coarse_hooks_refuse_a_null_context():
    """jaero_debug_coarse_poke / _launch / _peek: JAERO_EINVAL before any HIP call (burst bank, bad channel, bad grid: tests/test_gpu_coarse.py)."""
    L = capi.lib()
    st = capi.CoarseState()
    buf = (C.c_double * 8)()
    assert C.sizeof(capi.CoarseState) == 56  # 8 ints + 3 doubles
    assert L.jaero_debug_coarse_poke(None, 0, buf, buf, C.byref(st)) == capi.E_INVAL
    assert b"jaero_debug_coarse_poke" in L.jaero_last_error()
    assert L.jaero_debug_coarse_launch(None, None, 1, 0) == capi.E_INVAL
    assert b"jaero_debug_coarse_launch" in L.jaero_last_error()
    assert L.jaero_debug_coarse_peek(None, 0, buf, buf, C.byref(st)) == capi.E_INVAL
    assert b"jaero_debug_coarse_peek" in L.jaero_last_error()


def test_loop_hooks_refuse_a_null_context():
    """jaero_debug_loop_poke / _peek: JAERO_EINVAL before any HIP call (burst bank, bad channel, bad values: tests/test_gpu_loop_branches.py)."""
    L = capi.lib()
    st = capi.LoopState(10500.0, 8000.0, 0.0, 0.0, 0.0, 0.0)
    assert C.sizeof(capi.LoopState) == 48  # 6 doubles
    assert L.jaero_debug_loop_poke(None, 0, C.byref(st)) == capi.E_INVAL
    assert b"jaero_debug_loop_poke" in L.jaero_last_error()
    assert L.jaero_debug_loop_peek(None, 0, C.byref(st)) == capi.E_INVAL
    assert b"jaero_debug_loop_peek" in L.jaero_last_error()
    assert st.st_freq == 10500.0 and st.lf_y2 == 0.0


def test_burst_acquisition_hooks_refuse_a_null_context():
    """jaero_debug_burst_geom / _hilbert / _read_hist / _poke_cv / _trident: JAERO_EINVAL before any HIP call (a bank that is not a burst bank, bad
    channels, sizes, lists and grids: tests/test_gpu_burst_acq.py)."""
    L = capi.lib()
    assert C.sizeof(capi.BurstGeom) == 56 and C.sizeof(capi.TridentResult) == 40  # 12 ints + a long long; 2 ints + 4 doubles
    buf = (C.c_double * 8)()
    idx = (C.c_int * 2)()
    n = C.c_int(7)
    res = (capi.TridentResult * 2)()
    assert L.jaero_debug_burst_geom(None, C.byref(capi.BurstGeom())) == capi.E_INVAL
    assert b"jaero_debug_burst_geom" in L.jaero_last_error()
    assert L.jaero_debug_burst_hilbert(None, buf, 0, 1, buf) == capi.E_INVAL
    assert b"jaero_debug_burst_hilbert" in L.jaero_last_error()
    assert L.jaero_debug_burst_hilbert(None, buf, 5, 1, buf) == capi.E_INVAL
    assert L.jaero_debug_burst_read_hist(None, 0, 0, 1, buf) == capi.E_INVAL
    assert b"jaero_debug_burst_read_hist" in L.jaero_last_error()
    assert L.jaero_debug_burst_poke_cv(None, 0, 0, 1, buf) == capi.E_INVAL
    assert b"jaero_debug_burst_poke_cv" in L.jaero_last_error()
    assert L.jaero_debug_burst_trident(None, idx, idx, 1, 0, 0, res, C.byref(n)) == capi.E_INVAL
    assert b"jaero_debug_burst_trident" in L.jaero_last_error() and n.value == 7


def test_burst_front_hooks_refuse_a_null_context():
    """jaero_debug_burst_front_geom / _front / _front_peek / _front_events / _front_poke / _poke_bt: JAERO_EINVAL before any HIP call, and
    jaero_debug_ev_compact's argument checks (the rest: tests/test_gpu_burst_front.py).  jaero_burst_geom keeps its size."""
    L = capi.lib()
    assert C.sizeof(capi.BurstFrontGeom) == 64 and C.sizeof(capi.BurstFrontState) == 64  # 10 ints + 3 doubles; 5 doubles + 6 ints
    buf = (C.c_double * 64)()
    idx = (C.c_int * 64)()
    n = C.c_int(7)
    for name, args in (("jaero_debug_burst_front_geom", (C.byref(capi.BurstFrontGeom()),)), ("jaero_debug_burst_front", (buf, 0, 1, None, idx, idx, C.byref(n))),
                       ("jaero_debug_burst_front_peek", (0, C.byref(capi.BurstFrontState()), 7, 0, 1, buf)), ("jaero_debug_burst_front_events", (0, buf, 4, C.byref(n))),
                       ("jaero_debug_burst_front_poke", (0, 0, 0.0)), ("jaero_debug_burst_poke_bt", (0, 0, 1, buf))):
        assert getattr(L, name)(None, *args) == capi.E_INVAL, name
        assert name.encode() in L.jaero_last_error(), name
    assert n.value == 7
    masks = (C.c_uint64 * 1)()
    for m, ng in ((None, 1), (masks, 0), (masks, 65537)):
        assert L.jaero_debug_ev_compact(0, m, ng, idx, C.byref(n)) == capi.E_INVAL and b"jaero_debug_ev_compact" in L.jaero_last_error()
    assert L.jaero_debug_ev_compact(0, masks, 1, None, C.byref(n)) == capi.E_INVAL and L.jaero_debug_ev_compact(0, masks, 1, idx, None) == capi.E_INVAL


def test_burst_track_hooks_refuse_a_null_context():
    """jaero_debug_burst_track_geom / _track / _track_peek / _track_fill / _track_read: JAERO_EINVAL before any HIP call, and the argument checks
    that need no bank (the rest: tests/test_gpu_burst_track.py)."""
    L = capi.lib()
    assert C.sizeof(capi.BurstTrackGeom) == 48 and C.sizeof(capi.BurstTrackState) == 192  # 12 ints; 16 ints + 16 doubles
    buf = (C.c_double * 64)()
    idx = (C.c_int * 4)()
    res = (capi.TridentResult * 4)()
    st = capi.BurstTrackState()
    st.cntr = 7
    for name, args in (("jaero_debug_burst_track_geom", (C.byref(capi.BurstTrackGeom()),)), ("jaero_debug_burst_track", (1, 1, idx, idx, res, 1)),
                       ("jaero_debug_burst_track_peek", (0, C.byref(st))), ("jaero_debug_burst_track_fill", (-2, -2.0)),
                       ("jaero_debug_burst_track_read", (0, 0, buf, 64)), ("jaero_debug_burst_track_center_freq", (0, 1000.0))):
        assert getattr(L, name)(None, *args) == capi.E_INVAL, name
        assert name.encode() in L.jaero_last_error(), name
    assert st.cntr == 7
    assert L.jaero_debug_burst_track_geom(None, None) == capi.E_INVAL and L.jaero_debug_burst_track_peek(None, 0, None) == capi.E_INVAL
    assert L.jaero_debug_burst_track(None, 1, 2, idx, idx, res, 1) == capi.E_INVAL and b"first_of_write" in L.jaero_last_error()
    assert L.jaero_debug_burst_track_fill(None, 40000, 0.0) == capi.E_INVAL and b"int16" in L.jaero_last_error()
    assert L.jaero_debug_burst_track_read(None, 0, 2, buf, 64) == capi.E_INVAL and L.jaero_debug_burst_track_read(None, 0, 0, None, 64) == capi.E_INVAL


def test_viterbi_probe_refuses_what_the_kernels_do_not_implement():
    """jaero_debug_viterbi: JAERO_EINVAL before any HIP call for the combinations neither kernel implements (the launches themselves:
    tests/test_gpu_viterbi_modes.py).  A probe that passes these checks gets as far as the device (JAERO_ENODEV here, 0 on a GPU)."""
    L = capi.lib()
    assert C.sizeof(capi.ViterbiProbe) == 96  # 5 pointers + 13 ints, padded
    soft = np.full((64, 320), 128, np.uint8)
    out = np.zeros((64, 256), np.uint8)
    ov = np.zeros((64, 64), np.uint8)
    lens = np.full(64, 320, np.int32)

    def rc(**kw):
        a = dict(soft=soft.ctypes.data, nblocks=64, nsoft=304, out=out.ctypes.data, out_stride=256, out_want=152, layout=2)
        a.update(kw)
        q = capi.ViterbiProbe(**a)
        return L.jaero_debug_viterbi(0, C.byref(q))

    assert rc() in (0, capi.E_NODEV)
    assert rc(tiled=1, packed=1, out_want=150) in (0, capi.E_NODEV)
    bad = [dict(soft=None), dict(out=None), dict(layout=4), dict(nblocks=0), dict(pad=3), dict(out_start=-1), dict(out_want=0),
           dict(layout=1, tiled=1), dict(layout=1, packed=1),                      # tiled / packed exist only in the lane layout
           dict(tiled=1, nsoft=300), dict(tiled=1, pitch=320), dict(tiled=1, soft_misalign=4), dict(tiled=1, lens=lens.ctypes.data),
           dict(nsoft=54), dict(nsoft=40, pad=0), dict(layout=3, nsoft=54, pad=0),  # lanes below 4 * VT_ORDER steps
           dict(out_stride=151), dict(packed=1, out_stride=16), dict(packed=1, out_stride=22), dict(out_rows=63), dict(pitch=300),
           dict(update_overlap=1), dict(soft_misalign=16)]
    for kw in bad:
        assert rc(**kw) == capi.E_INVAL, kw
        assert b"jaero_debug_viterbi" in L.jaero_last_error(), kw
    assert rc(layout=1, nsoft=40) in (0, capi.E_NODEV)  # the wavefront layout takes what the lane layout is too short for
    for l0 in (322, 129, 26):
        lens[5] = l0
        assert rc(nsoft=320, lens=lens.ctypes.data) == capi.E_INVAL and b"lens[5]" in L.jaero_last_error()
    lens[5] = 128
    assert rc(nsoft=320, lens=lens.ctypes.data) in (0, capi.E_NODEV)
    ov[9, 62] = 63
    assert rc(overlap=ov.ctypes.data) == capi.E_INVAL and b"overlap[9]" in L.jaero_last_error()


@pytest.mark.parametrize("kind,power,fb,Fs,lbw,ok", [
    (capi.KIND_OQPSK, 14, 10500.0, 48000.0, 24000.0, True), (capi.KIND_OQPSK, 14, 10500.0, 48000.0, 24000.5, False),
    (capi.KIND_OQPSK, 14, 8400.0, 48000.0, 30000.0, False), (capi.KIND_MSK, 13, 1200.0, 48000.0, 24001.0, False),
    (capi.KIND_MSK, 13, 1200.0, 12000.0, 6000.0, True), (capi.KIND_MSK, 13, 1200.0, 12000.0, 6000.1, False),
    (capi.KIND_MSK, 13, 600.0, 24000.0, 12000.0, True), (capi.KIND_MSK, 13, 600.0, 24000.0, 18000.0, False),
    (capi.KIND_BURST_OQPSK, 13, 10500.0, 48000.0, 25000.0, False), (capi.KIND_BURST_MSK, 13, 1200.0, 48000.0, 48000.0, False),
])
def test_locking_bandwidth_above_half_the_sample_rate_is_refused(kind, power, fb, Fs, lbw, ok):
    """lockingbw > Fs / 2: the band limit's two edges meet and the reference's window loop overwrites its own entries,
    so jaero_create refuses it with JAERO_EINVAL -- for any channel of the bank, and before it looks for a device.  Up to Fs / 2 the settings
    pass (what comes back then is the device's answer)."""
    L = capi.lib()
    good = capi.Settings(kind, power, 1000.0, min(lbw, 1000.0), fb, Fs, 0.5)
    for sets in ([capi.Settings(kind, power, 1000.0, lbw, fb, Fs, 0.5)], [good, good, capi.Settings(kind, power, 1000.0, lbw, fb, Fs, 0.5)]):
        arr = (capi.Settings * len(sets))(*sets)
        h = C.c_void_p()
        rc = L.jaero_create(0, len(sets), C.addressof(arr), C.sizeof(capi.Settings), 0, 4096, 0, C.byref(h))
        if h.value:
            L.jaero_destroy(h)
        if ok:
            assert rc in (0, capi.E_NODEV)
        else:
            assert rc == capi.E_INVAL and not h.value and b"lockingbw" in L.jaero_last_error() and b"Fs / 2" in L.jaero_last_error()


def test_aerol_create_without_a_device():
    """jaero_aerol_create fails with ENODEV without a HIP device, as jaero_create does."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    L = capi.lib()
    h = C.c_void_p()
    assert L.jaero_aerol_create(0, 4, 10500, 4096, 0, C.byref(h)) == capi.E_NODEV and not h.value
    assert L.jaero_aerol_create(0, 4, 8400, 4096, 0, C.byref(h)) == capi.E_NODEV and not h.value


def _oracle_triggers(O, kind, cpu_reduce, writes):
    d = O.Demod(O.oqpsk_settings() if kind == "oqpsk" else O.msk_settings(), cpu_reduce=cpu_reduce)
    trig, base = [], 0
    rng = np.random.default_rng(0)
    for n in writes:
        x = rng.integers(-2000, 2000, n).astype(np.int16)
        # feed sample by sample so the estimate can be attributed to a sample index
        for i in range(n):
            d.write(x[i:i + 1])
            rows = d.take_status()
            if len(rows):
                trig.append(base + i)
        base += n
    return trig


@pytest.mark.parametrize("kind,power,cpu,writes", [
    ("oqpsk", 14, 0, [4096, 4096, 1000, 777, 5000, 3]),
    ("oqpsk", 14, 1, [30000, 30000, 12345, 40000]),
    ("msk", 13, 0, [2048, 1, 2047, 6000]),
])
def test_schedule_matches_reference_counters(oracle_mod, kind, power, cpu, writes):
    L = capi.lib()
    w = np.array(writes, dtype=np.int32)
    out = np.zeros(256, dtype=np.int64)
    nseg = C.c_int(0)
    n = L.jaero_debug_schedule(power, 48000, cpu, w.ctypes.data, len(writes), out.ctypes.data, 256, C.byref(nseg))
    assert n >= 0
    ref = _oracle_triggers(oracle_mod, kind, bool(cpu), writes)
    assert list(out[:n]) == ref
    assert nseg.value >= n


def test_shard_range_matches_the_python_helper():
    """jaero_shard_range (the C ABI's multi-GPU edge operations) = jaero_amd.dist.shard_range: contiguous, covering, in rank order."""
    from jaero_amd import dist

    L = capi.lib()
    for n, w in ((65536, 8), (32768, 8), (4096, 3), (7, 4), (0, 2), (5, 1)):
        prev = 0
        for r in range(w):
            lo, hi = C.c_int(), C.c_int()
            assert L.jaero_shard_range(n, r, w, C.byref(lo), C.byref(hi)) == 0
            assert (lo.value, hi.value) == dist.shard_range(n, r, w) and lo.value == prev
            prev = hi.value
        assert prev == n
    lo, hi = C.c_int(), C.c_int()
    assert L.jaero_shard_range(8, 2, 2, C.byref(lo), C.byref(hi)) != 0


def _brute_force_triggers(nfft, Fs, flags0, writes, events):
    """Every channel on its own, sample by sample, exactly as the reference's counters move (JAERO/oqpskdemodulator.cpp:410-431):
    ring write when coarseCounter >= Fs or not cpuReduce; fire when the ring pointer reaches a multiple of nfft (cpuReduce) or nfft/4."""
    nch = len(flags0)
    flags = np.array(flags0, dtype=np.int64)
    bb = np.zeros(nch, dtype=np.int64)
    cnt = np.zeros(nch, dtype=np.int64)
    out = []
    base = 0
    for w, ns in enumerate(writes):
        for (bw, ch, kind, val) in events:
            if bw != w:
                continue
            sel = slice(None) if ch < 0 else slice(ch, ch + 1)
            if kind == 0:
                flags[sel] = (flags[sel] & 8) | (val & 7)
            elif kind == 1:
                flags[sel] = (flags[sel] & ~8) | (8 if val else 0)
            else:
                bb[sel] = 0
                cnt[sel] = 0
        for i in range(ns):
            cpu = (flags & 4) != 0
            fill = (cnt >= Fs) | ~cpu
            bb = np.where(fill, (bb + 1) % nfft, bb)
            fire = fill & (bb % np.where(cpu, nfft, nfft // 4) == 0)
            for c in np.nonzero(fire)[0]:
                out.append((base + i, int(c)))
            cnt = np.where(fire, 0, cnt) + 1
        base += ns
    return out


@pytest.mark.parametrize("nch,seed", [(64, 1), (130, 2), (7, 3)])
def test_schedule_with_per_lane_flags_matches_brute_force(nch, seed):
    """The host scheduler with channels of one bank drawing AFC / SQL / cpuReduce independently, flags toggled and setSettings called for
    single channels between writes of odd sizes: which channel fires at which sample, against a per-channel brute-force simulation
    (mixed cpuReduce inside one wavefront had never run anywhere)."""
    L = capi.lib()
    rng = np.random.default_rng(seed)
    power, Fs = 9, 3000  # short cycles: 512-entry ring, the cpuReduce gate opens after 3000 samples
    flags0 = rng.integers(0, 8, nch).astype(np.int32)  # AFC | SQL | cpuReduce in any combination
    writes = [int(x) for x in rng.integers(1, 1500, 40)]
    events = []
    for w in sorted(rng.integers(1, len(writes), 24)):
        kind = int(rng.integers(0, 3))
        ch = int(rng.integers(-1, nch)) if rng.random() < 0.9 else -1
        events.append((int(w), ch, kind, int(rng.integers(0, 8)) if kind == 0 else int(rng.integers(0, 2))))
    ev = np.array(events, dtype=np.int32).reshape(-1, 4)
    w = np.array(writes, dtype=np.int32)
    cap = 1 << 16
    out = np.zeros((cap, 2), dtype=np.int64)
    nseg = C.c_int(0)
    n = L.jaero_debug_schedule_lanes(power, Fs, nch, flags0.ctypes.data, w.ctypes.data, len(writes), ev.ctypes.data, len(events),
                                     out.ctypes.data, cap, C.byref(nseg))
    assert 0 < n <= cap
    got = sorted((int(a), int(b)) for a, b in out[:n])
    want = sorted(_brute_force_triggers(1 << power, Fs, flags0, writes, events))
    assert got == want
    both = {bool(f & 4) for f in flags0}
    assert both == {True, False} and nseg.value >= len({s for s, _ in want})
