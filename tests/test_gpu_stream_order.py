"""GPU (-m gpu): a handle written from two streams in turn gives what it gives from one.

Every handle that takes a caller's stream orders a write on another stream than the previous one behind what it enqueued there
(DevHandle::order_behind, jaero_amd/csrc/host_common.h): one event recorded on the old stream, waited for on the new.  The demodulator bank's
use of it is covered by tests/test_gpu_parity.py; here the channeliser (int16 and with a capture front end), the rate meter and the
splitter run the same writes twice -- every write on the null stream, then alternating between two `torch.cuda.Stream`s, which do not
synchronise with the null stream or each other -- and every reader must return the same bytes.  The inputs are device tensors made before
the first write.  The alternating run happens twice: once with no host synchronisation up to the last write that produces output, read
there and after the last write, and once read after every write (a read waits for the stream of the last write only)."""
import numpy as np
import pytest

import chan_oracle as CO
from chan_cases import AUDIO, CH, white_full_scale

pytestmark = pytest.mark.gpu

HP = CO.HP
CHAN_WRITES = (5000, 8192, 3000, 12000, 4000)  # the hop is 8192: of 32 192 samples, one block completes in write 2 and two in write 4
RATE_WRITES = (3000, 4096, 2000, 7000)         # the segment is 4096: the first write only fills the pending row


def device_pieces(a, sizes, axis=0):
    """`a` cut along `axis` into contiguous device tensors of the sizes, all of them on the device before this returns."""
    import torch

    assert a.shape[axis] == sum(sizes)
    cuts = np.cumsum((0,) + tuple(sizes))
    pieces = [torch.from_numpy(np.ascontiguousarray(np.take(a, range(cuts[i], cuts[i + 1]), axis=axis))).cuda() for i in range(len(sizes))]
    torch.cuda.synchronize()
    return pieces


def stream_plans():
    """(name, the stream handle of write i, the writes to read after -- None: all): the single-stream reference first."""
    import torch

    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    alternate = lambda i: s[i % 2].cuda_stream
    assert alternate(0) != alternate(1) and 0 not in (alternate(0), alternate(1))
    return [("null stream", lambda i: 0, None), ("alternating, read late", alternate, (3, 4)), ("alternating, read every write", alternate, None)], s


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_channeliser(make, pieces, stream_of, read_at):
    """{write: (nout, staged, first, pcm)}: what the readers return after the writes `read_at`."""
    h = make()
    reads = {}
    for i, p in enumerate(pieces):
        nout = h.write(p, stream=stream_of(i))
        if read_at is None or i in read_at:
            z, first = h.read_staged() if h.capture is not None else (np.zeros(0), 0)
            reads[i] = (nout, z, first, h.read_pcm())
    h.close()
    return reads


def check_channeliser(make, pieces, staged_per_input=1.0):
    plans, _streams = stream_plans()
    ref = run_channeliser(make, pieces, plans[0][1], None)
    staged = np.ceil(np.cumsum(CHAN_WRITES) * staged_per_input).astype(np.int64)  # samples in front of the forward transform so far
    blocks = np.diff(np.concatenate([[0], staged // HP]))
    assert blocks.tolist() == [0, 1, 0, 1 if staged_per_input < 1.0 else 2, 0] and [ref[i][0] for i in range(5)] == (blocks * (HP // 16)).tolist()
    assert all(r[3].astype(float).std() > 100.0 for r in ref.values() if r[0] > 0), "the reference run's output is empty"
    for name, stream_of, read_at in plans[1:]:
        got = run_channeliser(make, pieces, stream_of, read_at)
        assert sorted(got) == sorted(read_at or ref)
        for i, g in got.items():
            w = ref[i]
            assert g[0] == w[0] and g[2] == w[2], (name, i)
            assert same(g[1], w[1]), (name, i, "the staged samples differ from the single-stream run")
            assert same(g[3], w[3]), (name, i, "the PCM differs from the single-stream run")


def two_channels(CHm, fs_c, seed):
    rng = np.random.default_rng(seed)
    return [(CHm.tune_word(float(rng.uniform(-fs_c / 2, fs_c / 2)), float(fs_c)), AUDIO, 1.0) for _ in range(2)]


def test_channeliser_int16(CH):
    """decim 16, two channels, ragged writes of 5 000, 8 192, 3 000, 12 000 and 4 000 I/Q samples."""
    fs_c = 768000
    chans, taps = two_channels(CH, fs_c, 1), CH.design_taps(16, ntaps=2049, beta=10.0)
    pieces = device_pieces(white_full_scale(sum(CHAN_WRITES), 11), CHAN_WRITES)
    make = lambda: CH.Channeliser(16, chans, taps=taps, max_write_iq=max(CHAN_WRITES))
    check_channeliser(make, pieces)


def test_channeliser_capture(CH):
    """The first resampling case of tests/test_gpu_chan_capture.py (cu8 at 1.2 MS/s into 768 kS/s, 16 / 25, K = 32: the smallest decimation
    and sample, with a raw history of K - 1 pairs that swaps buffers behind every write) under the same write pattern: 32 192 capture
    samples stage 20 603, so blocks complete in writes 2 and 4.  The staged samples of every write are compared as well as the PCM."""
    fs_c = 768000
    chans, taps = two_channels(CH, fs_c, 2), CH.design_taps(16, ntaps=2049, beta=10.0)
    raw = np.random.default_rng(12).integers(0, 256, size=(sum(CHAN_WRITES), 2), dtype=np.uint8)
    pieces = device_pieces(raw, CHAN_WRITES)
    cap = CH.Capture(fs_in=1200000, fmt="cu8", taps_per_phase=32)
    make = lambda: CH.Channeliser(16, chans, taps=taps, max_write_iq=max(CHAN_WRITES), capture=cap)
    check_channeliser(make, pieces, 16 / 25)


def test_rate_meter():
    """Two channels, writes of 3 000, 4 096, 2 000 and 7 000 samples: every write behind the first completes at least one segment."""
    from jaero_amd import capi, ratemeter

    capi.lib()
    pcm = np.random.default_rng(13).integers(-20000, 20000, size=(2, sum(RATE_WRITES))).astype(np.int16)
    pieces = device_pieces(pcm, RATE_WRITES, axis=1)
    plans, _streams = stream_plans()

    def run(stream_of, read_at):
        r = ratemeter.RateMeter(2, 48000.0, max_write_samples=max(RATE_WRITES))
        reads = {}
        for i, p in enumerate(pieces):
            done = r.write_device(p.data_ptr(), p.shape[1], stream=stream_of(i))
            if read_at is None or i in read_at:
                reads[i] = (done,) + r.read()
        r.close()
        return reads

    ref = run(plans[0][1], None)
    assert [ref[i][0] for i in range(4)] == [0, 1, 1, 1] and ref[3][2] == 3 and ref[3][1].max() > 0.0
    for name, stream_of, read_at in plans[1:]:
        got = run(stream_of, read_at and (3,))  # the sums hold every segment: one read behind the last write says it all
        assert sorted(got) == sorted(read_at and (3,) or ref)
        for i, g in got.items():
            w = ref[i]
            assert g[0] == w[0] and g[2] == w[2], (name, i, "segment counts differ")
            assert same(g[1], w[1]), (name, i, "the sums differ from the single-stream run")


def test_splitter_views(CH):
    """Two outputs (48 kHz x 2 channels, 24 kHz x 3).  A view's readers wait for the stream of the splitter's last write, which the view does
    not keep a copy of: its read_pcm right behind a write of the splitter on either stream equals the stand-alone twin's, which ran on the
    null stream."""
    fs_c = 768000
    rng = np.random.default_rng(3)
    outs = []
    for fs_out, nch in ((48000.0, 2), (24000.0, 3)):
        chans = [(CH.tune_word(float(rng.uniform(-fs_c / 2, fs_c / 2)), float(fs_c)), AUDIO, 1.0) for _ in range(nch)]
        outs.append((fs_out, chans, CH.design_taps(int(fs_c // fs_out), ntaps=2049, beta=10.0, fs_out=fs_out)))
    pieces = device_pieces(white_full_scale(sum(CHAN_WRITES), 14), CHAN_WRITES)
    mw = max(CHAN_WRITES)
    twins = [CH.Channeliser(int(fs_c // fs_out), chans, taps=taps, max_write_iq=mw, fs_out=fs_out) for fs_out, chans, taps in outs]
    ref = []
    for p in pieces:
        ref.append([(t.write(p), t.read_pcm()) for t in twins])
    assert [r[0][0] > 0 for r in ref] == [False, True, False, True, False]
    assert all(pcm.astype(float).std() > 100.0 for r in ref for n, pcm in r if n > 0)
    plans, _streams = stream_plans()
    for name, stream_of, read_at in plans[1:]:
        sp = CH.Splitter(fs_c, outs, max_write_iq=mw)
        for i, p in enumerate(pieces):
            nout = sp.write(p, stream=stream_of(i))
            assert list(nout) == [n for n, _ in ref[i]], (name, i)
            if read_at is None or i in read_at:
                for g, o in enumerate(sp.outputs):
                    assert same(o.read_pcm(), ref[i][g][1]), (name, i, g, "a view's PCM differs from its stand-alone twin's")
        sp.close()
    for t in twins:
        t.close()
