/* jaero_hip.h -- C ABI of libjaero_hip.so: the MI355X (gfx950) batched Aero demodulator.
 *
 * This is the drop-in boundary for the reference's demodulator hot path.  One `jaero_ctx` is a BANK of
 * `nchannels` independent demodulators of the same kind and rate living on one GPU; every entry point below
 * replaces one member of the reference's per-object QIODevice surface (citations are relative to
 * /root/reference/).  Plain pointers and sizes only -- no Qt, torch or HIP types in the signatures
 * (streams are passed as `void*` = hipStream_t, NULL = the default stream).
 *
 *   reference (one object per channel)                               this ABI (one call, all channels)
 *   ---------------------------------------------------------------  -----------------------------------------
 *   OqpskDemodulator(parent)+setSettings(Settings)+start()           jaero_create
 *     JAERO/oqpskdemodulator.cpp:8-117,175-289,312-315
 *   MskDemodulator(parent)+setSettings(Settings)+start()             jaero_create (kind = JAERO_KIND_MSK)
 *     JAERO/mskdemodulator.cpp:9-84,135-263,296-299
 *   setSettings on a live object                                     jaero_set_settings
 *   setAFC / setSQL / setCPUReduce                                   jaero_set_flags
 *     JAERO/oqpskdemodulator.cpp:149-163, JAERO/mskdemodulator.cpp:105-118
 *   DCDstatSlot(bool)            JAERO/oqpskdemodulator.cpp:679-684   jaero_set_dcd
 *   connect(AeroL::DataCarrierDetect -> DCDstatSlot)  JAERO/mainwindow.cpp:232-241   jaero_aerol_link_dcd
 *   CenterFreqChangedSlot(double) JAERO/oqpskdemodulator.cpp:291-310  jaero_center_freq_changed
 *   (two objects per stereo device: JAERO/audioburstoqpskdemodulator.cpp:8-10: channels are independent)  jaero_comm_* / jaero_fan_out_pcm / jaero_gather_softbits
 *   writeData(const char*,qint64) JAERO/oqpskdemodulator.cpp:334-627, jaero_write
 *                                 JAERO/mskdemodulator.cpp:313-488
 *   signal processDemodulatedSoftBits(QVector<short>)                jaero_read_softbits / jaero_softbits_view
 *     JAERO/oqpskdemodulator.h:66, emitted at oqpskdemodulator.cpp:583-591, mskdemodulator.cpp:472-477
 *   signals Plottables / MSESignal / EbNoMeasurmentSignal / SignalStatus   jaero_read_status / jaero_read_status_all (+ status log)
 *     emitted together at JAERO/oqpskdemodulator.cpp:670-675, JAERO/mskdemodulator.cpp:510-517
 *   FreqOffsetEstimateSlot + CoarseFreqEstimate::ProcessBasebandData  internal (runs inside jaero_write at the
 *     JAERO/oqpskdemodulator.cpp:414-428,629-677; coarsefreqestimate.cpp:90-137   same sample the reference does)
 *   JConvolutionalCodec::Decode_Continuous / Decode_soft              jaero_viterbi_* (batched, stateless blocks)
 *     JAERO/jconvolutionalcodec.cpp:151-201,90-119
 *   BurstOqpskDemodulator / BurstMskDemodulator: ctor+setSettings+start   jaero_create (kind = JAERO_KIND_BURST_*)
 *     JAERO/burstoqpskdemodulator.cpp:4-131,202-277  JAERO/burstmskdemodulator.cpp:9-84,150-325
 *   their writeData / writeDataSlot                                    jaero_write (same call)
 *     JAERO/burstoqpskdemodulator.cpp:300-737  JAERO/burstmskdemodulator.cpp:371-754
 *   their processDemodulatedSoftBits (with the -1 start-of-burst marker)  jaero_read_softbits (marker kept as -1)
 *   their SignalStatus / EbNoMeasurmentSignal / Plottables emissions   jaero_read_events
 *   every object's emissions of one class collected at once (a bank is many objects: no counterpart)   jaero_read_all
 *   channel_stereo / channel_select_other (two objects fed the L and R     two channels of one bank fed with
 *     samples of one interleaved stream, audioburstoqpskdemodulator.cpp:8-10)  JAERO_PCM_FRAME_MAJOR input
 *   stop() / destructor                                               jaero_destroy
 *
 * Conventions: every function returns 0 on success or a negative JAERO_E* code (the reference has no error
 * channel; this is additive).  The caller owns every buffer it passes; the library owns all device state.  One host
 * thread per ctx.  jaero_write is asynchronous on the given stream; the read_* calls synchronise that stream.
 * There is NO CPU fallback: if no gfx950 device is usable jaero_create fails with JAERO_ENODEV.
 */
#ifndef JAERO_HIP_H
#define JAERO_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JAERO_ABI_VERSION 1

/* demodulator kinds */
#define JAERO_KIND_MSK 0         /* MskDemodulator          JAERO/mskdemodulator.h:17                      */
#define JAERO_KIND_OQPSK 1       /* OqpskDemodulator        JAERO/oqpskdemodulator.h:15                    */
#define JAERO_KIND_BURST_MSK 2   /* BurstMskDemodulator     JAERO/burstmskdemodulator.h:22   (600 / 1200)  */
#define JAERO_KIND_BURST_OQPSK 3 /* BurstOqpskDemodulator   JAERO/burstoqpskdemodulator.h:19 (10500)       */

/* error codes */
#define JAERO_OK 0
#define JAERO_EINVAL (-1)   /* bad argument / unsupported settings combination        */
#define JAERO_ENODEV (-2)   /* no usable HIP device                                    */
#define JAERO_ENOMEM (-3)   /* device or host allocation failed                        */
#define JAERO_EHIP (-4)     /* a HIP runtime call failed (see jaero_last_error); also: every call but jaero_destroy on a bank whose
                             * jaero_write failed AFTER its first state-advancing launch (device state and the host's schedule mirror
                             * disagree: nothing can continue from there).  A write that failed earlier -- input copy, transpose --
                             * left the bank as it was and may be repeated. */
#define JAERO_EOVERFLOW (-5)/* soft-bit / log capacity exceeded since the last read    */
#define JAERO_ENOTSUP (-6)  /* kind / rate not implemented                             */
#define JAERO_W_RATE 1      /* (jaero_ingest_push only) warning: sample rate differs, data queued anyway */

/* jaero_create flags */
#define JAERO_FLAG_EBNO 1u            /* run the EbNo meters (OQPSKEbNoMeasure/MSKEbNoMeasure, diagnostic only)   */
#define JAERO_FLAG_STATUS_LOG 2u      /* keep one status row per FreqOffsetEstimateSlot call (tests)              */
#define JAERO_FLAG_CAPTURE_SYMBOLS 4u /* keep the soft symbol (pt_qpsk / pt_msk) + mse of every symbol (tests)     */
#define JAERO_FLAG_TRACE 8u           /* burst kinds: also log peak-detector firings and every trident check (tests)   */

/* burst event kinds (jaero_read_events): what the burst classes emit as Qt signals while demodulating */
#define JAERO_EV_SIGNAL 0  /* SignalStatus(value != 0)        burstoqpskdemodulator.cpp:511,542  burstmskdemodulator.cpp:545,593 */
#define JAERO_EV_EBNO 1    /* EbNoMeasurmentSignal(value)     burstoqpskdemodulator.cpp:581      burstmskdemodulator.cpp:637     */
#define JAERO_EV_FREQ 2    /* Plottables(freq_est = value)    burstoqpskdemodulator.cpp:275,484  burstmskdemodulator.cpp:196,342,538 */
#define JAERO_EV_PEAK 3    /* (JAERO_FLAG_TRACE) pdet.update() returned true                                                      */
#define JAERO_EV_TRIDENT 4 /* (JAERO_FLAG_TRACE) trident check ran: value = +metric accepted / -metric rejected                   */

/* PCM layouts accepted by jaero_write */
#define JAERO_PCM_CHANNEL_MAJOR 0 /* pcm[ch * nsamples + i]  : one contiguous mono stream per channel            */
#define JAERO_PCM_FRAME_MAJOR 1   /* pcm[i * nchannels + ch] : interleaved frames, like multichannel PCM audio   */

/* Mirrors OqpskDemodulator::Settings / MskDemodulator::Settings
 * (JAERO/oqpskdemodulator.h:20-39, JAERO/mskdemodulator.h:24-45). */
typedef struct jaero_settings
{
    int kind;                    /* JAERO_KIND_*                                   */
    int coarsefreqest_fft_power; /* 2^power point coarse-frequency FFT (13 or 14)  */
    double freq_center;          /* Hz                                             */
    double lockingbw;            /* Hz                                             */
    double fb;                   /* bit rate: 10500 or 8400 (OQPSK; 8400: continuous kind, fft power 14), 600 / 1200 (MSK) */
    double Fs;                   /* sample rate: 48000; MSK kind also 24000, 12000 */
    double signalthreshold;      /* mse threshold                                  */
} jaero_settings;

/* What the reference emits from FreqOffsetEstimateSlot, per channel. */
typedef struct jaero_status
{
    double mse;         /* MSESignal                               */
    double ebno;        /* EbNoMeasurmentSignal (0 unless JAERO_FLAG_EBNO) */
    double freq_est;    /* Plottables arg 1 = mixer2.GetFreqHz()   */
    double freq_center; /* Plottables arg 2 = mixer_center.GetFreqHz() */
    int signal;         /* SignalStatus                            */
    int n_estimates;    /* number of FreqOffsetEstimateSlot calls so far */
} jaero_status;

typedef struct jaero_ctx jaero_ctx;

/* Create a bank of nchannels demodulators on HIP device `device`.  All channels must agree on kind, fb, Fs and
 * coarsefreqest_fft_power (they share kernels and ring geometry); freq_center, lockingbw and signalthreshold are
 * per channel.  If `per_channel_stride` is 0, settings[0] is used for every channel.
 * max_write_samples bounds nsamples of one jaero_write (sizes staging buffers); softbit_capacity is the number of
 * soft bits each channel can hold between reads (0 = default: enough for 2*max_write_samples). */
int jaero_create(int device, int nchannels, const jaero_settings *settings, int per_channel_stride,
                 unsigned flags, int max_write_samples, int softbit_capacity, jaero_ctx **out);
void jaero_destroy(jaero_ctx *ctx);

/* setSettings on a live channel (channel = -1: every channel): the channel's state becomes what the reference's setSettings leaves behind
 * (JAERO/oqpskdemodulator.cpp:175-289, JAERO/mskdemodulator.cpp:135-263).
 *   - freq_center / lockingbw / signalthreshold of one or all channels: in place, enqueued on the stream of the bank's last jaero_write.
 *   - one channel of an 8400 bps bank (same fb / Fs / FFT power): in place as well; that channel's prefilter restarts as JFastFir::SetKernel
 *     leaves it (empty history, 2048 exact zeros in front of its first output, JAERO/oqpskdemodulator.cpp:278-283) while the transform blocks
 *     stay on the bank's grid of absolute multiples of 2048 samples -- the same filtered values up to transform round-off.
 *   - fb, Fs or the FFT power (shared by the channels of a bank), and a setSettings of a WHOLE 8400 bps bank (every prefilter restarts, the
 *     block grid with them): whole bank only (channel = -1, or a one-channel bank).  The bank is re-created behind the handle and receives what the reference keeps in the old
 *     object: oscillator phases, loop-filter / rotator / timing states, the symbol-rate windows (MSK: msema, the first entries of dt and
 *     delayedsmpl in buffer order), the EbNo meter of the OQPSK kind, the coarse ring and the smoothed spectrum, flags, unread outputs.
 *     Control plane: allocates and synchronises the device; pointers from the *_view calls are stale afterwards.  An OQPSK bank keeps Fs.
 *     The new bank exists beside the old one until the state has moved: a bank that fills more than half of the device memory cannot change
 *     rate this way (JAERO_ENOMEM, the old bank stays as it was).
 *   - burst banks (JAERO/burstoqpskdemodulator.cpp:202-277, JAERO/burstmskdemodulator.cpp:150-325), one or all channels, same fb and Fs: in
 *     place and on that stream too.  AGCs, EbNo meter, burst-timing averages and the Hilbert filter restart from empty, the peak detector is
 *     locked for twice its length and the trident buffer refills (and is checked once, whatever is in the air), mixer2 returns to
 *     freq_center; d1 / d2 / the peak detector's lines (burst MSK: delayedsmpl) keep their CONTENTS with the pointer back at zero, as
 *     DelayThing::setLength leaves them; startstop, the oscillator phases and RxDataBits survive (burst MSK: cntr = 0, mse = 10, dcd = false,
 *     new matched filters).  A Plottables row is appended to the channel's event log.
 *   - JAERO_EINVAL: another kind (another class in the reference), or fb / Fs / FFT power for one channel of several;
 *     Burst MSK with its other bit rate (600 <-> 1200 bps; whole bank): as for the continuous kinds a sibling bank takes the old one's place and
 *     receives what the reference keeps -- the DelayThings' first min(old, new) entries in storage order, startstop, oscillator phases, msema,
 *     unread outputs.
 *     JAERO_ENOTSUP: another Fs for a burst bank, another fb for burst OQPSK (create a new bank; the Qt
 *     adaptors of integration/qt do). */
int jaero_set_settings(jaero_ctx *ctx, int channel, const jaero_settings *s);
int jaero_set_flags(jaero_ctx *ctx, int channel, int afc, int sql, int cpu_reduce);
int jaero_set_dcd(jaero_ctx *ctx, int channel, int dcd);
/* CenterFreqChangedSlot: continuous kinds JAERO/oqpskdemodulator.cpp:291-310 / mskdemodulator.cpp:265-282; burst MSK
 * JAERO/burstmskdemodulator.cpp:327-342 (clamp, mixer2 follows under AFC or is pulled to within lockingbw/2, Plottables emission in the
 * event log); burst OQPSK: accepted, no effect -- the reference's slot is empty (burstoqpskdemodulator.cpp:284-289). */
int jaero_center_freq_changed(jaero_ctx *ctx, int channel, double freq_center_hz);

/* = writeData for every channel: nsamples of real int16 PCM per channel.  `pcm` is a host pointer
 * (is_device_ptr = 0; copied with hipMemcpyAsync) or a device pointer on the ctx's device (is_device_ptr = 1). */
int jaero_write(jaero_ctx *ctx, const int16_t *pcm, int nsamples, int layout, int is_device_ptr, void *stream);

/* Drain the soft bits channel `channel` produced (values 0..255 as the reference's QVector<short>), oldest first.
 * *n receives the count copied (<= cap).  Grouping into 32 (OQPSK) / 12 (MSK) emissions is the caller's. */
int jaero_read_softbits(jaero_ctx *ctx, int channel, int16_t *dst, int cap, int *n);
/* Batched drain: dst[ch * cap_per_channel + k], counts[ch].  Resets every channel's buffer. */
int jaero_read_softbits_all(jaero_ctx *ctx, int16_t *dst, int cap_per_channel, int *counts);
/* Device-side view for zero-copy consumers (RCCL gather, a downstream device decoder): int16 [nch][capacity]
 * and int32 counts[nch] on the ctx's device.  jaero_discard_softbits resets the counts on `stream`. */
int jaero_softbits_view(jaero_ctx *ctx, void **dev_softbits, void **dev_counts, int *capacity);
int jaero_discard_softbits(jaero_ctx *ctx, void *stream);

int jaero_read_status(jaero_ctx *ctx, int channel, jaero_status *st);
/* status log rows of 6 doubles [n, freq_est, freq_center, mse, ebno, signal] (JAERO_FLAG_STATUS_LOG) */
int jaero_read_status_log(jaero_ctx *ctx, int channel, double *rows, int caprows, int *nrows);
/* soft symbols rows of 3 doubles [re, im, mse] (JAERO_FLAG_CAPTURE_SYMBOLS) */
int jaero_read_symbols(jaero_ctx *ctx, int channel, double *rows, int caprows, int *nrows);

/* Burst kinds: rows of 3 doubles [absolute sample index (count of samples written before it), JAERO_EV_* kind, value],
 * oldest first, drained by the call.  The first row of every channel is the Plottables emission of setSettings. */
int jaero_read_events(jaero_ctx *ctx, int channel, double *rows, int caprows, int *nrows);

/* Batched K=7 r=1/2 {109,79} soft Viterbi (libcorrect semantics as used by JConvolutionalCodec).
 * jaero_viterbi_decode_soft: nblocks independent blocks of nsoft soft bytes each (0..255, 128 = erasure);
 *   = correct_convolutional_decode_soft per block; bits_out[b * (nsoft/2) + k] one byte per decoded bit
 *   (the first nsoft/2 - 6 are decoded data, the rest 0).
 * jaero_viterbi_continuous: = JConvolutionalCodec::Decode_Continuous for nstreams independent streams, one
 *   block of nsoft soft bytes each per call; the 62-byte overlap of each stream is kept in the ctx-less state
 *   buffer `overlap_state` (nstreams*64 bytes: bytes 0..61 = the kept soft bytes, byte 62 = how many are valid, 0 or
 *   62; zero it for a fresh stream).  nbits_out[s] receives the number of bits returned for stream s (nsoft/2, fewer
 *   on the first block of a stream, exactly as the reference).
 * Both take host pointers (is_device_ptr=0) or device pointers (1). */
int jaero_viterbi_decode_soft(int device, const uint8_t *soft, int nblocks, int nsoft, uint8_t *bits_out,
                              int is_device_ptr, void *stream);
int jaero_viterbi_continuous(int device, const uint8_t *soft, int nstreams, int nsoft, int paddinglength,
                             uint8_t *overlap_state, uint8_t *bits_out, int *nbits_out, int is_device_ptr, void *stream);

/* ---- Aero-L bit pipeline around the Viterbi (continuous P-channel path of AeroL::Decode, JAERO/aerol.cpp:1124-2039) ----
 * A jaero_aerol_ctx is a bank of nchannels AeroL objects in non-burst mode at one bit rate (600 / 1200 / 10500):
 *   AeroL(parent) + setSettings(fb,false)   JAERO/aerol.cpp:904-977,990-1072      jaero_aerol_create
 *   processDemodulatedSoftBits(QVector<short>)  JAERO/aerol.cpp:2077-2099         jaero_aerol_write (all channels at once; the soft
 *                                               bits can stay on the device: pass jaero_softbits_view's pointers, is_device_ptr = 1)
 *   the signal units Decode() checks and prints  JAERO/aerol.cpp:1583-1600          jaero_aerol_read_sus: rows of 16 int32
 *                                               [frame number, unit index k, 12 bytes (10 payload + CRC), crc_ok, frame-info word]
 *   DataCarrierDetect(bool) and the "Error short frame" notice  :1593-1596,1995-2010   jaero_aerol_read_events: rows of 3 int64
 *                                               [soft-bit index, kind (0 = DCD, 1 = short frame (value = its length), 2 = unique word), value]
 *   updateDCD() from the 1 s QTimer            JAERO/aerol.cpp:1109-1122          jaero_aerol_tick_dcd (call once per second of signal)
 * Of what follows a CRC-clean signal unit in the reference, the ISU / SSU reassembly and the ACARS header are here, off unless enabled
 * (jaero_aerol_isu_enable, below); message names, the joining of ACARS blocks and the plane database are text and control plane and stay with
 * the caller. */
typedef struct jaero_aerol_ctx jaero_aerol_ctx;
int jaero_aerol_create(int device, int nchannels, int fb, int max_softbits_per_write, int su_capacity, jaero_aerol_ctx **out);
void jaero_aerol_destroy(jaero_aerol_ctx *ctx);
/* soft[ch * stride + k], k < counts[ch] <= max_count <= stride; host pointers (copied) or device pointers.  Burst-mode banks read rows that are
 * 16-byte aligned (soft 16-byte aligned, stride a multiple of 8) eight entries per load and skip through inert stretches; other rows go bit by bit:
 * the same results, more slowly. */
int jaero_aerol_write(jaero_aerol_ctx *ctx, const int16_t *soft, const int *counts, int stride, int max_count, int is_device_ptr, void *stream);
int jaero_aerol_read_sus(jaero_aerol_ctx *ctx, int channel, int32_t *rows, int caprows, int *nrows);
int jaero_aerol_read_events(jaero_aerol_ctx *ctx, int channel, long long *rows, int caprows, int *nrows);
int jaero_aerol_tick_dcd(jaero_aerol_ctx *ctx, int *dcd_out /* optional [nchannels] */);
/* ---- burst mode: R / T channel packets (AeroL with setSettings(fb, burstmode = true), JAERO/aerol.cpp:996-1003,1062-1070) ----
 * The bank behind a burst demodulator bank (JAERO_KIND_BURST_OQPSK): unique word with tolerance 4 that has to come ~80 soft bits after
 * the demodulator's start-of-burst marker (JAERO/aerol.cpp:1192-1200), RTChannelDeleaveFECScram::update (JAERO/aerol.h:785-873: trial
 * decodes of the collected block at 2, 5, 8 .. 95 interleaver columns until the CRCs of an R packet or of a T packet's header and
 * signal units pass), end of signal after one second of bits.  At 600 / 1200 bps (behind JAERO_KIND_BURST_MSK): one detector, the word
 * within 250 soft bits of the marker, RTChannelDeleaveFECScram::updateMSK (aerol.h:631-782: R test at 5 blocks, the unit count read at 11,
 * the T packet decoded at the announced length), three seconds of bits.
 *   jaero_aerol_read_packets: rows of 16 int32 [packet number, chunk, 12 bytes (zero padded), total bytes of the packet, type]
 *       type 1 = R packet (20 bytes: 17 + CRC + the flush byte), 2 = T packet (6 header bytes incl. CRC, then 12 per signal unit)
 *   jaero_aerol_read_events additionally reports kind 3 = the " Bad R/T Packet" notice (JAERO/aerol.cpp:1289-1293,1531)
 * The reference drops the rest of the demodulator's current group of soft bits at the end of a signal; the bank re-derives the groups
 * from the stream (a marker is one entry, soft bits come in pairs, a group is complete at >= 32 entries after a pair).  The input is a burst
 * demodulator's output: a marker stands between pairs, never inside one (JAERO/burstoqpskdemodulator.cpp:546-585); for other streams the grouping,
 * and with it what is dropped at the end of a signal, is not the reference's. */
/* C channel (jaero_aerol_create with fb = 8400: AeroL::DecodeC aerol.cpp:2187-2502): jaero_aerol_read_sus rows are the three sub-band signal units of
 * a frame [frame, k, 12 bytes, crc_ok, 0]; jaero_aerol_read_voice rows are 304 bytes: uint32 frame number, then the 300 voice bytes
 * the reference hands to Voicesignal(data, hex). */
int jaero_aerol_read_voice(jaero_aerol_ctx *ctx, int channel, uint8_t *rows, int caprows, int *nrows);
int jaero_aerol_create_burst(int device, int nchannels, int fb, int max_softbits_per_write, int packet_row_capacity, jaero_aerol_ctx **out);
int jaero_aerol_read_packets(jaero_aerol_ctx *ctx, int channel, int32_t *rows, int caprows, int *nrows);
/* HIP-event time per kernel class since the last reset: which 0 = k_aerol_bits, 1 = Viterbi, 2 = k_aerol_post */
int jaero_aerol_profile_enable(jaero_aerol_ctx *ctx, int on);
int jaero_aerol_profile_read(jaero_aerol_ctx *ctx, int which, double *total_ms, int *launches, int reset);

/* ---- the data-carrier-detect wire: AeroL::DataCarrierDetect(bool) -> demodulator DCDstatSlot (JAERO/mainwindow.cpp:232-241) ----
 * jaero_aerol_link_dcd(ctx, bank) links an Aero-L bank to the demodulator bank that feeds it (bank = NULL: unlink).  The reference's direct
 * connection delivers an emission in the middle of writeData; a bank runs a whole write before the Aero-L bank sees its soft bits, so the link
 * is defined as the Qt adaptors of integration/qt behave, where soft bits are emitted after jaero_write returns:
 *   After every jaero_aerol_write and every jaero_aerol_tick_dcd on a linked handle, for each channel c < nchannels: if channel c made at
 *   least one DataCarrierDetect emission during that call, the bank's dcd of channel c becomes the value of the last one; if it made none,
 *   the bank's dcd is left as it is.
 * An emission is every `emit DataCarrierDetect(...)` of JAERO/aerol.cpp (:1120, :1607, :2008, :2025, :2383): what appends a kind-0 row to the
 * event log, whether the log had room for it or not.  :2008 fires at every unique word, not only on a change.  Emissions from before the link
 * was made (the constructor's `false` among them) are not replayed.  jaero_set_dcd keeps working on a linked bank and is overwritten by the
 * next emission.  The update is enqueued on the stream of the Aero-L call, behind its last kernel: no host round trip, no synchronisation.
 * Checks, in this order, before anything changes: null ctx (JAERO_EINVAL); bank on another device; channel counts differ; burst Aero-L bank
 * with a continuous bank or the reverse; the Aero-L bank's fb differs from the bank's; either side already linked to something else (all
 * JAERO_EINVAL); a burst bank (JAERO_ENOTSUP: the reference connects no slot of JAERO_KIND_BURST_OQPSK, mainwindow.cpp:234-237, and burst MSK
 * banks are not linked yet: only continuous banks -- MSK, OQPSK, the 8400 bps C channel -- are); a poisoned bank (JAERO_EHIP).
 * Streams: a linked jaero_aerol_write whose `stream` is not the stream of the bank's last jaero_write is JAERO_EINVAL and consumes nothing
 * (the chain's order -- bank write, then Aero-L write, on one stream -- satisfies it); jaero_aerol_tick_dcd uses the handle's last stream, and is
 * JAERO_EINVAL (nothing ticked) if the bank has written on another stream since.
 * Lifetime: jaero_destroy of a linked bank unlinks it first, jaero_aerol_destroy unlinks.  Unlinking synchronises once and makes the device's
 * dcd bits the bank's own.  While linked, a jaero_set_settings that would re-create the bank (another fb, Fs or FFT power, and every whole-bank
 * change of an 8400 bps bank) is JAERO_EINVAL and the bank stays as it was: unlink, change, link a matching Aero-L bank.  In-place changes
 * work as before.
 * Deliberately not here: emission-exact timing inside a write; burst banks. */
int jaero_aerol_link_dcd(jaero_aerol_ctx *ctx, jaero_ctx *bank);

/* ---- one-call reads of every channel ----
 * jaero_aerol_read_all hands over one output class of all channels.  With cnt_c the rows channel c holds and P_c = sum_{k <= c} cnt_k:
 * channel c is taken iff P_c <= caprows, so the taken channels are a prefix [0, taken).  Each taken channel's rows are copied, oldest first,
 * to rows + offsets[c] * rowbytes with offsets[c] = P_{c-1}; offsets[c] = offsets[taken] for c >= taken (offsets has nchannels + 1 entries);
 * *nchannels_taken = taken; *rows_pending = P_{nchannels-1} before the call (size a buffer with a caprows = 0 call).  A taken channel is left
 * as jaero_aerol_read_* with enough capacity leaves it (count 0, overflow bit of that class cleared); a channel not taken is not touched.
 * If a taken channel had its overflow bit set, everything is filled in and the call returns JAERO_EOVERFLOW, overflowed[c] = 1 saying where.
 * The rows are bit for bit the per-channel readers'.  Checks, in this order, before a device is touched: `what` is none of the classes
 * (JAERO_AEROL_MESSAGES is one only on a bank that has enabled a reassembly, jaero_aerol_isu_enable or jaero_aerol_rt_enable: with a null ctx or a bank that never enabled it is
 * refused here, as every value above JAERO_AEROL_VOICE was before that class existed), caprows < 0, null offsets / nchannels_taken, null rows with caprows > 0, null ctx (JAERO_EINVAL); then a class the bank's mode does not have gets
 * the per-channel reader's own error (SUS on a burst bank, PACKETS on any other: JAERO_ENOTSUP; VOICE on a bank that is not fb = 8400:
 * JAERO_EINVAL).  Synchronises the handle's last stream (twice).
 * jaero_aerol_profile2_read: as jaero_aerol_profile_read with which 0 .. 5; 3 = the kernels of jaero_aerol_read_all, 4 = the link kernel,
 * 5 = the reassembly kernel (jaero_aerol_isu_enable; on a burst bank jaero_aerol_rt_enable's).
 * jaero_read_all (below) is the same call for the demodulator bank's soft bits and logs: this paragraph defines both.
 * Deliberately not here: rows handed over in device memory. */
#define JAERO_AEROL_SUS 0      /* P and C banks: rows of 16 int32, as jaero_aerol_read_sus        */
#define JAERO_AEROL_PACKETS 1  /* burst banks:   rows of 16 int32, as jaero_aerol_read_packets    */
#define JAERO_AEROL_EVENTS 2   /* every bank:    rows of 3 int64,  as jaero_aerol_read_events     */
#define JAERO_AEROL_VOICE 3    /* C banks:       rows of 304 bytes, as jaero_aerol_read_voice     */
#define JAERO_AEROL_MESSAGES 4 /* P and burst banks that enabled their reassembly: rows of jaero_aerol_msg, as jaero_aerol_read_msgs; any other: JAERO_EINVAL */
int jaero_aerol_read_all(jaero_aerol_ctx *ctx, int what, void *rows, int caprows, int *offsets /* [nchannels + 1] */, int *nchannels_taken,
                         long long *rows_pending /* optional */, unsigned char *overflowed /* optional [nchannels] */);
int jaero_aerol_profile2_read(jaero_aerol_ctx *ctx, int which, double *total_ms, int *launches, int reset);
/* test hook: bytes of device memory the link, jaero_aerol_read_all, jaero_aerol_isu_enable and jaero_aerol_rt_enable have allocated for this bank so far (0 for a bank
 * that used none of them) */
long long jaero_aerol_debug_extra_bytes(const jaero_aerol_ctx *ctx);

/* ---- ISU user data and ACARS headers, reassembled on the device (ISUData::update JAERO/aerol.cpp:117-219, aerol.h:113-228; the header part of
 * ParserISU::parse aerol.cpp:340-470) ----
 * Off by default: a bank that never calls jaero_aerol_isu_enable allocates and launches what it did without it.  Continuous P-channel banks
 * (600 / 1200 / 10500 bps) only.  While enabled, each channel keeps one ISUData, updated with the 10 payload bytes d[0..9] of every CRC-clean
 * signal unit in stream order (aerol.cpp:1616-1943), whether or not the signal-unit log had room for the unit's row.  The definition, with the
 * reference's quirks (tests/isu_oracle.py restates it):
 *   Scratch item `a`: AESID, GESID, QNO, REFNO, SEQNO, NOOCT (NOOCTLESTINLASTSSU: user-data octets in the last SSU).  Zero at enable; it
 *     survives between units and is NOT cleared by a reset.
 *   List of items, ordered, at most 11: only an ISU ages it, the survivors' counts are distinct, an item leaves once its count exceeds 10.
 *   ISU, d[0] == 0x71: (1) count++ on every item, then every item with count > 10 is removed, in list order; (2) a.AESID = d[1..3] big-endian,
 *     a.GESID = d[4], a.QNO = d[5] >> 4, a.REFNO = d[5] & 15, a.SEQNO = d[6] & 63, a.NOOCT = d[7] >> 4, count = 0, user data = d[8..9];
 *     (3) the first item with equal (AESID, GESID, QNO, REFNO) is looked for -- none is found if a.NOOCT > 8; (4) found: overwritten in place,
 *     otherwise `a` is appended.
 *   SSU, (d[0] & 0xC0) == 0xC0: (1) only a.SEQNO = d[0] & 63, a.QNO = d[1] >> 4, a.REFNO = d[1] & 15 change; AESID, GESID and NOOCT stay what
 *     the last ISU left, so an SSU can only continue an item of the most recent ISU's aircraft, and behind an ISU with NOOCT > 8 every SSU is
 *     missing; (2) the first item with equal AESID and GESID, a.SEQNO + 1 == item.SEQNO, equal QNO and REFNO is looked for -- none is found if
 *     a.NOOCT > 8; (3) none: the SSU is "missing", nothing else changes; (4) otherwise item.SEQNO--; at 0 the bytes d[2 .. item.NOOCT + 1] are
 *     appended, the item is complete and a copy is emitted (it stays in the list with SEQNO 0); else d[2..9] are appended.  An SSU never
 *     touches a count.  (The test in (2) looks at a.NOOCT, not at the item's: an item appended with NOOCT > 8 can be found once a later ISU
 *     of the same aircraft has left a smaller a.NOOCT.  The reference then reads past the unit's ten bytes; here at most the eight bytes the
 *     unit has, d[2..9], are appended, which keeps nbytes <= 506.)
 *   Any other first byte: no effect.
 *   Reset (the list is cleared): at the short-frame notice (aerol.cpp:1995-1998, the kind-1 event of jaero_aerol_read_events) and at enable.
 *     (AeroL::setSettings resets it too; a bank's rate is fixed at create.)
 *   Emission: one jaero_aerol_msg per completed item, classified as ParserISU::parse does.  flags bit 0: AESID == 0, then no other bit.  Bit 1:
 *     the ACARS pattern, nbytes > 16, data[0] == data[1] == 0xFF, data[15] == 0x83 or 0x02.  With bit 1: bit 2 = text present (data[15] == 0x02),
 *     bit 3 = more to come (data[nbytes - 4] == 0x97), bit 4 = parity error (a byte of data[4..10], or with text a byte of data[16 .. nbytes - 5],
 *     has even parity), mode = data[3] & 0x7F, tak, label[0..1], bi = data[11..14] & 0x7F.  Without bit 1 those five bytes are 0.
 * jaero_aerol_isu_enable(ctx, msg_capacity): msg_capacity >= 1 enables with a log of that many rows per channel -- synchronises, allocates on
 * first use (about 6 KB per channel besides the log), clears the list, `a`, the log and the counters; 0 disables: later writes launch nothing
 * extra, the log stays readable.  Checks, in this order, before a device is touched: null ctx, msg_capacity < 0 (JAERO_EINVAL); a burst bank,
 * fb = 8400 (JAERO_ENOTSUP: DecodeC never calls ISUData; a burst bank's reassembly -- RISUData and the T packets' units, aerol.cpp:1395,1504-1513 --
 * is jaero_aerol_rt_enable, below).  An Aero-L bank has no poisoned state.
 * jaero_aerol_read_msgs: the per-channel reader, with jaero_aerol_read_sus's semantics (overflow bit 8 of the channel: messages completed while
 * the log was full were dropped; JAERO_EINVAL on a bank that never enabled).  JAERO_AEROL_MESSAGES of jaero_aerol_read_all: every channel's.
 * jaero_aerol_isu_stats: per channel four counters since enable -- ISU updates, SSU updates, missing SSUs, completed messages -- counted
 * whether or not the log had room.  Null ctx / stats, a bank that never enabled: JAERO_EINVAL. */
typedef struct jaero_aerol_msg
{
    int32_t frame, k;      /* as the signal-unit rows' frame number and unit index: the unit that completed the message (burst banks: the packet
                              number, and the unit's index inside the T packet; 0 for an R packet) */
    uint32_t aesid;
    uint8_t gesid, qno, refno, nooct;
    uint16_t nbytes;       /* 2 .. 506; rows of an R channel (flags bit 5): 0 .. 33 */
    uint16_t flags;        /* bits 0-4 as above; burst banks add bit 5 (32) = from RISUData, bit 6 (64) = an R signalling-information unit */
    uint8_t mode, tak, label[2], bi, pad[7];
    uint8_t data[512];     /* the raw user data, zero padded */
} jaero_aerol_msg;         /* 544 bytes */
int jaero_aerol_isu_enable(jaero_aerol_ctx *ctx, int msg_capacity);
int jaero_aerol_read_msgs(jaero_aerol_ctx *ctx, int channel, void *rows /* jaero_aerol_msg[caprows] */, int caprows, int *nrows);
int jaero_aerol_isu_stats(jaero_aerol_ctx *ctx, long long *stats /* [nchannels][4] */);

/* ---- R / T user data of a burst bank, reassembled on the device (RISUData::update JAERO/aerol.cpp:6-113, aerol.h:135-146,231-243; ISUData::update
 * behind the T packets' units, aerol.cpp:1488-1516; ParserISU::parse with downlink = burstmode, aerol.cpp:1397,1510) ----
 * Off by default: a burst bank that never calls jaero_aerol_rt_enable allocates and launches what it did without it.  Burst banks at 600 / 1200 /
 * 10500 bps.  While enabled, each channel keeps one ISUData and one RISUData, independent of each other, updated in stream order with every
 * packet the search accepts, whether or not the packet log had room for its rows.  There is no short-frame reset in burst mode (aerol.cpp:1993
 * guards it with !burstmode): the only reset is at enable.  The definition, with the reference's quirks (tests/rt_isu_oracle.py restates it):
 *   T packet (type 2, info bytes f[0 ..)): every unit k < numberofsus goes to ISUData::update as defined above, in packet order, with
 *     d = f[6 + 12 k .. 6 + 12 k + 9].  numberofsus = 1 + (blockptr - 320) / 192 at 10500 bps (C division: 0 for the two-column block), where
 *     every unit is CRC-clean by the packet test; = targetSUSize at 600 / 1200 bps, where AeroL makes no CRC test of its own: a unit whose CRC fails
 *     is fed all the same (aerol.h:732-766 counts, never rejects), and the block holds targetSUSize + 1 units, so the last unit sent is never looked at.
 *   R packet (type 1, 17 info bytes d[0..16]): only with d[1] & 0x08 is it user data and goes to RISUData::update; any other R packet changes nothing.
 *     (1) Ageing, on every update: count++ on every item, then every item with count > 10 is removed, in list order; so the list holds at most 11
 *         items and the survivors' counts are distinct.
 *     (2) The scratch item is cleared, then SEQINDICATOR = d[0] >> 4, SUTYPE = d[0] & 15, QNO = d[1] >> 4, REFNO = d[1] & 7,
 *         AESID = d[2..4] big-endian, GESID = d[5].
 *     (3) The first item with equal (GESID, AESID, QNO, REFNO) is looked for -- none is found if SUTYPE is 0 or above 11, so such a unit appends
 *         a fresh item (empty user data, filledarray 0) every time, as does a unit whose key is not in the list.  The item's count becomes 0.
 *     (4) SEQINDICATOR 1 -> (total, index) = (1, 0); 2, 3 -> (2, 0), (2, 1); 4, 5, 6 -> (3, 0), (3, 1), (3, 2); anything else (0, 0): total 0 never
 *         completes.  bytes = SUTYPE for SUTYPE 1 .. 11, else 0.  thisnum = 11 total - 11 + bytes.
 *     (5) When thisnum > 0: empty user data is sized to thisnum; user data longer than thisnum is cut to it; shorter user data is not grown by this step.
 *     (6) SUTYPE 15 (a signalling-information unit): the user data is cleared.  Any other SUTYPE: d[6 .. 6 + bytes) is written at 11 index, then
 *         filledarray |= 1 << index.
 *     (7) Complete: SUTYPE 15, or (filledarray, total) in {(7, 3), (3, 2), (1, 1)}.  A completed item is copied out and REMOVED from the list (ISUData
 *         keeps its item).
 *     Two corners the reference leaves to chance are decided here: a write past the user data's end grows it to reach (Qt's QByteRef::operator= ->
 *     expand, qbytearray.h:528-530; followed); and the bytes a resize or expand adds that no unit has written are indeterminate in the reference:
 *     they are 0 here.
 *   Emission: one jaero_aerol_msg per completed item, classified exactly as above (flags bits 0-4).  frame = the packet's number (row[0] of its rows
 *     in jaero_aerol_read_packets), k = the index of the T packet's unit that completed the message, 0 for an R packet.  Two origin bits are set
 *     whatever the classification says: bit 5 (32) the row comes from RISUData; bit 6 (64) it is an R signalling-information unit (nbytes 0).  R rows:
 *     qno = d[1] >> 4, refno = d[1] & 7, nooct = 0, nbytes 0 .. 33.
 * jaero_aerol_rt_enable(ctx, msg_capacity): msg_capacity >= 1 enables with a log of that many rows per channel -- synchronises, allocates on first
 * use (about 6.6 KB per channel besides the log), clears both lists, both scratch items, the log, its overflow bit and the counters; 0 disables:
 * later writes launch nothing extra, the log stays readable.  Checks, in this order, before a device is touched: null ctx, msg_capacity < 0
 * (JAERO_EINVAL); a bank that is not a burst bank -- a P bank, fb = 8400 -- (JAERO_ENOTSUP).  jaero_aerol_isu_enable on a burst bank stays
 * JAERO_ENOTSUP and jaero_aerol_isu_stats on one JAERO_EINVAL.
 * The readers are jaero_aerol_read_msgs and JAERO_AEROL_MESSAGES of jaero_aerol_read_all, as on a P bank (overflow bit 8; JAERO_EINVAL on a bank
 * that never enabled).
 * jaero_aerol_rt_stats: per channel eight counters since enable, counted whether or not a log had room -- T path: ISU updates, SSU updates, missing
 * SSUs, completed messages; R path: user-data packets fed, items newly appended, completed messages (signalling-information units among them),
 * signalling-information units.  Null ctx / stats, a bank that never enabled: JAERO_EINVAL. */
int jaero_aerol_rt_enable(jaero_aerol_ctx *ctx, int msg_capacity);
int jaero_aerol_rt_stats(jaero_aerol_ctx *ctx, long long *stats /* [nchannels][8] */);

/* ---- one-call reads of every channel of a demodulator bank ----
 * jaero_read_all is jaero_aerol_read_all (above: the prefix rule P_c <= caprows, offsets, *nchannels_taken, *rows_pending, the caprows = 0 sizing
 * call, overflowed / JAERO_EOVERFLOW, taken channels left as the per-channel reader leaves them, others untouched) for the demodulator bank's four
 * output classes, with cnt_c = the rows jaero_read_* of that class would hand over for channel c with unlimited capacity.  For the soft bits of a
 * burst bank that is what has been emitted: the pending tail (the current, incomplete group) stays with the channel, moved to the front of its
 * buffer, exactly as jaero_read_softbits leaves it; the -1 start-of-burst markers are handed over in place.  Overflow bits: 1 soft bits, 2 symbols,
 * 4 status log / events.  Rows are bit for bit the per-channel readers'.  Checks, in this order, before a device is touched: `what` is none of the
 * four, caprows < 0, null offsets / nchannels_taken, null rows with caprows > 0, null ctx (JAERO_EINVAL); a poisoned bank (JAERO_EHIP); then a
 * class the bank does not have gets the per-channel reader's own error (STATUS_LOG on a burst bank, EVENTS on a continuous one: JAERO_ENOTSUP; a
 * log or symbol buffer not enabled at create: JAERO_EINVAL).  Synchronises the bank's last stream (twice).  Works on a bank linked by
 * jaero_aerol_link_dcd and touches no flags.  jaero_read_softbits_all keeps its dense form (and JAERO_ENOTSUP on burst banks).
 * jaero_read_status_all: st[c] is bit for bit what the per-channel status call returns for channel c, for every kind: one kernel launch over all
 * channels, one copy, one synchronisation.  Null ctx / st: JAERO_EINVAL; a poisoned bank: JAERO_EHIP.
 * Their device scratch is allocated by the first call (a bank that never calls them allocates and launches what it always did) and belongs to the
 * bank object: after a jaero_set_settings that re-creates the bank behind the handle the next call allocates afresh.
 * jaero_profile2_read: as jaero_profile_read with which 0 .. 5; 5 = the kernels of these two calls (totals survive a rate change as the others). */
#define JAERO_BANK_SOFTBITS 0   /* every kind: rows of one int16, as jaero_read_softbits (burst: only what has been emitted; the -1 markers stay) */
#define JAERO_BANK_STATUS_LOG 1 /* continuous kinds, JAERO_FLAG_STATUS_LOG: rows of 6 doubles, as jaero_read_status_log */
#define JAERO_BANK_EVENTS 2     /* burst kinds: rows of 3 doubles, as jaero_read_events */
#define JAERO_BANK_SYMBOLS 3    /* JAERO_FLAG_CAPTURE_SYMBOLS: rows of 3 doubles, as jaero_read_symbols */
int jaero_read_all(jaero_ctx *ctx, int what, void *rows, int caprows, int *offsets /* [nchannels + 1] */, int *nchannels_taken,
                   long long *rows_pending /* optional */, unsigned char *overflowed /* optional [nchannels] */);
int jaero_read_status_all(jaero_ctx *ctx, jaero_status *st /* [nchannels] */);
int jaero_profile2_read(jaero_ctx *ctx, int which, double *total_ms, int *launches, int reset);
/* test hooks: device bytes the two calls have allocated for the bank so far (0 for a bank that never used them; -1 for a null ctx); per channel, the
 * soft bits held and (burst banks) how many of them are not yet emitted (synchronises, changes nothing) */
long long jaero_debug_read_all_bytes(const jaero_ctx *ctx);
int jaero_debug_softbit_counts(jaero_ctx *ctx, int *cnt, int *pending);

/* ---- batched ingest: the recAudio(QByteArray, quint32 sampleRate) -> dataReceived slot of every channel
 * (JAERO/zmq_audioreceiver.cpp:40-79 -> oqpskdemodulator.cpp:686-693, mskdemodulator.cpp:528-537) in front of one bank.
 * Messages arrive per channel, any size (<= 192000 bytes are taken, as the reference's receive buffer), any order;
 * jaero_ingest_pump turns what all channels have in common into jaero_write calls of chunk_samples from pinned memory.
 *   jaero_ingest_push   = dataReceived of one channel.  Returns 0; JAERO_W_RATE (> 0) when sample_rate != Fs for the OQPSK
 *                         kinds (the reference only logs "Sample rate not supported by demodulator" and demodulates anyway);
 *                         JAERO_ENOTSUP for the MSK kinds (the reference would re-apply its settings at the new rate; a bank
 *                         shares Fs); JAERO_EOVERFLOW when the channel's FIFO cannot take the message (nothing queued).
 *   jaero_ingest_queued = samples queued for `channel`, or (channel = -1) the count every channel has in common
 *   jaero_ingest_pump   = flush != 0 also writes the common remainder below one chunk; *chunks = jaero_write calls made
 *   jaero_ingest_stats  = [rate warnings, samples refused, samples per channel written]
 * The transport (sockets) is the caller's; nothing here blocks except on the staging buffer two chunks back. */
typedef struct jaero_ingest jaero_ingest;
int jaero_ingest_create(jaero_ctx *bank, int chunk_samples, int capacity_samples, jaero_ingest **out);
void jaero_ingest_destroy(jaero_ingest *ing);
int jaero_ingest_push(jaero_ingest *ing, int channel, const void *pcm_bytes, int nbytes, unsigned sample_rate);
int jaero_ingest_queued(const jaero_ingest *ing, int channel);
int jaero_ingest_pump(jaero_ingest *ing, int flush, void *stream, int *chunks);
int jaero_ingest_stats(const jaero_ingest *ing, long long *three);

/* ---- wideband I/Q channeliser (the other half): one capture in, the per-channel int16 audio of a whole bank out (at 48 kHz,
 * or at the 24 / 12 kHz of the reference's default MSK set-ups), on the device.  No counterpart in the reference (it has only the receiving end of per-channel audio); this text is the definition, and
 * tests/chan_oracle.py implements it literally in numpy.  A fast-convolution filter bank of fixed geometry: transform length N = 16384, hop
 * Hp = 8192 input samples, D = decim in {16, 32, 64, 128, 256} the TOTAL decimation from the capture to the output, out_rate in {48000, 24000, 12000}
 * the output's rate (capture rate Fs_in = out_rate D; out_rate is a label: it enters no arithmetic below and exists so that jaero_chan_feed
 * can check the bank), M = N / D bins per channel, Mo = M / 2 output samples per hop and channel.  jaero_chan_create is the 48 kHz channeliser of
 * D <= 64; jaero_chan2_create takes every D and out_rate.
 *   input      interleaved int16 I, Q; x[n] = I[n] + j Q[n], n counted from create, x[n] = 0 for n < 0
 *   taps       real prototype low-pass h[0 .. ntaps), 1 <= ntaps <= 8193, at the capture rate; G = DFT_N(h, zero padded), formed on the host
 *   channel c  tune  (uint32, centre = tune Fs_in / 2^32, read as a SIGNED 32-bit number t: negative centres exist),
 *              audio (uint32, audio offset = audio out_rate / 2^32), gain g > 0.
 *              b = (t + 2^17) >> 18 (arithmetic: the nearest bin), rho = t - b 2^18, w = (audio - rho D) mod 2^32.  Integer arithmetic only:
 *              no phase accumulator, no per-channel state besides these three numbers.
 *   block p    exists once (p + 1) Hp samples have been written.  s_p[i] = x[(p - 1) Hp + i], i < N; X_p = DFT_N(s_p) (forward), shared by
 *              all channels.  Y[q] = X_p[(b + q) mod N] G[q mod N], -M/2 <= q < M/2; w[r] = (1 / N) sum_q Y[q] e^(+j 2 pi q r / M), r < M;
 *              v[p Mo + r - Mo] = w[r] (-1)^(b (p - 1)) for Mo <= r < 2 Mo (the sign keeps the bin shift's phase continuous in time)
 *   output     y[m] = sat16(rint(g Re(v[m] e^(j 2 pi ((w m) mod 2^32) / 2^32)))), m the absolute (64-bit) output index, rint = round half to
 *              even, sat16 = clamp to [-32768, 32767]
 * i.e. a band-pass at the grid frequency nearest the requested centre (at most Fs_in / (2 N) off it: 23 .. 94 Hz at the capture rates of 48000 x 16 .. 64), an exact shift of the
 * requested centre to the audio offset, the real part.  After T input samples exactly floor(T / Hp) Mo samples per channel have been
 * produced, however the writes were cut; the rest of the input waits in the handle (latency below one hop).
 *   jaero_chan_create    arguments are checked before a device is looked for (JAERO_EINVAL: decim not 16 / 32 / 64, nchannels < 1, ntaps
 *                        outside [1, 8193], max_write_iq < 1, null pointers, a gain that is not finite and positive, a tap that is not
 *                        finite), then JAERO_ENODEV off gfx950 (no CPU fallback).  ch: nchannels entries.  max_write_iq: most I/Q pairs per write.
 *   jaero_chan2_create   the same checks in the same order with decim in {16, 32, 64, 128, 256} and, behind decim, out_rate in {48000, 24000,
 *                        12000}; jaero_chan_create(.., decim, ..) = jaero_chan2_create(.., decim, 48000, ..) behind its own check of decim.  The
 *                        handle is the same jaero_chan: every call below works on it.
 *   jaero_chan_write     niq I/Q pairs (2 niq int16; host or device pointer), enqueued on `stream`; *nout = samples per channel this write
 *                        produced (a multiple of Mo, at most (max_write_iq / Hp + 1) Mo; 0 when no block was completed).  niq < 0 or
 *                        niq > max_write_iq: JAERO_EINVAL, nothing consumed.  An error behind the first launch that advances the state
 *                        poisons the handle as a bank's write does: JAERO_EHIP from every later call but jaero_chan_destroy.
 *   jaero_chan_pcm_view  the last write's output on the device: int16 [nchannels][nsamples], compact (row stride = nsamples) -- what
 *                        jaero_write takes with JAERO_PCM_CHANNEL_MAJOR, is_device_ptr = 1.  Valid until the next write; ordered on the
 *                        write's stream.
 *   jaero_chan_read_pcm  the same on the host: synchronises, then copies row c to dst + c * cap_per_channel; JAERO_EINVAL if
 *                        cap_per_channel is below the last write's *nout.
 *   jaero_chan_retune    replaces (tune, audio, gain) of one channel from the first output sample of the next write on (synchronises first:
 *                        writes already enqueued keep the old words).  The phase is absolute in m, so nothing else is carried.
 *   jaero_chan_feed      = jaero_chan_write followed, when *nout > 0, by jaero_write(bank, that output, *nout, JAERO_PCM_CHANNEL_MAJOR, 1,
 *                        stream): no host copy, no synchronisation.  JAERO_EINVAL, before anything advances, for a bank on another device,
 *                        with another channel count, with a channel whose Fs is not the handle's out_rate, or whose max_write_samples is below (max_write_iq / Hp + 1) Mo.
 *   jaero_chan_profile_* HIP-event time per kernel since the last reset: which 0 = forward transform (k_chan_fwd), 1 = per-channel
 *                        synthesis (k_chan_synth).
 * Deliberately not here: sockets and SDR drivers, other decimations, other N or hop, per-channel filters,
 * burst and OQPSK banks at other rates than 48 kHz (the reference has none either), the multi-GPU fan-out of a capture (every rank creates a
 * channeliser over its shard and is handed the same I/Q), automatic gain control inside the synthesis (it would change the output's
 * definition: the survey below measures, the caller sets the gains), carrier finding on the device (jaero_amd.channeliser.find_carriers is
 * host numpy over the surveyed spectrum), modulation recognition beyond what the bit rate implies (the rate lines below measure that). */
typedef struct jaero_chan jaero_chan;
typedef struct jaero_chan_channel { uint32_t tune, audio; double gain; } jaero_chan_channel;
int jaero_chan_create(int device, int decim, int nchannels, const jaero_chan_channel *ch, const double *taps, int ntaps, int max_write_iq,
                      jaero_chan **out);
int jaero_chan2_create(int device, int decim, int out_rate, int nchannels, const jaero_chan_channel *ch, const double *taps, int ntaps,
                       int max_write_iq, jaero_chan **out);
void jaero_chan_destroy(jaero_chan *c);
int jaero_chan_write(jaero_chan *c, const int16_t *iq, int niq, int is_device_ptr, void *stream, int *nout);
int jaero_chan_pcm_view(jaero_chan *c, void **dev_pcm, int *nsamples);
int jaero_chan_read_pcm(jaero_chan *c, int16_t *dst, int cap_per_channel, int *nsamples);
int jaero_chan_retune(jaero_chan *c, int channel, const jaero_chan_channel *ch);
int jaero_chan_feed(jaero_chan *c, jaero_ctx *bank, const int16_t *iq, int niq, int is_device_ptr, void *stream, int *nout);
int jaero_chan_profile_enable(jaero_chan *c, int on);
int jaero_chan_profile_read(jaero_chan *c, int which, double *total_ms, int *launches, int reset);

/* ---- capture front end of the channeliser: SDR captures in their native formats and rates.  A handle from jaero_chan3_create takes cs16, cu8,
 * cs8 or cf32 I/Q at an integer rate fs_in, shifts the capture's centre by an exact integer phase word and resamples by the exact rational
 * ratio to the channeliser's rate Fs_c = out_rate D, on the device; everything behind that (synthesis, survey, feed, retune, pcm_view) is the
 * channeliser's above, unchanged.  This text is the definition; tests/chan_capture_oracle.py implements it literally in numpy.
 *   convert    x[n] in int16 LSB units, exact in fp64, per component v:  CS16 x = v;  CU8 x = (2 v - 255) 128;  CS8 x = 256 v;
 *              CF32 x = (double)v 32768, a component that is not finite is 0.  n counted from create (64-bit), x[n] = 0 for n < 0.
 *   mix        x'[n] = x[n] e^(j 2 pi ((shift n) mod 2^32) / 2^32), the phase read as a signed word as the synthesis reads its own;
 *              shift == 0: x' = x exactly, no multiplication happens.  (shift = cycles per input sample x 2^32; read as signed: either way.)
 *   resample   L / Mr = Fs_c / fs_in in lowest terms; only when L != 1 or Mr != 1.  For the staged index m (64-bit, from create):
 *              n_m = floor(m Mr / L), phi_m = (m Mr) mod L, z[m] = sum_{j = 0 .. K - 1} h[phi_m + j L] x'[n_m - j]: ascending j from 0.0, real
 *              and imaginary parts summed separately, every product and every sum rounded once.  z[m] exists once n_m <= T - 1: after T
 *              input samples exactly ceil(T L / Mr) staged samples exist, however the writes were cut.  h = rtaps[0 .. L K), K =
 *              taps_per_phase; jaero_amd.channeliser.design_resampler(fs_in, Fs_c, K, beta) is the design the tests use: n = L K,
 *              fc = 0.5 min(fs_in, Fs_c) / (fs_in L), h[i] = 2 fc sinc(2 fc (i - (n - 1) / 2)) kaiser(n, beta), scaled to sum h = L.
 *              The group delay (L K - 1) / (2 L fs_in) seconds is not compensated.  With L = Mr = 1, z = x'.
 *   channelise z takes the place of x in the channeliser's definition, in fp64 (never re-quantised).  Tune words are relative to Fs_c, after
 *              the shift.  After T input samples floor(ceil(T L / Mr) / Hp) Mo samples per channel have been produced.
 * Everything is a function of absolute indices only: staged samples and int16 output are bit-identical however the writes are cut.
 *   jaero_chan3_create       returns the same jaero_chan.  All arguments are checked before a device is looked for, JAERO_EINVAL in this
 *                            order: out null; cap null; unknown format; fs_in < 1; (with Fs_c = out_rate decim, where both are >= 1:)
 *                            L > 1024; fs_in > 8 Fs_c or Fs_c > 8 fs_in; (rates differ:) taps_per_phase outside 1 .. 64, rtaps null, a
 *                            resampler tap that is not finite; then jaero_chan2_create's own checks in its order; then a max_write_iq whose
 *                            ceil(max_write_iq L / Mr) + 1 + 2 Hp staged samples reach 2^31; then JAERO_ENODEV off gfx950 (no CPU fallback).  max_write_iq counts CAPTURE samples; a write completes at most
 *                            (ceil(max_write_iq L / Mr) + 1) / Hp + 1 blocks, and jaero_chan_feed / jaero_chan3_feed ask the bank for
 *                            that many times Mo as max_write_samples.
 *   jaero_chan3_write / _feed  jaero_chan_write / jaero_chan_feed with niq raw pairs in the handle's format.  They work on every handle: on
 *                            one from the older creates they forward to the old calls.  jaero_chan_write / jaero_chan_feed work on a
 *                            capture handle only when its format is JAERO_IQ_CS16; otherwise JAERO_EINVAL, nothing consumed.
 *   jaero_chan3_read_staged  synchronises, then copies what the last write staged: *npairs (re, im) pairs, the first being z[*first_index].
 *                            A reader (tests rest on it); JAERO_EINVAL on a handle without a capture front end or when cap_pairs is too small.
 *   jaero_chan3_profile_read HIP-event time since the last reset: which 0 = the staging kernel (k_capture_stage), 1 = the forward transform
 *                            over the fp64 history (k_capture_fwd); switched by jaero_chan_profile_enable.  jaero_chan_profile_read's
 *                            which = 0 stays k_chan_fwd (never launched by a capture handle), 1 the synthesis of either kind of handle.
 * Poisoning, stream ordering, retune, survey and pcm_view are the channeliser's.  Deliberately not here: real-valued (non-I/Q) captures, rates
 * whose reduced L exceeds 1024, ratios beyond 8, file containers (WAV, SigMF), SDR drivers, compensation of the resampler's delay. */
#define JAERO_IQ_CS16 0   /* int16 I, Q                       x = v                  */
#define JAERO_IQ_CU8  1   /* uint8 I, Q (offset binary)       x = (2 v - 255) * 128  */
#define JAERO_IQ_CS8  2   /* int8 I, Q                        x = v * 256            */
#define JAERO_IQ_CF32 3   /* float I, Q, full scale +-1.0     x = (double)v * 32768; a component that is not finite is 0 */
typedef struct jaero_capture {
    int format;            /* JAERO_IQ_*                                                                  */
    int fs_in;             /* capture rate, Hz                                                            */
    uint32_t shift;        /* centre shift, cycles per input sample * 2^32 (signed reading: either way)   */
    int taps_per_phase;    /* K, 1 .. 64; ignored when fs_in == out_rate * decim                          */
    const double *rtaps;   /* resampler prototype h[0 .. L K), NULL when fs_in == out_rate * decim        */
} jaero_capture;
int jaero_chan3_create(int device, const jaero_capture *cap, int decim, int out_rate, int nchannels, const jaero_chan_channel *ch,
                       const double *taps, int ntaps, int max_write_iq, jaero_chan **out);   /* returns the same jaero_chan */
int jaero_chan3_write(jaero_chan *c, const void *iq, int niq, int is_device_ptr, void *stream, int *nout);
int jaero_chan3_feed(jaero_chan *c, jaero_ctx *bank, const void *iq, int niq, int is_device_ptr, void *stream, int *nout);
int jaero_chan3_read_staged(jaero_chan *c, double *reim, int cap_pairs, int *npairs, long long *first_index);
int jaero_chan3_profile_read(jaero_chan *c, int which, double *total_ms, int *launches, int reset); /* 0 = staging kernel, 1 = forward transform */

/* ---- survey of a channeliser's capture: where the carriers are and how strong each channel is, measured on the device from the forward
 * transforms X_p every write leaves behind (the notation is the channeliser's above).  Off at create; while off, a write launches and
 * allocates nothing more than before.  This text is the definition; tests/chan_survey_oracle.py implements it literally in numpy.
 *   spectrum   (Welch, the Hann window applied in the frequency domain)
 *              H_p[k] = X_p[k] / 2 - (X_p[(k - 1) mod N] + X_p[(k + 1) mod N]) / 4;   S[k] = sum_p |H_p[k]|^2, k < N, over every block
 *              completed since the spectrum was enabled or reset, added in ascending p.  S[k] / (nblocks N^2 3 / 8) is LSB^2 per bin and
 *              sums to the mean |x|^2 of a stationary input.
 *   level      E_c = sum_p sum_{-M/2 <= q < M/2} |X_p[(b_c + q) mod N] G[q mod N] / N|^2 over the n_c blocks completed since the levels
 *              were enabled or reset, or since a retune last changed channel c's TUNE word (b changes: sum and count start again with the
 *              next write); a retune that changes only audio or gain keeps both.  E_c / n_c is the mean square of the channel's complex
 *              output sample w[r] before sign, rotation and gain (Parseval over the M-point transform, both halves of the circular block),
 *              so the int16 output at gain g has an RMS of about g sqrt(E_c / (2 n_c)).
 *   determinism  both sums are independent of how the writes were cut, bit for bit: a block's terms are formed by the same instructions
 *              whatever the launch shape, the reduction over q has a fixed shape, terms join the running sum strictly in block order,
 *              and there are no floating-point atomics.
 *   jaero_survey_enable        what: bit 0 spectrum, bit 1 levels, 0 = off (JAERO_EINVAL for bits outside 0..3).  Synchronises, allocates what
 *                              is enabled for the first time, clears the sums and counts of what is enabled.
 *   jaero_survey_reset         synchronises, then clears the sums and counts of what is enabled.
 *   jaero_survey_read_psd      synchronises on the handle's last stream; sums[16384] = S, *nblocks = the blocks in it.
 *   jaero_survey_read_levels   the same for sums[nchannels] = E_c, nblocks[nchannels] = n_c.  Reading a part that is not enabled: JAERO_EINVAL.
 *   jaero_survey_profile_read  HIP-event time since the last reset: which 0 = k_chan_psd, 1 = k_chan_level; switched by
 *                              jaero_chan_profile_enable.  A launch that also serves the activity below (spectrum + peak, levels + block
 *                              statistics: one fused launch each) is timed once, under the activity's slot, and does not count here.
 *   jaero_chan2_retune_all     jaero_chan_retune of every channel (ch: nchannels entries) behind one synchronisation, with one copy: the
 *                              call that applies surveyed centres and gains to a bank.  Every gain is checked before anything changes;
 *                              a channel's level restarts by the same rule.
 * Null arguments: JAERO_EINVAL.  A poisoned handle: JAERO_EHIP; a HIP failure inside the survey's launches poisons the handle as any other
 * failure inside a write. */
int jaero_survey_enable(jaero_chan *c, int what);
int jaero_survey_reset(jaero_chan *c);
int jaero_survey_read_psd(jaero_chan *c, double *sums, long long *nblocks);
int jaero_survey_read_levels(jaero_chan *c, double *sums, long long *nblocks);
int jaero_survey_profile_read(jaero_chan *c, int which, double *total_ms, int *launches, int reset);
int jaero_chan2_retune_all(jaero_chan *c, const jaero_chan_channel *ch);

/* ---- activity: the second, independent part of the survey.  The survey's two measurements are means over every block, so a carrier that
 * is on in 5 % of the blocks is diluted by 13 dB in S and its level is low by the duty cycle.  The activity keeps the EXTREMES and the
 * DISTRIBUTION of the same per-block terms instead of their sum: where the burst channels of a capture are, how strong a burst is and how
 * often a channel is on.  Measured on the device behind every write (it hangs off the same place as the survey, so it works on every
 * handle, jaero_chan3_create's included), under the survey's determinism rules: a function of absolute block indices only, no
 * floating-point atomics, bit-identical however the writes are cut.  Off at create; a handle that never enables it allocates and launches
 * nothing more than before.  Notation: the channeliser's and the survey's above.  This text is the definition;
 * tests/chan_activity_oracle.py implements it literally in numpy.
 *   peak-hold spectrum
 *              P[k] = max_p |H_p[k]|^2, k < N, over every block completed since the part was enabled or reset; 0 before the first block.
 *              |H_p[k]|^2 is formed by exactly the instructions the spectrum uses: after one block with both parts on, P == S bit for
 *              bit.  P[k] / (N^2 3 / 8) is LSB^2 per bin, the spectrum's unit.
 *   block statistics, per channel c
 *              e_{c,p} = sum_{-M/2 <= q < M/2} |X_p[(b_c + q) mod N] G[q mod N] / N|^2: the term the level adds for block p, formed exactly
 *              as the level forms it (same products, same 16-lane partial sums, same xor butterfly): after one block with levels on too,
 *              emax_c == emin_c == E_c bit for bit.  The statistics run over the n_c blocks since the part was enabled or reset, or since a
 *              retune last changed channel c's TUNE word (the level's restart rule; a retune that changes only audio or gain keeps
 *              everything):
 *              emax_c = max_p e_{c,p};  when_c = the smallest absolute block index p (counted from create, as blocks_done counts) at which
 *              the maximum is reached;  emin_c = min_p e_{c,p};  hist_c[i], i < 64 = the number of blocks with bin(e_{c,p}) = i, uint32;
 *              bin(e) = min(63, max(0, ilogb(e) + 32)), bin(0) = 0: each bin is one binary order of magnitude (3.01 dB), an integer
 *              function of the fp64 exponent, no logarithm.  With n_c = 0: emax = 0, emin = +inf, when = -1, hist all zero.
 *   jaero_activity_enable      what: JAERO_ACT_PEAK | JAERO_ACT_BLOCKS, 0 = off (JAERO_EINVAL for bits outside 0..3, checked before the null
 *                              ctx as jaero_survey_enable does).  Synchronises, allocates what is enabled for the first time (the
 *                              |G|^2 / N^2 table too when the levels never built it), clears what is enabled.
 *   jaero_activity_reset       synchronises, then clears what is enabled.  It does not touch the survey, nor jaero_survey_reset the activity.
 *   jaero_activity_read_peak   synchronises on the handle's last stream; peak[16384] = P, *nblocks = the blocks in it.
 *   jaero_activity_read_blocks the same for emax, emin, when, nblocks (nchannels entries each) and hist ([nchannels][JAERO_ACT_BINS], may be
 *                              NULL).  Reading a part that is not enabled: JAERO_EINVAL.
 *   jaero_activity_profile_read HIP-event time since the last reset: which 0 = k_chan_psd launches that keep the peak, 1 = k_chan_level
 *                              launches that take the block statistics; switched by jaero_chan_profile_enable.  The spectrum and the
 *                              peak are kept by one launch over one pass of the three loads, the levels and the statistics by one launch
 *                              over one walk of the channels' bins; such a fused launch is timed once, here, and not under
 *                              jaero_survey_profile_read.
 *   jaero_chan_retune, jaero_chan2_retune_all restart a moved channel's block statistics together with its level.
 * Null arguments: JAERO_EINVAL before a device is touched.  A poisoned handle: JAERO_EHIP; a HIP failure inside the activity's launches
 * poisons the handle as any other failure inside a write.  Deliberately not here: thresholds or detection decisions on the device (the
 * histogram and the extremes are the measurement; jaero_amd.channeliser.duty_cycle and find_carriers decide in numpy), a time series of
 * block levels, modulation recognition (the bit rate is measured by the rate lines below). */
#define JAERO_ACT_PEAK 1
#define JAERO_ACT_BLOCKS 2
#define JAERO_ACT_BINS 64
int jaero_activity_enable(jaero_chan *c, int what);
int jaero_activity_reset(jaero_chan *c);
int jaero_activity_read_peak(jaero_chan *c, double *peak, long long *nblocks);
int jaero_activity_read_blocks(jaero_chan *c, double *emax, double *emin, long long *when, long long *nblocks, unsigned *hist);
int jaero_activity_profile_read(jaero_chan *c, int which, double *total_ms, int *launches, int reset);

/* ---- splitter: one capture into several banks at their own rates.  A jaero_chan produces one output rate for one bank; a capture that holds
 * 10.5 k and 8400 bps carriers (48 kHz) beside 1200 and 600 bps ones (24 and 12 kHz) would need one handle per bank, each copying the same
 * I/Q and repeating the same capture-wide front end (staging, the 16384-point forward transform of every hop).  A jaero_split has ONE front
 * end, one spectrum X_p per hop, and 1 .. 8 outputs, each with its own out_rate, channels and prototype.
 *   definition output g is, bit for bit and in every reader (int16 PCM, *nout, the survey's levels and spectrum, the activity's block
 *              statistics and peak-hold spectrum), what a stand-alone handle produces that was created with decim D_g = fs_c / out_rate_g,
 *              out_rate_g, the output's channels and taps (jaero_chan2_create; with `cap`, jaero_chan3_create with the same jaero_capture)
 *              and the same max_write_iq, and is fed the same writes, cut the same way.  It holds by construction: X_p is a function of the
 *              input and of absolute block indices only and comes from the same forward-transform launches; the blocks a write completes
 *              depend only on max_write_iq and the capture's ratio; each output launches the stand-alone handle's synthesis, survey and
 *              activity kernels with the same (nchannels, blocks, first block).  No kernel is new.
 *   jaero_split_create   cap NULL: int16 I/Q at fs_c; otherwise the capture front end above with Fs_c = fs_c, and max_write_iq counts CAPTURE
 *                        samples.  Two outputs may share a D and differ in taps and channels.  Tune words are relative to fs_c, audio words
 *                        to the output's out_rate.  All arguments are checked before a device is looked for, JAERO_EINVAL in this order: out
 *                        null; outs null; noutputs outside 1 .. 8; fs_c < 1; for each output in order: out_rate not 48000 / 24000 / 12000,
 *                        fs_c / out_rate not exactly 16, 32, 64, 128 or 256, then jaero_chan2_create's own checks of that output in their
 *                        order (max_write_iq < 1 among them); with cap: jaero_chan3_create's checks of the capture in their order (format,
 *                        fs_in, L, the ratio, taps_per_phase, rtaps, its taps), then the staged-sample bound on max_write_iq; then
 *                        JAERO_ENODEV off gfx950 (no CPU fallback).
 *   jaero_split_write    niq raw pairs in the handle's format (int16 without cap): one copy of the input, one staging launch on a capture
 *                        handle, one forward-transform launch over the nblk blocks the write completes, then for each output in order its
 *                        synthesis and, where enabled, its survey / activity launches, all on `stream`; nout[g] = nblk Mo_g (nout:
 *                        noutputs entries).  niq < 0 or niq > max_write_iq: JAERO_EINVAL, nothing consumed.  Stream changes and poisoning
 *                        are jaero_chan_write's: an event from the previous stream; an error behind the first launch that advances the
 *                        state poisons the splitter and every view (JAERO_EHIP from every later call but the destroys).
 *   jaero_split_output   *view = a borrowed jaero_chan for output g: owned by the splitter, valid until jaero_split_destroy, the same pointer
 *                        at every call.  Every call that reads or tunes works on it as on a stand-alone handle: jaero_chan_pcm_view,
 *                        jaero_chan_read_pcm, jaero_chan_retune, jaero_chan2_retune_all, jaero_survey_*, jaero_activity_*,
 *                        jaero_chan_profile_read (which 0 reports 0 launches: the forward transform is the splitter's), jaero_survey_ /
 *                        jaero_activity_profile_read; those that synchronise use the stream of the splitter's last write.  The spectrum and
 *                        the peak-hold spectrum may be enabled on any view and are computed for it from the shared X_p: enabling them on
 *                        several views repeats that work (the same numbers several times).  The calls that consume input or own the handle
 *                        -- jaero_chan_write, jaero_chan_feed, jaero_chan3_write, jaero_chan3_feed, jaero_chan3_read_staged -- return
 *                        JAERO_EINVAL on a view, change nothing and name the call to use; jaero_chan_destroy on a view does nothing.
 *   jaero_split_feed     banks: noutputs entries, a NULL entry's output is produced and not fed.  Before anything advances: jaero_chan_feed's
 *                        checks of every non-null bank against its output (device, channel count, every Fs == out_rate_g, max_write_samples
 *                        >= nblk_max Mo_g), and one bank in two entries: JAERO_EINVAL.  Then the write; then, for each non-null bank with
 *                        nout[g] > 0 in output order, jaero_write(bank_g, view g's pcm, nout[g], JAERO_PCM_CHANNEL_MAJOR, 1, stream).  A
 *                        bank's failure is returned, the banks behind it are not fed and the splitter is poisoned: the banks are no longer
 *                        at one point of the capture.
 *   jaero_split_info     any of the three may be NULL; nblk_max = the most blocks a write completes.
 *   jaero_split_profile_* enable switches the front end's and every view's timers; read: which 0 = the forward transform (k_chan_fwd, or
 *                        k_capture_fwd with cap), 1 = the staging kernel (0 launches without cap).  The outputs' kernels are read on the views.
 * Null handles: JAERO_EINVAL.  Deliberately not here: outputs on separate streams, other decimations, N or hop, adding or removing outputs
 * or channels after create, jaero_chan3_read_staged on a splitter, the multi-GPU fan-out of a capture, a shared survey spectrum for
 * several views. */
typedef struct jaero_chan_output {
    int out_rate;                    /* 48000, 24000 or 12000 */
    int nchannels;
    const jaero_chan_channel *ch;    /* tune words relative to fs_c, audio words to out_rate */
    const double *taps; int ntaps;   /* this output's prototype, at fs_c */
} jaero_chan_output;
typedef struct jaero_split jaero_split;
int  jaero_split_create(int device, const jaero_capture *cap /* NULL: int16 I/Q at fs_c */, int fs_c,
                        int noutputs, const jaero_chan_output *outs, int max_write_iq, jaero_split **out);
void jaero_split_destroy(jaero_split *s);
int  jaero_split_write(jaero_split *s, const void *iq, int niq, int is_device_ptr, void *stream,
                       int *nout /* [noutputs] */);
int  jaero_split_feed(jaero_split *s, jaero_ctx *const *banks /* [noutputs]; a NULL entry: produced, not fed */,
                      const void *iq, int niq, int is_device_ptr, void *stream, int *nout /* [noutputs] */);
int  jaero_split_output(jaero_split *s, int output, jaero_chan **view);
int  jaero_split_info(const jaero_split *s, int *noutputs, int *fs_c, int *nblk_max);
int  jaero_split_profile_enable(jaero_split *s, int on);          /* the front end and every output */
int  jaero_split_profile_read(jaero_split *s, int which /* 0 forward transform (either kind), 1 staging kernel */,
                              double *total_ms, int *launches, int reset);

/* ---- rate lines: what a channel's bit rate is, measured from the int16 PCM a bank is fed (a channeliser's output or any other).  The
 * spectrum of the SQUARED signal is the measurement JAERO trusts for acquisition (CoarseFreqEstimate): MSK with h = 0.5, squared, is
 * Sunde's FSK with two lines at 2 f_audio +- fb / 2; OQPSK with the reference's RRC pulses, squared, has two lines at 2 f_audio +- 1 / T =
 * 2 f_audio +- fb / 2.  Either way the lines are fb apart whatever the carrier offset is, and their midpoint gives the offset.  The device
 * measures (one 4096-point fp64 transform per channel and segment), jaero_amd.ratemeter.classify_rates decides in numpy.  A handle
 * jaero_rate is independent of every other handle: nchannels rows of int16, one row per channel; the sample rate enters no device
 * arithmetic.  This text is the definition; tests/rate_oracle.py implements it literally in numpy.
 *   L = 4096.  Segment j of a row y is y[j L .. (j + 1) L), samples counted from create: consecutive, not overlapping.
 *   q[i]   = y[i]^2 - (sum_i y[i]^2) / L over the segment.  EXACT in fp64: the squares are integers below 2^31, their sum an integer below
 *            2^43, the mean a multiple of 2^-12 below 2^31, the difference a multiple of 2^-12 below 2^31 in magnitude -- 43 bits.
 *   Z      = DFT_L(q), Z[k] = sum_i q[i] e^(-j 2 pi k i / L).
 *   H[k]   = Z[k] / 2 - (Z[(k - 1) mod L] + Z[(k + 1) mod L]) / 4: the Hann window, applied in the frequency domain as the survey does.
 *   R_c[k] = sum_j |H_j[k]|^2 for 0 <= k <= L / 2: JAERO_RATE_BINS = 2049 doubles per channel, bin k at k fs / L Hz of the squared signal.
 *            The sum runs over every segment completed since create or the last reset, added in ascending j; nseg is their number, the
 *            same for every channel.
 * Rules, the survey's: after T samples per row exactly floor(T / L) segments are in R, however the writes were cut; R is bit-identical for
 * every cutting of the same rows and for host and device input (no floating-point atomics; a segment's terms are formed by the same
 * instructions whatever the launch shape; terms join the sum in segment order); a row of zeros, or of any constant, gives R_c == 0
 * exactly (q is then exactly zero; no two rows and no two segments share a transform).
 *   jaero_rate_create    arguments are checked before a device is looked for: nchannels < 1, max_write_samples < 1 or out == NULL are
 *                        JAERO_EINVAL; then JAERO_ENODEV off gfx950.
 *   jaero_rate_write     pcm is compact channel-major [nchannels][nsamples]: what jaero_chan_pcm_view hands out and jaero_write takes with
 *                        JAERO_PCM_CHANNEL_MAJOR; host or device memory.  *nseg_done = the segments this write completed.  nsamples < 0 or
 *                        > max_write_samples: JAERO_EINVAL, nothing consumed.  Asynchronous on `stream`; a write on another stream than the
 *                        previous one waits for it.  A failure behind the first launch that advances state poisons the handle (JAERO_EHIP
 *                        from then on), as a channeliser's write does.
 *   jaero_rate_reset     synchronises on the handle's last stream, clears R and nseg.  The pending partial segment is kept: the segment
 *                        grid stays absolute.
 *   jaero_rate_read      synchronises on the handle's last stream; sums[nchannels][2049] = R, *nseg.
 *   jaero_rate_profile_* HIP-event time since the last reset: which 0 = the line kernel (k_rate_lines; k_rate_lines_gated on a gated handle).
 * Deliberately not here: the decision (classify_rates is host numpy over 16 KB per channel; its selections run on the device since: "rate
 * lines, read on the device" below), modulation recognition beyond what the rate
 * implies, other L.  A burst channel's lines are diluted by its duty cycle, R being a sum over every segment: the gated rate lines below
 * take its rate while it is on. */
typedef struct jaero_rate jaero_rate;
#define JAERO_RATE_L 4096
#define JAERO_RATE_BINS 2049
int jaero_rate_create(int device, int nchannels, int max_write_samples, jaero_rate **out);
void jaero_rate_destroy(jaero_rate *r);
int jaero_rate_write(jaero_rate *r, const int16_t *pcm, int nsamples, int is_device_ptr, void *stream, int *nseg_done);
int jaero_rate_reset(jaero_rate *r);
int jaero_rate_read(jaero_rate *r, double *sums /* [nchannels][2049] */, long long *nseg);
int jaero_rate_profile_enable(jaero_rate *r, int on);
int jaero_rate_profile_read(jaero_rate *r, int which /* 0 = the line kernel */, double *total_ms, int *launches, int reset);

/* ---- gated rate lines: the rate lines of a channel summed over the segments in which it is on.  R above is a sum over every segment; a
 * segment in which a burst channel is off adds noise floor and no line, so a burst channel's score falls for as long as it stays off.
 * The measurement that decides is one the line kernel makes anyway: the exact integer sum of y^2 over the segment.  A jaero_rate handle
 * switched over by jaero_gate_enable compares it with a gate per channel and adds a segment to a channel's R only where it reaches the
 * gate.  This text is the definition; tests/rate_gate_oracle.py implements it literally on tests/rate_oracle.py's segment_terms.
 *   E_j(c) = sum_i y[i]^2 over segment j of channel c (L = 4096 and the segment grid of the rate lines): an unsigned 64-bit integer below 2^43.
 *   g(c)   the channel's gate, an unsigned 64-bit integer, 0 at create.  Any value is allowed.
 *   Segment j JOINS channel c iff E_j(c) >= g(c), with the gate in force when the write that completes the segment is made.
 *   R_c[k] = sum of |H_j[k]|^2 over the joined segments only, in ascending j; the arithmetic of a term is exactly that of the rate lines.
 *   Per channel, over the segments completed since the last reset, four unsigned 64-bit numbers: emax = max E_j, emin = min E_j (over every
 *            segment, joined or not), njoin = the segments joined, ejoin = sum of E_j over the joined.  With no segment yet: 0, 2^64 - 1, 0, 0.
 *            nseg counts every completed segment, joined or not, and is the same for every channel.
 * What follows: with every gate 0, R is bit-identical to the ungated handle's; a channel's R is bit-identical to the R of an ungated handle
 * that was fed only that channel's joined segments, in order; R and the four numbers are bit-identical for every cutting of the writes and
 * for host and device input; a row of zeros joins under gate 0 with R == 0 exactly and never joins under a gate > 0; whether a neighbour
 * joins changes no bit of a channel's R (a channel that does not join does not touch its row).
 *   jaero_gate_enable  on != 0: the gated state; on == 0: the state at create, in which the handle behaves as it did before these calls
 *                      existed (k_rate_lines alone is launched, no gate is looked at, no number kept).  Every call synchronises on the
 *                      handle's last stream and clears R, nseg and the four numbers, as a reset does; the pending partial segment and the
 *                      gates stay.
 *   jaero_gate_set     gate[nchannels].  Synchronises on the handle's last stream; holds for the segments completed by later writes; clears
 *                      nothing.  JAERO_EINVAL while off.
 *   jaero_gate_read    synchronises; stats[nchannels][4] = emax, emin, njoin, ejoin; gate[nchannels] (may be NULL) = the gates; *nseg.
 *                      JAERO_EINVAL while off.
 * jaero_rate_reset additionally clears the four numbers and keeps the gates; jaero_rate_read, _write and _profile_* keep their meaning, and
 * timer slot 0 counts whichever line kernel ran (k_rate_lines or k_rate_lines_gated).  A null handle or argument is JAERO_EINVAL with the
 * function's name in jaero_last_error(), before any device is touched; a poisoned handle answers JAERO_EHIP here as everywhere.
 * Deliberately not here: gating by the channeliser's activity blocks (another grid).  Gates chosen on the device and a histogram of segment
 * energies are the one-pass gates below. */
int jaero_gate_enable(jaero_rate *r, int on);
int jaero_gate_set(jaero_rate *r, const unsigned long long *gate /* [nchannels] */);
int jaero_gate_read(jaero_rate *r, unsigned long long *stats /* [nchannels][4]: emax, emin, njoin, ejoin */, unsigned long long *gate /* [nchannels], may be null */, long long *nseg);

/* ---- one-pass gates: the flow above needs the signal twice (measure under gate 0, set the gates, measure again), and one click sets emax
 * and with it the midpoint.  Here the device chooses every gate itself, segment by segment, from the SECOND largest energy, and can count
 * every segment's energy in a histogram.  This text is the definition; tests/rate_auto_oracle.py implements it literally.  Everything is
 * an unsigned 64-bit integer; there is no tolerance anywhere.
 *   Per channel: the four numbers above; e2, the second largest segment energy, with multiplicity (two segments of the largest energy:
 *   e2 == emax), 0 at reset; start, 2^64 - 1 at reset; the gate g, 0 at reset.
 *   Segment number s (0-based since the last reset, every completed segment counted) with energy E, under JAERO_GATE_AUTO, in this order:
 *     if E > emax: e2 = emax, emax = E; else if E > e2: e2 = E
 *     emin = min(emin, E)
 *     g' = (e2 + emin) / 2 (rounded down) if e2 > 0 and 2 e2 >= 3 emin, else 0
 *     join = E >= g';  restart = g == 0 and g' > 0 and join
 *     restart:   R_c = |H_s|^2 (assigned, not added), njoin = 1, ejoin = E, start = s
 *     else join: R_c += |H_s|^2, njoin += 1, ejoin += E
 *     g = g'
 *   What follows: the result depends only on the sequence of E -- cuts and input memory change no bit of R and none of the numbers; a
 *   channel's R is bit-identical to an ungated handle's that was fed only its joined segments from `start` on, in order; a channel whose
 *   segments differ by less than 3 / 2 never leaves gate 0, is the ungated handle bit for bit, and keeps start == 2^64 - 1; a row of zeros
 *   keeps gate 0, joins everything and has R == 0 exactly; a channel that starts inside a burst and then falls silent never restarts (the
 *   quiet segment lowers emin, the gate rises, the quiet segment does not join); one that is quiet first restarts at its second loud
 *   segment, and what it summed under gate 0 is thrown away; one click cannot move the gate, because it only ever becomes emax; a
 *   neighbour in the same workgroup changes nothing.  njoin / (nseg - start) is the duty cycle since the restart.
 *   Limits: two clicks set e2; a dropout (a segment of zeros) sets emin for good; the segments joined while the gate was still rising
 *   stay in R.
 *   The histogram (JAERO_GATE_HIST): every completed segment, joined or not, adds 1 to bin E for E < 8, else to bin
 *   8 (e - 2) + ((E >> (e - 3)) & 7) with e = floor(log2 E): eight bins an octave, 0.28 to 0.51 dB wide.  The lower edge of bin b >= 8 is
 *   (8 + b mod 8) << (b div 8 - 1).  E <= 4096 * 32768^2 = 2^42 lands in bin 320, the last.  Counts are 32-bit.
 *   jaero_gate2_enable     mode 0, JAERO_GATE_MANUAL, JAERO_GATE_AUTO, or either of the two | JAERO_GATE_HIST; anything else is JAERO_EINVAL
 *                          and leaves the handle as it was.  jaero_gate_enable(r, on) is jaero_gate2_enable(r, on ? 1 : 0).  Every call
 *                          synchronises and clears R, nseg, the four numbers, e2, start and the histogram; the pending partial segment
 *                          stays; the gates stay, except that a new mode with AUTO sets them all to 0 (going AUTO -> MANUAL therefore
 *                          freezes the device's gates for a second pass).  Under MANUAL | HIST the decision is E >= g with the given gate.
 *   jaero_gate2_read       stats[nchannels][6] = emax, emin, njoin, ejoin, e2, start; gate (may be NULL); *nseg.  JAERO_EINVAL unless AUTO.
 *   jaero_gate2_read_hist  hist[nchannels][321], *nseg.  JAERO_EINVAL unless HIST.
 * jaero_gate_read works in every mode but 0; jaero_gate_set is JAERO_EINVAL under AUTO and changes nothing; jaero_rate_reset under AUTO
 * also zeroes the gates, e2 and start, and under HIST the histogram.  A handle that never uses these calls launches k_rate_lines and
 * k_rate_lines_gated alone; a mode with AUTO or HIST launches k_rate_lines_auto, which timer slot 0 then counts.
 * Deliberately not here: a gate taken from the histogram on the device (jaero_amd.ratemeter.hist_extremes and suggest_gate are host
 * arithmetic), ratios other than 3 / 2. */
#define JAERO_GATE_MANUAL 1   /* what jaero_gate_enable(r, 1) gives */
#define JAERO_GATE_AUTO   2   /* the device chooses every gate, segment by segment */
#define JAERO_GATE_HIST   4   /* also count every completed segment in a histogram of E; only together with MANUAL or AUTO */
#define JAERO_GATE_HBINS  321
int jaero_gate2_enable(jaero_rate *r, int mode);
int jaero_gate2_read(jaero_rate *r, unsigned long long *stats /* [nchannels][6]: emax, emin, njoin, ejoin, e2, start */, unsigned long long *gate /* [nchannels], may be null */, long long *nseg);
int jaero_gate2_read_hist(jaero_rate *r, unsigned *hist /* [nchannels][321] */, long long *nseg);

/* ---- rate lines, read on the device: what jaero_amd.ratemeter.classify_rates does to R before its log10 is selection -- a median, a
 * three-bin maximum, a search over pairs of bins -- and jaero_lines_classify does it where R lies, so that about 8 + 12 nd bytes a channel
 * come back in place of 16 392.  This text is the definition; tests/rate_lines_oracle.py implements it literally.
 *   Inputs: a handle's sums R_c[0 .. 2048] (non-negative doubles); kmin; nd distances d[0 .. nd), integers that the host forms as
 *   round(fb / (fs / 4096)): the device never sees fs.
 *   Per channel c:
 *   floor     the median of R_c[kmin .. 2048]: the middle order statistic for an odd count, (lo + hi) / 2 of the two middle ones for an
 *             even count (what numpy.median gives).
 *   P[k]      max(R_c[k - 1], R_c[k], R_c[k + 1]), clipped at k = 0 and k = 2048.
 *   per distance i: skipped when kmin + d[i] >= 2049: score[i] = 0, where[i] = -1.  Otherwise
 *   score[i]  = max over kmin <= a < 2049 - d[i] of min(P[a], P[a + d[i]]), and
 *   where[i]  = the SMALLEST a that attains that maximum (the three-bin maximum makes plateaus of equal P: ties are the normal case).
 *   No arithmetic but the one halving: floor and score are elements of R (or that mean) bit for bit, and a channel's result does not depend
 *   on nchannels or on its neighbours.  jaero_amd.ratemeter.decide_rates takes the decision from there on the host (log10, argmax,
 *   threshold), which makes it equal to classify_rates' unconditionally.
 *   jaero_lines_classify  checked before any HIP call, JAERO_EINVAL with the argument's name: a null handle or output pointer, nd outside
 *                         1 .. 8, a d[i] < 1, kmin outside 1 .. 2047.  Then as jaero_rate_read: synchronises on the handle's last stream,
 *                         launches k_rate_classify on it, copies out floor[nchannels], score[nchannels][nd], where[nchannels][nd] and
 *                         *nseg.  kernel_ms (may be NULL) receives the launch's HIP-event time.  Works in every gate mode and changes no
 *                         state of the handle: R, nseg, the gates, the numbers and the pending segment stay.  The result buffers are
 *                         device allocations of the handle, made by the first call.
 * jaero_rate_profile_read keeps refusing which != 0: this launch is timed by its own argument.
 * Deliberately not here: the decision itself (log10 and the threshold are host arithmetic over nd numbers a channel), other row lengths. */
int jaero_lines_classify(jaero_rate *r, int kmin, int nd, const int *d, double *floor /* [nchannels] */, double *score /* [nchannels][nd] */,
                         int *where /* [nchannels][nd] */, long long *nseg, double *kernel_ms /* may be null */);
/* Test hook: overwrites R with sums[nchannels][2049] and the segment count with nseg >= 0 (synchronises), so that the classifier can be run
 * on rows that no signal produces. */
int jaero_debug_rate_poke(jaero_rate *r, const double *sums /* [nchannels][2049] */, long long nseg);

/* Host-only debugging aid (no device needed): the sample indices at which jaero_write would run the coarse-frequency
 * estimate for a fresh channel fed `nwrites` writes of write_sizes[i] samples.  Returns the number of triggers
 * (>= 0; up to `cap` are stored) or a negative error. */
int jaero_debug_schedule(int fft_power, int Fs, int cpu_reduce, const int *write_sizes, int nwrites,
                         long long *trigger_samples, int cap, int *segments_out);

/* Host-only: the same for `nch` channels of one bank that hold their own flags (flags0[ch]: 1 AFC, 2 SQL, 4 cpuReduce, 8 DCD) and change them
 * between writes: events[k] = {before_write, channel (-1: all), kind (0 jaero_set_flags bits, 1 jaero_set_dcd, 2 jaero_set_settings), value}.
 * Stores (sample, channel) pairs, one per firing of a channel's estimate (JAERO/oqpskdemodulator.cpp:410-431 with per-object cpuReduce). */
int jaero_debug_schedule_lanes(int fft_power, int Fs, int nch, const int *flags0, const int *write_sizes, int nwrites,
                               const int *events, int nevents, long long *trig_sample_channel, int cap, int *segments_out);

/* Test hook: the 8400 bps prefilter kernel alone.  n complex samples (re, im interleaved, host pointers) through the kernel
 * RRC(alpha, 2049 taps, 48 kHz, fsym symbols/s) with JFastFir's latency for nfft = 4096 (out[m] = sum_k h[k] x[m - 2048 - k]):
 * JFastFir::SetKernel + update as JAERO/oqpskdemodulator.cpp:278-283,366-368 use it and JAERO/tests/jfastfir_tests.cpp:31-58 pins it. */
int jaero_debug_prefilter(int device, const double *in_reim, int n, double alpha, double fsym, double *out_reim);
/* Test hook: the first n prefiltered complex samples (re, im pairs) of the last jaero_write of an 8400 bps bank, channel ch
 * (cval_prefiltered, JAERO/oqpskdemodulator.cpp:343-381). */
int jaero_debug_read_prefiltered(jaero_ctx *ctx, int channel, double *out_reim, int n);
/* Test hooks: the prefilter stage of an 8400 bps bank on its own (k_pre8400_mix, k_pre8400_commit, k_pre8400_fft, k_pre8400_restart), launched by
 * the code jaero_write and jaero_set_settings launch it with.  JAERO_EINVAL before any launch: null ctx, a bank that is not 8400 bps, a channel
 * outside [0, nchannels), nsamples outside 1 .. max_write_samples, stretches outside {0, 1, 8}, a state out of range, a ring window that is
 * not wholly among the last `ring` samples written.  write / poke / restart mark the bank as the coarse hooks do (a later jaero_write or setter
 * returns JAERO_EHIP); peek, read_ring and jaero_debug_read_prefiltered only read and may be called between real writes.
 *   jaero_debug_pre8400_write     the prefilter stage of one write of host PCM for the whole bank and nothing behind it; advances the bank's
 *                                 sample count and previous write length.  stretches: 0 = as jaero_write chooses, 1 or 8 = forced.
 *   jaero_debug_pre8400_poke      one channel's oscillator pointer and step (both in [0, 19999)), the sum of mixer2's frequency over the
 *                                 previous write (the next write's oscillator runs at fsum / nprev) and hold, the absolute sample index up
 *                                 to which the channel's outputs are exact zeros.  n0 / nprev / ring / cap are outputs of peek only.
 *   jaero_debug_pre8400_peek      the same back, with the bank's samples written so far, previous write length, ring length and capacity.
 *   jaero_debug_pre8400_restart   the launch jaero_set_settings makes for one channel of several.
 *   jaero_debug_pre8400_read_ring n down-mixed samples (re, im pairs) of a channel's history from absolute sample index first_abs_index on. */
typedef struct jaero_pre8400_state
{
    double ptr, step, fsum;
    long long hold;
    long long n0;
    int nprev, ring, cap;
} jaero_pre8400_state;
int jaero_debug_pre8400_write(jaero_ctx *ctx, const int16_t *pcm, int layout, int nsamples, int stretches);
int jaero_debug_pre8400_poke(jaero_ctx *ctx, int channel, const jaero_pre8400_state *st);
int jaero_debug_pre8400_peek(jaero_ctx *ctx, int channel, jaero_pre8400_state *st);
int jaero_debug_pre8400_restart(jaero_ctx *ctx, int channel);
int jaero_debug_pre8400_read_ring(jaero_ctx *ctx, int channel, long long first_abs_index, int n, double *out_reim);
/* Test hook: the Viterbi decoder picks its layout by size (one block per wavefront below 16 384 blocks, one per lane from there); tests
 * force one so that both meet the oracle at small sizes.  mode: 0 = by size (default), 1 = wave, 2 = lanes.  Process-wide. */
int jaero_debug_viterbi_layout(int mode);
/* Test hook: ONE launch of the Viterbi decoder through the library's own launch function, every parameter of that launch in the caller's
 * hands (the public entry points fix most of them).  All buffers are host memory; the call stages them, launches, synchronises and copies back.
 *   soft           row-major [nblocks][pitch] (pitch 0: nsoft), or tiled != 0: [wavefronts = ceil(nblocks / 64)][nsoft / 16][64][16] (whole wavefronts)
 *   soft_misalign  0 .. 15 bytes added to the 16-byte aligned device address of soft (row-major only)
 *   overlap        NULL, or [nblocks][64] as jaero_viterbi_continuous keeps it (byte 62 = the length, at most 62); with update_overlap != 0 the
 *                  overlap update kernel runs behind the decoder with the same valid / tiled / pitch and the buffer is copied back
 *   out            [out_rows][out_stride] bytes (out_rows 0: nblocks), copied to the device BEFORE the launch and NOT cleared, copied back whole:
 *                  a byte the decoder did not write comes back as the caller left it.  Decoded bit k of the stream overlap[:len] ++ soft ++ pad x 128
 *                  (k < (stream length) / 2 - 6) goes to position k - out_start when 0 <= k - out_start < min(out_want, row length / 2): one byte
 *                  per bit, or packed != 0: bit (k - out_start) & 31 of the 32-bit word (k - out_start) >> 5 of the row, where a word that receives a
 *                  bit is written whole (its other bits 0) and a word that receives none is not written
 *   valid          NULL, or [nblocks]: rows with 0 are skipped (output and overlap untouched)
 *   lens           NULL, or [nblocks]: each row's own length (even, 28 .. nsoft; row-major only)
 *   layout         0 = as the library chooses by size, 1 = one block per wavefront (k_viterbi), 2 = one block per lane, k_viterbi_lanes,
 *                  3 = one block per lane, k_viterbi_lanes_x2 (which the library itself takes above four wavefronts per compute unit)
 * JAERO_EINVAL before any HIP call for what the kernels do not implement: tiled or packed in the wavefront layout, tiled with nsoft % 16 != 0 (or
 * with lens, pitch, soft_misalign), a lane-layout row of fewer than 28 steps ((length + pad) / 2), lens[b] odd or above nsoft, out_stride below
 * the window (packed: whole words, a multiple of 4), an overlap length above 62. */
typedef struct jaero_viterbi_probe
{
    const uint8_t *soft;
    int nblocks, nsoft, pitch, tiled, soft_misalign, pad;
    uint8_t *overlap;
    uint8_t *out;
    int out_rows, out_stride, out_start, out_want, packed, layout, update_overlap;
    const int *valid;
    const int *lens;
} jaero_viterbi_probe;
int jaero_debug_viterbi(int device, const jaero_viterbi_probe *q);
/* Test hook: a continuous bank picks its sample-loop layout at jaero_create by size (one front / back pair per workgroup up to two channel
 * groups per CU, four pairs above); tests force one so that both meet the oracle at small sizes.  mode: 0 = by size (default), 1 = one
 * pair, 2 = four pairs.  Affects only the kernels chosen by size (k_oqpsk_fb at both rates, k_msk_fb at 80 taps), and only banks created
 * (or re-created by a rate change) after the call.  Process-wide. */
int jaero_debug_sample_loop_layout(int mode);
/* Test hook: the whole instantiation of the kernel this bank launches for class `which` (0 = sample loop / burst demodulator, 1 = coarse
 * estimate / trident check; jaero_profile_kernel's numbering), spelled as `nm -C` prints it, e.g. "k_oqpsk_fb<55, 36, true, false, 4, false>";
 * kernels that are not templates give their plain name.  JAERO_EOVERFLOW if it does not fit in cap bytes. */
int jaero_debug_kernel_variant(jaero_ctx *ctx, int which, char *buf, int cap);

/* Test hooks: a continuous bank's own coarse-estimate kernel (jaero_debug_kernel_variant(ctx, 1): the function, block, dynamic LDS and twiddles
 * jaero_write launches) run on state the test supplies.  All three synchronise the bank first and mark it as a bank whose write failed part-way
 * (its schedule mirror no longer describes the device): a later jaero_write or setter returns JAERO_EHIP; only these hooks, the readers of the
 * status log and jaero_destroy go on working.  JAERO_EINVAL: null ctx, burst bank, channel outside [0, nchannels), values out of range.
 *   jaero_debug_coarse_poke   one channel's ring (nfft re, im pairs in RING order: entry k is bbcycbuff[k]) and smoothed spectrum y (nfft), each
 *                             optional (NULL: left alone), and, when st != NULL, the scalars the estimate's slot reads: bb_ptr in [0, nfft),
 *                             emptying, flags (1 AFC, 2 SQL, 4 cpuReduce, 8 DCD), countdown, countdown2, coarse_cnt, mse, m2_freq, mc_freq (both
 *                             >= 0; the wave tables' steps are set to match, as jaero_create forms them).  nest and log_cnt are outputs only.
 *   jaero_debug_coarse_launch one launch over channels[0 .. nlist) (distinct; NULL: all channels in order, nlist = nchannels) with `grid`
 *                             workgroups: 0 = as jaero_write (min(nlist, one or two per CU)), else 1 <= grid <= that number, so that a few
 *                             channels run as several persistent estimates of one workgroup.
 *   jaero_debug_coarse_peek   the same values back for any channel; ring / y / st each optional. */
typedef struct jaero_coarse_state
{
    int bb_ptr, emptying, flags, countdown, countdown2, coarse_cnt;
    int nest, log_cnt; /* estimates so far; status-log rows stored (JAERO_FLAG_STATUS_LOG) */
    double mse, m2_freq, mc_freq;
} jaero_coarse_state;
int jaero_debug_coarse_poke(jaero_ctx *ctx, int channel, const double *ring_reim, const double *y, const jaero_coarse_state *st);
int jaero_debug_coarse_launch(jaero_ctx *ctx, const int *channels, int nlist, int grid);
int jaero_debug_coarse_peek(jaero_ctx *ctx, int channel, double *ring_reim, double *y, jaero_coarse_state *st);
/* Test hooks: the slow state of a continuous bank's sample loop, which no signal of a few seconds moves far (tests/test_gpu_loop_branches.py):
 * the symbol oscillator's frequency st_freq (OQPSK: held within 0.1 Hz of the bit rate by the loop; MSK: fb / 2, fixed), mixer2's frequency
 * m2_freq, and the carrier loop filter's last two inputs lf_x1, lf_x2 and outputs lf_y1, lf_y2, newest first (OQPSK only; MSK banks keep
 * what is poked and never read it).  Poke writes all six and sets the two wave tables' steps to match, as jaero_create forms them; the
 * phases stay.  Both synchronise the bank.  Unlike the coarse hooks they leave the bank usable: the write schedule does not depend on these
 * values, and a jaero_write behind a poke continues from them.  JAERO_EINVAL: null ctx or state, a burst bank, channel outside
 * [0, nchannels), a negative frequency, a value that is not finite.  A poisoned bank: JAERO_EHIP. */
typedef struct jaero_loop_state
{
    double st_freq, m2_freq, lf_x1, lf_x2, lf_y1, lf_y2;
} jaero_loop_state;
int jaero_debug_loop_poke(jaero_ctx *ctx, int channel, const jaero_loop_state *st);
int jaero_debug_loop_peek(jaero_ctx *ctx, int channel, jaero_loop_state *st);
/* Test hooks: the band-aware estimate kernel.  A 2^14-point bank that is not an 8400 bps bank holds, beside its generic kernel (what
 * jaero_debug_kernel_variant(ctx, 1) and jaero_profile_kernel(ctx, 1) keep naming), k_coarse6_b7 for channels whose locking band ends on the
 * slot boundaries it is built for (startbin 7 * 512, expectedpeakbin 1792: lockingbw 10500 Hz at 48 kHz); jaero_write and
 * jaero_debug_coarse_launch split every list of estimates by the channels' class, which follows jaero_set_settings.
 *   jaero_debug_coarse_band          the band kernel's variant string ("" if the bank has none) and the estimates launched on the generic and
 *                                    on the band kernel since jaero_create (either pointer may be NULL).
 *   jaero_debug_coarse_force_generic on != 0: every estimate of this bank takes the generic kernel (what tests compare the band kernel with).
 *   jaero_debug_coarse_band_class    host only: 1 if a channel with these settings is in the band kernel's class. */
int jaero_debug_coarse_band(jaero_ctx *ctx, char *buf, int cap, long long *est_generic, long long *est_band);
int jaero_debug_coarse_force_generic(jaero_ctx *ctx, int on);
int jaero_debug_coarse_band_class(int fft_power, double Fs, double fb, double lockingbw);

/* Test hooks: a burst bank's transform kernels on their own (k_hist_push_frames / _chmajor, k_hilbert_fft, k_ev_compact and the bank's k_trident
 * instantiation, jaero_debug_kernel_variant(ctx, 1)), launched by the lines jaero_write launches them with.  All synchronise the bank first.
 * JAERO_EINVAL before any launch: null ctx, a bank that is not a burst bank, a channel outside [0, nchannels), values out of range.  hilbert,
 * poke_cv and trident mark the bank as the coarse hooks do (a later jaero_write or setter returns JAERO_EHIP); geom and read_hist only read and
 * may be called between real writes.
 *   jaero_debug_burst_geom      the geometry the kernels run with, the trident grid jaero_write uses and the samples written so far.
 *   jaero_debug_burst_hilbert   one write's history push (either layout, host PCM, 1 .. max_write_samples) and the k_hilbert_fft launch of each of
 *                               its segments, cut as jaero_write cuts them; nothing behind it.  Advances the bank's sample count.  out_im
 *                               [nchannels][nsamples] (host) receives im y of every segment.
 *   jaero_debug_burst_read_hist n samples of a channel's PCM history from absolute sample index first_abs_index on; the window lies wholly
 *                               among the last hist_len samples written.
 *   jaero_debug_burst_poke_cv   real parts of the ring of AGC'd analytic samples by absolute sample index: sample a lives at slot a mod cv_len
 *                               (mathematical modulo; a may be negative: the trident window of an early event starts before the stream);
 *                               1 <= n <= cv_len.
 *   jaero_debug_burst_trident   fills every trident result of the bank (padding channels included) with a sentinel, gives the listed channels
 *                               (distinct, any order, nlist in 0 .. nchannels) their event positions ev_pos[k] in [0, maxseg) and every other
 *                               channel none, then launches k_ev_compact and the trident kernel for a segment that starts at sample n0 >= 0 with
 *                               `grid` workgroups (0 = as jaero_write, else 1 .. tri_grid).  results[k] = the result of channels[k]; *nchanged =
 *                               the entries of the whole bank that no longer hold the sentinel. */
typedef struct jaero_burst_geom
{
    int kind, nch, nchp, maxseg, hist_len, hil_lat, cv_len, D1, tri_sz, nb, nt, tri_grid;
    long long nsamples;
} jaero_burst_geom;
typedef struct jaero_trident_result
{
    int ok, pad; /* ok: the part of the acceptance test that depends on the window alone */
    double freq, phase_deg, vol_gain, metric;
} jaero_trident_result;
int jaero_debug_burst_geom(jaero_ctx *ctx, jaero_burst_geom *out);
int jaero_debug_burst_hilbert(jaero_ctx *ctx, const int16_t *pcm, int layout, int nsamples, double *out_im);
int jaero_debug_burst_read_hist(jaero_ctx *ctx, int channel, long long first_abs_index, int n, int16_t *out);
int jaero_debug_burst_poke_cv(jaero_ctx *ctx, int channel, long long first_abs_index, int n, const double *re);
int jaero_debug_burst_trident(jaero_ctx *ctx, const int *channels, const int *ev_pos, int nlist, long long n0, int grid,
                              jaero_trident_result *results, int *nchanged);

/* Test hooks: a burst bank's per-sample detector k_burst_front<false / true> with k_ev_compact behind it, launched by the lines jaero_write
 * launches them with (the choice between the two instantiations and its count of samples included), and nothing behind them: no trident check, no
 * demodulator.  The rules of the hooks above hold: all synchronise the bank first and return JAERO_EINVAL before any launch for a null ctx, a bank
 * that is not a burst bank, a channel or a value out of range; front, front_poke and poke_bt mark the bank (a later jaero_write or setter returns
 * JAERO_EHIP), front_geom, front_peek and front_events only read and may be called between real writes.  front_peek, front_events, front_poke and poke_bt take a channel in
 * [0, nchp): the padding lanes of the last wavefront run the detector too, and a test has to show that what they find reaches no event list.
 *   jaero_debug_burst_front_geom  the lengths of the detector's rings and what else jaero_burst_geom does not tell (that struct keeps its size).
 *   jaero_debug_burst_front       ONE segment of 1 <= n <= min(maxseg, max_write_samples) samples: the history push of host PCM (either layout, as jaero_debug_burst_hilbert
 *                                 takes it); then, with im == NULL, k_hilbert_fft as in jaero_write, else im[nchannels][n] (host) copied into the
 *                                 segment's imaginary parts in the kernel's layout in its place (padding lanes get zeros), so that a test sets both
 *                                 parts of the analytic sample: re of sample m is -pcm[m - hil_lat - 1024] / 32768; then k_burst_front and
 *                                 k_ev_compact.  Advances the bank's sample count by n.  ev_pos[nchannels]: every channel's BI_EV_POS (the sample of
 *                                 the segment at which its trident buffer filled, or -1); ev_list[nchannels]: its first *ev_count entries are the
 *                                 channels k_ev_compact listed, the others are left alone.
 *   jaero_debug_burst_front_peek  st (may be NULL): the detector's scalars of one channel.  ring >= 0 (JAERO_FRONT_RING_*) with n >= 1: n entries of
 *                                 that ring from absolute sample index first on (sample a lives at slot a mod the ring's length, mathematical
 *                                 modulo); the window lies wholly among the last `length` samples before the bank's sample count (before the
 *                                 stream starts the rings hold zeros, or what poke_bt put there).  ring < 0: no ring is read.
 *   jaero_debug_burst_front_events  the first min(ev_cnt, caprows) rows (sample, kind, value) of a channel's event log, which stay where they
 *                                 are (jaero_read_events refuses a marked bank); *nrows = ev_cnt.  With JAERO_FLAG_TRACE the detector logs a
 *                                 kind-3 row for every firing.
 *   jaero_debug_burst_front_poke  one scalar of one channel: JAERO_FRONT_CNTDOWN in [0, 2 PL], _MAXPOSCD in [-1, 2 PL], _TRI_PTR in [0, tri_sz + 1],
 *                                 _BT_HOLD in [0, bt_lag] (whole numbers), _LASTDY any finite value.  Poking BT_HOLD also raises the bank's own
 *                                 count of samples to hold to at least that value, so that the launch line picks k_burst_front<true> as it does
 *                                 behind a jaero_set_settings.
 *   jaero_debug_burst_poke_bt     entries of the peak detector's ring (the burst-timing signal of the last 2 PL + 1 samples) by absolute sample
 *                                 index, negative indices allowed as in poke_cv; 1 <= n <= bt_len.
 *   jaero_debug_ev_compact        k_ev_compact alone on buffers of its own, no bank: masks[ngroups] (host; bit l of masks[g] = channel 64 g + l),
 *                                 1 <= ngroups <= 65536.  The device list of 64 * ngroups entries is filled with bytes 0xA5 before the launch and
 *                                 copied whole to list_out[64 * ngroups]: what lies behind *count_out must still hold 0xA5A5A5A5. */
#define JAERO_FRONT_RING_AGC 0
#define JAERO_FRONT_RING_CVRE 1
#define JAERO_FRONT_RING_CVIM 2
#define JAERO_FRONT_RING_MA1RE 3
#define JAERO_FRONT_RING_MA1IM 4
#define JAERO_FRONT_RING_MAV1 5
#define JAERO_FRONT_RING_FA 6
#define JAERO_FRONT_RING_BT 7
#define JAERO_FRONT_CNTDOWN 0
#define JAERO_FRONT_MAXPOSCD 1
#define JAERO_FRONT_TRI_PTR 2
#define JAERO_FRONT_BT_HOLD 3
#define JAERO_FRONT_LASTDY 4
typedef struct jaero_burst_front_geom
{
    int PL, bt_len, bt_lag, agc_len, ma1_len, mav1_len, fa_len, fa_lag, ev_cap, ngroups;
    double pd_thr, bt_w, fa_w;
} jaero_burst_front_geom;
typedef struct jaero_burst_front_state
{
    double agc_sum, ma1_re, ma1_im, mav1_sum, lastdy;
    int cntdown, maxposcd, tri_ptr, ev_pos, ev_cnt, bt_hold;
} jaero_burst_front_state;
int jaero_debug_burst_front_geom(jaero_ctx *ctx, jaero_burst_front_geom *out);
int jaero_debug_burst_front(jaero_ctx *ctx, const int16_t *pcm, int layout, int n, const double *im, int *ev_pos, int *ev_list, int *ev_count);
int jaero_debug_burst_front_peek(jaero_ctx *ctx, int channel, jaero_burst_front_state *st, int ring, long long first_abs_index, int n, double *out);
int jaero_debug_burst_front_events(jaero_ctx *ctx, int channel, double *rows, int caprows, int *nrows);
int jaero_debug_burst_front_poke(jaero_ctx *ctx, int channel, int field, double value);
int jaero_debug_burst_poke_bt(jaero_ctx *ctx, int channel, long long first_abs_index, int n, const double *values);
int jaero_debug_ev_compact(int device, const unsigned long long *masks, int ngroups, int *list_out, int *count_out);

/* Test hooks: a burst bank's tracking kernel (jaero_debug_kernel_variant(ctx, 0): k_burst_oqpsk_demod<CAPSYM> or k_burst_msk_fb<CAPSYM, FIRN, LDSN>)
 * on its own, launched by the line jaero_write launches it with; no history push, no Hilbert transform, no detector and no trident check run.
 * The rules of the hooks above hold: all synchronise the bank first and return JAERO_EINVAL before any launch for a null ctx, a bank that is not
 * a burst bank, a channel or a value out of range; track and track_fill mark the bank (a later jaero_write or setter returns JAERO_EHIP: set the
 * flags first), track_geom, track_peek and track_read only read.  track_peek and track_read take a channel in [0, nchp), track's list one in
 * [0, nchannels): a padding lane never gets a verdict, and a test has to show that what the padding lanes compute reaches no row of a channel.
 *   jaero_debug_burst_track_geom  the lengths the tracking chain runs with, FIRN / LDSN of the instantiation the bank launches and JD_EBNO_TAIL.
 *   jaero_debug_burst_track       ONE segment of 1 <= n <= min(maxseg, max_write_samples) samples.  Every channel of the bank, padding lanes
 *                                 included, gets event position -1; the listed channels (distinct, any order, nlist in 0 .. nchannels) get
 *                                 ev_pos[k] in [0, n) and verdicts[k] as their trident result, taken as given.  Then the tracking kernel with n0 =
 *                                 the bank's sample count and first_of_write (0 / 1) as given; the count advances by n.  The kernel reads val of
 *                                 sample m at absolute index m - D1 - D2 of the ring jaero_debug_burst_poke_cv fills.
 *   jaero_debug_burst_track_peek  the chain's scalars of one channel.  Burst OQPSK has no fir_pos .. gcnt, mc_freq and diff_last (0), burst MSK
 *                                 no yui, insertpre and lastmse (0 / as created).
 *   jaero_debug_burst_track_fill  every soft row (all soft_cap entries of all nchp channels) = soft_value, every symbol row entry = sym_value:
 *                                 before the first launch, so that a store outside the counted part of a row shows.
 *   jaero_debug_burst_track_read  what = 0: a channel's whole soft row (caprows >= soft_cap int16); what = 1: its whole symbol log (caprows >=
 *                                 sym_cap rows of 3 doubles), entries behind the counts included.  Events: jaero_debug_burst_front_events. */
typedef struct jaero_burst_track_geom
{
    int D2, soft_cap, sym_cap, ev_cap, msema_len, win_ring, agc2_len, eb_len, startstopstart, firn, ldsn, ebno_tail;
} jaero_burst_track_geom;
typedef struct jaero_burst_track_state
{
    int startstop, cntr, yui, insertpre, nrx, soft_cnt, sym_cnt, ev_cnt, overflow, msema_pos;
    int fir_pos, eb_pos, dly_pos, d8_pos, a1_pos, gcnt; /* burst MSK: the rings that advance only while the channel's gate is open */
    double mse, lastmse, m2_freq, st_freq, vol_gain, eb_ebno, rot_freq, agc2_sum, eb_esum, eb_e2sum, msema_sum;
    double mc_freq, diff_last, m2_ptr, st_ptr, stq_ptr;
} jaero_burst_track_state;
int jaero_debug_burst_track_geom(jaero_ctx *ctx, jaero_burst_track_geom *out);
int jaero_debug_burst_track(jaero_ctx *ctx, int n, int first_of_write, const int *channels, const int *ev_pos, const jaero_trident_result *verdicts, int nlist);
int jaero_debug_burst_track_peek(jaero_ctx *ctx, int channel, jaero_burst_track_state *st);
int jaero_debug_burst_track_fill(jaero_ctx *ctx, int soft_value, double sym_value);
int jaero_debug_burst_track_read(jaero_ctx *ctx, int channel, int what, void *rows, int caprows);
/* k_burst_msk_center_freq between two segments of the hook above: what jaero_center_freq_changed launches for one channel in [0, nchannels) of a
 * burst MSK bank (any other bank: JAERO_EINVAL), stamped with the bank's sample count = the next segment's first sample.  Marks the bank. */
int jaero_debug_burst_track_center_freq(jaero_ctx *ctx, int channel, double hz);

/* ------------------------------------------------------------------------------------------------ multi-GPU edge operations
 * The path shards by channel with no steady-state exchange (the reference runs its two stereo burst channels as two unrelated objects,
 * JAERO/audioburstoqpskdemodulator.cpp:8-10); the north star names two operations at the edges: fan out shared PCM, gather decoded bits.
 * One jaero_comm per GPU (one process or thread each): RCCL point-to-point sends over xGMI, grouped per call; contiguous channel ranges
 * [rank * N / W, (rank + 1) * N / W) (jaero_shard_range), the same as jaero_amd/dist.py.  RCCL is loaded on first use (dlopen): hosts with
 * one GPU never need it.  world = 1 with id = NULL is a communicator without RCCL (both operations are local copies).
 * ANY RCCL error invalidates the jaero_comm: a group that failed half-queued is closed, the communicator is aborted (ncclCommAbort) and every
 * later call on it returns JAERO_EHIP -- destroy it and create a new one on every rank. */
typedef struct jaero_comm jaero_comm;
#define JAERO_COMM_ID_BYTES 128
int jaero_shard_range(int nch_total, int rank, int world, int *lo, int *hi);
int jaero_comm_get_unique_id(void *id_128_bytes);            /* on one rank; hand the 128 bytes to the others (= ncclGetUniqueId) */
int jaero_comm_create(int device, int rank, int world, const void *id_128_bytes, jaero_comm **out);
void jaero_comm_destroy(jaero_comm *comm);
/* rank `src` holds frame-major PCM [nsamples][nch_total] on its device (the layout jaero_write takes with JAERO_PCM_FRAME_MAJOR); every
 * rank receives its channel slice, contiguous, [nsamples][hi - lo], in d_mine.  Enqueued on `stream`. */
int jaero_fan_out_pcm(jaero_comm *comm, int src, const int16_t *d_frames_all, int nsamples, int nch_total, int16_t *d_mine, void *stream);
/* every rank's soft-bit rows [hi - lo][cap] and counts [hi - lo] (the buffers behind jaero_softbits_view) arrive on rank `dst` as
 * [nch_total][cap] / [nch_total].  Enqueued on `stream`. */
int jaero_gather_softbits(jaero_comm *comm, int dst, const int16_t *d_soft, const int *d_counts, int nch_total, int cap,
                          int16_t *d_soft_all, int *d_counts_all, void *stream);

/* introspection */
int jaero_abi_version(void);
int jaero_num_channels(const jaero_ctx *ctx);
const char *jaero_strerror(int code);
const char *jaero_last_error(void);
/* Time (ms) the GPU spent in each kernel class over the jaero_write calls since the last reset, measured with HIP
 * events on the launch stream; enabled by jaero_profile_enable(ctx,1).  which: 0 = sample-loop kernel,
 * 1 = coarse-frequency kernel (burst kinds: trident check), 2 = PCM transpose / history push, 3 = Hilbert FIR (burst),
 * 4 = burst front end (burst).  *launches receives the launch count. */
int jaero_profile_enable(jaero_ctx *ctx, int on);
int jaero_profile_read(jaero_ctx *ctx, int which, double *total_ms, int *launches, int reset);
/* The name (up to the template arguments) of the kernel this bank launches for class `which`, as a profiler prints it: lets a harness
 * check that counter summaries it holds (profiles/pmc_summary*.json) belong to the kernel that actually ran. */
int jaero_profile_kernel(jaero_ctx *ctx, int which, char *buf, int cap);

#ifdef __cplusplus
}
#endif
#endif /* JAERO_HIP_H */
