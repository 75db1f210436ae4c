// chan_host.h -- host side of the wideband I/Q channeliser (k_chan.h; SURVEY 8 row f3, the channeliser half).
//
// One jaero_chan turns interleaved int16 I/Q at out_rate x D (out_rate 48, 24 or 12 kHz: a label that enters no arithmetic) into one compact channel-major int16 array per write: exactly what jaero_write
// takes with JAERO_PCM_CHANNEL_MAJOR, is_device_ptr = 1.  State between writes: the input history (previous hop + the partial hop a ragged
// write leaves; two buffers, the tail of one is copied to the head of the other behind every write that completed a block), the number of
// blocks done, and the channels' parameters.  Everything about frequency is integer arithmetic on the host (chan_param).
#pragma once
#include "k_chan.h" // (here and not among the kernel headers at the top of jaero_hip.hip: tests cite that file's lines by number)
#include "k_chan_capture.h"

// What jaero_chan3_create adds to a handle (capture_host.h): the capture's description in lowest terms, the raw history and the counts.
struct ChanCapture
{
    int format = 0, fs_in = 0, K = 1, L = 1, Mr = 1, bps = 4; // bps: bytes per raw I/Q pair
    unsigned shift = 0;
    bool resample = false;
    char *d_raw[2] = {nullptr, nullptr}; // [K - 1 + max_write_iq] raw pairs each; d_raw[rcur] holds the last K - 1 pairs, then the write's
    int rcur = 0;
    double *d_hp = nullptr;              // [L][K]: hp[phi K + j] = h[phi + j L]
    double2 *d_z[2] = {nullptr, nullptr}; // the channeliser's history in fp64, [2 Hp + smax] each, used as d_in is
    long long T = 0, m = 0;              // capture samples taken, staged samples made
    const double2 *last_ptr = nullptr;   // what the last write staged (jaero_chan3_read_staged)
    int last_n = 0;
    long long last_first = 0;
};

// A channeliser is two halves.  The front end consumes input: the histories, the spectrum d_spec of the blocks the last write completed, the
// forward transform's twiddles, the counts, the optional capture, and the stream state every call of its outputs goes by.
struct ChanOut;
struct ChanFront : DevHandle
{
    int max_write_iq = 0, nblk_max = 0;
    DevMem mem;
    int *d_in[2] = {nullptr, nullptr}; // [2 Hp + max_write_iq] dwords (I, Q) each; d_in[cur] holds: previous hop, then `pending` samples
    int cur = 0, pending = 0;
    long long blocks_done = 0;
    double2 *d_spec = nullptr; // [nblk_max][N]
    double2 *d_tw = nullptr;   // [N]: W_N^k (wg_fft14_e32)
    std::unique_ptr<ChanCapture> cap; // null unless jaero_chan3_create or jaero_split_create gave a capture
    KernelTimer timer{8};      // 0 k_chan_fwd, 4 k_capture_stage, 5 k_capture_fwd (the numbering is the outputs': their slots stay empty here)
    std::vector<ChanOut *> outs; // whose kernels run behind the forward transform, in output order: one, or a splitter's
};

// An output turns d_spec into channels: the response, the synthesis' twiddles, the channels' parameters, the PCM, the survey and the activity.
struct ChanOut
{
    ChanFront *front = nullptr; // whose d_spec it reads
    int decim = 0, out_rate = 0, nch = 0;
    int M = 0, Mo = 0;
    DevMem mem;
    double2 *d_gm = nullptr;   // [M]
    double2 *d_twm = nullptr;  // [32]
    ChanParam *d_par = nullptr;
    int16_t *d_pcm = nullptr;  // [nch][nout of the last write], capacity nch * nblk_max * Mo
    int last_nout = 0;
    std::vector<jaero_chan_channel> channels;
    KernelTimer timer{8};      // 1 k_chan_synth, 2 k_chan_psd, 3 k_chan_level,
                               // 6 k_chan_psd and 7 k_chan_level whenever the launch serves the activity (fused with the survey's part or not)
    // the survey (jaero_survey_*): nothing below exists before the first enable
    int survey = 0;            // bit 0 spectrum, bit 1 levels
    double *d_psd = nullptr;   // [N]: S
    double *d_lvl = nullptr;   // [nch]: E
    double *d_g2 = nullptr;    // [M]: |G[q mod N]|^2 / N^2 at q = i - M / 2
    long long psd_blocks = 0;  // blocks in S
    long long lvl_blocks = 0;  // blocks surveyed for levels since enable / reset; channel c's count is lvl_blocks - lvl_start[c]
    std::vector<long long> lvl_start;
    // the activity (jaero_activity_*): nothing below exists before the first enable
    int activity = 0;          // bit 0 peak-hold spectrum, bit 1 block statistics
    double *d_peak = nullptr;  // [N]: P
    ChanAct act{};             // emax, emin, when [nch], hist [nch][64]
    long long peak_blocks = 0; // blocks in P
    long long act_blocks = 0;  // blocks whose statistics were taken since enable / reset; channel c's count is act_blocks - act_start[c]
    std::vector<long long> act_start;
};

// The handle: an output, with the front end it owns -- or without one, as jaero_split_output hands it out: a view, whose front is its splitter's
// (split_host.h).  A view refuses the calls that consume input or own the handle, and names the splitter's call.
struct jaero_chan : ChanOut
{
    std::unique_ptr<ChanFront> own;
};
#define CHANVIEWCHK(c, who, use) do { if (!(c)->own) return fail(JAERO_EINVAL, who ": the handle is an output of a splitter (jaero_split_output); use " use); } while (0)

static bool chan_channel_ok(const jaero_chan_channel &ch) { return __builtin_isfinite(ch.gain) && ch.gain > 0; }

// b = nearest bin of the tuning word read as a signed number, rho = what is left, w = audio - rho D (mod 2^32)
static ChanParam chan_param(const jaero_chan_channel &ch, int decim)
{
    const long long t = (long long)(int32_t)ch.tune;
    const long long b = (t + (1ll << 17)) >> 18; // arithmetic shift
    const long long rho = t - b * (1ll << 18);
    ChanParam p;
    p.b = (int)b;
    p.w = (unsigned)((unsigned long long)((long long)ch.audio - rho * decim)); // mod 2^32
    p.gain = ch.gain;
    return p;
}

// G[q mod N] / N for the M bins a channel keeps, in the inverse transform's input order (k < M / 2: q = k, else q = k - M); G = DFT_N of the
// zero-padded taps, summed directly (M x L products) from one table of exp(-2 pi i k / N)
static std::vector<double2> chan_response(const double *taps, int ntaps, int M)
{
    const std::vector<double2> tw = twiddles(CHAN_N, CHAN_N);
    std::vector<double2> g(M);
    for (int k = 0; k < M; k++)
    {
        const int q = (k < M / 2 ? k : k - M) & (CHAN_N - 1);
        double re = 0, im = 0;
        for (int n = 0; n < ntaps; n++)
        {
            const double2 w = tw[(unsigned)(q * n) & (CHAN_N - 1)];
            re += taps[n] * w.x; im += taps[n] * w.y;
        }
        g[k] = make_double2(re / CHAN_N, im / CHAN_N);
    }
    return g;
}

extern "C" void jaero_chan_destroy(jaero_chan *c)
{
    if (!c || !c->own) return; // a view goes with its splitter (jaero_split_destroy)
    c->own->teardown();
    delete c;
}

// who: the create the messages name (a splitter names its own and the output)
static int chan_check_create(const char *who, int decim, int out_rate, int nchannels, const jaero_chan_channel *ch, const double *taps, int ntaps, int max_write_iq)
{
    if (!ch || !taps) return fail(JAERO_EINVAL, "%s: null channels / taps", who);
    if (decim != 16 && decim != 32 && decim != 64 && decim != 128 && decim != 256)
        return fail(JAERO_EINVAL, "%s: decim %d is not 16, 32, 64, 128 or 256", who, decim);
    if (out_rate != 48000 && out_rate != 24000 && out_rate != 12000)
        return fail(JAERO_EINVAL, "%s: out_rate %d is not 48000, 24000 or 12000", who, out_rate);
    if (nchannels < 1) return fail(JAERO_EINVAL, "%s: nchannels %d < 1", who, nchannels);
    if (ntaps < 1 || ntaps > CHAN_N / 2 + 1) return fail(JAERO_EINVAL, "%s: ntaps %d outside [1, %d]", who, ntaps, CHAN_N / 2 + 1);
    if (max_write_iq < 1) return fail(JAERO_EINVAL, "%s: max_write_iq %d < 1", who, max_write_iq);
    for (int i = 0; i < nchannels; i++)
        if (!chan_channel_ok(ch[i])) return fail(JAERO_EINVAL, "%s: channel %d: gain %g is not finite and positive", who, i, ch[i].gain);
    for (int i = 0; i < ntaps; i++)
        if (!__builtin_isfinite(taps[i])) return fail(JAERO_EINVAL, "%s: tap %d is not finite", who, i);
    return 0;
}

// Everything behind the checks and the device, in two functions so that a splitter can build one front end and several outputs.  smax = 0: an
// int16 front end (history d_in, max_write_iq samples a write); smax > 0: a capture's, whose fp64 history (capture_host.h) takes at most smax
// staged samples a write -- d_in is not allocated.
static int chan_build_front(ChanFront *f, int device, int max_write_iq, long long smax)
{
    int rc = 0;
    f->device = device; f->max_write_iq = max_write_iq;
    f->nblk_max = smax > 0 ? (int)((smax + 1) / CHAN_HP + 1) : max_write_iq / CHAN_HP + 1; // the most blocks a write completes
    if (smax == 0)
    {
        const size_t nin = 2 * (size_t)CHAN_HP + (size_t)max_write_iq;
        DA(f->mem, f->d_in[0], nin);
        DA(f->mem, f->d_in[1], nin);
    }
    DA(f->mem, f->d_spec, (size_t)f->nblk_max * CHAN_N);
    DA(f->mem, f->d_tw, CHAN_N);
    HIPCHK(hipMemcpy(f->d_tw, twiddles(CHAN_N, CHAN_N).data(), sizeof(double2) * CHAN_N, hipMemcpyHostToDevice));
    HIPCHK(hipFuncSetAttribute((const void *)k_chan_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, C6_XCH * (int)sizeof(double)));
    return 0;
}

// an output behind the front end `f`, which is built: the last of f's outputs so far
static int chan_build_out(ChanOut *c, ChanFront *f, int decim, int out_rate, int nchannels, const jaero_chan_channel *ch, const double *taps, int ntaps)
{
    int rc = 0;
    c->front = f;
    c->decim = decim; c->out_rate = out_rate; c->nch = nchannels;
    c->M = CHAN_N / decim; c->Mo = c->M / 2;
    c->channels.assign(ch, ch + nchannels);
    DA(c->mem, c->d_gm, c->M);
    DA(c->mem, c->d_twm, 32);
    DA(c->mem, c->d_par, nchannels);
    DA(c->mem, c->d_pcm, (size_t)nchannels * f->nblk_max * c->Mo);
    std::vector<ChanParam> par(nchannels);
    for (int i = 0; i < nchannels; i++) par[i] = chan_param(ch[i], decim);
    HIPCHK(hipMemcpy(c->d_par, par.data(), sizeof(ChanParam) * nchannels, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_gm, chan_response(taps, ntaps, c->M).data(), sizeof(double2) * c->M, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_twm, twiddles(c->M, 32).data(), sizeof(double2) * 32, hipMemcpyHostToDevice));
    f->outs.push_back(c);
    return 0;
}

// a stand-alone handle: one of each
static int chan_build(std::unique_ptr<jaero_chan> &c, int device, int decim, int out_rate, int nchannels, const jaero_chan_channel *ch,
                      const double *taps, int ntaps, int max_write_iq, long long smax)
{
    c->own.reset(new (std::nothrow) ChanFront());
    if (!c->own) return fail(JAERO_ENOMEM, "jaero_chan2_create: out of memory");
    const int rc = chan_build_front(c->own.get(), device, max_write_iq, smax);
    return rc ? rc : chan_build_out(c.get(), c->own.get(), decim, out_rate, nchannels, ch, taps, ntaps);
}

// decim: the total decimation from the capture to the output; out_rate: what the output is called (jaero_chan_feed compares it with the bank's Fs)
extern "C" int jaero_chan2_create(int device, int decim, int out_rate, int nchannels, const jaero_chan_channel *ch, const double *taps, int ntaps,
                                  int max_write_iq, jaero_chan **out)
{
    if (!out) return fail(JAERO_EINVAL, "jaero_chan2_create: out is null");
    *out = nullptr;
    { const int rc = chan_check_create("jaero_chan2_create", decim, out_rate, nchannels, ch, taps, ntaps, max_write_iq); if (rc) return rc; }
    { const int rc = open_device(device); if (rc) return rc; }
    std::unique_ptr<jaero_chan> c(new (std::nothrow) jaero_chan());
    if (!c) return fail(JAERO_ENOMEM, "jaero_chan2_create: out of memory");
    const int rc = chan_build(c, device, decim, out_rate, nchannels, ch, taps, ntaps, max_write_iq, 0);
    if (rc) return rc;
    *out = c.release();
    return 0;
}

// the 48 kHz channeliser of ABI 1: its own range of decim, everything else is jaero_chan2_create's
extern "C" int jaero_chan_create(int device, int decim, int nchannels, const jaero_chan_channel *ch, const double *taps, int ntaps,
                                 int max_write_iq, jaero_chan **out)
{
    if (out) *out = nullptr;
    if (decim != 16 && decim != 32 && decim != 64) return fail(JAERO_EINVAL, "jaero_chan_create: decim %d is not 16, 32 or 64", decim);
    return jaero_chan2_create(device, decim, 48000, nchannels, ch, taps, ntaps, max_write_iq, out);
}

// f(D) with the output's decimation as a std::integral_constant: the instantiation of a kernel family that serves it
template <class F>
static void by_decim(int decim, F f)
{
    if (decim == 16) f(std::integral_constant<int, 16>());
    else if (decim == 32) f(std::integral_constant<int, 32>());
    else if (decim == 64) f(std::integral_constant<int, 64>());
    else if (decim == 128) f(std::integral_constant<int, 128>());
    else f(std::integral_constant<int, 256>());
}

// levels, block statistics or both in one pass over spec (p0: absolute index of the write's first block, for `when`)
template <bool LEVEL, bool ACT>
static void chan_launch_level(const ChanOut *c, int nblk, long long p0, hipStream_t st)
{
    by_decim(c->decim, [&](auto d) {
        hipLaunchKernelGGL((k_chan_level<decltype(d)::value, LEVEL, ACT>), dim3((unsigned)((c->nch + CHAN_LVL_THREADS / CHAN_LVL_T - 1) / (CHAN_LVL_THREADS / CHAN_LVL_T))),
                           dim3(CHAN_LVL_THREADS), 0, st, (const double2 *)c->front->d_spec, (const double *)c->d_g2, (const ChanParam *)c->d_par,
                           c->d_lvl, c->nch, nblk, c->act, p0);
    });
}

static void chan_launch_synth(const ChanOut *c, int nblk, long long p0, hipStream_t st)
{
    const long long nitems = (long long)c->nch * nblk;
    by_decim(c->decim, [&](auto d) {
        using Shape = ChanShape<decltype(d)::value>;
        hipLaunchKernelGGL(k_chan_synth<decltype(d)::value>, dim3((unsigned)((nitems + Shape::ITEMS - 1) / Shape::ITEMS)), dim3(Shape::THREADS), 0, st,
                           (const double2 *)c->front->d_spec, (const double2 *)c->d_gm, (const double2 *)c->d_twm, (const ChanParam *)c->d_par, c->d_pcm,
                           c->nch, nblk, p0);
    });
}

// An output's half of what a write does behind its forward transform of nblk > 0 blocks, the first of them block p0: the synthesis, then the
// survey's and the activity's kernels when enabled, over its front end's d_spec.
static int chan_outputs(ChanOut *c, int nblk, long long p0, hipStream_t st)
{
    int pi = c->timer.begin(1, st);
    chan_launch_synth(c, nblk, p0, st);
    LAUNCHCHK("k_chan_synth");
    c->timer.end(pi, st);
    // one launch of k_chan_psd serves the survey's spectrum, the activity's peak or both; timed under the activity's slot when it serves that
    const bool sum = c->survey & 1, peak = c->activity & 1;
    if (sum || peak)
    {
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(CHAN_N / CHAN_PSD_THREADS), dim3(CHAN_PSD_THREADS), 0, st, (const double2 *)c->front->d_spec, c->d_psd, nblk,
                               c->d_peak);
        };
        pi = c->timer.begin(peak ? 6 : 2, st);
        if (sum && peak) go(k_chan_psd<true, true>);
        else if (sum) go(k_chan_psd<true, false>);
        else go(k_chan_psd<false, true>);
        LAUNCHCHK("k_chan_psd");
        c->timer.end(pi, st);
        if (sum) c->psd_blocks += nblk;
        if (peak) c->peak_blocks += nblk;
    }
    // and one of k_chan_level the levels, the block statistics or both
    const bool lvl = c->survey & 2, blk = c->activity & 2;
    if (lvl || blk)
    {
        pi = c->timer.begin(blk ? 7 : 3, st);
        if (lvl && blk) chan_launch_level<true, true>(c, nblk, p0, st);
        else if (lvl) chan_launch_level<true, false>(c, nblk, p0, st);
        else chan_launch_level<false, true>(c, nblk, p0, st);
        LAUNCHCHK("k_chan_level");
        c->timer.end(pi, st);
        if (lvl) c->lvl_blocks += nblk;
        if (blk) c->act_blocks += nblk;
    }
    return 0;
}

// What every write does first (who: the entry point the messages name): the checks, the write's stream ordered behind the last one's (a bank
// fed from it included), and the results of the write zeroed -- nout[g] and last_nout of output g, and what the capture staged.
static int chan_write_enter(ChanFront *f, const void *iq, int niq, hipStream_t st, int *nout, const char *who)
{
    if (niq < 0 || (niq > 0 && !iq)) return fail(JAERO_EINVAL, "%s: bad arguments", who);
    if (niq > f->max_write_iq) return fail(JAERO_EINVAL, "%s: niq %d exceeds max_write_iq %d", who, niq, f->max_write_iq);
    POISONCHK(f, who, POISON_CHAN);
    HIPCHK(hipSetDevice(f->device));
    { const int rc = f->order_behind(st); if (rc) return rc; }
    for (size_t g = 0; g < f->outs.size(); g++) f->outs[g]->last_nout = nout[g] = 0;
    if (f->cap) { f->cap->last_n = 0; f->cap->last_first = f->cap->m; f->cap->last_ptr = nullptr; }
    return 0;
}

// What every write does behind its forward transform of nblk > 0 blocks: every output's kernels, in output order (each with the (nch, nblk, p0)
// it would launch with were it the only one), then the last hop and what lies behind it (`total` samples wait in `hist`, of `elem` bytes
// each) become the head of the other history buffer `other`.
static int chan_after_fwd(ChanFront *f, int nblk, int total, const void *hist, void *other, size_t elem, hipStream_t st)
{
    for (ChanOut *o : f->outs) { const int rc = chan_outputs(o, nblk, f->blocks_done, st); if (rc) return rc; }
    const int rest = total - nblk * CHAN_HP;
    HIPCHK(hipMemcpyAsync(other, (const char *)hist + (size_t)nblk * CHAN_HP * elem, elem * (size_t)(CHAN_HP + rest), hipMemcpyDeviceToDevice, st));
    f->cur ^= 1;
    f->pending = rest;
    f->blocks_done += nblk;
    return 0;
}

// and last: the write is in, output g has nblk * Mo new samples a channel
static int chan_write_leave(ChanFront *f, int nblk, int *nout, PoisonGuard &guard)
{
    HIPCHK(hipGetLastError());
    for (size_t g = 0; g < f->outs.size(); g++) f->outs[g]->last_nout = nout[g] = nblk * f->outs[g]->Mo;
    guard.commit();
    return 0;
}

static int capture_write(ChanFront *f, const void *iq, int niq, int is_device_ptr, void *stream, int *nout, const char *who);

// the write of an int16 front end; nout: one entry per output
static int chan_write(ChanFront *f, const int16_t *iq, int niq, int is_device_ptr, void *stream, int *nout, const char *who)
{
    hipStream_t st = (hipStream_t)stream;
    { const int rc = chan_write_enter(f, iq, niq, st, nout, who); if (rc) return rc; }
    if (niq == 0) return 0;
    int *in = f->d_in[f->cur];
    HIPCHK(hipMemcpyAsync(in + CHAN_HP + f->pending, iq, sizeof(int) * (size_t)niq, is_device_ptr ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    PoisonGuard guard(*f); // from here on the history, the block count and the device buffers advance together or not at all
    const int total = f->pending + niq;
    const int nblk = total / CHAN_HP;
    f->pending = total;
    if (nblk > 0)
    {
        const int pi = f->timer.begin(0, st);
        hipLaunchKernelGGL(k_chan_fwd, dim3(nblk), dim3(C2_THREADS), C6_XCH * sizeof(double), st, (const int *)in, f->d_spec, (const double2 *)f->d_tw);
        LAUNCHCHK("k_chan_fwd");
        f->timer.end(pi, st);
        { const int rc = chan_after_fwd(f, nblk, total, in, f->d_in[f->cur ^ 1], sizeof(int), st); if (rc) return rc; }
    }
    return chan_write_leave(f, nblk, nout, guard);
}

extern "C" int jaero_chan_write(jaero_chan *c, const int16_t *iq, int niq, int is_device_ptr, void *stream, int *nout)
{
    if (!c || !nout || niq < 0 || (niq > 0 && !iq)) return fail(JAERO_EINVAL, "jaero_chan_write: bad arguments");
    CHANVIEWCHK(c, "jaero_chan_write", "jaero_split_write");
    if (c->own->cap)
    {
        if (c->own->cap->format != JAERO_IQ_CS16)
            return fail(JAERO_EINVAL, "jaero_chan_write: the handle's capture format is %d, not int16 I/Q; use jaero_chan3_write", c->own->cap->format);
        return capture_write(c->own.get(), iq, niq, is_device_ptr, stream, nout, "jaero_chan_write");
    }
    return chan_write(c->own.get(), iq, niq, is_device_ptr, stream, nout, "jaero_chan_write");
}

extern "C" int jaero_chan_pcm_view(jaero_chan *c, void **dev_pcm, int *nsamples)
{
    if (!c || !dev_pcm || !nsamples) return fail(JAERO_EINVAL, "jaero_chan_pcm_view: null argument");
    POISONCHK(c->front, "jaero_chan_pcm_view", POISON_CHAN);
    *dev_pcm = c->d_pcm;
    *nsamples = c->last_nout;
    return 0;
}

extern "C" int jaero_chan_read_pcm(jaero_chan *c, int16_t *dst, int cap_per_channel, int *nsamples)
{
    if (!c || !dst || !nsamples || cap_per_channel < 0) return fail(JAERO_EINVAL, "jaero_chan_read_pcm: bad arguments");
    POISONCHK(c->front, "jaero_chan_read_pcm", POISON_CHAN);
    if (cap_per_channel < c->last_nout)
        return fail(JAERO_EINVAL, "jaero_chan_read_pcm: cap_per_channel %d is below the last write's %d samples", cap_per_channel, c->last_nout);
    QUIESCE(c->front);
    *nsamples = c->last_nout;
    if (c->last_nout > 0)
        HIPCHK(hipMemcpy2D(dst, sizeof(int16_t) * (size_t)cap_per_channel, c->d_pcm, sizeof(int16_t) * (size_t)c->last_nout,
                           sizeof(int16_t) * (size_t)c->last_nout, (size_t)c->nch, hipMemcpyDeviceToHost));
    return 0;
}

// The block statistics of channels [first, end) as they are before a channel's first block: when = -1 (what the kernel reads as "no block
// yet"; emax and emin are then not read, and are zeroed only so that the memory is defined), hist = 0.
static int activity_clear_blocks(ChanOut *c, int first, int end)
{
    const size_t n = (size_t)(end - first);
    HIPCHK(hipMemset(c->act.emax + first, 0, sizeof(double) * n));
    HIPCHK(hipMemset(c->act.emin + first, 0, sizeof(double) * n));
    HIPCHK(hipMemset(c->act.when + first, 0xff, sizeof(long long) * n));
    HIPCHK(hipMemset(c->act.hist + (size_t)first * CHAN_ACT_BINS, 0, sizeof(unsigned) * CHAN_ACT_BINS * n));
    for (int i = first; i < end; i++) c->act_start[i] = c->act_blocks;
    return 0;
}

extern "C" int jaero_chan_retune(jaero_chan *c, int channel, const jaero_chan_channel *ch)
{
    if (!c || !ch || channel < 0 || channel >= c->nch) return fail(JAERO_EINVAL, "jaero_chan_retune: bad arguments");
    if (!chan_channel_ok(*ch)) return fail(JAERO_EINVAL, "jaero_chan_retune: gain %g is not finite and positive", ch->gain);
    POISONCHK(c->front, "jaero_chan_retune", POISON_CHAN);
    QUIESCE(c->front); // the writes enqueued so far keep the old words
    const ChanParam p = chan_param(*ch, c->decim);
    PoisonGuard guard(*c->front); // the words, the sum and the count change together or not at all
    HIPCHK(hipMemcpy(c->d_par + channel, &p, sizeof p, hipMemcpyHostToDevice));
    if ((c->survey & 2) && ch->tune != c->channels[channel].tune) // another b: the level starts again with the next write
    {
        HIPCHK(hipMemset(c->d_lvl + channel, 0, sizeof(double)));
        c->lvl_start[channel] = c->lvl_blocks;
    }
    if ((c->activity & 2) && ch->tune != c->channels[channel].tune) // and so do its block statistics
    {
        const int rc = activity_clear_blocks(c, channel, channel + 1);
        if (rc) return rc;
    }
    c->channels[channel] = *ch;
    guard.commit();
    return 0;
}

// jaero_chan_retune of every channel behind one synchronisation, with one copy; nothing changes unless every gain is valid
extern "C" int jaero_chan2_retune_all(jaero_chan *c, const jaero_chan_channel *ch)
{
    if (!c || !ch) return fail(JAERO_EINVAL, "jaero_chan2_retune_all: null argument");
    for (int i = 0; i < c->nch; i++)
        if (!chan_channel_ok(ch[i])) return fail(JAERO_EINVAL, "jaero_chan2_retune_all: channel %d: gain %g is not finite and positive", i, ch[i].gain);
    POISONCHK(c->front, "jaero_chan2_retune_all", POISON_CHAN);
    QUIESCE(c->front); // the writes enqueued so far keep the old words
    std::vector<ChanParam> par(c->nch);
    for (int i = 0; i < c->nch; i++) par[i] = chan_param(ch[i], c->decim);
    PoisonGuard guard(*c->front); // the words, the sums and the counts change together or not at all
    HIPCHK(hipMemcpy(c->d_par, par.data(), sizeof(ChanParam) * c->nch, hipMemcpyHostToDevice));
    if ((c->survey & 2) || (c->activity & 2))
    {
        int first = -1; // the channels whose tune word changes, cleared a run at a time
        for (int i = 0; i <= c->nch; i++)
        {
            const bool moved = i < c->nch && ch[i].tune != c->channels[i].tune;
            if (moved && first < 0) first = i;
            if (!moved && first >= 0)
            {
                if (c->survey & 2) HIPCHK(hipMemset(c->d_lvl + first, 0, sizeof(double) * (size_t)(i - first)));
                if (c->activity & 2) { const int rc = activity_clear_blocks(c, first, i); if (rc) return rc; }
                first = -1;
            }
            if (moved && (c->survey & 2)) c->lvl_start[i] = c->lvl_blocks;
        }
    }
    c->channels.assign(ch, ch + c->nch);
    guard.commit();
    return 0;
}

// what a feed checks on the bank before anything advances
static int chan_feed_check(const ChanOut *c, const jaero_ctx *bank, const char *who)
{
    if (bank->device != c->front->device) return fail(JAERO_EINVAL, "%s: the bank is on device %d, the channeliser on %d", who, bank->device, c->front->device);
    if (bank->o_nch != c->nch) return fail(JAERO_EINVAL, "%s: the bank has %d channels, the channeliser %d", who, bank->o_nch, c->nch);
    for (const jaero_settings &s : bank->settings)
        if (s.Fs != (double)c->out_rate)
            return fail(JAERO_EINVAL, "%s: the bank runs at Fs = %g; the channeliser's output is %d", who, s.Fs, c->out_rate);
    const int nblk_max = c->front->nblk_max;
    if (bank->max_write < nblk_max * c->Mo)
        return fail(JAERO_EINVAL, "%s: the bank's max_write_samples %d is below the %d blocks a write can complete * %d = %d", who, bank->max_write,
                    nblk_max, c->Mo, nblk_max * c->Mo);
    return 0;
}

extern "C" int jaero_chan_feed(jaero_chan *c, jaero_ctx *bank, const int16_t *iq, int niq, int is_device_ptr, void *stream, int *nout)
{
    if (!c || !bank || !nout) return fail(JAERO_EINVAL, "jaero_chan_feed: null argument");
    CHANVIEWCHK(c, "jaero_chan_feed", "jaero_split_feed");
    { const int rc = chan_feed_check(c, bank, "jaero_chan_feed"); if (rc) return rc; }
    int rc = jaero_chan_write(c, iq, niq, is_device_ptr, stream, nout);
    if (rc || *nout <= 0) return rc;
    return jaero_write(bank, c->d_pcm, *nout, JAERO_PCM_CHANNEL_MAJOR, 1, stream);
}

extern "C" int jaero_chan_profile_enable(jaero_chan *c, int on)
{
    if (!c) return fail(JAERO_EINVAL, "jaero_chan_profile_enable: null ctx");
    c->timer.on = on != 0;
    if (c->own) c->own->timer.on = on != 0; // (a view's front end is switched by jaero_split_profile_enable)
    return 0;
}

// The handle's total of timer slot `slot`: the front end's kernels (0, 4, 5) are timed by the front end the handle owns -- a view owns none, and
// reports the empty slots of its own timer: those kernels are its splitter's (jaero_split_profile_read).
static int chan_timer_read(jaero_chan *c, int slot, double *total_ms, int *launches, int reset)
{
    const bool fwd = slot == 0 || slot == 4 || slot == 5;
    return (fwd && c->own ? c->own->timer : c->timer).read(c->front->device, slot, total_ms, launches, reset);
}

extern "C" int jaero_chan_profile_read(jaero_chan *c, int which, double *total_ms, int *launches, int reset)
{
    if (!c || which < 0 || which > 1) return fail(JAERO_EINVAL, "jaero_chan_profile_read: bad arguments");
    return chan_timer_read(c, which, total_ms, launches, reset);
}

// ------------------------------------------------------------------------------------------ survey
static int survey_clear(ChanOut *c)
{
    if (c->survey & 1)
    {
        HIPCHK(hipMemset(c->d_psd, 0, sizeof(double) * CHAN_N));
        c->psd_blocks = 0;
    }
    if (c->survey & 2)
    {
        HIPCHK(hipMemset(c->d_lvl, 0, sizeof(double) * (size_t)c->nch));
        c->lvl_blocks = 0;
        c->lvl_start.assign(c->nch, 0);
    }
    return 0;
}

// The table k_chan_level multiplies by, built by whichever of the levels and the block statistics is enabled first: |G / N|^2 of the
// response the synthesis multiplies by, from its order (k < M / 2: q = k, else q = k - M) to ascending q
static int chan_build_g2(ChanOut *c)
{
    if (c->d_g2) return 0;
    int rc = 0;
    double *d_g2 = nullptr;
    DA(c->mem, d_g2, c->M);
    std::vector<double2> gm(c->M);
    std::vector<double> g2(c->M);
    HIPCHK(hipMemcpy(gm.data(), c->d_gm, sizeof(double2) * c->M, hipMemcpyDeviceToHost));
    for (int i = 0; i < c->M; i++)
    {
        const double2 g = gm[(i - c->M / 2) & (c->M - 1)];
        g2[i] = g.x * g.x + g.y * g.y;
    }
    HIPCHK(hipMemcpy(d_g2, g2.data(), sizeof(double) * c->M, hipMemcpyHostToDevice));
    c->d_g2 = d_g2;
    return 0;
}

extern "C" int jaero_survey_enable(jaero_chan *c, int what)
{
    if (what < 0 || what > 3) return fail(JAERO_EINVAL, "jaero_survey_enable: what %d has bits outside 0..3", what);
    if (!c) return fail(JAERO_EINVAL, "jaero_survey_enable: null ctx");
    POISONCHK(c->front, "jaero_survey_enable", POISON_CHAN);
    QUIESCE(c->front); // the writes enqueued so far are surveyed as they were enqueued
    int rc = 0;
    if ((what & 1) && !c->d_psd) DA(c->mem, c->d_psd, CHAN_N);
    if (what & 2)
    {
        if (!c->d_lvl) DA(c->mem, c->d_lvl, c->nch);
        if ((rc = chan_build_g2(c))) return rc; // the levels can be enabled only with the table in place
    }
    c->survey = what;
    rc = survey_clear(c);
    if (rc) c->survey = 0; // a failed clear leaves the survey off
    return rc;
}

extern "C" int jaero_survey_reset(jaero_chan *c)
{
    if (!c) return fail(JAERO_EINVAL, "jaero_survey_reset: null ctx");
    POISONCHK(c->front, "jaero_survey_reset", POISON_CHAN);
    QUIESCE(c->front);
    return survey_clear(c);
}

extern "C" int jaero_survey_read_psd(jaero_chan *c, double *sums, long long *nblocks)
{
    if (!c || !sums || !nblocks) return fail(JAERO_EINVAL, "jaero_survey_read_psd: null argument");
    if (!(c->survey & 1)) return fail(JAERO_EINVAL, "jaero_survey_read_psd: the spectrum is not enabled (jaero_survey_enable bit 0)");
    POISONCHK(c->front, "jaero_survey_read_psd", POISON_CHAN);
    QUIESCE(c->front);
    HIPCHK(hipMemcpy(sums, c->d_psd, sizeof(double) * CHAN_N, hipMemcpyDeviceToHost));
    *nblocks = c->psd_blocks;
    return 0;
}

extern "C" int jaero_survey_read_levels(jaero_chan *c, double *sums, long long *nblocks)
{
    if (!c || !sums || !nblocks) return fail(JAERO_EINVAL, "jaero_survey_read_levels: null argument");
    if (!(c->survey & 2)) return fail(JAERO_EINVAL, "jaero_survey_read_levels: the levels are not enabled (jaero_survey_enable bit 1)");
    POISONCHK(c->front, "jaero_survey_read_levels", POISON_CHAN);
    QUIESCE(c->front);
    HIPCHK(hipMemcpy(sums, c->d_lvl, sizeof(double) * (size_t)c->nch, hipMemcpyDeviceToHost));
    for (int i = 0; i < c->nch; i++) nblocks[i] = c->lvl_blocks - c->lvl_start[i];
    return 0;
}

extern "C" int jaero_survey_profile_read(jaero_chan *c, int which, double *total_ms, int *launches, int reset)
{
    if (!c || which < 0 || which > 1) return fail(JAERO_EINVAL, "jaero_survey_profile_read: bad arguments");
    return chan_timer_read(c, 2 + which, total_ms, launches, reset);
}

// ------------------------------------------------------------------------------------------ activity
static_assert(CHAN_ACT_BINS == JAERO_ACT_BINS, "the kernel's row of hist is the ABI's");
static int activity_clear(ChanOut *c)
{
    if (c->activity & 1)
    {
        HIPCHK(hipMemset(c->d_peak, 0, sizeof(double) * CHAN_N));
        c->peak_blocks = 0;
    }
    if (c->activity & 2)
    {
        c->act_blocks = 0;
        c->act_start.assign(c->nch, 0);
        return activity_clear_blocks(c, 0, c->nch);
    }
    return 0;
}

extern "C" int jaero_activity_enable(jaero_chan *c, int what)
{
    if (what < 0 || what > 3) return fail(JAERO_EINVAL, "jaero_activity_enable: what %d has bits outside 0..3", what);
    if (!c) return fail(JAERO_EINVAL, "jaero_activity_enable: null ctx");
    POISONCHK(c->front, "jaero_activity_enable", POISON_CHAN);
    QUIESCE(c->front); // the writes enqueued so far are measured as they were enqueued
    int rc = 0;
    if ((what & 1) && !c->d_peak) DA(c->mem, c->d_peak, CHAN_N);
    if (what & 2)
    {
        if (!c->act.emax) DA(c->mem, c->act.emax, c->nch);
        if (!c->act.emin) DA(c->mem, c->act.emin, c->nch);
        if (!c->act.when) DA(c->mem, c->act.when, c->nch);
        if (!c->act.hist) DA(c->mem, c->act.hist, (size_t)c->nch * CHAN_ACT_BINS);
        if ((rc = chan_build_g2(c))) return rc; // the statistics can be enabled only with the table in place
    }
    c->activity = what;
    rc = activity_clear(c);
    if (rc) c->activity = 0; // a failed clear leaves the activity off
    return rc;
}

extern "C" int jaero_activity_reset(jaero_chan *c)
{
    if (!c) return fail(JAERO_EINVAL, "jaero_activity_reset: null ctx");
    POISONCHK(c->front, "jaero_activity_reset", POISON_CHAN);
    QUIESCE(c->front);
    return activity_clear(c);
}

extern "C" int jaero_activity_read_peak(jaero_chan *c, double *peak, long long *nblocks)
{
    if (!c || !peak || !nblocks) return fail(JAERO_EINVAL, "jaero_activity_read_peak: null argument");
    if (!(c->activity & 1)) return fail(JAERO_EINVAL, "jaero_activity_read_peak: the peak-hold spectrum is not enabled (jaero_activity_enable bit 0)");
    POISONCHK(c->front, "jaero_activity_read_peak", POISON_CHAN);
    QUIESCE(c->front);
    HIPCHK(hipMemcpy(peak, c->d_peak, sizeof(double) * CHAN_N, hipMemcpyDeviceToHost));
    *nblocks = c->peak_blocks;
    return 0;
}

extern "C" int jaero_activity_read_blocks(jaero_chan *c, double *emax, double *emin, long long *when, long long *nblocks, unsigned *hist)
{
    if (!c || !emax || !emin || !when || !nblocks) return fail(JAERO_EINVAL, "jaero_activity_read_blocks: null argument");
    if (!(c->activity & 2)) return fail(JAERO_EINVAL, "jaero_activity_read_blocks: the block statistics are not enabled (jaero_activity_enable bit 1)");
    POISONCHK(c->front, "jaero_activity_read_blocks", POISON_CHAN);
    QUIESCE(c->front);
    const size_t n = (size_t)c->nch;
    HIPCHK(hipMemcpy(emax, c->act.emax, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(emin, c->act.emin, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(when, c->act.when, sizeof(long long) * n, hipMemcpyDeviceToHost));
    if (hist) HIPCHK(hipMemcpy(hist, c->act.hist, sizeof(unsigned) * CHAN_ACT_BINS * n, hipMemcpyDeviceToHost));
    for (int i = 0; i < c->nch; i++)
    {
        nblocks[i] = c->act_blocks - c->act_start[i];
        if (nblocks[i] == 0) { emax[i] = 0.0; emin[i] = __builtin_inf(); when[i] = -1; } // the definition's values of a channel without a block
    }
    return 0;
}

extern "C" int jaero_activity_profile_read(jaero_chan *c, int which, double *total_ms, int *launches, int reset)
{
    if (!c || which < 0 || which > 1) return fail(JAERO_EINVAL, "jaero_activity_profile_read: bad arguments");
    return chan_timer_read(c, 6 + which, total_ms, launches, reset);
}

#include "capture_host.h"
#include "split_host.h"
