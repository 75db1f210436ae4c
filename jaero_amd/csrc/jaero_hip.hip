// jaero_hip.hip -- libjaero_hip.so: C ABI (include/jaero_hip.h) + host-side bank scheduler for the gfx950 kernels.
//
// Host responsibilities (everything numerical happens in the kernels):
//   * own the per-bank device state (layout: jaero_device.h),
//   * split each jaero_write at the samples where the reference runs its coarse-frequency estimate synchronously
//     inside writeData (bbcycbuff_ptr % (bbnfft/4) == 0, JAERO/oqpskdemodulator.cpp:416) -- a host mirror of the two
//     integer counters involved (bbcycbuff_ptr, coarseCounter) predicts those samples exactly, so no device->host
//     round trip is needed in steady state,
//   * launch [sample kernel] [coarse kernel] [sample kernel] ... on the caller's stream.
// No CPU fallback exists: without a HIP device jaero_create fails.
#include <hip/hip_runtime.h>
#include <assert.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/jaero_hip.h"
#include "jaero_device.h"
#include "k_oqpsk_fb.h"
#include "k_msk.h"
#include "k_msk_fb.h"
#include "k_pre8400.h"
#include "k_coarse.h"
#include "wg_fft.h"
#include "k_coarse6.h"
#include "k_viterbi.h"
#include "k_viterbi_lanes.h"
#include "burst_device.h"
#include "k_burst_front.h"
#include "k_burst_demod.h"
#include "k_burst_msk_fb.h"
#include "k_burst_settings.h"
#include "k_aerol.h"
#include "k_aerol_burst.h"

static thread_local std::string g_last_error;
static int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}
#define HIPCHK(x)                                                                                        \
    do {                                                                                                 \
        hipError_t _e = (x);                                                                             \
        if (_e != hipSuccess) return fail(JAERO_EHIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// right behind a kernel launch inside jaero_write: a launch that was refused (bad configuration, missing LDS attribute) is reported by
// name at the launch that failed, not as a stale error at the end of the call
#define LAUNCHCHK(what)                                                                                  \
    do {                                                                                                 \
        hipError_t _e = hipGetLastError();                                                               \
        if (_e != hipSuccess) return fail(JAERO_EHIP, "launch of %s failed: %s (%s:%d)", what, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
#include "host_common.h"

// k_msk_samples: matched-filter history slots kept in LDS (the rest in VGPRs)
#define MSK_LDSN_40 24 // of 40 taps (1200 bps at 24 kHz, 600 bps at 12 kHz)
#define MSK_LDSN_20 12 // of 20 taps (1200 bps at 12 kHz)

// Host mirror of the two integer counters that decide WHEN the reference runs its coarse-frequency estimate
// (bbcycbuff_ptr and coarseCounter, JAERO/oqpskdemodulator.cpp:410-431 == JAERO/mskdemodulator.cpp:350-368).
// A "segment" is a run of samples handed to one sample-kernel launch; it ends at the first sample (over all channels)
// whose ring write makes bbcycbuff_ptr % (cpuReduce ? nfft : nfft/4) == 0.  For that sample only the ring write
// ("A-part") is done; the rest of the sample ("B-part") runs in the next segment, after the coarse kernel.
struct Mirror
{
    int nch = 0, nchp = 0, nfft = 0, Fs_int = 0;
    std::vector<int> flags, bbptr, cnt;
    int pending = 0;        // A-part of the next sample already done
    long long nB_total = 0; // B-parts executed so far (uniform ring slots derive from it)
    std::vector<int> fired; // channels whose estimate fires at the end of the last planned segment

    // number of A-steps (>=1) until channel ch fires, given its coarseCounter before its next A-step
    long long steps_to_trigger(int ch, int cnt_before_first_a) const
    {
        if (!(flags[ch] & JF_CPUREDUCE))
        {
            const int q = nfft / 4;
            return q - (bbptr[ch] % q);
        }
        long long j0 = (long long)Fs_int - cnt_before_first_a + 1;
        if (j0 < 1) j0 = 1;
        const int r = nfft - (bbptr[ch] % nfft);
        return j0 + r - 1;
    }
    // Plans the segment starting at sample `pos` of a write of `nsamples`; returns its length n (samples pos..pos+n-1),
    // sets skip_a/only_a, fills `fired`, updates the counters, and returns the position the next segment starts at.
    int next_segment(int pos, int nsamples, int &n, int &skip_a, int &only_a)
    {
        long long dmin = (long long)1 << 60;
        for (int ch = 0; ch < nch; ch++)
        {
            const long long d = steps_to_trigger(ch, cnt[ch] + (pending ? 1 : 0));
            if (d < dmin) dmin = d;
        }
        const int first_a = pos + (pending ? 1 : 0);
        const long long trig_sample = (long long)first_a + dmin - 1;
        const bool trig = trig_sample < nsamples;
        const int end = trig ? (int)trig_sample + 1 : nsamples;
        n = end - pos;
        skip_a = pending;
        only_a = trig ? 1 : 0;
        const int acount = n - (pending ? 1 : 0);
        const int bcount = n - (trig ? 1 : 0);
        fired.clear();
        for (int ch = 0; ch < nchp; ch++)
        {
            const int cnt0 = cnt[ch] + (pending ? 1 : 0);
            long long fills;
            if (!(flags[ch] & JF_CPUREDUCE)) fills = acount;
            else
            {
                long long j0 = (long long)Fs_int - cnt0 + 1;
                if (j0 < 1) j0 = 1;
                fills = (long long)acount - (j0 - 1);
                if (fills < 0) fills = 0;
            }
            const bool f = trig && ch < nch && steps_to_trigger(ch, cnt0) == dmin;
            bbptr[ch] = (int)((bbptr[ch] + fills) % nfft);
            cnt[ch] += bcount;
            if (f) { cnt[ch] = 0; fired.push_back(ch); }
        }
        nB_total += bcount;
        pending = trig ? 1 : 0;
        return trig ? end - 1 : end;
    }
};

// One hot-path kernel of a bank as jaero_create / burst_create chose it: the instantiation, its launch shape, the dynamic LDS it is given
// (set as its attribute at create and requested by every launch, from this one number) and the name bench.py finds its counters under in
// profiles/ (jaero_profile_kernel).  What decides the choice is fixed for the bank's life: the flags, the bank's size, the rate -- a rate
// change creates a new bank (rebank_with_carry_over, burst_rebank) and with it new records.
template <class Fn>
struct KernelRec
{
    Fn fn = nullptr;
    int grid = 0; // workgroups (the coarse estimate: at most that many, persistent over the list)
    int block = 0;
    int lds = 0;  // dynamic LDS bytes
    int ldsn = 0; // sample loop: filter history slots in LDS (a launch's first ring slot = B-parts so far mod ldsn)
    const char *name = "";
    std::string variant; // the whole instantiation as `nm -C` spells it (test hook jaero_debug_kernel_variant)
};

// "k<a, b, ...>" with the template arguments spelled as `nm -C` prints them (bool as true / false)
static std::string targ(bool v) { return v ? "true" : "false"; }
static std::string targ(int v) { return std::to_string(v); }
template <class... T>
static std::string instantiation(const char *kernel, T... args)
{
    std::string s = kernel;
    const char *sep = "<";
    ((s += sep, s += targ(args), sep = ", "), ...);
    return s + ">";
}
using OqpskSampleFn = void (*)(JGeom, JPtrs, const int16_t *, int, int, int, int, int, JTaps28, const double2 *, int);
using MskSampleFn = void (*)(JGeom, JPtrs, const int16_t *, int, int, int, int, int, int, int);
using CoarseFn = void (*)(JGeom, JPtrs, const int *, int, const double2 *);
using BurstDemodFn = void (*)(BGeom, BPtrs, int, long long, int);
using TridentFn = void (*)(BGeom, BPtrs, long long);

// A demodulator bank.  What it keeps as a DevHandle (host_common.h):
//   last_stream, order_ev  a write on another stream than the previous one waits for what was enqueued on that one (setters included)
//   poisoned               a launch inside a write failed: the host's schedule mirror has advanced past the device state
// (tests/device_prims.py cites lines of validate_settings and fill_geometry below by number)
struct jaero_ctx : DevHandle
{
    JGeom g{};
    JPtrs p{};
    unsigned flags = 0;
    int max_write = 0;
    int soft_cap_req = 0; // softbit_capacity as given to jaero_create (0 = default for the rate): a re-created bank asks for the same
    DevMem mem;
    // device helpers
    int16_t *d_pcm_frames = nullptr; // [max_write][nchp] staging for channel-major / host input
    int16_t *d_pcm_raw = nullptr;    // [nch*max_write] staging for host input
    double2 *d_tw = nullptr;
    int *d_emitted = nullptr; // burst banks: per-channel count of soft bits already emitted (jaero_softbits_view)
    std::vector<int> dly_t0; // MSK: shared delay-line slot at which each channel's delayedsmpl pointer last restarted (jaero_set_settings)
    // the sample loop (OQPSK: k_oqpsk_fb; MSK: k_msk_fb, or k_msk_samples for 40 and 20 taps) and the coarse estimate (k_coarse6*)
    KernelRec<OqpskSampleFn> oq_loop;
    KernelRec<MskSampleFn> msk_loop;
    KernelRec<CoarseFn> coarse; CoarseBand<KernelRec<CoarseFn>> band; // band: k_coarse6_b7 beside the generic kernel (k_coarse6.h, update_band_class)
    JTaps28 oq_taps{}; // the 28 distinct values of the (bitwise symmetric) 55-tap RRC, scalar operands of k_oqpsk_fb's filter
    // fb == 8400 (k_pre8400.h): prefilter buffers, samples written so far, size of the previous write
    bool pre8400 = false;
    JPre pre{};
    long long pre_n0 = 0;
    int pre_nprev = 0;
    int *d_chanlist = nullptr;
    jaero_status *d_status = nullptr;
    int16_t *d_pack = nullptr; size_t pack_elems = 0;
    // host mirrors
    std::vector<jaero_settings> settings;
    Mirror m;
    // burst kinds (JAERO_KIND_BURST_*): their own geometry / state (burst_device.h); g/p above stay unused
    bool burst = false;
    BGeom bg{};
    BPtrs bp{};
    KernelRec<BurstDemodFn> bdemod; // k_burst_oqpsk_demod or k_burst_msk_fb
    KernelRec<TridentFn> trident;
    long long nsamples_total = 0; // samples written so far (uniform ring slots and event time stamps derive from it)
    int bt_hold_left = 0;         // burst: samples behind the last jaero_set_settings for which k_burst_front<true> must run (bt_d1 refilled with zeros)
    // generic views of the per-channel output buffers (either kind)
    int o_nchp = 0, o_nch = 0, o_soft_cap = 0, o_sym_cap = 0;
    int16_t *o_soft = nullptr; double *o_sym = nullptr;
    int *o_soft_cnt = nullptr, *o_sym_cnt = nullptr, *o_overflow = nullptr, *o_flags = nullptr;
    int *o_nrx = nullptr; // burst: soft bits pushed but not yet emitted (RxDataBits.size()), kept at the tail of the buffer
    KernelTimer timer{6}; SweepBufs sweep; jaero_status *d_status_all = nullptr; // jaero_profile_read's five kernel classes + 5 = jaero_read_all / jaero_read_status_all's kernels; their scratch, allocated by the first call
};

// ------------------------------------------------------------------------------------------ small kernels
__global__ void k_transpose_pcm(const int16_t *__restrict__ src /*[nch][n]*/, int16_t *__restrict__ dst /*[n][nchp]*/, int nch,
                                int nchp, int n)
{
    __shared__ int16_t tile[64][65];
    const int c0 = blockIdx.x * 64, i0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6; // 256 threads: 4 rows per pass
    for (int r = ty; r < 64; r += 4)
    {
        const int c = c0 + r, i = i0 + tx;
        tile[r][tx] = (c < nch && i < n) ? src[(size_t)c * n + i] : (int16_t)0;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4)
    {
        const int i = i0 + r, c = c0 + tx;
        if (i < n && c < nchp) dst[(size_t)i * nchp + c] = tile[tx][r];
    }
}

__global__ void k_center_freq(const JGeom g, const JPtrs p, int ch_first, int nch_apply, double freq_center_in)
{
    // CenterFreqChangedSlot (oqpskdemodulator.cpp:291-310, mskdemodulator.cpp:265-282); one block per channel
    const int ch = ch_first + blockIdx.x;
    if (blockIdx.x >= nch_apply) return;
    const int nchp = g.nchp;
    if (threadIdx.x == 0)
    {
        double fc = freq_center_in;
        const double fb = g.fb, Fs = g.Fs;
        if (g.kind == 1 && g.fb == 8400) {} // no clamp at 8400 bps (oqpskdemodulator.cpp:293: `if(fb!=8400)`)
        else if (g.kind == 1)
        {
            if (fc < (0.5 * fb)) fc = 0.5 * fb;
            if (fc > (Fs / 2.0 - 0.5 * fb)) fc = Fs / 2.0 - 0.5 * fb;
        }
        else
        {
            if (fc < (0.75 * fb)) fc = 0.75 * fb;
            if (fc > (Fs / 2.0 - 0.75 * fb)) fc = Fs / 2.0 - 0.75 * fb;
        }
        double *S = p.S + ch;
        const int flags = p.I[(size_t)I_FLAGS * nchp + ch];
        const double lbw = S[(size_t)S_LOCKINGBW * nchp];
        // mixer_center.SetFreq(freq_center,Fs)  (DSP.cpp:142-149)
        double mc_freq = fc;
        if (mc_freq < 0) mc_freq = 0;
        double mc_step = (mc_freq) * ((double)JD_WTSIZE) / ((float)Fs);
        double mc_ptr = S[(size_t)S_MC_PTR * nchp];
        while (((int)mc_ptr) >= JD_WTSIZE) mc_ptr -= JD_WTSIZE;
        double m2_freq = S[(size_t)S_M2_FREQ * nchp], m2_step = S[(size_t)S_M2_STEP * nchp];
        if (flags & JF_AFC) jd_wt_setfreq(m2_freq, m2_step, mc_freq, Fs);
        if ((m2_freq - mc_freq) > (lbw / 2.0)) jd_wt_setfreq(m2_freq, m2_step, mc_freq + (lbw / 2.0), Fs);
        if ((m2_freq - mc_freq) < (-lbw / 2.0)) jd_wt_setfreq(m2_freq, m2_step, mc_freq - (lbw / 2.0), Fs);
        S[(size_t)S_MC_FREQ * nchp] = mc_freq; S[(size_t)S_MC_STEP * nchp] = mc_step; S[(size_t)S_MC_PTR * nchp] = mc_ptr;
        S[(size_t)S_M2_FREQ * nchp] = m2_freq; S[(size_t)S_M2_STEP * nchp] = m2_step;
    }
    double2 *ring = p.bbring + (size_t)ch * g.nfft;
    for (int i = threadIdx.x; i < g.nfft; i += blockDim.x) ring[i] = make_double2(0.0, 0.0); // bbcycbuff[j]=0
}

__global__ void k_status(const JGeom g, const JPtrs p, int ch_first, int n, jaero_status *out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int ch = ch_first + k, nchp = g.nchp;
    jaero_status st;
    st.mse = p.S[(size_t)S_MSE * nchp + ch];
    st.ebno = p.S[(size_t)S_EB_EBNO * nchp + ch];
    st.freq_est = p.S[(size_t)S_M2_FREQ * nchp + ch];
    st.freq_center = p.S[(size_t)S_MC_FREQ * nchp + ch];
    st.signal = (st.mse > p.S[(size_t)S_THRESH * nchp + ch]) ? 0 : 1;
    st.n_estimates = p.I[(size_t)I_NEST * nchp + ch];
    out[k] = st;
}

__global__ void k_pack_soft(const int *__restrict__ soft_cnt, const int16_t *__restrict__ soft, int soft_cap, int16_t *dst, int capc)
{
    const int ch = blockIdx.x;
    const int cnt = min(soft_cnt[ch], capc);
    const int16_t *src = soft + (size_t)ch * soft_cap;
    for (int k = threadIdx.x; k < cnt; k += blockDim.x) dst[(size_t)ch * capc + k] = src[k];
}

__global__ void k_status_burst(const BGeom g, const BPtrs p, int ch_first, int n, jaero_status *out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int ch = ch_first + k, nchp = g.nchp;
    jaero_status st;
    st.mse = p.S[(size_t)BS_MSE * nchp + ch];
    st.ebno = p.S[(size_t)BS_EB_EBNO * nchp + ch];
    st.freq_est = p.S[(size_t)BS_M2_FREQ * nchp + ch];
    st.freq_center = (g.kind == JAERO_KIND_BURST_MSK_D) ? p.S[(size_t)BS_MC_FREQ * nchp + ch] : st.freq_est;
    st.signal = p.I[(size_t)BI_STARTSTOP * nchp + ch] > 0 ? 1 : 0; // between SignalStatus(true) and SignalStatus(false)
    st.n_estimates = p.I[(size_t)BI_EV_CNT * nchp + ch];
    out[k] = st;
}

// ------------------------------------------------------------------------------------------ helpers
// the readers of a bank's per-channel outputs: drain channel ch of `b`, then report `ovbit` of its overflow word
static int read_output(jaero_ctx *c, const char *who, const RowBuf &b, int ch, void *rows, int caprows, int *nrows, int ovbit, const int *pending = nullptr)
{
    const int rc = drain_rows(who, c->device, c->last_stream, c->o_nch, b, ch, rows, caprows, nrows, pending);
    return rc ? rc : report_overflow(c->o_overflow + ch, ovbit, ch);
}

// The end of a rate change (rebank_with_carry_over, burst_rebank): the new bank takes the old one's place behind the handle and keeps the
// handle's kernel timings -- the launches since the last jaero_profile_read included, whose events go with the old bank -- and host flag
// mirror.  The old bank goes when `n` does.
using BankPtr = std::unique_ptr<jaero_ctx, void (*)(jaero_ctx *)>;
static void swap_in(jaero_ctx *c, BankPtr n)
{
    c->timer.collect();
    n->timer.on = c->timer.on;
    n->timer.slots = c->timer.slots;
    n->m.flags = c->m.flags; n->band.force_generic = c->band.force_generic; n->band.est_generic = c->band.est_generic; n->band.est_band = c->band.est_band;
    std::swap(*c, *n);
}

// RootRaisedCosine::design (JAERO/DSP.h:316-338)
static std::vector<double> rrc_design(double alpha, int firsize, double samplerate, double symbol_freq)
{
    if ((firsize % 2) == 0) firsize += 1;
    std::vector<double> P(firsize);
    double T = (samplerate) / (symbol_freq);
    for (int i = 0; i < firsize; i++)
    {
        if (i == ((firsize - 1) / 2)) P[i] = (4.0 * alpha + M_PI - M_PI * alpha) / (M_PI * sqrt(T));
        else
        {
            double fi = (((double)i) - ((double)(firsize - 1)) / 2.0);
            if (fabs(1.0 - pow(4.0 * alpha * fi / T, 2)) < 0.0000000001)
                P[i] = (alpha * ((M_PI - 2.0) * cos(M_PI / (4.0 * alpha)) + (M_PI + 2.0) * sin(M_PI / (4.0 * alpha))) / (M_PI * sqrt(2.0 * T)));
            else
                P[i] = (4.0 * alpha / (M_PI * sqrt(T)) * (cos((1.0 + alpha) * M_PI * fi / T) + T / (4.0 * alpha * fi) * sin((1.0 - alpha) * M_PI * fi / T)) / (1.0 - pow(4.0 * alpha * fi / T, 2)));
        }
    }
    return P;
}

// weighting used by Delay<double>::update (JAERO/DSP.h:357-374) for ring position 0
static double delay_weight(double fractdelay)
{
    int size = (int)ceil(fractdelay) + 1;
    double dptr = 0.0 - fractdelay;
    while (floor(dptr) < 0) dptr += (double)size;
    int iptr = (int)floor(dptr);
    return dptr - (double)iptr;
}

static int validate_settings(const jaero_settings &s)
{
    if (s.kind < JAERO_KIND_MSK || s.kind > JAERO_KIND_BURST_OQPSK) return fail(JAERO_ENOTSUP, "kind %d not implemented", s.kind);
    const bool oq = s.kind == JAERO_KIND_OQPSK || s.kind == JAERO_KIND_BURST_OQPSK;
    // the continuous MSK demodulator also runs at 24 and 12 kHz (MskDemodulator::dataReceived re-applies its settings with the sample rate
    // of the incoming audio, JAERO/mskdemodulator.cpp:528-537): matched filters of 2 Fs / fb = 20, 40, 80 or 160 taps
    const bool fs_ok = s.Fs == 48000 || (s.kind == JAERO_KIND_MSK && (s.Fs == 24000 || s.Fs == 12000));
    if (!fs_ok) return fail(JAERO_ENOTSUP, "Fs = %g is not implemented (48000; continuous MSK also 24000 and 12000)", s.Fs);
    // fb = 8400 (C channel): the continuous demodulator with a 2^14-point coarse FFT (k_pre8400.h)
    const bool allow84 = s.kind == JAERO_KIND_OQPSK && s.coarsefreqest_fft_power == 14;
    if (oq && s.fb != 10500 && !(s.fb == 8400 && allow84))
        return fail(JAERO_ENOTSUP, "OQPSK: fb must be 10500, or 8400 for the continuous demodulator with coarsefreqest_fft_power 14");
    if (!oq && s.fb != 600 && s.fb != 1200) return fail(JAERO_ENOTSUP, "MSK: fb must be 600 or 1200");
    const bool burst = s.kind >= JAERO_KIND_BURST_MSK;
    if (!burst && s.coarsefreqest_fft_power != 13 && s.coarsefreqest_fft_power != 14) return fail(JAERO_ENOTSUP, "coarsefreqest_fft_power must be 13 or 14");
    if (const int rc = check_tuning_range(s.lockingbw, s.freq_center, s.Fs)) return rc; // lockingbw in (0, Fs / 2], freq_center >= 0
    return 0;
}

// per-channel scalar initial state = constructor + setSettings of the reference
// stride = the column pitch of S / I (the bank's nchp, or 1 for a one-column scratch with ch = 0: jaero_set_settings)
static void init_channel_scalars(const jaero_ctx *c, const jaero_settings &s, std::vector<double> &S, std::vector<int> &I, int ch, bool fresh, int stride = 0)
{
    const int nchp = stride > 0 ? stride : c->g.nchp;
    auto SS = [&](int f) -> double & { return S[(size_t)f * nchp + ch]; };
    auto II = [&](int f) -> int & { return I[(size_t)f * nchp + ch]; };
    double fc = s.freq_center;
    if (fc > ((s.Fs / 2.0) - (s.lockingbw / 2.0))) fc = ((s.Fs / 2.0) - (s.lockingbw / 2.0));
    const double step_fc = (fc < 0 ? 0 : fc) * ((double)JD_WTSIZE) / ((float)(double)(int)s.Fs);
    SS(S_M2_FREQ) = fc < 0 ? 0 : fc; SS(S_M2_STEP) = step_fc;
    SS(S_MC_FREQ) = fc < 0 ? 0 : fc; SS(S_MC_STEP) = step_fc;
    const double stf = (s.kind == JAERO_KIND_OQPSK) ? s.fb : s.fb / 2;
    SS(S_ST_FREQ) = stf; SS(S_ST_STEP) = stf * ((double)JD_WTSIZE) / ((float)(double)(int)s.Fs);
    SS(S_LOCKINGBW) = s.lockingbw; SS(S_THRESH) = s.signalthreshold;
    if (fresh)
    {
        SS(S_PRE_PTR) = 0; SS(S_PRE_FSUM) = 0;
        SS(S_PRE_STEP) = 8000.0 * ((double)JD_WTSIZE) / ((float)(double)(int)s.Fs); // mixer_fir_pre.SetFreq(freq_center, Fs) in the ctor: 8000 Hz
        SS(S_M2_PTR) = 0; SS(S_MC_PTR) = 0; SS(S_ST_PTR) = 0; SS(S_ST_LAST) = 0;
        SS(S_MSE) = (s.kind == JAERO_KIND_OQPSK) ? 100.0 : 10.0;
        SS(S_DIFF_LAST) = -1.0;
        II(I_COUNTDOWN) = 4; II(I_COUNTDOWN2) = 5; II(I_EMPTYING) = 1;
    }
    if (s.kind == JAERO_KIND_MSK) SS(S_MSE) = 10.0; // setSettings resets mse (mskdemodulator.cpp:180)
}

static void fill_geometry(JGeom &g, const jaero_settings &s, int nch, unsigned flags)
{
    memset(&g, 0, sizeof g);
    g.kind = s.kind; g.nch = nch; g.nchp = (nch + 63) / 64 * 64; g.ngroups = g.nchp / 64;
    g.Fs = s.Fs; g.fb = s.fb; g.Fs_int = (int)s.Fs;
    g.nfft_log2 = s.coarsefreqest_fft_power; g.nfft = 1 << g.nfft_log2;
    g.ebno_len = (int)(2 * s.Fs);
    g.flags = flags;
    if (s.kind == JAERO_KIND_OQPSK)
    {
        g.fir_n = 55;
        g.agc_len = (int)round(4 * s.Fs);
        g.marg_len = 800; g.dt_len = 401; g.pm_len = 400; g.msema_len = 400;
        g.ee = 0.4;
        double T = s.Fs / (s.fb / 2);
        g.w4 = delay_weight(T / 4.0); g.w8 = delay_weight(T / 8.0);
        g.res_b0 = 0.00032714218939589035; g.res_b1 = 0; g.res_b2 = 0.00032714218939589035;
        g.res_a1 = -0.39005299948210803; g.res_a2 = 0.99934571562120822;
        if (s.fb == 8400) // the 10 Hz resonator and ee of oqpskdemodulator.cpp:231-251
        {
            g.res_b0 = 0.0012845857864470789; g.res_b1 = 0; g.res_b2 = -0.0012845857864470789;
            g.res_a1 = -0.90681461999279889; g.res_a2 = 0.99743082842710584;
            g.ee = 0.65;
        }
        g.lf_b0 = 0.0010275610653672064; g.lf_b1 = 0.0020551221307344128; g.lf_b2 = 0.0010275610653672064;
        g.lf_a1 = -1.9207386815577139; g.lf_a2 = 0.92509247310306331;
        g.stref_freq = s.fb;
        g.sps = 1; g.sps2 = 1;
    }
    else
    {
        g.sps = (int)(s.Fs / s.fb); g.sps2 = g.sps / 2;
        g.fir_n = 2 * g.sps;
        g.agc_len = (int)round(1 * s.Fs);
        g.marg_len = g.sps; g.dt_len = g.sps / 2 + 1; g.pm_len = 1; g.msema_len = 600;
        // resonator and sampling-point offset: mskdemodulator.cpp:196-233 (one resonator for every rate other than 48 kHz)
        if (s.fb >= 1200)
        {
            g.correctionfactor = 0.6;
            g.res_a1 = -1.993312819378528; g.res_a2 = 0.999476538254407;
            g.res_b0 = 2.617308727964618e-04; g.res_b1 = 0; g.res_b2 = -2.617308727964618e-04;
            g.ee = 0.025;
            if (s.Fs != 48000) g.ee = 0.05;
        }
        else
        {
            g.correctionfactor = 1.0;
            g.res_a1 = -1.998196509168551; g.res_a2 = 0.999738234875681;
            g.res_b0 = 1.308825621597620e-04; g.res_b1 = 0; g.res_b2 = -1.308825621597620e-04;
            g.ee = 0.025;
            if (s.Fs != 48000) g.ee = 0.0125;
        }
        if (s.Fs != 48000)
        {
            g.res_a1 = -1.974342917561558; g.res_a2 = 0.998953350377616;
            g.res_b0 = 5.233248111921052e-04; g.res_b1 = 0; g.res_b2 = -5.233248111921052e-04;
        }
        g.stref_freq = s.fb / 2;
    }
    g.win_len = ((flags & JAERO_FLAG_EBNO) && g.ebno_len > g.agc_len) ? g.ebno_len : g.agc_len;
}

template <class Fn>
static hipError_t set_lds_attribute(const KernelRec<Fn> &r)
{
    return hipFuncSetAttribute((const void *)r.fn, hipFuncAttributeMaxDynamicSharedMemorySize, r.lds);
}

// f(EBNO, CAPSYM) with the bank's two flags as std::true_type / std::false_type: the instantiation of a kernel family that serves the bank
template <class F>
static auto by_flags(unsigned flags, F f)
{
    const std::true_type y;
    const std::false_type n;
    const bool eb = (flags & JAERO_FLAG_EBNO) != 0, cs = (flags & JAERO_FLAG_CAPTURE_SYMBOLS) != 0;
    return eb ? (cs ? f(y, y) : f(y, n)) : (cs ? f(n, y) : f(n, n));
}

// Tables of the overlap-save filters (k_pre8400_fft, k_hilbert_fft), in buffers of `m`: H = DFT_4096(taps, zero-padded) / 4096 and
// exp(-2 pi i k / 4096), summed in long double on the host.  kernel_fn = the kernel whose dynamic LDS limit is raised to the 128 KiB exchange buffer.
static int fft4096_tables(DevMem &m, const std::vector<double> &taps, double2 **d_H, double2 **d_tw, const void *kernel_fn)
{
    const int N = 2 * PRE_L;
    std::vector<long double> cr(N), ci(N);
    for (int k = 0; k < N; k++) { const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)N; cr[k] = cosl(a); ci[k] = sinl(a); }
    std::vector<double2> H(N), tw(N);
    for (int k = 0; k < N; k++)
    {
        long double sr = 0, si = 0;
        for (int j = 0; j < (int)taps.size(); j++) { const int e = (int)(((long long)k * j) & (N - 1)); sr += (long double)taps[j] * cr[e]; si += (long double)taps[j] * ci[e]; }
        H[k].x = (double)(sr / N); H[k].y = (double)(si / N);
        tw[k].x = (double)cr[k]; tw[k].y = (double)ci[k];
    }
    int rc;
    if ((rc = dalloc(m, d_H, N, false)) || (rc = dalloc(m, d_tw, N, false))) return rc;
    HIPCHK(hipMemcpy(*d_H, H.data(), sizeof(double2) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(*d_tw, tw.data(), sizeof(double2) * N, hipMemcpyHostToDevice));
    HIPCHK(hipFuncSetAttribute(kernel_fn, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 2 * PRE_L * (int)sizeof(double)));
    return 0;
}

#include "burst_host.h"

// ------------------------------------------------------------------------------------------ create / destroy
extern "C" int jaero_abi_version(void) { return JAERO_ABI_VERSION; }
extern "C" const char *jaero_last_error(void) { return g_last_error.c_str(); }
extern "C" const char *jaero_strerror(int code)
{
    switch (code)
    {
    case JAERO_OK: return "ok";
    case JAERO_EINVAL: return "invalid argument";
    case JAERO_ENODEV: return "no usable HIP device";
    case JAERO_ENOMEM: return "out of memory";
    case JAERO_EHIP: return "HIP runtime error";
    case JAERO_EOVERFLOW: return "output capacity exceeded";
    case JAERO_ENOTSUP: return "not supported";
    default: return "unknown error";
    }
}
extern "C" int jaero_num_channels(const jaero_ctx *ctx) { return ctx ? ctx->o_nch : 0; }

extern "C" void jaero_destroy(jaero_ctx *c)
{
    if (!c) return;
    dcd_unlink_bank(c);
    // this bank's work only (its last stream and the default stream its control-plane copies use): other banks keep running until hipFree's
    // own implicit synchronisation, which cannot be avoided
    c->teardown();
    hipStreamSynchronize(0);
#ifdef FB_TRACE_BUILD
    if (!c->burst)
    {
        // trace build only: what the traced pair of this bank's sample loop accumulated, one JSON line on stderr per destroyed bank
        unsigned long long tr[20] = {0}, z[20] = {0};
        if (hipMemcpyFromSymbol(tr, HIP_SYMBOL(g_fb_trace), sizeof(tr)) == hipSuccess && tr[8] + tr[18] > 0)
        {
            fprintf(stderr, "{\"fb_trace\": {\"channels\": %d, \"clock_hz\": 100000000", c->o_nch);
            for (int h = 0; h < 2; h++)
            {
                fprintf(stderr, ", \"%s\": {\"samples\": %llu, \"ticks\": [", h ? "back" : "front", tr[h * 10 + 8]);
                for (int k = 0; k < 8; k++) fprintf(stderr, "%s%llu", k ? ", " : "", tr[h * 10 + k]);
                fprintf(stderr, "]}");
            }
            fprintf(stderr, "}}\n");
        }
        hipMemcpyToSymbol(HIP_SYMBOL(g_fb_trace), z, sizeof(z));
    }
#endif
    delete c; // its device memory and timing events with it
}

static void launch_pre8400_filter(const JGeom &g, const JPtrs &p, const JPre &q, int n, long long n0, hipStream_t st)
{
    hipLaunchKernelGGL(k_pre8400_fft, dim3(g.nchp / 4, (int)(((n0 + n - 1) >> 11) - (n0 >> 11) + 1)), dim3(PF_THREADS), 4 * 2 * PRE_L * (int)sizeof(double), st, g, p, q, n, n0);
}

// The launches of a write in front of the sample loop, shared by jaero_write / jaero_set_settings and the test hooks jaero_debug_pre8400_*
// (tests/test_gpu_pre8400.py runs these, not a copy of them).
// The write's PCM on the device as frames: uploaded unless it is there already, transposed unless it is frame-major.
static int stage_pcm(jaero_ctx *c, const int16_t *pcm, int nsamples, int layout, int is_device_ptr, hipStream_t st, const int16_t **frames, int *stride)
{
    const int nch = c->g.nch, nchp = c->g.nchp;
    const int16_t *dsrc = pcm;
    if (!is_device_ptr)
    {
        HIPCHK(hipMemcpyAsync(c->d_pcm_raw, pcm, sizeof(int16_t) * (size_t)nch * nsamples, hipMemcpyHostToDevice, st));
        dsrc = c->d_pcm_raw;
    }
    if (layout == JAERO_PCM_FRAME_MAJOR) { *frames = dsrc; *stride = nch; }
    else
    {
        const int pi = c->timer.begin(2, st);
        hipLaunchKernelGGL(k_transpose_pcm, dim3(nchp / 64, (nsamples + 63) / 64), dim3(256), 0, st, dsrc, c->d_pcm_frames, nch, nchp, nsamples);
        LAUNCHCHK("k_transpose_pcm");
        c->timer.end(pi, st);
        *frames = c->d_pcm_frames; *stride = nchp;
    }
    return 0;
}
// eight stretches per write once there are fewer channel groups than eight per SIMD (k_pre8400.h)
static int pre8400_stretches(const JGeom &g, int nsamples) { return (g.ngroups >= 8192 || nsamples < 512) ? 1 : 8; }
// the whole write is prefiltered first (oqpskdemodulator.cpp:343-381); its oscillator takes the mean of mixer2's frequency over the
// previous write (:607-608).  Advances pre_n0.
static int launch_pre8400_stage(jaero_ctx *c, const int16_t *frames, int stride, int nsamples, int ntb, hipStream_t st)
{
    const JGeom &g = c->g;
    hipLaunchKernelGGL(k_pre8400_mix, dim3(g.ngroups, ntb), dim3(64), 0, st, g, c->p, c->pre, frames, stride, nsamples, c->pre_n0, c->pre_nprev);
    LAUNCHCHK("k_pre8400_mix");
    hipLaunchKernelGGL(k_pre8400_commit, dim3(g.ngroups), dim3(64), 0, st, g, c->p, c->pre_nprev);
    LAUNCHCHK("k_pre8400_commit");
    launch_pre8400_filter(g, c->p, c->pre, nsamples, c->pre_n0, st);
    LAUNCHCHK("the 8400 bps prefilter");
    c->pre_n0 += nsamples;
    return 0;
}
// setSettings on one channel of several: its prefilter starts again at the bank's current sample (k_pre8400_restart)
static int launch_pre8400_restart(jaero_ctx *c, int channel, hipStream_t st)
{
    hipLaunchKernelGGL(k_pre8400_restart, dim3(16), dim3(256), 0, st, c->g, c->pre, channel, c->pre_n0);
    LAUNCHCHK("k_pre8400_restart");
    return 0;
}

// The sample-loop records: front / back pair kernels (k_oqpsk_fb.h, k_msk_fb.h) and the single-wavefront MSK kernel (k_msk.h).  The kernel
// and its spelled-out name come from the same E / C pick of by_flags.
template <int PAIRS, bool PRE8400>
static KernelRec<OqpskSampleFn> oqpsk_fb_rec(const JGeom &g, unsigned flags)
{
    return by_flags(flags, [&](auto E, auto C) -> KernelRec<OqpskSampleFn> {
        return {k_oqpsk_fb<55, FB_LDSN, E, C, PAIRS, PRE8400>, (g.ngroups + PAIRS - 1) / PAIRS, PAIRS * 128,
                PAIRS * fb_pair_doubles<FB_LDSN>() * (int)sizeof(double), FB_LDSN, "k_oqpsk_fb<",
                instantiation("k_oqpsk_fb", 55, FB_LDSN, (bool)E, (bool)C, PAIRS, PRE8400)};
    });
}
template <int FIRN, int LDSN, int PAIRS, int TB>
static KernelRec<MskSampleFn> msk_fb_rec(const JGeom &g, unsigned flags)
{
    return by_flags(flags, [&](auto E, auto C) -> KernelRec<MskSampleFn> {
        return {k_msk_fb<FIRN, LDSN, E, C, PAIRS, TB>, (g.ngroups + PAIRS - 1) / PAIRS, PAIRS * 128,
                PAIRS * mfb_pair_doubles<FIRN, LDSN, TB>() * (int)sizeof(double), LDSN, "k_msk_fb<",
                instantiation("k_msk_fb", FIRN, LDSN, (bool)E, (bool)C, PAIRS, TB)};
    });
}
template <int FIRN, int LDSN>
static KernelRec<MskSampleFn> msk_samples_rec(const JGeom &g, unsigned flags)
{
    return by_flags(flags, [&](auto E, auto C) -> KernelRec<MskSampleFn> {
        return {k_msk_samples<FIRN, LDSN, E, C>, g.ngroups, 64, msk_samples_lds_bytes<FIRN, LDSN>(), LDSN, "k_msk_samples<",
                instantiation("k_msk_samples", FIRN, LDSN, (bool)E, (bool)C)};
    });
}

// test hook jaero_debug_sample_loop_layout: 0 = by size (the product behaviour), 1 = one pair per workgroup, 2 = four pairs per workgroup
static int g_sample_loop_layout = 0;
extern "C" int jaero_debug_sample_loop_layout(int mode)
{
    if (mode < 0 || mode > 2) return fail(JAERO_EINVAL, "jaero_debug_sample_loop_layout: mode must be 0 (by size), 1 (one pair) or 2 (four pairs)");
    g_sample_loop_layout = mode;
    return 0;
}

// after every write of S_LOCKINGBW for channels [lo, hi): create, jaero_set_settings, the carry-over into a new bank
static void update_band_class(jaero_ctx *c, int lo, int hi)
{
    if (c->band.cls.size() != c->settings.size()) c->band.cls.assign(c->settings.size(), 0);
    for (int ch = lo; ch < hi; ch++)
        c->band.cls[ch] = c->band.rec.fn && coarse_band_class_of(c->g.nfft_log2, c->g.Fs, c->g.fb, c->settings[ch].lockingbw);
}
extern "C" int jaero_debug_coarse_band_class(int fft_power, double Fs, double fb, double lockingbw)
{
    return coarse_band_class_of(fft_power, Fs, fb, lockingbw);
}

// The continuous bank's sample-loop and coarse-estimate kernels, with their LDS attributes
static int choose_kernels(jaero_ctx *c, int ncu)
{
    const JGeom &g = c->g;
    const bool big = g_sample_loop_layout ? g_sample_loop_layout == 2 : g.ngroups > 2 * ncu;
    if (g.kind == JAERO_KIND_OQPSK)
    {
        // front / back pairs (k_oqpsk_fb.h; at 8400 bps the two halves take turns, see there).  Four pairs per workgroup put one front and one
        // back wavefront on every SIMD of a CU -- worth it once there are more channel groups than two per CU; smaller banks get one pair per
        // workgroup (two SIMDs per 64 channels).
        if (c->pre8400) c->oq_loop = big ? oqpsk_fb_rec<4, true>(g, c->flags) : oqpsk_fb_rec<1, true>(g, c->flags);
        else c->oq_loop = big ? oqpsk_fb_rec<4, false>(g, c->flags) : oqpsk_fb_rec<1, false>(g, c->flags);
        HIPCHK(set_lds_attribute(c->oq_loop));
    }
    else
    {
        switch (g.fir_n) // 2 Fs / fb taps: validate_settings admits only the rates that give 160, 80, 40 or 20
        {
        case 160: // two pairs per workgroup, each wavefront alone on a SIMD (k_msk_fb.h, MFB2_*)
            c->msk_loop = msk_fb_rec<160, MFB2_LDSN, 2, MFB2_TB>(g, c->flags);
            break;
        case 80:
            // front / back pairs (k_msk_fb.h).  Banks of at most two channel groups per CU: one pair per workgroup, the halves on different
            // SIMDs, 36 history entries per arm in LDS and 44 in registers (256 channels: 82 -> 113 Msamples/s).  Larger banks: four pairs per
            // workgroup, each pair on one SIMD, 32 entries in LDS, 26 in the front half's and the 22 oldest in the back half's registers
            // (65 536 channels: 9.2 -> 10.6 Gsamples/s).
            c->msk_loop = big ? msk_fb_rec<80, MFB4_LDSN, 4, MFB4_TB>(g, c->flags) : msk_fb_rec<80, MFB_LDSN, 1, MFB1_TB>(g, c->flags);
            break;
        case 40: c->msk_loop = msk_samples_rec<40, MSK_LDSN_40>(g, c->flags); break;
        default: assert(g.fir_n == 20); c->msk_loop = msk_samples_rec<20, MSK_LDSN_20>(g, c->flags);
        }
        HIPCHK(set_lds_attribute(c->msk_loop));
    }
    // register-resident FFTs persistent over the estimate list (k_coarse6.h): 2^14 = 32 x 32 x 16 on one 512-thread workgroup per CU (the whole
    // register file, ~130 KiB of LDS; at 8400 bps the window table behind it), 2^13 = 32 x 16 x 16 on 256 threads, two workgroups per CU
    if (g.nfft_log2 == 13) c->coarse = {k_coarse6_13, 2 * ncu, 256, C6_XCH13 * (int)sizeof(double), 0, "k_coarse6_13", "k_coarse6_13"};
    else if (c->pre8400) c->coarse = {k_coarse6_w8400, ncu, C2_THREADS, (C6_XCH + C4_TABN) * (int)sizeof(double), 0, "k_coarse6_w8400", "k_coarse6_w8400"};
    else c->coarse = {k_coarse6, ncu, C2_THREADS, C6_XCH * (int)sizeof(double), 0, "k_coarse6", "k_coarse6"};
    HIPCHK(set_lds_attribute(c->coarse));
    c->band.rec = {};
    if (c->coarse.fn == (CoarseFn)k_coarse6)
    {
        c->band.rec = {k_coarse6_b7, ncu, C2_THREADS, C6_XCH * (int)sizeof(double), 0, "k_coarse6_b7", "k_coarse6_b7"};
        HIPCHK(set_lds_attribute(c->band.rec));
    }
    update_band_class(c, 0, (int)c->settings.size());
    return 0;
}

// jaero_create of a continuous bank, behind `new jaero_ctx`: what it allocated before a failure goes with jaero_destroy
static int bank_create(jaero_ctx *c, const std::vector<jaero_settings> &sets, const hipDeviceProp_t &prop, int softbit_capacity)
{
    const jaero_settings &s0 = sets[0];
    const int nchannels = (int)sets.size(), max_write_samples = c->max_write;
    const unsigned flags = c->flags;
    int rc = 0;
    fill_geometry(c->g, s0, nchannels, flags);
    JGeom &g = c->g;
    if (softbit_capacity <= 0)
        softbit_capacity = (int)ceil(2.0 * max_write_samples * g.fb / g.Fs) + 64;
    g.soft_cap = (softbit_capacity + 7) & ~7; // 16-byte aligned rows: what the Aero-L bank's fast input path wants when it reads this buffer in place
    g.sym_cap = (flags & JAERO_FLAG_CAPTURE_SYMBOLS) ? g.soft_cap / 2 + 8 : 0;
    g.log_cap = (flags & JAERO_FLAG_STATUS_LOG) ? (int)ceil(g.soft_cap * g.Fs / g.fb / (g.nfft / 4)) + 16 : 0;
    const int nchp = g.nchp, ng = g.ngroups;

    DevMem &m = c->mem;
    DA(m, c->p.S, (size_t)S_NFIELDS * nchp);
    DA(m, c->p.I, (size_t)I_NFIELDS * nchp);
    DA(m, c->p.win, (size_t)ng * g.win_len * 64);
    DA(m, c->p.bbring, (size_t)nchp * g.nfft);
    DA(m, c->p.y, (size_t)nchp * g.nfft);
    DA(m, c->p.marg, (size_t)nchp * g.marg_len);
    DA(m, c->p.dt, (size_t)nchp * g.dt_len);
    DA(m, c->p.pm, (size_t)nchp * g.pm_len);
    DA(m, c->p.msema, (size_t)nchp * g.msema_len);
    DA(m, c->p.firsave, (size_t)ng * 2 * g.fir_n * 64);
    if (g.kind == JAERO_KIND_OQPSK && g.fb == 8400)
    {
        c->pre8400 = true;
        int ring = 1;
        // a write's first transform block starts up to 2047 samples before the write and looks 4096 samples further back
        while (ring < max_write_samples + 3 * PRE_L) ring <<= 1;
        c->pre.ring = ring;
        c->pre.cap = max_write_samples;
        DA(m, c->pre.xring, (size_t)ring * nchp);
        DA(m, c->pre.cidx, (size_t)max_write_samples * nchp);
        DA(m, c->pre.out, (size_t)max_write_samples * nchp);
        DA(m, c->pre.hold, (size_t)nchp); // zeros (DA clears): nothing held
        double *d_pre_taps = nullptr;
        DA(m, d_pre_taps, PRE_K);
        const std::vector<double> pt = rrc_design(0.6, 2048, g.Fs, g.fb / 2); // rrc_pre_imp (oqpskdemodulator.cpp:281)
        if ((int)pt.size() != PRE_K) return fail(JAERO_EHIP, "prefilter design returned %zu taps", pt.size());
        HIPCHK(hipMemcpy(d_pre_taps, pt.data(), sizeof(double) * PRE_K, hipMemcpyHostToDevice));
        c->pre.taps = d_pre_taps;
        double2 *dH = nullptr, *dtw = nullptr;
        if ((rc = fft4096_tables(m, pt, &dH, &dtw, (const void *)k_pre8400_fft))) return rc;
        c->pre.H = dH; c->pre.tw = dtw;
    }
    if (g.kind == JAERO_KIND_MSK) { DA(m, c->p.dly, (size_t)ng * (g.sps + 1) * 64); DA(m, c->p.dly8, (size_t)ng * (g.sps2 + 1) * 64); }
    // k_oqpsk_fb keeps the symbol-instant windows marg / dt / pm / msema in one combined record ring
    static_assert(JD_SYMREC_LEN == 800, "the combined symbol-record ring of k_oqpsk_fb assumes the reference's window lengths (800 / 400 / 400 / 400)");
    if (g.kind == JAERO_KIND_OQPSK) DA(m, c->p.symrec, (size_t)nchp * JD_SYMREC_LEN * 8);
    DA(m, c->p.soft, (size_t)nchp * g.soft_cap);
    if (g.sym_cap) DA(m, c->p.sym, (size_t)nchp * g.sym_cap * 3);
    if (g.log_cap) DA(m, c->p.slog, (size_t)nchp * g.log_cap * 6);
    DA(m, c->d_pcm_frames, (size_t)max_write_samples * nchp);
    DA(m, c->d_pcm_raw, (size_t)max_write_samples * nchannels);
    DA(m, c->d_chanlist, nchp);
    DA(m, c->d_status, nchp);
    DA(m, c->d_tw, g.nfft);
    double2 *d_cis = nullptr;
    double *d_taps = nullptr;
    DA(m, d_cis, JD_WTSIZE);
    DA(m, d_taps, 2 * g.fir_n);
    c->p.cis = d_cis; c->p.taps2 = d_taps;

    {
        HIPCHK(hipMemcpy(d_cis, cis_table().data(), sizeof(double2) * JD_WTSIZE, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->d_tw, twiddles(g.nfft, g.nfft).data(), sizeof(double2) * g.nfft, hipMemcpyHostToDevice));
        const std::vector<double> taps = g.kind == JAERO_KIND_OQPSK ? rrc_design(g.fb == 8400 ? 0.6 : 1.0, 55, g.Fs, g.fb / 2) : half_sine_taps(g.sps);
        HIPCHK(hipMemcpy(d_taps, doubled_taps(taps).data(), sizeof(double) * 2 * g.fir_n, hipMemcpyHostToDevice));
        if (g.kind == JAERO_KIND_OQPSK)
        {
            for (int i = 0; i < 55; i++)
                if (memcmp(&taps[i], &taps[54 - i], sizeof(double)) != 0)
                    return fail(JAERO_ENOTSUP, "matched-filter taps are not bitwise symmetric: k_oqpsk_fb takes the 28 distinct taps as scalar arguments");
            for (int i = 0; i < 28; i++) c->oq_taps.t[i] = taps[i];
        }
    }
    // scalar state
    {
        std::vector<double> S((size_t)S_NFIELDS * nchp, 0.0);
        std::vector<int> I((size_t)I_NFIELDS * nchp, 0);
        c->settings.resize(nchp);
        for (int ch = 0; ch < nchp; ch++)
        {
            const jaero_settings &s = sets[ch < nchannels ? ch : 0];
            c->settings[ch] = s;
            init_channel_scalars(c, s, S, I, ch, true);
        }
        HIPCHK(hipMemcpy(c->p.S, S.data(), S.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->p.I, I.data(), I.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    c->o_nch = nchannels; c->o_nchp = nchp; c->o_soft_cap = g.soft_cap; c->o_sym_cap = g.sym_cap;
    c->o_soft = c->p.soft; c->o_sym = c->p.sym;
    c->o_soft_cnt = c->p.I + (size_t)I_SOFT_CNT * nchp; c->o_sym_cnt = c->p.I + (size_t)I_SYM_CNT * nchp;
    c->o_overflow = c->p.I + (size_t)I_OVERFLOW * nchp; c->o_flags = c->p.I + (size_t)I_FLAGS * nchp;
    c->m.nch = nchannels; c->m.nchp = nchp; c->m.nfft = g.nfft; c->m.Fs_int = g.Fs_int;
    c->m.flags.assign(nchp, 0); c->m.bbptr.assign(nchp, 0); c->m.cnt.assign(nchp, 0);
    if ((rc = choose_kernels(c, prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256))) return rc;
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

extern "C" int jaero_create(int device, int nchannels, const jaero_settings *settings, int per_channel_stride, unsigned flags,
                            int max_write_samples, int softbit_capacity, jaero_ctx **out)
{
    if (!out || !settings || nchannels <= 0 || max_write_samples <= 0) return fail(JAERO_EINVAL, "jaero_create: bad arguments");
    *out = nullptr;
    // the settings are judged before the device is opened: what they refuse does not depend on one
    std::vector<jaero_settings> sets(nchannels);
    for (int ch = 0; ch < nchannels; ch++)
        sets[ch] = per_channel_stride ? *(const jaero_settings *)((const char *)settings + (size_t)ch * per_channel_stride) : settings[0];
    const jaero_settings &s0 = sets[0];
    int rc = validate_settings(s0);
    if (rc) return rc;
    for (int ch = 1; ch < nchannels; ch++)
    {
        const jaero_settings &s = sets[ch];
        if (s.kind != s0.kind || s.fb != s0.fb || s.Fs != s0.Fs || s.coarsefreqest_fft_power != s0.coarsefreqest_fft_power)
            return fail(JAERO_EINVAL, "channel %d: kind/fb/Fs/fft_power must match channel 0 within one bank", ch);
        if ((rc = validate_settings(s))) return rc;
    }
    hipDeviceProp_t prop;
    if ((rc = open_device(device, &prop))) return rc;

    jaero_ctx *c = new jaero_ctx();
    c->device = device;
    c->flags = flags;
    c->max_write = max_write_samples;
    c->soft_cap_req = softbit_capacity;
    rc = s0.kind >= JAERO_KIND_BURST_MSK ? burst_create(c, sets, prop, softbit_capacity) : bank_create(c, sets, prop, softbit_capacity);
    if (rc) { jaero_destroy(c); return rc; }
    *out = c;
    return 0;
}

// ------------------------------------------------------------------------------------------ control surface
// flags[ch] = (flags[ch] & ~mask) | bits for ch in [lo, hi): by value, on the stream of the last write (as the write that follows will
// be, see jaero_write) -- no host buffer is in flight, so a second call right behind the first cannot disturb it
__global__ void k_set_flag_bits(int *flags, int lo, int hi, int mask, int bits)
{
    const int ch = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (ch < hi) flags[ch] = (flags[ch] & ~mask) | bits;
}
static int upload_flags(jaero_ctx *c, int lo, int hi, int mask, int bits)
{
    hipLaunchKernelGGL(k_set_flag_bits, dim3((hi - lo + 255) / 256), dim3(256), 0, c->last_stream, c->o_flags, lo, hi, mask, bits);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int jaero_set_flags(jaero_ctx *c, int channel, int afc, int sql, int cpu_reduce)
{
    POISONCHK(c, "jaero_set_flags", POISON_BANK);
    if (!c || channel < -1 || channel >= c->o_nch) return fail(JAERO_EINVAL, "jaero_set_flags: bad channel");
    HIPCHK(hipSetDevice(c->device));
    const int lo = channel < 0 ? 0 : channel, hi = channel < 0 ? c->o_nchp : channel + 1;
    const int bits = (afc ? JF_AFC : 0) | (sql ? JF_SQL : 0) | (cpu_reduce ? JF_CPUREDUCE : 0);
    for (int ch = lo; ch < hi; ch++) c->m.flags[ch] = (c->m.flags[ch] & JF_DCD) | bits;
    return upload_flags(c, lo, hi, JF_AFC | JF_SQL | JF_CPUREDUCE, bits);
}

extern "C" int jaero_set_dcd(jaero_ctx *c, int channel, int dcd)
{
    POISONCHK(c, "jaero_set_dcd", POISON_BANK);
    if (!c || channel < -1 || channel >= c->o_nch) return fail(JAERO_EINVAL, "jaero_set_dcd: bad channel");
    HIPCHK(hipSetDevice(c->device));
    const int lo = channel < 0 ? 0 : channel, hi = channel < 0 ? c->o_nchp : channel + 1;
    for (int ch = lo; ch < hi; ch++) c->m.flags[ch] = (c->m.flags[ch] & ~JF_DCD) | (dcd ? JF_DCD : 0);
    return upload_flags(c, lo, hi, JF_DCD, dcd ? JF_DCD : 0);
}

extern "C" int jaero_center_freq_changed(jaero_ctx *c, int channel, double hz)
{
    POISONCHK(c, "jaero_center_freq_changed", POISON_BANK);
    if (!c || channel < -1 || channel >= c->o_nch) return fail(JAERO_EINVAL, "jaero_center_freq_changed: bad channel");
    HIPCHK(hipSetDevice(c->device));
    if (c->burst)
    {
        // BurstOqpskDemodulator::CenterFreqChangedSlot does nothing (burstoqpskdemodulator.cpp:284-289)
        if (c->bg.kind == JAERO_KIND_BURST_OQPSK) return 0;
        // BurstMskDemodulator::CenterFreqChangedSlot (burstmskdemodulator.cpp:327-342), on the bank's stream like every other call
        return burst_launch_center_freq(c, channel, hz);
    }
    const int lo = channel < 0 ? 0 : channel, n = channel < 0 ? c->g.nch : 1;
    hipLaunchKernelGGL(k_center_freq, dim3(n), dim3(256), 0, c->last_stream, c->g, c->p, lo, n, hz);
    HIPCHK(hipGetLastError());
    return 0;
}

// setSettings on live channels [ch_lo, ch_hi): the scalar fields it rewrites, the counters it restarts and the rings it recreates
// (= zeroes), for those channels' columns only.  blockIdx.x = channel - ch_lo, blockIdx.y strides over ring slots.
struct JSetVals
{
    int nS, nI;
    int fS[40]; double vS[40];   // S[fS[k]][ch] = vS[k]
    int fI[16]; int vI[16];      // I[fI[k]][ch] = vI[k]
    int zero_eb, zero_msk;       // MSK also recreates the EbNo meter, marg and the quadrature delay line
    int dly_rot;                 // MSK: slots by which the channel's delayedsmpl column is rotated (see below)
};
__global__ void k_apply_settings(const JGeom g, const JPtrs p, int ch_lo, const JSetVals v)
{
    const int ch = ch_lo + blockIdx.x, nchp = g.nchp;
    const int grp = ch >> 6, lane = ch & 63;
    if (blockIdx.y == 0)
    {
        for (int k = threadIdx.x; k < v.nS; k += blockDim.x) p.S[(size_t)v.fS[k] * nchp + ch] = v.vS[k];
        for (int k = threadIdx.x; k < v.nI; k += blockDim.x) p.I[(size_t)v.fI[k] * nchp + ch] = v.vI[k];
    }
    const int tid = blockIdx.y * blockDim.x + threadIdx.x, nth = gridDim.y * blockDim.x;
    // OQPSK: the AGC is re-created but the EbNo meter keeps its buffer, and both live in the one window ring: I_AGC_HOLD instead of zeros
    if (v.zero_eb) for (int s = tid; s < g.win_len; s += nth) p.win[((size_t)grp * g.win_len + s) * 64 + lane] = 0.0;
    for (int s = tid; s < 2 * g.fir_n; s += nth) p.firsave[((size_t)grp * 2 * g.fir_n + s) * 64 + lane] = 0.0;
    if (v.zero_msk)
    {
        for (int s = tid; s < g.marg_len; s += nth) p.marg[(size_t)ch * g.marg_len + s] = 0.0;
        for (int s = tid; s < g.sps2 + 1; s += nth) p.dly8[((size_t)grp * (g.sps2 + 1) + s) * 64 + lane] = 0.0;
        // delayedsmpl.setLength(SPS) keeps the buffer's contents and restarts its pointer at 0 (DSP.h:446-453).  Here the ring slot is
        // shared by the 64 channels of a wavefront (slot = samples so far mod SPS+1), so restarting ONE channel's pointer means
        // rotating that channel's column by the distance between the shared slot now and the slot its pointer last restarted at.
        if (tid == 0 && v.dly_rot > 0)
        {
            const int L = g.sps + 1; // 41 or 81
            double2 tmp[96];
            for (int s = 0; s < L; s++) tmp[s] = p.dly[((size_t)grp * L + s) * 64 + lane];
            for (int s = 0; s < L; s++) p.dly[((size_t)grp * L + (s + v.dly_rot) % L) * 64 + lane] = tmp[s];
        }
    }
}

// setSettings on the channels [lo, hi) of a bank whose kind, rates and FFT size stay what they are: only those channels' columns are touched,
// by one small kernel on the stream of the last jaero_write (no device synchronisation, no copy of the bank's state)
static int apply_live_settings(jaero_ctx *c, int lo, int hi, const jaero_settings *s)
{
    const JGeom &g = c->g;
    HIPCHK(hipSetDevice(c->device));
    const int nchp = g.nchp;
    // what init_channel_scalars(fresh = false) writes, computed once (the same for every addressed channel) on a one-column scratch
    std::vector<double> S((size_t)S_NFIELDS, 0.0);
    std::vector<int> I((size_t)I_NFIELDS, 0);
    init_channel_scalars(c, *s, S, I, 0, false, 1);
    JSetVals v{};
    auto setS = [&](int f, double x) { v.fS[v.nS] = f; v.vS[v.nS] = x; v.nS++; };
    auto setI = [&](int f, int x) { v.fI[v.nI] = f; v.vI[v.nI] = x; v.nI++; };
    for (int f : {S_M2_FREQ, S_M2_STEP, S_MC_FREQ, S_MC_STEP, S_ST_FREQ, S_ST_STEP, S_LOCKINGBW, S_THRESH}) setS(f, S[(size_t)f]);
    if (g.kind == JAERO_KIND_OQPSK)
        for (int f : {S_AGC_SUM, S_D1, S_D41_1, S_D41_2, S_D41_3, S_D42_1, S_D42_2, S_D42_3, S_D8_1, S_D8_2, S_RES_X1, S_RES_X2, S_RES_Y1, S_RES_Y2}) setS(f, 0.0);
    else
    {
        setS(S_MSE, 10.0); // setSettings resets mse (mskdemodulator.cpp:180)
        for (int f : {S_AGC_SUM, S_RES_X1, S_RES_X2, S_RES_Y1, S_RES_Y2, S_EB_ESUM, S_EB_E2SUM, S_EB_EBNO, S_MARG_SUM, S_MFB_A0_RE, S_MFB_A0_IM}) setS(f, 0.0);
        setI(I_MARG_POS, 0); setI(I_DT_POS, 0);
        v.zero_eb = 1; v.zero_msk = 1;
    }
    setI(I_BB_PTR, 0); setI(I_COARSE_CNT, 0);
    if (g.kind == JAERO_KIND_OQPSK) setI(I_AGC_HOLD, g.agc_len); // new AGC(4, Fs): an empty window; the ring's position and contents stay (the meter's)
    else setI(I_AGC_POS, 0);
    for (int ch = lo; ch < hi; ch++)
    {
        c->settings[ch] = *s;
        c->m.bbptr[ch] = 0; c->m.cnt[ch] = 0;
    }
    update_band_class(c, lo, hi);
    const int ny = (hi - lo) >= 256 ? 4 : 64; // one channel: 64 blocks share its 192 000-slot AGC column; the whole bank: four per channel
    if (g.kind == JAERO_KIND_MSK)
    {
        // runs of channels whose delayedsmpl pointer last restarted at the same shared slot get one launch each (normally: one run)
        const int L = g.sps + 1;
        const int now = (int)(c->m.nB_total % L);
        if (c->dly_t0.empty()) c->dly_t0.assign(nchp, 0);
        for (int a = lo; a < hi;)
        {
            int b = a + 1;
            while (b < hi && c->dly_t0[b] == c->dly_t0[a]) b++;
            v.dly_rot = ((now - c->dly_t0[a]) % L + L) % L;
            hipLaunchKernelGGL(k_apply_settings, dim3(b - a, ny), dim3(256), 0, c->last_stream, g, c->p, a, v);
            for (int ch = a; ch < b; ch++) c->dly_t0[ch] = now;
            a = b;
        }
    }
    else hipLaunchKernelGGL(k_apply_settings, dim3(hi - lo, ny), dim3(256), 0, c->last_stream, g, c->p, lo, v);
    HIPCHK(hipGetLastError());
    return 0;
}

// k_carry_dly: MSK delayedsmpl.setLength(SamplesPerSymbol) keeps the buffer's first min(old, new) entries IN BUFFER ORDER and restarts the
// pointer at 0 (DSP.h:446-453).  Buffer index j of channel ch lives in the old bank's shared slot (t0[ch] + j) mod Lo (t0 = the shared slot at
// which the channel's pointer last restarted) and in slot j of the new bank, whose shared slot counter starts at 0.
__global__ void k_carry_dly(const double2 *__restrict__ od, int Lo, const int *__restrict__ t0, double2 *__restrict__ nd, int Ln, int nchp)
{
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nchp) return;
    const int grp = ch >> 6, lane = ch & 63, keep = Lo < Ln ? Lo : Ln, s0 = t0[ch];
    for (int j = 0; j < keep; j++) nd[((size_t)grp * Ln + j) * 64 + lane] = od[((size_t)grp * Lo + (s0 + j) % Lo) * 64 + lane];
}

// setSettings that changes what a bank fixes (bit rate, sample rate, FFT size; any setSettings of an 8400 bps bank, whose prefilter restarts):
// the reference rebuilds AGC, matched filters, delays, resonator (and at 8400 bps the prefilter) INSIDE the old object, which keeps its oscillator
// phases, loop-filter and rotator states, moving-average windows, the coarse ring's contents and the smoothed spectrum (oqpskdemodulator.cpp:
// 175-289, mskdemodulator.cpp:135-263).  Here: a sibling bank is created for the new settings, those survivors are copied into it, the same
// in-place setSettings as above runs on it, and it takes the place of the old bank behind the handle.  Whole banks only; control plane (it
// allocates and synchronises).  Outputs not read yet move along; device pointers obtained from the views are stale.
static int rebank_with_carry_over(jaero_ctx *c, const jaero_settings *s)
{
    const JGeom og = c->g;
    LINKCHK(c);
    if (c->poisoned) return fail(JAERO_EHIP, "jaero_set_settings: a launch inside an earlier jaero_write failed; this bank's state cannot be carried over");
    if (og.kind == JAERO_KIND_OQPSK && s->Fs != og.Fs) return fail(JAERO_ENOTSUP, "jaero_set_settings: an OQPSK bank keeps its sample rate");
    QUIESCE(c);
    jaero_ctx *n = nullptr;
    int rc = jaero_create(c->device, og.nch, s, 0, c->flags, c->max_write, c->soft_cap_req, &n);
    if (rc) return rc;
    BankPtr nb(n, jaero_destroy); // goes again on every early return
    const JGeom &ng = n->g;
    const int nchp = og.nchp;
    if ((rc = carry(n->p.S, c->p.S, sizeof(double) * (size_t)S_NFIELDS * nchp)) || (rc = carry(n->p.I, c->p.I, sizeof(int) * (size_t)I_NFIELDS * nchp))) return rc;
    {
        // outputs not read yet (soft bits, captured symbols, status rows) move to the new bank's buffers; its capacities follow the new rate
        std::vector<int> cnt(3 * (size_t)nchp);
        static_assert(I_SYM_CNT == I_SOFT_CNT + 1 && I_LOG_CNT == I_SOFT_CNT + 2, "output counters are consecutive columns");
        HIPCHK(hipMemcpy(cnt.data(), c->p.I + (size_t)I_SOFT_CNT * nchp, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
        int mx[3] = {0, 0, 0};
        for (int k = 0; k < 3; k++) for (int ch = 0; ch < og.nch; ch++) mx[k] = cnt[(size_t)k * nchp + ch] > mx[k] ? cnt[(size_t)k * nchp + ch] : mx[k];
        if (mx[0] > ng.soft_cap || mx[1] > ng.sym_cap || mx[2] > ng.log_cap)
            return fail(JAERO_EINVAL, "jaero_set_settings: unread outputs (%d soft bits, %d symbols, %d status rows) exceed the new bank's buffers; read them first", mx[0], mx[1], mx[2]);
        if ((rc = carry_rows(n->p.soft, ng.soft_cap, c->p.soft, og.soft_cap, sizeof(int16_t), mx[0], nchp)) ||
            (rc = carry_rows(n->p.sym, ng.sym_cap, c->p.sym, og.sym_cap, 3 * sizeof(double), mx[1], nchp)) ||
            (rc = carry_rows(n->p.slog, ng.log_cap, c->p.slog, og.log_cap, 6 * sizeof(double), mx[2], nchp)))
            return rc;
    }
    // windows that survive: msema (both kinds); marg / dt / pm of the OQPSK demodulator (MSK: marg is new, dt keeps a prefix, below)
    if ((rc = carry(n->p.msema, c->p.msema, sizeof(double) * (size_t)nchp * og.msema_len))) return rc;
    if (og.kind == JAERO_KIND_OQPSK)
    {
        if ((rc = carry(n->p.marg, c->p.marg, sizeof(double) * (size_t)nchp * og.marg_len)) || (rc = carry(n->p.dt, c->p.dt, sizeof(double2) * (size_t)nchp * og.dt_len)) ||
            (rc = carry(n->p.pm, c->p.pm, sizeof(double) * (size_t)nchp * og.pm_len)))
            return rc;
        // k_oqpsk_fb keeps the four windows in one record ring
        if (c->p.symrec && n->p.symrec && (rc = carry(n->p.symrec, c->p.symrec, sizeof(double) * (size_t)nchp * JD_SYMREC_LEN * 8))) return rc;
        // the OQPSK EbNo meter is only told the new rates (setup_update, DSP.cpp:723-727): its window -- the newest ebno_len entries of the window
        // ring, at the position that came over with I -- stays; the AGC is new (I_AGC_HOLD, set by apply_live_settings below)
        if ((c->flags & JAERO_FLAG_EBNO) && og.win_len == ng.win_len && (rc = carry(n->p.win, c->p.win, sizeof(double) * (size_t)og.ngroups * og.win_len * 64))) return rc;
    }
    else
    {
        const int keep = og.dt_len < ng.dt_len ? og.dt_len : ng.dt_len; // dt.setLength: DelayThing keeps the first entries (DSP.h:446-453)
        if ((rc = carry_rows(n->p.dt, ng.dt_len, c->p.dt, og.dt_len, sizeof(double2), keep, nchp)) ||
            (rc = carry(n->p.pm, c->p.pm, sizeof(double) * (size_t)nchp * (og.pm_len < ng.pm_len ? og.pm_len : ng.pm_len))))
            return rc;
        DevMem tmp;
        int *d_t0 = nullptr;
        if (c->dly_t0.empty()) c->dly_t0.assign(nchp, 0);
        DA(tmp, d_t0, nchp);
        HIPCHK(hipMemcpy(d_t0, c->dly_t0.data(), sizeof(int) * nchp, hipMemcpyHostToDevice));
        // the old bank's shared slot counter stands at nB_total: a channel whose pointer restarted at slot t0 has its buffer index 0 there
        hipLaunchKernelGGL(k_carry_dly, dim3((nchp + 255) / 256), dim3(256), 0, 0, (const double2 *)c->p.dly, og.sps + 1, (const int *)d_t0, (double2 *)n->p.dly, ng.sps + 1, nchp);
        hipStreamSynchronize(0); // this copy's stream only: other banks on the GPU keep running
    }
    {
        // bbcycbuff.resize / y.resize: same size = untouched, otherwise the first entries stay (new ones are zero)
        const int keep = og.nfft < ng.nfft ? og.nfft : ng.nfft;
        if ((rc = carry_rows(n->p.bbring, ng.nfft, c->p.bbring, og.nfft, sizeof(double2), keep, nchp)) ||
            (rc = carry_rows(n->p.y, ng.nfft, c->p.y, og.nfft, sizeof(double), keep, nchp)))
            return rc;
    }
    if (og.kind == JAERO_KIND_OQPSK)
    {
        // mixer_fir_pre is not touched by setSettings: its phase stays.  Its frequency is set at the end of every write to mixer2_freq_sum / i
        // (oqpskdemodulator.cpp:607-608; applied here by k_pre8400_mix at the start of the next write from S_PRE_FSUM / nprev), and that sum
        // only grows in the 8400 bps branch (:447): after a write at another rate the reference's prefilter oscillator stands at 0 Hz, which
        // is what its first 8400 bps write then mixes with.  Same here: sum 0 over the length of the last write.
        n->pre_nprev = c->pre_nprev;
        if (!c->pre8400) HIPCHK(hipMemset(n->p.S + (size_t)S_PRE_FSUM * nchp, 0, sizeof(double) * (size_t)nchp));
    }
    if ((rc = apply_live_settings(n, 0, ng.nchp, s))) return rc; // the padding lanes too: their window positions came over with I and must fit the new lengths
    if (n->quiesce() || hipStreamSynchronize(0) != hipSuccess) return fail(JAERO_EHIP, "jaero_set_settings: carry-over failed");
    swap_in(c, std::move(nb));
    return 0;
}

extern "C" int jaero_set_settings(jaero_ctx *c, int channel, const jaero_settings *s)
{
    // setSettings on a live object (oqpskdemodulator.cpp:175-289, mskdemodulator.cpp:135-263): retunes the mixers
    // (phase kept), recreates AGC / matched filters / timing delays / resonator, restarts the coarse ring pointer.
    if (!c || !s || channel < -1 || channel >= c->o_nch) return fail(JAERO_EINVAL, "jaero_set_settings: bad arguments");
    POISONCHK(c, "jaero_set_settings", POISON_BANK);
    int rc = validate_settings(*s);
    if (rc) return rc;
    if (c->burst) return burst_set_settings(c, channel, s);
    const JGeom &g = c->g;
    if (s->kind != g.kind) return fail(JAERO_EINVAL, "jaero_set_settings: the kind of a bank is fixed (another demodulator class in the reference); create a new bank");
    const bool whole = channel < 0 || g.nch == 1;
    if (s->fb != g.fb || s->Fs != g.Fs || s->coarsefreqest_fft_power != g.nfft_log2)
    {
        if (!whole) return fail(JAERO_EINVAL, "jaero_set_settings: fb/Fs/fft_power are shared by the channels of a bank; change them for the whole bank (channel = -1)");
        return rebank_with_carry_over(c, s);
    }
    if (c->pre8400)
    {
        // fb = 8400: setSettings also re-creates the prefilter (JFastFir::SetKernel: empty history, 2048 zeros of latency, transform blocks
        // re-aligned to that moment).  The whole bank: re-created behind the handle, blocks re-aligned.  One channel of several: its column
        // of the prefilter history is emptied and its outputs held at exact zeros for 2048 samples (k_pre8400_restart); the transform blocks
        // stay on the bank's grid (round 5; refused until then)
        if (whole) return rebank_with_carry_over(c, s);
        HIPCHK(hipSetDevice(c->device));
        if ((rc = launch_pre8400_restart(c, channel, c->last_stream))) return rc;
        return apply_live_settings(c, channel, channel + 1, s);
    }
    HIPCHK(hipSetDevice(c->device));
    return apply_live_settings(c, channel < 0 ? 0 : channel, channel < 0 ? g.nch : channel + 1, s);
}

// ------------------------------------------------------------------------------------------ profiling
extern "C" int jaero_profile_enable(jaero_ctx *c, int on)
{
    if (!c) return fail(JAERO_EINVAL, "null ctx");
    c->timer.on = on != 0;
    return 0;
}
extern "C" int jaero_profile_read(jaero_ctx *c, int which, double *total_ms, int *launches, int reset)
{
    if (!c || which < 0 || which > 4) return fail(JAERO_EINVAL, "jaero_profile_read: bad arguments");
    return c->timer.read(c->device, which, total_ms, launches, reset);
}

extern "C" int jaero_profile2_read(jaero_ctx *c, int which, double *total_ms, int *launches, int reset)
{
    if (!c || which < 0 || which > 5) return fail(JAERO_EINVAL, "jaero_profile2_read: bad arguments");
    return c->timer.read(c->device, which, total_ms, launches, reset);
}

extern "C" int jaero_profile_kernel(jaero_ctx *c, int which, char *buf, int cap)
{
    if (!c || !buf || cap < 2 || which < 0 || which > 4) return fail(JAERO_EINVAL, "jaero_profile_kernel: bad arguments");
    const char *nm = "";
    if (c->burst)
    {
        const char *bn[5] = {c->bdemod.name, c->trident.name, "k_hist_push", "k_hilbert_fft", "k_burst_front"};
        nm = bn[which];
    }
    else if (which == 0) nm = c->g.kind == JAERO_KIND_OQPSK ? c->oq_loop.name : c->msk_loop.name;
    else if (which == 1) nm = c->coarse.name;
    else if (which == 2) nm = "k_transpose_pcm";
    snprintf(buf, (size_t)cap, "%s", nm);
    return 0;
}

extern "C" int jaero_debug_kernel_variant(jaero_ctx *c, int which, char *buf, int cap)
{
    if (!c || !buf || cap < 2 || which < 0 || which > 1) return fail(JAERO_EINVAL, "jaero_debug_kernel_variant: bad arguments (which: 0 or 1)");
    const std::string *v;
    if (c->burst) v = which == 0 ? &c->bdemod.variant : &c->trident.variant;
    else if (which == 0) v = c->g.kind == JAERO_KIND_OQPSK ? &c->oq_loop.variant : &c->msk_loop.variant;
    else v = &c->coarse.variant;
    if ((int)v->size() >= cap) return fail(JAERO_EOVERFLOW, "jaero_debug_kernel_variant: %zu characters do not fit in %d", v->size(), cap);
    snprintf(buf, (size_t)cap, "%s", v->c_str());
    return 0;
}

// ------------------------------------------------------------------------------------------ write
// one segment of the sample loop; nb0 = B-parts executed before it (the ring slots it starts at derive from it)
static void launch_samples(jaero_ctx *c, const int16_t *frames, int stride, int n, int skipA, int onlyA, long long nb0, int pos, hipStream_t st)
{
    const JGeom &g = c->g;
    if (g.kind == JAERO_KIND_OQPSK)
    {
        const KernelRec<OqpskSampleFn> &r = c->oq_loop;
        const double2 *pf = c->pre8400 ? (const double2 *)(c->pre.out + (size_t)pos * 4) : nullptr; // row `pos` of every channel group (JD_G4)
        hipLaunchKernelGGL(r.fn, dim3(r.grid), dim3(r.block), r.lds, st, g, c->p, frames, stride, n, skipA, onlyA, (int)(nb0 % r.ldsn), c->oq_taps, pf, c->pre.cap);
    }
    else
    {
        const KernelRec<MskSampleFn> &r = c->msk_loop;
        hipLaunchKernelGGL(r.fn, dim3(r.grid), dim3(r.block), r.lds, st, g, c->p, frames, stride, n, skipA, onlyA, (int)(nb0 % r.ldsn), (int)(nb0 % (g.sps + 1)),
                           (int)(nb0 % (g.sps2 + 1)));
    }
}

// the bank's estimate kernel over a list (d_list = nullptr: channels 0 .. nlist - 1) on `grid` workgroups, each persistent over its share
static void launch_coarse_grid(jaero_ctx *c, const int *d_list, int nlist, int grid, hipStream_t st)
{
    const KernelRec<CoarseFn> &r = c->coarse;
    hipLaunchKernelGGL(r.fn, dim3(grid), dim3(r.block), r.lds, st, c->g, c->p, d_list, nlist, c->d_tw);
}
static int coarse_grid(const jaero_ctx *c, int nlist) { return nlist < c->coarse.grid ? nlist : c->coarse.grid; }
// The estimates of h_list[0 .. nlist) (nullptr: channels 0 .. nlist - 1, the whole bank) on at most `grid` workgroups per launch, each on the
// kernel its channel's band class names: one launch when the list is of one class -- with d_chanlist filled from h_list, or no list at all --
// and otherwise two, the band part first, the order within each part kept.  async: the list is copied on the stream (jaero_write).
static int launch_coarse_lists(jaero_ctx *c, const int *h_list, int nlist, int grid, hipStream_t st, bool async)
{
    int nband = 0;
    if (c->band.rec.fn && !c->band.force_generic)
        for (int k = 0; k < nlist; k++) nband += c->band.cls[h_list ? h_list[k] : k];
    const int *src = h_list;
    if (nband != 0 && nband != nlist)
    {
        c->band.split.resize((size_t)nlist);
        int a = 0, b = nband;
        for (int k = 0; k < nlist; k++)
        {
            const int ch = h_list ? h_list[k] : k;
            c->band.split[(size_t)(c->band.cls[ch] ? a++ : b++)] = ch;
        }
        src = c->band.split.data();
    }
    if (src)
    {
        if (async) HIPCHK(hipMemcpyAsync(c->d_chanlist, src, sizeof(int) * (size_t)nlist, hipMemcpyHostToDevice, st));
        else HIPCHK(hipMemcpy(c->d_chanlist, src, sizeof(int) * (size_t)nlist, hipMemcpyHostToDevice));
    }
    const int ngen = nlist - nband;
    if (nband)
    {
        const KernelRec<CoarseFn> &r = c->band.rec;
        hipLaunchKernelGGL(r.fn, dim3(grid < nband ? grid : nband), dim3(r.block), r.lds, st, c->g, c->p, src ? c->d_chanlist : nullptr, nband, c->d_tw);
    }
    if (ngen) launch_coarse_grid(c, src ? c->d_chanlist + nband : nullptr, ngen, grid < ngen ? grid : ngen, st);
    c->band.est_band += nband; c->band.est_generic += ngen;
    return 0;
}

extern "C" int jaero_write(jaero_ctx *c, const int16_t *pcm, int nsamples, int layout, int is_device_ptr, void *stream)
{
    if (!c || !pcm || nsamples < 0) return fail(JAERO_EINVAL, "jaero_write: bad arguments");
    if (nsamples == 0) return 0;
    if (nsamples > c->max_write) return fail(JAERO_EINVAL, "jaero_write: nsamples %d exceeds max_write_samples %d", nsamples, c->max_write);
    if (layout != JAERO_PCM_CHANNEL_MAJOR && layout != JAERO_PCM_FRAME_MAJOR) return fail(JAERO_EINVAL, "jaero_write: bad layout");
    if (c->poisoned) return fail(JAERO_EHIP, "jaero_write: an earlier write of this bank failed part-way (its schedule mirror is ahead of the device state): destroy the bank and create a new one");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    { const int rc = c->order_behind(st); if (rc) return rc; } // setters, discards and earlier writes were enqueued on last_stream
    // poisoned is raised where the first launch that advances device state or the schedule mirror is about to be enqueued (a failed copy of
    // the input, transpose or history push leaves both as they were: the caller may simply write again) and lowered when the whole write is in
    if (c->burst) return burst_write(c, pcm, nsamples, layout, is_device_ptr, st);
    const JGeom &g = c->g;
    const int nch = g.nch;

    const int16_t *frames = nullptr;
    int stride = 0;
    { const int rc = stage_pcm(c, pcm, nsamples, layout, is_device_ptr, st, &frames, &stride); if (rc) return rc; }

    PoisonGuard guard(*c); // from here on device state and mirror advance together or not at all
    if (c->pre8400)
    {
        const int rc = launch_pre8400_stage(c, frames, stride, nsamples, pre8400_stretches(g, nsamples), st);
        if (rc) return rc;
    }
    if (g.kind == JAERO_KIND_OQPSK) c->pre_nprev = nsamples; // (at every rate: a bank re-created for 8400 bps needs the length of the last write, rebank_with_carry_over)
    int pos = 0;
    while (pos < nsamples)
    {
        int n = 0, skip_a = 0, only_a = 0;
        const long long nb0 = c->m.nB_total; // ring slots are those at the START of the segment
        const int next = c->m.next_segment(pos, nsamples, n, skip_a, only_a);
        if (n > 0)
        {
            const int pi = c->timer.begin(0, st);
            launch_samples(c, frames + (size_t)pos * stride, stride, n, skip_a, only_a, nb0, pos, st);
            LAUNCHCHK("the sample loop");
            c->timer.end(pi, st);
        }
        if (only_a)
        {
            const int nlist = (int)c->m.fired.size();
            const int pi = c->timer.begin(1, st);
            { const int rc = launch_coarse_lists(c, nlist != nch ? c->m.fired.data() : nullptr, nlist, coarse_grid(c, nlist), st, true); if (rc) return rc; }
            LAUNCHCHK("the coarse-frequency estimate");
            c->timer.end(pi, st);
        }
        pos = next;
    }
    HIPCHK(hipGetLastError());
    guard.commit();
    return 0;
}

// ------------------------------------------------------------------------------------------ test hooks: the estimate kernel alone
// (tests/test_gpu_coarse.py).  A poked bank's schedule mirror (Mirror::bbptr, flags) no longer matches the device: poisoned, as after a
// write that failed part-way.
static int coarse_hook_enter(jaero_ctx *c, const char *who, int channel)
{
    if (!c) return fail(JAERO_EINVAL, "%s: null ctx", who);
    if (c->burst) return fail(JAERO_EINVAL, "%s: a burst bank has no coarse-frequency estimate", who);
    if (channel < 0 || channel >= c->g.nch) return fail(JAERO_EINVAL, "%s: channel %d outside [0, %d)", who, channel, c->g.nch);
    QUIESCE(c);
    c->poisoned = true;
    return 0;
}
extern "C" int jaero_debug_coarse_poke(jaero_ctx *c, int ch, const double *ring_reim, const double *y, const jaero_coarse_state *st)
{
    int rc = coarse_hook_enter(c, "jaero_debug_coarse_poke", ch);
    if (rc) return rc;
    const JGeom &g = c->g;
    const size_t N = (size_t)g.nfft, nchp = (size_t)g.nchp;
    if (st && (st->bb_ptr < 0 || st->bb_ptr >= g.nfft || !(st->m2_freq >= 0) || !(st->mc_freq >= 0) || st->emptying < 0 || st->countdown < 0 ||
               st->countdown2 < 0 || st->coarse_cnt < 0 || (st->flags & ~(JF_AFC | JF_SQL | JF_CPUREDUCE | JF_DCD))))
        return fail(JAERO_EINVAL, "jaero_debug_coarse_poke: state out of range (bb_ptr in [0, nfft), counters and frequencies >= 0, flags 0..15)");
    if (ring_reim) HIPCHK(hipMemcpy(c->p.bbring + (size_t)ch * N, ring_reim, sizeof(double2) * N, hipMemcpyHostToDevice));
    if (y) HIPCHK(hipMemcpy(c->p.y + (size_t)ch * N, y, sizeof(double) * N, hipMemcpyHostToDevice));
    if (st)
    {
        const double wt = ((double)JD_WTSIZE) / ((float)(double)g.Fs_int); // WaveTable::SetFreq's step, as init_channel_scalars forms it
        const std::pair<int, int> iv[] = {{I_BB_PTR, st->bb_ptr}, {I_EMPTYING, st->emptying}, {I_FLAGS, st->flags}, {I_COUNTDOWN, st->countdown},
                                          {I_COUNTDOWN2, st->countdown2}, {I_COARSE_CNT, st->coarse_cnt}};
        const std::pair<int, double> dv[] = {{S_MSE, st->mse}, {S_M2_FREQ, st->m2_freq}, {S_M2_STEP, st->m2_freq * wt}, {S_MC_FREQ, st->mc_freq},
                                             {S_MC_STEP, st->mc_freq * wt}};
        for (const auto &[f, v] : iv) HIPCHK(hipMemcpy(c->p.I + (size_t)f * nchp + ch, &v, sizeof(int), hipMemcpyHostToDevice));
        for (const auto &[f, v] : dv) HIPCHK(hipMemcpy(c->p.S + (size_t)f * nchp + ch, &v, sizeof(double), hipMemcpyHostToDevice));
    }
    return 0;
}
extern "C" int jaero_debug_coarse_peek(jaero_ctx *c, int ch, double *ring_reim, double *y, jaero_coarse_state *st)
{
    int rc = coarse_hook_enter(c, "jaero_debug_coarse_peek", ch);
    if (rc) return rc;
    const JGeom &g = c->g;
    const size_t N = (size_t)g.nfft, nchp = (size_t)g.nchp;
    if (ring_reim) HIPCHK(hipMemcpy(ring_reim, c->p.bbring + (size_t)ch * N, sizeof(double2) * N, hipMemcpyDeviceToHost));
    if (y) HIPCHK(hipMemcpy(y, c->p.y + (size_t)ch * N, sizeof(double) * N, hipMemcpyDeviceToHost));
    if (st)
    {
        const std::pair<int, int *> iv[] = {{I_BB_PTR, &st->bb_ptr}, {I_EMPTYING, &st->emptying}, {I_FLAGS, &st->flags}, {I_COUNTDOWN, &st->countdown},
                                            {I_COUNTDOWN2, &st->countdown2}, {I_COARSE_CNT, &st->coarse_cnt}, {I_NEST, &st->nest}, {I_LOG_CNT, &st->log_cnt}};
        const std::pair<int, double *> dv[] = {{S_MSE, &st->mse}, {S_M2_FREQ, &st->m2_freq}, {S_MC_FREQ, &st->mc_freq}};
        if ((rc = peek_fields(c->p.I, nchp, ch, iv)) || (rc = peek_fields(c->p.S, nchp, ch, dv))) return rc;
    }
    return 0;
}
extern "C" int jaero_debug_coarse_launch(jaero_ctx *c, const int *channels, int nlist, int grid)
{
    int rc = coarse_hook_enter(c, "jaero_debug_coarse_launch", 0);
    if (rc) return rc;
    const int nch = c->g.nch;
    if (channels ? (nlist < 1 || nlist > nch) : nlist != nch)
        return fail(JAERO_EINVAL, "jaero_debug_coarse_launch: nlist %d (a list of 1 .. %d channels, or NULL with all %d)", nlist, nch, nch);
    if (channels)
    {
        std::vector<char> seen((size_t)nch, 0);
        for (int k = 0; k < nlist; k++)
        {
            if (channels[k] < 0 || channels[k] >= nch || seen[(size_t)channels[k]])
                return fail(JAERO_EINVAL, "jaero_debug_coarse_launch: entry %d (channel %d) is outside [0, %d) or listed twice", k, channels[k], nch);
            seen[(size_t)channels[k]] = 1;
        }
    }
    const int gmax = coarse_grid(c, nlist);
    if (grid < 0 || grid > gmax) return fail(JAERO_EINVAL, "jaero_debug_coarse_launch: grid %d (0 = as jaero_write, else 1 .. %d for %d channels)", grid, gmax, nlist);
    if ((rc = launch_coarse_lists(c, channels, nlist, grid ? grid : gmax, c->last_stream, false))) return rc;
    LAUNCHCHK("the coarse-frequency estimate");
    QUIESCE(c);
    return 0;
}
// ------------------------------------------------------------------------------------------ test hooks: the sample loop's slow state
// (tests/test_gpu_loop_branches.py).  The symbol oscillator's and mixer2's frequency and the carrier loop filter's history live in S between
// launches and nowhere else: the schedule mirror does not depend on them, so the bank is not poisoned and goes on taking writes.
static const int LOOP_FIELDS[6] = {S_ST_FREQ, S_M2_FREQ, S_LF_X1, S_LF_X2, S_LF_Y1, S_LF_Y2};
#define LOOP_HOOK_ENTER(who)                                                                                                                       \
    if (!c) return fail(JAERO_EINVAL, who ": null ctx");                                                                                           \
    if (!st) return fail(JAERO_EINVAL, who ": null state");                                                                                        \
    if (c->burst) return fail(JAERO_EINVAL, who ": a burst bank has no continuous sample loop");                                                   \
    if (ch < 0 || ch >= c->g.nch) return fail(JAERO_EINVAL, who ": channel %d outside [0, %d)", ch, c->g.nch);                                     \
    POISONCHK(c, who, POISON_BANK)
extern "C" int jaero_debug_loop_poke(jaero_ctx *c, int ch, const jaero_loop_state *st)
{
    LOOP_HOOK_ENTER("jaero_debug_loop_poke");
    const double v[6] = {st->st_freq, st->m2_freq, st->lf_x1, st->lf_x2, st->lf_y1, st->lf_y2};
    for (double x : v)
        if (!std::isfinite(x)) return fail(JAERO_EINVAL, "jaero_debug_loop_poke: a value is not finite");
    if (st->st_freq < 0 || st->m2_freq < 0) return fail(JAERO_EINVAL, "jaero_debug_loop_poke: st_freq and m2_freq must be >= 0");
    QUIESCE(c);
    const size_t nchp = (size_t)c->g.nchp;
    // WaveTable::SetFreq's step, in init_channel_scalars' order of operations: (freq * WTSIZE) / Fs, the quotient the kernels' own SetFreq forms
    const float fs = (float)(double)c->g.Fs_int;
    const std::pair<int, double> steps[] = {{S_ST_STEP, st->st_freq * ((double)JD_WTSIZE) / fs}, {S_M2_STEP, st->m2_freq * ((double)JD_WTSIZE) / fs}};
    for (int k = 0; k < 6; k++) HIPCHK(hipMemcpy(c->p.S + (size_t)LOOP_FIELDS[k] * nchp + ch, &v[k], sizeof(double), hipMemcpyHostToDevice));
    for (const auto &[f, x] : steps) HIPCHK(hipMemcpy(c->p.S + (size_t)f * nchp + ch, &x, sizeof(double), hipMemcpyHostToDevice));
    return 0;
}
extern "C" int jaero_debug_loop_peek(jaero_ctx *c, int ch, jaero_loop_state *st)
{
    LOOP_HOOK_ENTER("jaero_debug_loop_peek");
    QUIESCE(c);
    const std::pair<int, double *> v[] = {{S_ST_FREQ, &st->st_freq}, {S_M2_FREQ, &st->m2_freq}, {S_LF_X1, &st->lf_x1}, {S_LF_X2, &st->lf_x2},
                                          {S_LF_Y1, &st->lf_y1}, {S_LF_Y2, &st->lf_y2}};
    return peek_fields(c->p.S, (size_t)c->g.nchp, ch, v);
}
#undef LOOP_HOOK_ENTER
extern "C" int jaero_debug_coarse_band(jaero_ctx *c, char *buf, int cap, long long *est_generic, long long *est_band)
{
    if (!c || !buf || cap < 2) return fail(JAERO_EINVAL, "jaero_debug_coarse_band: bad arguments");
    if (c->burst) return fail(JAERO_EINVAL, "jaero_debug_coarse_band: a burst bank has no coarse-frequency estimate");
    const std::string &v = c->band.rec.variant; // empty: the bank has no band-aware kernel
    if ((int)v.size() >= cap) return fail(JAERO_EOVERFLOW, "jaero_debug_coarse_band: %zu characters do not fit in %d", v.size(), cap);
    snprintf(buf, (size_t)cap, "%s", v.c_str());
    if (est_generic) *est_generic = c->band.est_generic;
    if (est_band) *est_band = c->band.est_band;
    return 0;
}
extern "C" int jaero_debug_coarse_force_generic(jaero_ctx *c, int on)
{
    if (!c || c->burst) return fail(JAERO_EINVAL, "jaero_debug_coarse_force_generic: a continuous bank's handle");
    c->band.force_generic = on != 0;
    return 0;
}

// Host-only: the segmentation jaero_write would perform for one channel with the given flags over a sequence of
// writes; returns the global sample indices at which the coarse estimate fires (used by CPU tests; no device needed).
extern "C" int jaero_debug_schedule(int fft_power, int Fs, int cpu_reduce, const int *write_sizes, int nwrites,
                                    long long *trigger_samples, int cap, int *segments_out)
{
    if (!write_sizes || !trigger_samples || fft_power < 4 || fft_power > 20) return fail(JAERO_EINVAL, "jaero_debug_schedule: bad arguments");
    Mirror m;
    m.nch = 1; m.nchp = 64; m.nfft = 1 << fft_power; m.Fs_int = Fs;
    m.flags.assign(64, cpu_reduce ? JF_CPUREDUCE : 0); m.bbptr.assign(64, 0); m.cnt.assign(64, 0);
    long long base = 0;
    int ntrig = 0, nseg = 0;
    for (int w = 0; w < nwrites; w++)
    {
        int pos = 0;
        const int ns = write_sizes[w];
        while (pos < ns)
        {
            int n, sa, oa;
            const int next = m.next_segment(pos, ns, n, sa, oa);
            nseg++;
            if (oa) { if (ntrig < cap) trigger_samples[ntrig] = base + pos + n - 1; ntrig++; }
            pos = next;
        }
        base += ns;
    }
    if (segments_out) *segments_out = nseg;
    return ntrig;
}

// Host-only: the same for a whole group of channels that draw their flags independently and change them between writes -- the part of the
// scheduler that decides which lanes of a wavefront fire at which sample (Mirror::steps_to_trigger / next_segment / fired).
// events[k] = {before_write, channel (-1: all), kind, value}: kind 0 = setAFC/SQL/CPUReduce bits (JF_*), kind 1 = DCD, kind 2 = setSettings
// (the channel's ring position and counter restart); applied before write `before_write`.  Records (sample, channel) per firing.
extern "C" int jaero_debug_schedule_lanes(int fft_power, int Fs, int nch, const int *flags0, const int *write_sizes, int nwrites,
                                          const int *events, int nevents, long long *trig_sample_channel, int cap, int *segments_out)
{
    if (!write_sizes || !trig_sample_channel || !flags0 || (nevents > 0 && !events) || nch < 1 || fft_power < 4 || fft_power > 20)
        return fail(JAERO_EINVAL, "jaero_debug_schedule_lanes: bad arguments");
    Mirror m;
    m.nch = nch; m.nchp = (nch + 63) / 64 * 64; m.nfft = 1 << fft_power; m.Fs_int = Fs;
    m.flags.assign(m.nchp, 0); m.bbptr.assign(m.nchp, 0); m.cnt.assign(m.nchp, 0);
    for (int ch = 0; ch < nch; ch++) m.flags[ch] = flags0[ch] & (JF_AFC | JF_SQL | JF_CPUREDUCE | JF_DCD);
    long long base = 0;
    int ntrig = 0, nseg = 0;
    for (int w = 0; w < nwrites; w++)
    {
        for (int k = 0; k < nevents; k++)
        {
            const int *e = events + 4 * k;
            if (e[0] != w) continue;
            if (e[1] < -1 || e[1] >= nch) return fail(JAERO_EINVAL, "jaero_debug_schedule_lanes: bad channel in event %d", k);
            const int lo = e[1] < 0 ? 0 : e[1], hi = e[1] < 0 ? m.nchp : e[1] + 1;
            for (int ch = lo; ch < hi; ch++)
            {
                if (e[2] == 0) m.flags[ch] = (m.flags[ch] & JF_DCD) | (e[3] & (JF_AFC | JF_SQL | JF_CPUREDUCE)); // jaero_set_flags
                else if (e[2] == 1) m.flags[ch] = (m.flags[ch] & ~JF_DCD) | (e[3] ? JF_DCD : 0);               // jaero_set_dcd
                else { m.bbptr[ch] = 0; m.cnt[ch] = 0; }                                                        // jaero_set_settings
            }
        }
        int pos = 0;
        const int ns = write_sizes[w];
        while (pos < ns)
        {
            int n, sa, oa;
            const int next = m.next_segment(pos, ns, n, sa, oa);
            nseg++;
            if (oa)
                for (int ch : m.fired)
                {
                    if (ntrig < cap) { trig_sample_channel[2 * ntrig] = base + pos + n - 1; trig_sample_channel[2 * ntrig + 1] = ch; }
                    ntrig++;
                }
            pos = next;
        }
        base += ns;
    }
    if (segments_out) *segments_out = nseg;
    return ntrig;
}

// Test hook: the 8400 bps prefilter kernel (k_pre8400_fft) alone (one channel, unity up-mix) on n complex samples, kernel RRC(alpha, 2048 taps + 1, 48 kHz, fsym):
// out[m] = sum_k h[k] x[m - 2048 - k], what JFastFir::update returns for SetKernel(points, 4096) -- the operation the reference's
// own test vectors pin (JAERO/tests/jfastfir_tests.cpp:31-58, tests/test_jfastfir_vectors.py).
extern "C" int jaero_debug_prefilter(int device, const double *in_reim, int n, double alpha, double fsym, double *out_reim)
{
    if (!in_reim || !out_reim || n <= 0) return fail(JAERO_EINVAL, "jaero_debug_prefilter: bad arguments");
    int rc = open_device(device);
    if (rc) return rc;
    const std::vector<double> taps = rrc_design(alpha, 2048, 48000.0, fsym);
    if ((int)taps.size() != PRE_K) return fail(JAERO_EINVAL, "prefilter design returned %zu taps", taps.size());
    JGeom g{}; g.nch = 1; g.nchp = 64; g.ngroups = 1;
    JPtrs p{};
    JPre q{};
    int ring = 1;
    while (ring < n + 3 * PRE_L + 64) ring <<= 1;
    q.ring = ring;
    q.cap = n;
    DevMem m;
    double2 *d_cis = nullptr, *dH = nullptr, *dtw = nullptr;
    double *d_taps = nullptr;
    DA(m, q.xring, (size_t)ring * 64);
    DA(m, q.cidx, (size_t)n * 64);
    DA(m, q.out, (size_t)n * 64);
    DA(m, q.hold, 64);
    DA(m, d_cis, 4);
    DA(m, d_taps, PRE_K);
    const double2 one[4] = {{1.0, 0.0}, {1.0, 0.0}, {1.0, 0.0}, {1.0, 0.0}}; // table entry 0 = cis(0): the up-mix multiplies by its conjugate
    HIPCHK(hipMemcpy(d_cis, one, sizeof one, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_taps, taps.data(), sizeof(double) * PRE_K, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy2D(q.xring, sizeof(double2) * 4, in_reim, sizeof(double2), sizeof(double2), (size_t)n, hipMemcpyHostToDevice)); // channel 0 of every slot (PRE_XI)
    p.cis = d_cis; q.taps = d_taps;
    if ((rc = fft4096_tables(m, taps, &dH, &dtw, (const void *)k_pre8400_fft))) return rc;
    q.H = dH; q.tw = dtw;
    launch_pre8400_filter(g, p, q, n, 0LL, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy2D(out_reim, sizeof(double2), q.out, sizeof(double2) * 4, sizeof(double2), (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------------ test hooks: the 8400 bps prefilter stage alone
// (tests/test_gpu_pre8400.py), through stage_pcm / launch_pre8400_stage / launch_pre8400_restart as jaero_write and jaero_set_settings call them.
static int pre8400_hook_enter(jaero_ctx *c, const char *who, int channel, bool poison)
{
    if (!c) return fail(JAERO_EINVAL, "%s: null ctx", who);
    if (c->burst || !c->pre8400) return fail(JAERO_EINVAL, "%s: not an 8400 bps bank", who);
    if (channel < 0 || channel >= c->g.nch) return fail(JAERO_EINVAL, "%s: channel %d outside [0, %d)", who, channel, c->g.nch);
    QUIESCE(c);
    if (poison) c->poisoned = true;
    return 0;
}
extern "C" int jaero_debug_pre8400_write(jaero_ctx *c, const int16_t *pcm, int layout, int nsamples, int stretches)
{
    if (c && c->pre8400 && (!pcm || nsamples <= 0 || nsamples > c->max_write))
        return fail(JAERO_EINVAL, "jaero_debug_pre8400_write: nsamples %d (1 .. max_write_samples %d of host PCM)", nsamples, c->max_write);
    if (layout != JAERO_PCM_CHANNEL_MAJOR && layout != JAERO_PCM_FRAME_MAJOR) return fail(JAERO_EINVAL, "jaero_debug_pre8400_write: bad layout");
    if (stretches != 0 && stretches != 1 && stretches != 8) return fail(JAERO_EINVAL, "jaero_debug_pre8400_write: stretches %d (0 = as jaero_write, 1 or 8)", stretches);
    int rc = pre8400_hook_enter(c, "jaero_debug_pre8400_write", 0, true);
    if (rc) return rc;
    hipStream_t st = c->last_stream;
    const int16_t *frames = nullptr;
    int stride = 0;
    if ((rc = stage_pcm(c, pcm, nsamples, layout, 0, st, &frames, &stride))) return rc;
    if ((rc = launch_pre8400_stage(c, frames, stride, nsamples, stretches ? stretches : pre8400_stretches(c->g, nsamples), st))) return rc;
    c->pre_nprev = nsamples;
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
extern "C" int jaero_debug_pre8400_poke(jaero_ctx *c, int ch, const jaero_pre8400_state *st)
{
    if (!st) return fail(JAERO_EINVAL, "jaero_debug_pre8400_poke: null state");
    if (!(st->ptr >= 0 && st->ptr < (double)JD_WTSIZE) || !(st->step >= 0 && st->step < (double)JD_WTSIZE) || !(fabs(st->fsum) < 1e300) || st->hold < 0)
        return fail(JAERO_EINVAL, "jaero_debug_pre8400_poke: state out of range (ptr and step in [0, %d), fsum finite, hold >= 0)", JD_WTSIZE);
    int rc = pre8400_hook_enter(c, "jaero_debug_pre8400_poke", ch, true);
    if (rc) return rc;
    const size_t nchp = (size_t)c->g.nchp;
    const std::pair<int, double> dv[] = {{S_PRE_PTR, st->ptr}, {S_PRE_STEP, st->step}, {S_PRE_FSUM, st->fsum}};
    for (const auto &[f, v] : dv) HIPCHK(hipMemcpy(c->p.S + (size_t)f * nchp + ch, &v, sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->pre.hold + ch, &st->hold, sizeof(long long), hipMemcpyHostToDevice));
    return 0;
}
extern "C" int jaero_debug_pre8400_peek(jaero_ctx *c, int ch, jaero_pre8400_state *st)
{
    if (!st) return fail(JAERO_EINVAL, "jaero_debug_pre8400_peek: null state");
    int rc = pre8400_hook_enter(c, "jaero_debug_pre8400_peek", ch, false);
    if (rc) return rc;
    const size_t nchp = (size_t)c->g.nchp;
    const std::pair<int, double *> dv[] = {{S_PRE_PTR, &st->ptr}, {S_PRE_STEP, &st->step}, {S_PRE_FSUM, &st->fsum}};
    for (const auto &[f, v] : dv) HIPCHK(hipMemcpy(v, c->p.S + (size_t)f * nchp + ch, sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&st->hold, c->pre.hold + ch, sizeof(long long), hipMemcpyDeviceToHost));
    st->n0 = c->pre_n0; st->nprev = c->pre_nprev; st->ring = c->pre.ring; st->cap = c->pre.cap;
    return 0;
}
extern "C" int jaero_debug_pre8400_restart(jaero_ctx *c, int ch)
{
    int rc = pre8400_hook_enter(c, "jaero_debug_pre8400_restart", ch, true);
    if (rc) return rc;
    if ((rc = launch_pre8400_restart(c, ch, c->last_stream))) return rc;
    QUIESCE(c);
    return 0;
}
extern "C" int jaero_debug_pre8400_read_ring(jaero_ctx *c, int ch, long long first, int n, double *out_reim)
{
    if (!out_reim) return fail(JAERO_EINVAL, "jaero_debug_pre8400_read_ring: null output");
    int rc = pre8400_hook_enter(c, "jaero_debug_pre8400_read_ring", ch, false);
    if (rc) return rc;
    const long long ring = c->pre.ring, oldest = c->pre_n0 > ring ? c->pre_n0 - ring : 0;
    if (n <= 0 || first < oldest || first > c->pre_n0 - n)
        return fail(JAERO_EINVAL, "jaero_debug_pre8400_read_ring: samples [%lld, %lld + %d) are not all among the last %lld of the %lld written", first, first, n, ring, c->pre_n0);
    const int slot = (int)(first & (ring - 1)), n1 = n < (int)(ring - slot) ? n : (int)(ring - slot);
    HIPCHK(hipMemcpy2D(out_reim, sizeof(double2), c->pre.xring + PRE_XI(slot, ch, c->pre.ring), sizeof(double2) * 4, sizeof(double2), (size_t)n1, hipMemcpyDeviceToHost));
    if (n > n1) HIPCHK(hipMemcpy2D(out_reim + 2 * (size_t)n1, sizeof(double2), c->pre.xring + PRE_XI(0, ch, c->pre.ring), sizeof(double2) * 4, sizeof(double2), (size_t)(n - n1), hipMemcpyDeviceToHost));
    return 0;
}

// Test hook: the prefiltered samples of the last write of an 8400 bps bank (cval_prefiltered, oqpskdemodulator.cpp:343-381), channel ch.
extern "C" int jaero_debug_read_prefiltered(jaero_ctx *c, int ch, double *out_reim, int n)
{
    if (!c || !out_reim || !c->pre8400 || ch < 0 || ch >= c->g.nch || n <= 0 || n > c->pre_nprev) return fail(JAERO_EINVAL, "jaero_debug_read_prefiltered: bad arguments");
    QUIESCE(c);
    HIPCHK(hipMemcpy2D(out_reim, sizeof(double2), c->pre.out + JD_G4(0, ch, c->pre.cap), sizeof(double2) * 4, sizeof(double2), (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------------ outputs
extern "C" int jaero_read_softbits(jaero_ctx *c, int ch, int16_t *dst, int cap, int *n)
{
    POISONCHK(c, "jaero_read_softbits", POISON_BANK);
    if (!c) return fail(JAERO_EINVAL, "jaero_read_softbits: null ctx");
    return read_output(c, "jaero_read_softbits", {c->o_soft, c->o_soft_cnt, c->o_soft_cap, sizeof(int16_t)}, ch, dst, cap, n, 1, c->o_nrx);
}

extern "C" int jaero_read_softbits_all(jaero_ctx *c, int16_t *dst, int capc, int *counts)
{
    POISONCHK(c, "jaero_read_softbits_all", POISON_BANK);
    if (!c || !dst || !counts || capc <= 0) return fail(JAERO_EINVAL, "jaero_read_softbits_all: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->last_stream;
    const int nch = c->o_nch, nchp = c->o_nchp;
    const size_t need = (size_t)nch * capc;
    if (need > c->pack_elems)
    {
        const int rc = dalloc(c->mem, &c->d_pack, need, false);
        if (rc) return rc;
        c->pack_elems = need;
    }
    hipLaunchKernelGGL(k_pack_soft, dim3(nch), dim3(256), 0, st, c->o_soft_cnt, c->o_soft, c->o_soft_cap, c->d_pack, capc);
    HIPCHK(hipMemcpyAsync(dst, c->d_pack, need * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    std::vector<int> cnt(nchp), ov(nchp);
    HIPCHK(hipMemcpyAsync(cnt.data(), c->o_soft_cnt, sizeof(int) * nchp, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ov.data(), c->o_overflow, sizeof(int) * nchp, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int rc = 0;
    for (int ch = 0; ch < nch; ch++)
    {
        counts[ch] = cnt[ch] < capc ? cnt[ch] : capc;
        if (cnt[ch] > capc || (ov[ch] & 1)) rc = JAERO_EOVERFLOW;
    }
    if (c->burst)
        return fail(JAERO_ENOTSUP, "jaero_read_softbits_all: burst banks keep a pending (not yet emitted) tail per channel; use jaero_read_softbits");
    HIPCHK(hipMemsetAsync(c->o_soft_cnt, 0, sizeof(int) * nchp, st));
    if (rc)
    {
        HIPCHK(hipMemsetAsync(c->o_overflow, 0, sizeof(int) * nchp, st));
        return fail(rc, "at least one channel produced more soft bits than fit (cap_per_channel=%d or device capacity)", capc);
    }
    return 0;
}

// burst banks: only what the reference would have emitted (groups completed so far) is handed on; the pending tail stays
__global__ void k_burst_emitted(const int *__restrict__ cnt, const int *__restrict__ nrx, int *__restrict__ emitted, int nch)
{
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch < nch) emitted[ch] = cnt[ch] - nrx[ch];
}
// after the emitted part was consumed: move the pending tail to the front of the channel's buffer
__global__ void k_burst_keep_tail(int *__restrict__ cnt, const int *__restrict__ nrx, int16_t *__restrict__ soft, int cap, int nch)
{
    const int ch = blockIdx.x;
    if (ch >= nch) return;
    const int c = cnt[ch], pend = nrx[ch], first = c - pend;
    int16_t *row = soft + (size_t)ch * cap;
    // pend is at most one group (< 64 entries): one wavefront, read everything before writing
    const int t = threadIdx.x;
    int16_t v = 0;
    if (t < pend) v = row[first + t];
    __syncthreads();
    if (t < pend) row[t] = v;
    if (t == 0) cnt[ch] = pend;
}

extern "C" int jaero_softbits_view(jaero_ctx *c, void **dev_softbits, void **dev_counts, int *capacity)
{
    POISONCHK(c, "jaero_softbits_view", POISON_BANK);
    if (!c) return fail(JAERO_EINVAL, "null ctx");
    if (dev_softbits) *dev_softbits = c->o_soft;
    if (c->burst && dev_counts)
    {
        HIPCHK(hipSetDevice(c->device));
        if (!c->d_emitted)
        {
            const int rc = dalloc(c->mem, &c->d_emitted, c->o_nchp, false);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(k_burst_emitted, dim3((c->o_nch + 255) / 256), dim3(256), 0, c->last_stream, c->o_soft_cnt, c->o_nrx, c->d_emitted, c->o_nch);
        *dev_counts = c->d_emitted;
        if (capacity) *capacity = c->o_soft_cap;
        return 0;
    }
    if (dev_counts) *dev_counts = c->o_soft_cnt;
    if (capacity) *capacity = c->o_soft_cap;
    return 0;
}

extern "C" int jaero_discard_softbits(jaero_ctx *c, void *stream)
{
    POISONCHK(c, "jaero_discard_softbits", POISON_BANK);
    if (!c) return fail(JAERO_EINVAL, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    { const int rc = c->order_behind((hipStream_t)stream); if (rc) return rc; }
    if (c->burst)
    {
        // what jaero_softbits_view reported as emitted is gone; the not yet emitted tail of every channel moves to the front
        hipLaunchKernelGGL(k_burst_keep_tail, dim3(c->o_nch), dim3(64), 0, (hipStream_t)stream, c->o_soft_cnt, c->o_nrx, c->o_soft, c->o_soft_cap, c->o_nch);
        HIPCHK(hipGetLastError());
        return 0;
    }
    HIPCHK(hipMemsetAsync(c->o_soft_cnt, 0, sizeof(int) * c->o_nchp, (hipStream_t)stream));
    HIPCHK(hipMemsetAsync(c->o_sym_cnt, 0, sizeof(int) * c->o_nchp, (hipStream_t)stream));
    return 0;
}

extern "C" int jaero_read_status(jaero_ctx *c, int ch, jaero_status *stt)
{
    POISONCHK(c, "jaero_read_status", POISON_BANK);
    if (!c || !stt || ch < 0 || ch >= c->o_nch) return fail(JAERO_EINVAL, "jaero_read_status: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    if (c->burst) hipLaunchKernelGGL(k_status_burst, dim3(1), dim3(64), 0, c->last_stream, c->bg, c->bp, ch, 1, c->d_status);
    else hipLaunchKernelGGL(k_status, dim3(1), dim3(64), 0, c->last_stream, c->g, c->p, ch, 1, c->d_status);
    HIPCHK(hipMemcpyAsync(stt, c->d_status, sizeof(jaero_status), hipMemcpyDeviceToHost, c->last_stream));
    QUIESCE(c);
    return 0;
}

extern "C" int jaero_read_status_log(jaero_ctx *c, int ch, double *rows, int caprows, int *nrows)
{
    POISONCHK(c, "jaero_read_status_log", POISON_BANK);
    if (!c) return fail(JAERO_EINVAL, "jaero_read_status_log: null ctx");
    if (c->burst) return fail(JAERO_ENOTSUP, "burst banks have an event log (jaero_read_events), not a status log");
    return read_output(c, "jaero_read_status_log", {c->p.slog, c->p.I + (size_t)I_LOG_CNT * c->g.nchp, c->g.log_cap, 6 * sizeof(double)}, ch, rows, caprows, nrows, 4);
}
extern "C" int jaero_read_symbols(jaero_ctx *c, int ch, double *rows, int caprows, int *nrows)
{
    POISONCHK(c, "jaero_read_symbols", POISON_BANK);
    if (!c) return fail(JAERO_EINVAL, "jaero_read_symbols: null ctx");
    return read_output(c, "jaero_read_symbols", {c->o_sym, c->o_sym_cnt, c->o_sym_cap, 3 * sizeof(double)}, ch, rows, caprows, nrows, 2);
}
extern "C" int jaero_read_events(jaero_ctx *c, int ch, double *rows, int caprows, int *nrows)
{
    POISONCHK(c, "jaero_read_events", POISON_BANK);
    if (!c) return fail(JAERO_EINVAL, "jaero_read_events: null ctx");
    if (!c->burst) return fail(JAERO_ENOTSUP, "continuous banks have a status log (jaero_read_status_log), not an event log");
    return read_output(c, "jaero_read_events", {c->bp.evlog, c->bp.I + (size_t)BI_EV_CNT * c->bg.nchp, c->bg.ev_cap, 3 * sizeof(double)}, ch, rows, caprows, nrows, 4);
}

// ------------------------------------------------------------------------------------------ Viterbi
// Two layouts of the same decoder: one block per wavefront (k_viterbi: ~57 SIMD cycles per step and block, fills the chip from a few
// thousand blocks) and one block per lane (k_viterbi_lanes: ~12 cycles per step and block, but needs >= 64 blocks per SIMD-wave to
// pay off).  The lane layout wins once the per-wavefront layout has more than ~14 waves queued per SIMD.
#define VL_MIN_BLOCKS 16384
static inline size_t viterbi_hist_bytes(int nblocks) { return (size_t)((nblocks + 63) / 64) * VT_CAP * 64 * sizeof(unsigned long long); }
static int g_viterbi_layout = 0; // test hook jaero_debug_viterbi_layout: 0 = by size (the product behaviour), 1 = wave, 2 = lanes
extern "C" int jaero_debug_viterbi_layout(int mode)
{
    if (mode < 0 || mode > 2) return fail(JAERO_EINVAL, "jaero_debug_viterbi_layout: mode must be 0 (by size), 1 (wave) or 2 (lanes)");
    g_viterbi_layout = mode;
    return 0;
}
static inline bool viterbi_use_lanes(int nblocks, int nsoft, int pad)
{
    if ((nsoft + pad) / 2 < 4 * VT_ORDER) return false;
    if (g_viterbi_layout == 1) return false;
    if (g_viterbi_layout == 2) return true;
    return nblocks >= VL_MIN_BLOCKS;
}
static void viterbi_launch(hipStream_t st, const uint8_t *d_soft, int nsoft, const uint8_t *d_ov, int pad, uint8_t *d_out, int out_stride,
                           int out_start, int out_want, int nblocks, const int *valid, unsigned long long *hist, int tiled = 0, int packed = 0, int force_lanes = 0, int pitch = 0, const int *lens = nullptr,
                           int entry = 0) // entry (jaero_debug_viterbi only): 0 = the lane layout's entry point by size, 1 = k_viterbi_lanes, 2 = k_viterbi_lanes_x2
{
    if (pitch <= 0) pitch = nsoft; // distance between the rows of d_soft (row-major input only)
    if (out_want > nsoft / 2) out_want = nsoft / 2; // a block of nsoft soft bytes yields at most nsoft / 2 bits (Decode_soft, Decode_Continuous' mid(pad + 1, n / 2))
    if (hist && (tiled || force_lanes || viterbi_use_lanes(nblocks, nsoft, pad))) // tiled input / packed output exist only in the lane layout
    {
        const int waves = (nblocks + 63) / 64;
        int ncu = 256;
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0);
        if (entry ? entry == 1 : waves <= ncu * 4) // one wavefront per SIMD is enough: use the entry point that cannot be stacked two to a SIMD
            hipLaunchKernelGGL(k_viterbi_lanes, dim3(waves), dim3(64), 0, st, d_soft, nsoft, d_ov, pad, d_out, out_stride, out_start, out_want, nblocks,
                               valid, hist, tiled, packed, pitch, lens);
        else
            hipLaunchKernelGGL(k_viterbi_lanes_x2, dim3(waves), dim3(64), 0, st, d_soft, nsoft, d_ov, pad, d_out, out_stride, out_start, out_want, nblocks,
                               valid, hist, tiled, packed, pitch, lens);
    }
    else
        hipLaunchKernelGGL(k_viterbi, dim3(nblocks), dim3(64), 0, st, d_soft, nsoft, d_ov, pad, d_out, out_stride, out_start, out_want, nblocks, valid, lens, pitch);
}
static int viterbi_run(int device, const uint8_t *soft, int nblocks, int nsoft, int pad, uint8_t *overlap, uint8_t *bits_out,
                       int out_stride, int out_start, int out_want, int is_device_ptr, hipStream_t st)
{
    int rc = open_device(device);
    if (rc) return rc;
    const uint8_t *d_soft = soft; uint8_t *d_out = bits_out; uint8_t *d_ov = overlap;
    const size_t out_bytes = (size_t)nblocks * out_stride;
    DevMem stage; // host input: staged in device buffers of this call
    if (!is_device_ptr)
    {
        uint8_t *t_soft = nullptr;
        if ((rc = dalloc(stage, &t_soft, (size_t)nblocks * nsoft, false)) || (rc = dalloc(stage, &d_out, out_bytes, false))) return rc;
        HIPCHK(hipMemcpyAsync(t_soft, soft, (size_t)nblocks * nsoft, hipMemcpyHostToDevice, st));
        d_soft = t_soft;
        if (overlap)
        {
            if ((rc = dalloc(stage, &d_ov, (size_t)nblocks * 64, false))) return rc;
            HIPCHK(hipMemcpyAsync(d_ov, overlap, (size_t)nblocks * 64, hipMemcpyHostToDevice, st));
        }
    }
    HIPCHK(hipMemsetAsync(d_out, 0, out_bytes, st));
    void *t_hist = nullptr;
    if (viterbi_use_lanes(nblocks, nsoft, pad)) HIPCHK(hipMallocAsync(&t_hist, viterbi_hist_bytes(nblocks), st));
    viterbi_launch(st, d_soft, nsoft, (const uint8_t *)d_ov, pad, d_out, out_stride, out_start, out_want, nblocks, nullptr, (unsigned long long *)t_hist);
    const hipError_t le = hipGetLastError();
    if (t_hist) HIPCHK(hipFreeAsync(t_hist, st)); // stream-ordered, behind the launch (or in place of it)
    if (le != hipSuccess) return fail(JAERO_EHIP, "launch of the Viterbi decoder failed: %s", hipGetErrorString(le));
    if (!is_device_ptr)
    {
        HIPCHK(hipMemcpyAsync(bits_out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return 0;
}

extern "C" int jaero_viterbi_decode_soft(int device, const uint8_t *soft, int nblocks, int nsoft, uint8_t *bits_out, int is_device_ptr, void *stream)
{
    if (!soft || !bits_out || nblocks <= 0 || nsoft < 4 * VT_ORDER || (nsoft & 1)) return fail(JAERO_EINVAL, "jaero_viterbi_decode_soft: bad arguments");
    return viterbi_run(device, soft, nblocks, nsoft, 0, nullptr, bits_out, nsoft / 2, 0, nsoft / 2, is_device_ptr, (hipStream_t)stream);
}

__global__ void k_viterbi_overlap_update(const uint8_t *__restrict__ soft, int nsoft, uint8_t *__restrict__ overlap, int nstreams,
                                         const int *__restrict__ valid = nullptr, int tiled = 0, int pitch = 0)
{
    // soft_bits_overlap_buffer_uchar = soft_bits_in.right(62); resize(62)  (jconvolutionalcodec.cpp:197-198)
    const int b = blockIdx.x;
    if (b >= nstreams) return;
    if (valid && !valid[b]) return;
    const int k = 62;
    const int t = threadIdx.x;
    if (t < k)
    {
        uint8_t v = 0;
        // byte q of row b: row-major, or the tiled layout of k_viterbi_lanes ([wavefront][16-byte group][lane][16])
        auto at = [&](int q) -> uint8_t {
            return tiled ? soft[(size_t)(b >> 6) * 64 * nsoft + ((size_t)(q >> 4) * 64 + (b & 63)) * 16 + (q & 15)] : soft[(size_t)b * (pitch > 0 ? pitch : nsoft) + q];
        };
        if (nsoft >= k) v = at(nsoft - k + t);
        else if (t < nsoft) v = at(t);
        overlap[(size_t)b * 64 + t] = v;
    }
    if (t == 62) overlap[(size_t)b * 64 + 62] = (uint8_t)k;
}

extern "C" int jaero_viterbi_continuous(int device, const uint8_t *soft, int nstreams, int nsoft, int paddinglength, uint8_t *overlap_state,
                                        uint8_t *bits_out, int *nbits_out, int is_device_ptr, void *stream)
{
    if (!soft || !bits_out || !overlap_state || nstreams <= 0 || nsoft < 64 || (nsoft & 1) || paddinglength < 0 || (paddinglength & 1))
        return fail(JAERO_EINVAL, "jaero_viterbi_continuous: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int want = nsoft / 2;
    // host needs each stream's overlap length to report nbits (first call of a stream returns fewer bits)
    std::vector<uint8_t> hov;
    const uint8_t *ovh = overlap_state;
    if (is_device_ptr)
    {
        hov.resize((size_t)nstreams * 64);
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipMemcpyAsync(hov.data(), overlap_state, hov.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ovh = hov.data();
    }
    if (nbits_out)
        for (int b = 0; b < nstreams; b++)
        {
            const int total = (int)ovh[(size_t)b * 64 + 62] + nsoft + paddinglength;
            int nb = total / 2 - (paddinglength + 1);
            if (nb > want) nb = want;
            if (nb < 0) nb = 0;
            nbits_out[b] = nb;
        }
    int rc = viterbi_run(device, soft, nstreams, nsoft, paddinglength, overlap_state, bits_out, want, paddinglength + 1, want, is_device_ptr, st);
    if (rc) return rc;
    if (is_device_ptr)
    {
        hipLaunchKernelGGL(k_viterbi_overlap_update, dim3(nstreams), dim3(64), 0, st, soft, nsoft, overlap_state, nstreams);
        HIPCHK(hipGetLastError());
    }
    else
    {
        for (int b = 0; b < nstreams; b++)
        {
            uint8_t *ov = overlap_state + (size_t)b * 64;
            memset(ov, 0, 64);
            memcpy(ov, soft + (size_t)b * nsoft + nsoft - 62, 62);
            ov[62] = 62;
        }
    }
    return 0;
}

// Test hook: ONE viterbi_launch (and, on request, one k_viterbi_overlap_update) with every parameter of the launch in the caller's hands.
// The output buffer goes to the device as the caller filled it and comes back whole: what the kernels did not write still holds the caller's bytes.
extern "C" int jaero_debug_viterbi(int device, const jaero_viterbi_probe *q)
{
#define VPFAIL(...) return fail(JAERO_EINVAL, "jaero_debug_viterbi: " __VA_ARGS__)
    if (!q || !q->soft || !q->out) VPFAIL("null probe, soft or out");
    if (q->nblocks < 1 || q->nblocks > (1 << 20) || q->nsoft < 4 * VT_ORDER || q->nsoft > (1 << 20)) VPFAIL("nblocks %d (1 .. 2^20), nsoft %d (%d .. 2^20)", q->nblocks, q->nsoft, 4 * VT_ORDER);
    if (q->layout < 0 || q->layout > 3) VPFAIL("layout %d: 0 = by size, 1 = wave, 2 = lanes (1, 1), 3 = lanes x2", q->layout);
    if (q->pad < 0 || (q->pad & 1) || q->pad > 4096) VPFAIL("pad %d (even, 0 .. 4096)", q->pad);
    if (q->out_start < 0 || q->out_want < 1) VPFAIL("out_start %d (>= 0), out_want %d (>= 1)", q->out_start, q->out_want);
    if (q->soft_misalign < 0 || q->soft_misalign > 15) VPFAIL("soft_misalign %d (0 .. 15)", q->soft_misalign);
    const int tiled = q->tiled != 0, packed = q->packed != 0;
    const int pitch = q->pitch > 0 ? q->pitch : q->nsoft;
    if (pitch < q->nsoft) VPFAIL("pitch %d below nsoft %d", pitch, q->nsoft);
    const int out_rows = q->out_rows > 0 ? q->out_rows : q->nblocks;
    if (out_rows < q->nblocks) VPFAIL("out_rows %d below nblocks %d", out_rows, q->nblocks);
    if (q->update_overlap && !q->overlap) VPFAIL("update_overlap without an overlap buffer");
    int minlen = q->nsoft;
    if (q->lens)
        for (int b = 0; b < q->nblocks; b++)
        {
            const int l = q->lens[b];
            if (l < 4 * VT_ORDER || l > q->nsoft || (l & 1)) VPFAIL("lens[%d] = %d (even, %d .. nsoft %d)", b, l, 4 * VT_ORDER, q->nsoft);
            if (l < minlen) minlen = l;
        }
    if (q->overlap)
        for (int b = 0; b < q->nblocks; b++)
            if (q->overlap[(size_t)b * 64 + 62] > 62) VPFAIL("overlap[%d][62] = %d: an overlap is at most 62 bytes", b, (int)q->overlap[(size_t)b * 64 + 62]);
    // the layout the launch will take
    const bool lanes = q->layout >= 2 || (q->layout == 0 && (tiled || viterbi_use_lanes(q->nblocks, q->nsoft, q->pad)));
    if (!lanes && (tiled || packed)) VPFAIL("tiled input and packed output exist only in the lane layout");
    if (tiled && (q->nsoft % 16 != 0 || q->lens || q->pitch > 0 || q->soft_misalign)) VPFAIL("tiled input: nsoft %d a multiple of 16, no lens, pitch or misalignment", q->nsoft);
    if (lanes && (minlen + q->pad) / 2 < 4 * VT_ORDER) VPFAIL("the lane layout needs %d steps, the shortest row has %d", 4 * VT_ORDER, (minlen + q->pad) / 2);
    if (packed ? (q->out_stride % 4 != 0 || q->out_stride < (q->out_want + 31) / 32 * 4) : q->out_stride < q->out_want)
        VPFAIL("out_stride %d too small for a window of %d %s (packed rows: whole 32-bit words)", q->out_stride, q->out_want, packed ? "bits" : "bytes");
#undef VPFAIL
    int rc = open_device(device);
    if (rc) return rc;
    const int waves = (q->nblocks + 63) / 64;
    const size_t soft_bytes = tiled ? (size_t)waves * 64 * q->nsoft : (size_t)q->nblocks * pitch;
    const size_t out_bytes = (size_t)out_rows * q->out_stride;
    DevMem m;
    uint8_t *d_soft = nullptr, *d_out = nullptr, *d_ov = nullptr;
    int *d_valid = nullptr, *d_lens = nullptr;
    unsigned long long *d_hist = nullptr;
    DA(m, d_soft, soft_bytes + q->soft_misalign);
    const size_t guard = 256; // bytes in front of and behind the device copy of out: a store there is reported, not lost
    DA(m, d_out, out_bytes + 2 * guard);
    HIPCHK(hipMemset(d_out, 0xC3, out_bytes + 2 * guard));
    d_out += guard;
    d_soft += q->soft_misalign;
    HIPCHK(hipMemcpy(d_soft, q->soft, soft_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_out, q->out, out_bytes, hipMemcpyHostToDevice)); // not cleared: the caller's bytes show what was not written
    if (q->overlap) { DA(m, d_ov, (size_t)q->nblocks * 64); HIPCHK(hipMemcpy(d_ov, q->overlap, (size_t)q->nblocks * 64, hipMemcpyHostToDevice)); }
    if (q->valid) { DA(m, d_valid, q->nblocks); HIPCHK(hipMemcpy(d_valid, q->valid, sizeof(int) * (size_t)q->nblocks, hipMemcpyHostToDevice)); }
    if (q->lens) { DA(m, d_lens, q->nblocks); HIPCHK(hipMemcpy(d_lens, q->lens, sizeof(int) * (size_t)q->nblocks, hipMemcpyHostToDevice)); }
    if (lanes) DA(m, d_hist, viterbi_hist_bytes(q->nblocks) / sizeof(unsigned long long));
    // layout 1: no history scratch = the wave kernel whatever jaero_debug_viterbi_layout says; 2, 3: the lane layout forced, with its entry point
    viterbi_launch(0, d_soft, q->nsoft, d_ov, q->pad, d_out, q->out_stride, q->out_start, q->out_want, q->nblocks, d_valid, q->layout == 1 ? nullptr : d_hist, tiled, packed,
                   q->layout >= 2, q->pitch, d_lens, q->layout >= 2 ? q->layout - 1 : 0);
    LAUNCHCHK("the Viterbi decoder");
    if (q->update_overlap)
    {
        hipLaunchKernelGGL(k_viterbi_overlap_update, dim3(q->nblocks), dim3(64), 0, 0, (const uint8_t *)d_soft, q->nsoft, d_ov, q->nblocks, (const int *)d_valid, tiled, q->pitch);
        LAUNCHCHK("k_viterbi_overlap_update");
    }
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(q->out, d_out, out_bytes, hipMemcpyDeviceToHost));
    uint8_t g[2 * guard];
    HIPCHK(hipMemcpy(g, d_out - guard, guard, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(g + guard, d_out + out_bytes, guard, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < 2 * guard; i++)
        if (g[i] != 0xC3) return fail(JAERO_EHIP, "jaero_debug_viterbi: the decoder wrote %s the output buffer (guard byte %zu)", i < guard ? "in front of" : "behind", i % guard);
    if (q->overlap) HIPCHK(hipMemcpy(q->overlap, d_ov, (size_t)q->nblocks * 64, hipMemcpyDeviceToHost));
    return 0;
}

#include "aerol_host.h"
#include "ingest_host.h"
#include "edge_host.h"
#include "chan_host.h"
#include "rate_host.h"

// ------------------------------------------------------------------------------------------ one-call reads of every channel
// (here, behind aerol_host.h: the sweep's kernels stay where they were in the code object, behind the banks' own)
// jaero_read_all: one output class of every channel (sweep_host.h, k_aerol_sweep.h).  The RowBufs are the per-channel readers'; a burst
// bank's soft bits keep their pending tail (o_nrx).  The scratch (jaero_ctx::sweep, d_status_all) is allocated by the first call and goes with
// the bank object at a rate change (swap_in): the bank that takes its place allocates afresh.
extern "C" int jaero_read_all(jaero_ctx *c, int what, void *rows, int caprows, int *offsets, int *nchannels_taken, long long *rows_pending,
                              unsigned char *overflowed)
{
    const char *who = "jaero_read_all";
    if (what < JAERO_BANK_SOFTBITS || what > JAERO_BANK_SYMBOLS) return fail(JAERO_EINVAL, "%s: what = %d is none of JAERO_BANK_SOFTBITS / STATUS_LOG / EVENTS / SYMBOLS", who, what);
    if (caprows < 0) return fail(JAERO_EINVAL, "%s: caprows < 0", who);
    if (!offsets || !nchannels_taken) return fail(JAERO_EINVAL, "%s: null offsets / nchannels_taken", who);
    if (!rows && caprows > 0) return fail(JAERO_EINVAL, "%s: null rows with caprows > 0", who);
    if (!c) return fail(JAERO_EINVAL, "%s: null ctx", who);
    POISONCHK(c, "jaero_read_all", POISON_BANK);
    RowBuf b{};
    int ovbit = 0;
    const int *pending = nullptr;
    switch (what)
    {
    case JAERO_BANK_SOFTBITS:
        b = RowBuf{c->o_soft, c->o_soft_cnt, c->o_soft_cap, sizeof(int16_t)};
        ovbit = 1;
        pending = c->burst ? c->o_nrx : nullptr;
        break;
    case JAERO_BANK_STATUS_LOG:
        if (c->burst) return fail(JAERO_ENOTSUP, "%s: burst banks have an event log (JAERO_BANK_EVENTS), not a status log", who);
        b = RowBuf{c->p.slog, c->p.I + (size_t)I_LOG_CNT * c->g.nchp, c->g.log_cap, 6 * sizeof(double)};
        ovbit = 4;
        break;
    case JAERO_BANK_EVENTS:
        if (!c->burst) return fail(JAERO_ENOTSUP, "%s: continuous banks have a status log (JAERO_BANK_STATUS_LOG), not an event log", who);
        b = RowBuf{c->bp.evlog, c->bp.I + (size_t)BI_EV_CNT * c->bg.nchp, c->bg.ev_cap, 3 * sizeof(double)};
        ovbit = 4;
        break;
    default:
        b = RowBuf{c->o_sym, c->o_sym_cnt, c->o_sym_cap, 3 * sizeof(double)};
        ovbit = 2;
        break;
    }
    if (!b.base || !b.cnt) return fail(JAERO_EINVAL, "%s: this output was not enabled at create (or does not exist for this kind)", who);
    return sweep_log({who, c->sweep, c->device, c->last_stream, c->mem, c->timer, 5, c->o_nch}, b, c->o_overflow, ovbit, pending, rows, caprows, offsets,
                     nchannels_taken, rows_pending, overflowed);
}

// every channel's jaero_read_status in one launch, one copy and one synchronisation
extern "C" int jaero_read_status_all(jaero_ctx *c, jaero_status *stt)
{
    if (!c || !stt) return fail(JAERO_EINVAL, "jaero_read_status_all: bad arguments");
    POISONCHK(c, "jaero_read_status_all", POISON_BANK);
    HIPCHK(hipSetDevice(c->device));
    const int nch = c->o_nch;
    if (!c->d_status_all)
    {
        const int rc = dalloc(c->mem, &c->d_status_all, nch, false);
        if (rc) return rc;
    }
    hipStream_t st = c->last_stream;
    const int pi = c->timer.begin(5, st);
    if (c->burst) hipLaunchKernelGGL(k_status_burst, dim3((nch + 255) / 256), dim3(256), 0, st, c->bg, c->bp, 0, nch, c->d_status_all);
    else hipLaunchKernelGGL(k_status, dim3((nch + 255) / 256), dim3(256), 0, st, c->g, c->p, 0, nch, c->d_status_all);
    c->timer.end(pi, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(stt, c->d_status_all, sizeof(jaero_status) * (size_t)nch, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// test hook: device bytes jaero_read_all / jaero_read_status_all have allocated for the bank so far
extern "C" long long jaero_debug_read_all_bytes(const jaero_ctx *c)
{
    if (!c) return -1;
    return c->sweep.bytes() + (c->d_status_all ? (long long)sizeof(jaero_status) * c->o_nch : 0);
}

// test hook: per channel, the soft bits held and (burst banks) how many of them are not yet emitted
extern "C" int jaero_debug_softbit_counts(jaero_ctx *c, int *cnt, int *pending)
{
    if (!c || !cnt || !pending) return fail(JAERO_EINVAL, "jaero_debug_softbit_counts: bad arguments");
    POISONCHK(c, "jaero_debug_softbit_counts", POISON_BANK);
    QUIESCE(c);
    const size_t n = sizeof(int) * (size_t)c->o_nch;
    HIPCHK(hipMemcpy(cnt, c->o_soft_cnt, n, hipMemcpyDeviceToHost));
    if (c->burst && c->o_nrx) HIPCHK(hipMemcpy(pending, c->o_nrx, n, hipMemcpyDeviceToHost));
    else memset(pending, 0, n);
    return 0;
}

