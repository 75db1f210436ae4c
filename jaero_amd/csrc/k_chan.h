// k_chan.h -- the wideband I/Q channeliser in front of the demodulator banks: a fast-convolution (overlap-save) filter bank, DESIGN 18.
//
// No counterpart in the reference (it only has the receiving end of per-channel audio, zmq_audioreceiver.cpp:40-79); the definition is
// include/jaero_hip.h's, and tests/chan_oracle.py implements it literally in numpy.  Fixed geometry: N = 16384-point forward transform every
// Hp = N / 2 input samples, shared by all channels (k_chan_fwd); per channel and block the M = N / D bins around the channel's nearest grid
// frequency times the prototype's response, an M-point inverse transform of which the second half is kept (overlap-save), the sign that
// makes the bin shift continuous in absolute time, the rotation to the audio offset by an integer phase, gain, rint, clamp (k_chan_synth).
//
// The M-point transform: M = R1 x R2, T = R2 threads per (channel, block) item, all inside one wavefront.
//   n = R2 n1 + n2        r = k1 + R1 k2        (n1, k1 < R1;  n2, k2 < R2)
//   pass 1 (thread n2): FFT_R1 over n1, x W_M^(n2 k1)       exchange through LDS, a plane at a time: L = k1 (R2 + 1) + n2
//   pass 2 (thread k1, h): FFT over n2 -> k2; only k2 >= R2 / 2 (r >= M / 2) is kept, what leads to the other outputs is dead code
//   256 = 16 x 16 (T = 16), 1024 = 32 x 32 (T = 32): thread k1 does the R2-point FFT.  512 = 16 x 32 (T = 32): the 32-point FFT of row k1
//   is split over two threads by one decimation-in-frequency step: thread (k1, h) forms (a[n] + (-1)^h a[n + 16]) W_32^(h n) and its FFT16
//   gives k2 = 2 j + h -- sign and twiddle are per-thread VALUES, so both halves run the same instructions.
//   D is the TOTAL decimation from the capture to the output, whatever the output rate is called (48, 24 or 12 kHz).  The two small shapes
//   mirror two of the above with 8-point transforms: 64 = 8 x 8 (T = 8) is the 256 case, 128 = 8 x 16 (T = 16) the 512 case with
//   W_16^(h n) in the split step.  Their threads hold 4 outputs each and store them as one 8-byte word.
// The inverse transform is the forward one on swapped planes.  Index maps and bank behaviour: tests/test_chan_fft_model.py,
// tests/test_chan_rates_fft_model.py (the two small shapes).
#pragma once
#include "wg_fft.h" // wg_fft14_e32, regfft<>, regfft32_seq, c4_twiddle16

#define CHAN_N 16384
#define CHAN_HP 8192

struct ChanParam // one channel, from (tune, audio, gain) on the host (chan_host.h)
{
    int b;          // nearest bin of the tuning word: (t + 2^17) >> 18
    unsigned w;     // phase word per output sample: audio - rho * D  (mod 2^32)
    double gain;
};

// ------------------------------------------------------------------------------------------ forward transform
// One workgroup per block of the write: window j = in[j * Hp .. j * Hp + N) of the history buffer (previous hop, the partial hop left by
// ragged writes, the new samples; interleaved int16 I, Q read as one dword) -> fp64 -> wg_fft14_e32 -> spec[j][N].
__global__ __launch_bounds__(C2_THREADS) void k_chan_fwd(const int *__restrict__ in, double2 *__restrict__ spec, const double2 *__restrict__ tw)
{
    extern __shared__ __attribute__((aligned(16))) double xch[];
    const int t = threadIdx.x;
    const int *__restrict__ src = in + (size_t)blockIdx.x * CHAN_HP;
    double2 *__restrict__ dst = spec + (size_t)blockIdx.x * CHAN_N;
    CV<32> d;
#pragma unroll
    for (int s = 0; s < 32; s++)
    {
        const int v = src[s * C2_THREADS + t];
        d.r[s] = (double)(short)(v & 0xffff);
        d.i[s] = (double)(v >> 16);
    }
    wg_fft14_e32(d, xch, tw, t);
#pragma unroll
    for (int s = 0; s < 32; s++) dst[s * C2_THREADS + t] = make_double2(d.r[s], d.i[s]);
}

// ------------------------------------------------------------------------------------------ per-channel synthesis
template <int D>
struct ChanShape
{
    static constexpr int M = CHAN_N / D, MO = M / 2;
    static constexpr int R1 = M == 1024 ? 32 : M >= 256 ? 16 : 8;             // pass 1: points per thread
    static constexpr int R2 = M == 64 ? 8 : (M == 256 || M == 128) ? 16 : 32; // = T, threads per item
    static constexpr int P2 = M == 1024 ? 32 : M >= 256 ? 16 : 8;             // pass 2: points per thread's FFT
    static constexpr int SPLIT = R2 / P2;              // 2: a row's FFT_R2 shared by two threads
    static constexpr int T = R2;
    static constexpr int ITEMS = M == 1024 ? 4 : 256 / T; // (channel, block) items per workgroup
    static constexpr int THREADS = ITEMS * T;          // 128 (M = 1024), else 256
    static constexpr int ROW = R2 + 1;                 // odd row stride of the exchange: 16 lanes that differ in k1 hit 16 bank pairs
    static constexpr int XCH = R1 * ROW;               // doubles per item
    static constexpr int OUTS = MO / T;                // int16 each thread stores: 16 (M = 1024), 8 (512, 256), 4 (128, 64)
};

// exchange address of (k1, n2)
template <int D> __device__ __forceinline__ constexpr int chan_xaddr(int k1, int n2) { return k1 * ChanShape<D>::ROW + n2; }

// v[k] *= step^k (k < 32), the powers by products of depth <= 6 as c4_twiddle16
__device__ __forceinline__ void chan_twiddle32(CV<32> &v, const double2 step)
{
#pragma clang fp contract(fast)
    double2 B[4], A[8];
    twiddle_powers<32>(make_double2(1.0, 0.0), step, B, A);
#pragma unroll
    for (int k = 1; k < 32; k++)
    {
        const double2 w = (k < 4) ? B[k & 3] : cmul2(A[k >> 2], B[k & 3]);
        const double r = v.r[k] * w.x - v.i[k] * w.y, i = v.r[k] * w.y + v.i[k] * w.x;
        v.r[k] = r; v.i[k] = i;
    }
}

// v[k] *= step^k (k < 8)
__device__ __forceinline__ void chan_twiddle8(CV<8> &v, const double2 step)
{
#pragma clang fp contract(fast)
    double2 w[8];
    w[1] = step; w[2] = cmul2(step, step); w[3] = cmul2(w[2], step); w[4] = cmul2(w[2], w[2]);
    w[5] = cmul2(w[4], step); w[6] = cmul2(w[4], w[2]); w[7] = cmul2(w[4], w[3]);
#pragma unroll
    for (int k = 1; k < 8; k++)
    {
        const double r = v.r[k] * w[k].x - v.i[k] * w[k].y, i = v.r[k] * w[k].y + v.i[k] * w[k].x;
        v.r[k] = r; v.i[k] = i;
    }
}

template <int L> __device__ __forceinline__ void chan_twiddle(CV<L> &v, const double2 step)
{
    if constexpr (L == 32) chan_twiddle32(v, step);
    else if constexpr (L == 16) c4_twiddle16(v, step);
    else chan_twiddle8(v, step);
}

template <int L> __device__ __forceinline__ void chan_fft(CV<L> &in, CV<L> &out)
{
    if constexpr (L == 32) regfft32_seq(in, out);
    else regfft<L>(in, out);
}

// spec: [nblk][N] of this write; gm: [M] the prototype's response at q = k (k < M / 2), k - M (else), already / N; twm: W_M^k, k < 32;
// pcm: [nch][nblk * MO]; p0: absolute index of the write's first block.
template <int D>
__global__ __launch_bounds__(ChanShape<D>::THREADS) void k_chan_synth(const double2 *__restrict__ spec, const double2 *__restrict__ gm,
                                                                      const double2 *__restrict__ twm, const ChanParam *__restrict__ par,
                                                                      int16_t *__restrict__ pcm, int nch, int nblk, long long p0)
{
#pragma clang fp contract(fast)
    using S = ChanShape<D>;
    constexpr int M = S::M, MO = S::MO, R1 = S::R1, R2 = S::R2, P2 = S::P2, T = S::T;
    __shared__ __attribute__((aligned(16))) double xch_all[S::ITEMS * S::XCH];
    const int u = threadIdx.x % T, li = threadIdx.x / T;
    double *xch = xch_all + li * S::XCH;
    const long long nitems = (long long)nch * nblk;
    const long long item_raw = (long long)blockIdx.x * S::ITEMS + li;
    const bool live = item_raw < nitems;
    const long long item = live ? item_raw : nitems - 1; // a workgroup's spare lanes redo the last item and store nothing: every barrier is met
    const int j = (int)(item / nch), c = (int)(item - (long long)j * nch); // block-major: a block's spectrum stays in L2 for all channels
    const ChanParam cp = par[c];
    const double2 *__restrict__ X = spec + (size_t)j * CHAN_N;

    // ---- gather + pass 1: thread n2 = u holds k = R2 n1 + u ----
    CV<R1> a, A;
#pragma unroll
    for (int n1 = 0; n1 < R1; n1++)
    {
        const int k = R2 * n1 + u;
        const int q = k < M / 2 ? k : k - M;
        const double2 x = X[(cp.b + q) & (CHAN_N - 1)], g = gm[k];
        // Y = X G; the inverse transform is the forward one of the swapped planes
        a.i[n1] = x.x * g.x - x.y * g.y;
        a.r[n1] = x.x * g.y + x.y * g.x;
    }
    chan_fft<R1>(a, A);
    chan_twiddle<R1>(A, twm[u]); // W_M^n2
    // ---- exchange (a plane at a time) + the split's radix-2 step ----
    const int k1 = u % R1, h = u / R1; // h = 0 unless SPLIT == 2
    CV<P2> e, E;
    const double sg = h ? -1.0 : 1.0;
#pragma unroll
    for (int k = 0; k < R1; k++) xch[chan_xaddr<D>(k, u)] = A.r[k];
    jd_lds_barrier();
#pragma unroll
    for (int n = 0; n < P2; n++)
    {
        if constexpr (S::SPLIT == 2) e.r[n] = xch[chan_xaddr<D>(k1, n)] + sg * xch[chan_xaddr<D>(k1, n + P2)];
        else e.r[n] = xch[chan_xaddr<D>(k1, n)];
    }
    jd_lds_barrier();
#pragma unroll
    for (int k = 0; k < R1; k++) xch[chan_xaddr<D>(k, u)] = A.i[k];
    jd_lds_barrier();
#pragma unroll
    for (int n = 0; n < P2; n++)
    {
        if constexpr (S::SPLIT == 2) e.i[n] = xch[chan_xaddr<D>(k1, n)] + sg * xch[chan_xaddr<D>(k1, n + P2)];
        else e.i[n] = xch[chan_xaddr<D>(k1, n)];
    }
    if constexpr (S::SPLIT == 2) chan_twiddle<P2>(e, h ? make_double2(jd_w64r(64 / R2), jd_w64i(64 / R2)) : make_double2(1.0, 0.0)); // W_R2^(h n)
    // ---- pass 2: only the outputs with k2 >= R2 / 2 are used below ----
    chan_fft<P2>(e, E);

    // ---- sign, rotation to the audio offset, gain, rint, clamp; through LDS so that every thread stores one contiguous run ----
    jd_lds_barrier(); // the exchange buffer is free
    int16_t *stage = (int16_t *)xch;
    const long long p = p0 + j;
    const double sgn = ((cp.b & 1) && ((p + 1) & 1)) ? -cp.gain : cp.gain; // (-1)^(b (p - 1)) g
    const unsigned m0 = (unsigned)((unsigned long long)p * (unsigned)MO);  // m mod 2^32 of the block's first output
#pragma unroll
    for (int jj = 0; jj < P2 / 2; jj++)
    {
        const int k2 = S::SPLIT == 2 ? 2 * (jj + P2 / 2) + h : jj + P2 / 2; // >= R2 / 2
        const int ml = k1 + R1 * (k2 - R2 / 2);                             // r - MO
        const int s = jj + P2 / 2;
        const double vr = E.i[s], vi = E.r[s]; // swapped back
        const unsigned ph = cp.w * (m0 + (unsigned)ml);
        double sn, cs;
        sincospi((double)(int)ph * (1.0 / 2147483648.0), &sn, &cs); // 2 pi ph / 2^32, ph as a signed word: (-pi, pi]
        double y = rint(sgn * (vr * cs - vi * sn));
        y = fmin(fmax(y, -32768.0), 32767.0);
        stage[ml] = (int16_t)(int)y;
    }
    jd_lds_barrier();
    if (live)
    {
        if constexpr (S::OUTS % 8 == 0)
        {
            typedef int chan_v4 __attribute__((ext_vector_type(4)));
            const chan_v4 *sv = (const chan_v4 *)stage;
            chan_v4 *__restrict__ dst = (chan_v4 *)(pcm + ((size_t)c * nblk + j) * MO);
#pragma unroll
            for (int v = 0; v < S::OUTS / 8; v++) dst[v * T + u] = sv[v * T + u];
        }
        else // OUTS == 4: the item's Mo samples are T 8-byte words, one per lane
        {
            static_assert(S::OUTS == 4, "a thread's outputs are whole 16-byte words or one 8-byte word");
            typedef int chan_v2 __attribute__((ext_vector_type(2)));
            const chan_v2 *sv = (const chan_v2 *)stage;
            chan_v2 *__restrict__ dst = (chan_v2 *)(pcm + ((size_t)c * nblk + j) * MO);
            dst[u] = sv[u];
        }
    }
}

// ------------------------------------------------------------------------------------------ survey (jaero_survey_*, DESIGN 18 "Survey")
// Two running sums over the forward transforms k_chan_fwd has just left in spec, launched behind k_chan_synth when enabled.  Both are
// independent of how the writes were cut: a block's term is formed by the same instructions whatever the launch shape, and a sum takes its
// terms strictly in block order (one owner per sum, no atomics).  The library is built with -ffp-contract=off and nothing here turns
// contraction on: every product and sum below rounds once, as the numpy definition's (tests/chan_survey_oracle.py).

// Capture spectrum: S[k] += |H_p[k]|^2, H_p[k] = X_p[k] / 2 - (X_p[k - 1] + X_p[k + 1]) / 4 (indices mod N): the Hann window applied in the
// frequency domain.  Thread k owns bin k over the write's blocks in order; one load and one store of S[k] per write.  The neighbours are
// plain loads: a wavefront's three loads cover bins k0 - 1 .. k0 + 64, so the outer two ask for the lines the centre load asks for, and
// the kernel moves 256 KB per block whatever is done here.  One wavefront per workgroup, 256 workgroups: with three loads in flight per
// thread and block the walk over the blocks is bound by latency, and this spreads it over every CU.  Neither choice has been measured
// against its alternative (neighbours by shuffle, wider workgroups); the whole kernel is timed in DESIGN 18.
#define CHAN_PSD_THREADS 64
// SUM: S[k] += |H_p[k]|^2 (the survey's spectrum).  PEAK: P[k] = max(P[k], |H_p[k]|^2) (the activity's peak-hold spectrum, jaero_activity_*):
// the same term, formed once, so that S and P of one block are the same bits.  Either or both in one pass over the three loads; a pointer
// whose part is off is never touched.  <true, false> must stay the code of a kernel that only sums (profiles/chan_activity_isa.md).
template <bool SUM, bool PEAK>
__global__ __launch_bounds__(CHAN_PSD_THREADS) void k_chan_psd(const double2 *__restrict__ spec, double *__restrict__ S, int nblk,
                                                               double *__restrict__ P)
{
    static_assert(SUM || PEAK, "a launch that keeps nothing");
    const int k = blockIdx.x * CHAN_PSD_THREADS + threadIdx.x; // the grid is N / CHAN_PSD_THREADS workgroups: k < N
    const int km = (k - 1) & (CHAN_N - 1), kp = (k + 1) & (CHAN_N - 1);
    double s = 0.0, pk = 0.0;
    if constexpr (SUM) s = S[k];
    if constexpr (PEAK) pk = P[k];
    for (int j = 0; j < nblk; j++)
    {
        const double2 *__restrict__ X = spec + (size_t)j * CHAN_N;
        const double2 a = X[km], x = X[k], b = X[kp];
        const double hr = 0.5 * x.x - 0.25 * (a.x + b.x), hi = 0.5 * x.y - 0.25 * (a.y + b.y);
        const double v = hr * hr + hi * hi;
        if constexpr (SUM) s += v;
        if constexpr (PEAK) pk = v > pk ? v : pk;
    }
    if constexpr (SUM) S[k] = s;
    if constexpr (PEAK) P[k] = pk;
}

// Per-channel level: E[c] += sum_q |X_p[(b + q) mod N]|^2 g2[q + M / 2], -M/2 <= q < M/2, g2 = |G[q mod N]|^2 / N^2 (built at enable from
// the response k_chan_synth multiplies by), for the write's blocks in order.  One channel per group of T = 16 lanes: lane u takes the bins
// q = -M/2 + u + 16 i in ascending i (a load instruction of the group reads 256 contiguous bytes of the bin run, which may wrap at N as
// k_chan_synth's), one accumulator per lane, then a 4-step xor butterfly inside the group (every lane ends with the same sum: the shape is
// fixed), and lane 0 adds the block's sum to the running one it loaded once and stores once.  T = 16 for every M: 16 channels per
// workgroup fill the chip from 4096 channels on, and M / 16 = 4 .. 64 independent 16-byte loads per lane and block hide the L2 latency.
// The table sits in LDS (M doubles).  Spare groups of the last workgroup redo the last channel and store nothing.
//
// ACT: the activity's block statistics (jaero_activity_*) of the same block sums e_{c,p} = acc, so that levels + statistics walk spec once.
// Behind the butterfly every lane of the group holds acc, so nothing is exchanged: lane 0 keeps emax / emin / when over the write's
// blocks in registers (one load and one store of each per write), and the 64-bin histogram lives in the group's registers too -- lane u
// counts the bins u, u + 16, u + 32, u + 48 with four compares per block and adds its four counts to its own words of the channel's row
// once per write.  One owner per word, plain loads and stores, integers: no atomics, and the result is independent of how the writes were
// cut.  when[c] < 0 says that the channel has no block yet (emax / emin are then not read).  <D, true, false> must stay the code of a
// kernel that only sums the levels (profiles/chan_activity_isa.md).
#define CHAN_LVL_T 16
#define CHAN_LVL_THREADS 256
#define CHAN_ACT_BINS 64
struct ChanAct // the block statistics' state, one entry (one row of hist) per channel
{
    double *emax, *emin;   // [nch]
    long long *when;       // [nch]: absolute block index of emax, -1 before the first block
    unsigned *hist;        // [nch][CHAN_ACT_BINS]
};

// bin(e) = min(63, max(0, ilogb(e) + 32)), bin(0) = 0: from the exponent field (0 and the subnormals have field 0: bin 0)
__device__ __forceinline__ int chan_act_bin(double e)
{
    const int ex = (int)((unsigned long long)__double_as_longlong(e) >> 52 & 0x7ff) - 1023 + 32;
    return ex < 0 ? 0 : ex > CHAN_ACT_BINS - 1 ? CHAN_ACT_BINS - 1 : ex;
}

template <int D, bool LEVEL, bool ACT>
__global__ __launch_bounds__(CHAN_LVL_THREADS) void k_chan_level(const double2 *__restrict__ spec, const double *__restrict__ g2,
                                                                 const ChanParam *__restrict__ par, double *__restrict__ E, int nch, int nblk,
                                                                 ChanAct act, long long p0)
{
    static_assert(LEVEL || ACT, "a launch that keeps nothing");
    static_assert(CHAN_ACT_BINS == 4 * CHAN_LVL_T, "four bins per lane");
    constexpr int M = CHAN_N / D, T = CHAN_LVL_T, PER = M / T, UNROLL = PER < 8 ? PER : 8;
    __shared__ double tbl[M];
    for (int i = threadIdx.x; i < M; i += CHAN_LVL_THREADS) tbl[i] = g2[i];
    __syncthreads();
    const int u = threadIdx.x % T;
    const int c_raw = blockIdx.x * (CHAN_LVL_THREADS / T) + threadIdx.x / T;
    const bool live = c_raw < nch;
    const int c = live ? c_raw : nch - 1;
    const int k0 = par[c].b - M / 2 + u;
    const bool owner = live && u == 0;
    double e = 0.0;
    if constexpr (LEVEL) e = owner ? E[c] : 0.0;
    double emax = 0.0, emin = 0.0;
    long long when = -1;
    unsigned h0 = 0, h1 = 0, h2 = 0, h3 = 0;
    if constexpr (ACT)
    {
        when = act.when[c];
        if (when >= 0) { emax = act.emax[c]; emin = act.emin[c]; }
    }
    for (int j = 0; j < nblk; j++)
    {
        const double2 *__restrict__ X = spec + (size_t)j * CHAN_N;
        double acc = 0.0;
#pragma unroll UNROLL
        for (int i = 0; i < PER; i++)
        {
            const double2 x = X[(k0 + i * T) & (CHAN_N - 1)];
            acc += (x.x * x.x + x.y * x.y) * tbl[i * T + u];
        }
#pragma unroll
        for (int m = T / 2; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, T);
        if constexpr (LEVEL) e += acc;
        if constexpr (ACT)
        {
            const bool first = when < 0;
            if (first || acc > emax) { emax = acc; when = p0 + j; } // strictly above: the smallest block index of the maximum stays
            if (first || acc < emin) emin = acc;
            const int bin = chan_act_bin(acc) - u;
            h0 += bin == 0; h1 += bin == T; h2 += bin == 2 * T; h3 += bin == 3 * T;
        }
    }
    if constexpr (LEVEL) { if (owner) E[c] = e; }
    if constexpr (ACT)
    {
        if (owner) { act.emax[c] = emax; act.emin[c] = emin; act.when[c] = when; }
        if (live)
        {
            unsigned *__restrict__ row = act.hist + (size_t)c * CHAN_ACT_BINS + u;
            row[0] += h0; row[T] += h1; row[2 * T] += h2; row[3 * T] += h3;
        }
    }
}
