// k_chan_capture.h -- the capture front end of the channeliser (jaero_chan3_*, DESIGN 18 "Capture front end"): raw SDR samples in their own
// format and at their own rate -> the fp64 stream z[m] at the channeliser's rate Fs_c = out_rate x D that k_capture_fwd transforms.
//
// The definition is include/jaero_hip.h's ("capture front end"); tests/chan_capture_oracle.py implements it literally in numpy.  Per staged
// sample m (an absolute count), with L / Mr = Fs_c / fs_in in lowest terms:
//   convert  x[n]  = the raw pair as fp64 in int16 LSB units (exact for every format; a cf32 component that is not finite is 0)
//   mix      x'[n] = x[n] e^(j 2 pi ((shift n) mod 2^32) / 2^32), the word read as a signed number, by sincospi as k_chan_synth's rotation
//   resample z[m]  = sum_{j < K} h[phi + j L] x'[n_m - j],  n_m = floor(m Mr / L), phi = (m Mr) mod L, ascending j from 0.0, real and
//            imaginary sums apart, every product and sum rounded once (the library is built with -ffp-contract=off; nothing here turns
//            contraction on)
// Everything is a function of absolute indices: the staged stream is the same bits however the writes were cut.
//
// Shape of k_capture_stage<FMT, MIX, true>: a workgroup of 256 threads owns a run of CAP_RUN = 256 consecutive outputs.  The inputs the run
// needs, n_(first) - (K - 1) .. n_(last) -- at most 8 (CAP_RUN - 1) + 1 + K of them, since Mr / L <= 8 -- are converted and mixed ONCE into
// LDS as double2 (one sincospi per input sample, not K), then lane i forms output i from LDS with the coefficients stored phase-major
// (hp[phi K + j] = h[phi + j L]: K contiguous doubles per lane).  <FMT, MIX, false> (equal rates) has no LDS, no taps: a thread converts and
// mixes one sample.  MIX = false (shift == 0) has no trig and no multiplication: a pure format conversion costs neither.
#pragma once
#include "k_chan.h"

#define CAP_RUN 256
#define CAP_THREADS 256
#define CAP_MAXK 64
#define CAP_XS (8 * CAP_RUN + CAP_MAXK) // double2 entries: 8 (CAP_RUN - 1) + 1 + K <= CAP_XS for K <= 64

// raw pair k of the buffer as fp64 in int16 LSB units
template <int FMT> __device__ __forceinline__ double2 cap_convert(const void *__restrict__ raw, long long k)
{
    if constexpr (FMT == JAERO_IQ_CS16)
    {
        const int v = ((const int *)raw)[k];
        return make_double2((double)(short)(v & 0xffff), (double)(v >> 16));
    }
    else if constexpr (FMT == JAERO_IQ_CU8)
    {
        const int v = ((const unsigned short *)raw)[k];
        return make_double2((double)((2 * (v & 0xff) - 255) * 128), (double)((2 * (v >> 8) - 255) * 128));
    }
    else if constexpr (FMT == JAERO_IQ_CS8)
    {
        const int v = ((const unsigned short *)raw)[k];
        return make_double2((double)((int)(signed char)(v & 0xff) * 256), (double)((int)(signed char)(v >> 8) * 256));
    }
    else
    {
        const float2 v = ((const float2 *)raw)[k];
        const double re = (double)v.x * 32768.0, im = (double)v.y * 32768.0; // finite float x 2^15: exact, and finite in fp64
        return make_double2(__builtin_isfinite(v.x) ? re : 0.0, __builtin_isfinite(v.y) ? im : 0.0);
    }
}

// x'[n]: sample n (absolute) of the capture, converted and mixed; 0 outside what the buffer holds (n < 0 included).
// raw[k] is sample nraw0 + k, k < nraw.
template <int FMT, bool MIX>
__device__ __forceinline__ double2 cap_sample(const void *__restrict__ raw, long long nraw0, int nraw, long long n, unsigned shift)
{
    const long long k = n - nraw0;
    if (n < 0 || k < 0 || k >= nraw) return make_double2(0.0, 0.0);
    const double2 x = cap_convert<FMT>(raw, k);
    if constexpr (!MIX) return x;
    else
    {
        const unsigned ph = shift * (unsigned)(unsigned long long)n; // (shift n) mod 2^32
        double sn, cs;
        sincospi((double)(int)ph * (1.0 / 2147483648.0), &sn, &cs); // 2 pi ph / 2^32, ph as a signed word: (-pi, pi]
        return make_double2(x.x * cs - x.y * sn, x.x * sn + x.y * cs);
    }
}

// out[i] = z[m0 + i], i < nout.  q0 = floor(m0 Mr / L), r0 = (m0 Mr) mod L (from the host's 64-bit counts); hp: [L][K] phase-major.
template <int FMT, bool MIX, bool RESAMPLE>
__global__ __launch_bounds__(CAP_THREADS) void k_capture_stage(const void *__restrict__ raw, long long nraw0, int nraw, unsigned shift,
                                                               const double *__restrict__ hp, int L, int Mr, int K, long long q0, int r0,
                                                               double2 *__restrict__ out, int nout)
{
    const int t = threadIdx.x;
    if constexpr (!RESAMPLE)
    {
        const long long i = (long long)blockIdx.x * CAP_THREADS + t;
        if (i < nout) out[i] = cap_sample<FMT, MIX>(raw, nraw0, nraw, q0 + i, shift);
    }
    else
    {
        __shared__ __attribute__((aligned(16))) double2 xs[CAP_XS];
        const int i0 = blockIdx.x * CAP_RUN;                 // the run's first output, relative to the launch
        const int cnt = min(CAP_RUN, nout - i0);             // >= 1: the grid is ceil(nout / CAP_RUN)
        // (m0 + i0) Mr = q0 L + r0 + i0 Mr: the run's own quotient and remainder, once per workgroup
        const unsigned long long tb = (unsigned long long)r0 + (unsigned long long)i0 * (unsigned)Mr;
        const long long qb = q0 + (long long)(tb / (unsigned)L);
        const unsigned rb = (unsigned)(tb % (unsigned)L);
        const long long n_lo = qb - (K - 1);
        int nin = (int)((rb + (unsigned)(cnt - 1) * (unsigned)Mr) / (unsigned)L) + K; // n_lo .. n of the run's last output
        nin = min(nin, CAP_XS);                                                       // holds by Mr / L <= 8, K <= 64 (create checks both)
        for (int k = t; k < nin; k += CAP_THREADS) xs[k] = cap_sample<FMT, MIX>(raw, nraw0, nraw, n_lo + k, shift);
        __syncthreads();
        if (t < cnt)
        {
            const unsigned tt = rb + (unsigned)t * (unsigned)Mr;  // < 1024 + 255 x 8192
            const int top = (int)(tt / (unsigned)L) + (K - 1);    // LDS index of x'[n_m]
            const double *__restrict__ h = hp + (size_t)(tt % (unsigned)L) * K;
            double ar = 0.0, ai = 0.0;
            for (int j = 0; j < K; j++)
            {
                const double c = h[j];
                const double2 x = xs[top - j];
                ar = ar + c * x.x;
                ai = ai + c * x.y;
            }
            out[i0 + t] = make_double2(ar, ai);
        }
    }
}

// ------------------------------------------------------------------------------------------ forward transform over the fp64 history
// k_chan_fwd with another load: window j = in[j * Hp .. j * Hp + N) of the double2 history -> wg_fft14_e32 -> spec[j][N].
__global__ __launch_bounds__(C2_THREADS) void k_capture_fwd(const double2 *__restrict__ in, double2 *__restrict__ spec, const double2 *__restrict__ tw)
{
    extern __shared__ __attribute__((aligned(16))) double xch[];
    const int t = threadIdx.x;
    const double2 *__restrict__ src = in + (size_t)blockIdx.x * CHAN_HP;
    double2 *__restrict__ dst = spec + (size_t)blockIdx.x * CHAN_N;
    CV<32> d;
#pragma unroll
    for (int s = 0; s < 32; s++)
    {
        const double2 v = src[s * C2_THREADS + t];
        d.r[s] = v.x;
        d.i[s] = v.y;
    }
    wg_fft14_e32(d, xch, tw, t);
#pragma unroll
    for (int s = 0; s < 32; s++) dst[s * C2_THREADS + t] = make_double2(d.r[s], d.i[s]);
}
