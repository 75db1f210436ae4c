// k_rate.h -- the rate meter's line kernel (include/jaero_hip.h, "rate lines"; DESIGN 18, "Rate lines"): the Hann-windowed power spectrum
// of the SQUARED int16 signal of every channel, one 4096-point fp64 transform per channel and segment, summed over segments.
//
//   grid ceil(nch / 2), 512 threads = 2 channels x 256 threads, 64 KiB LDS.  The transform is k_pre8400_fft's (pf_fft4096<NC>: thread
//   (c = tid % NC, T = tid / NC) holds index T + 256 s of channel NC blockIdx.x + c in slot s on entry and on exit) with NC = 2 channels
//   per workgroup instead of 4: at 1024 threads a thread has 128 registers and the kernel spilled 15 of them to scratch; at 512 it needs
//   108, spills nothing, and two workgroups share a CU -- the same 4 wavefronts per SIMD.  One workgroup owns its channels' rows of R and
//   walks the launch's completed segments in ascending order; every segment ends in the read-modify-write of those rows, so the terms join
//   the sum in segment order without atomics, by the same instructions whatever the write sizes are.
//   Per segment:
//     stage   the segment's NC x 4096 int16 into LDS.  Sample i of segment j is sample p = 4096 j + i of (pending, then this write): below
//             `fill` it comes from the pending buffer, above from the write.  Both parts are read as aligned 16-byte words by the 256
//             consecutive threads lc = tid >> 8 of a channel (a row of the write starts at any even address: the first and the last word
//             of a run are then read whole -- an aligned word that holds one valid byte lies inside that byte's page -- and only the
//             valid int16 of a word are kept).
//     square  y^2 as integers (< 2^31), their sum over the segment as a 64-bit integer (< 2^43: 16 per thread, xor butterfly over the
//             64 / NC T of a wavefront, the 4 NC wavefronts through LDS), q = y^2 - sum / 4096 in fp64: every step exact.
//     Z       = DFT_4096(q + 0 i).  No packing of two rows or two segments into one transform (a neighbour's round-off would leak into a
//             weak or zero row; two segments would break the count or the cut rules).
//     Hann    in the frequency domain, H[k] = Z[k] / 2 - (Z[k - 1] + Z[k + 1]) / 4, the neighbours through LDS (plane by plane), the
//             indices mod 4096.
//     R[k]   += |H[k]|^2 for k <= 2048: slots 0 .. 7 of every thread, slot 8 of T = 0.
//   A channel past nch (the last workgroup's) is staged as zeros and stores nothing.
#pragma once
#include "k_pre8400.h" // pf_fft4096

#define RATE_L 4096
#define RATE_BINS 2049
#define RATE_NC 2                // channels per workgroup
#define RATE_THREADS (256 * RATE_NC)
#define RATE_STG (RATE_L + 32)   // int16 per channel of the staging area: the channels' reads of a wavefront's 32 T fall on different banks

// the int16 src[0 .. count) to dst[0 .. count) in LDS, by the 256 threads t of one channel, in aligned 16-byte loads
__device__ __forceinline__ void rate_stage_run(const int16_t *__restrict__ src, int count, int16_t *dst, int t)
{
    if (count <= 0) return;
    const unsigned long long a = (unsigned long long)src, a0 = a & ~15ull;
    const int lead = (int)((a - a0) >> 1);                  // int16 of the first word that lie in front of src
    const int nwords = (lead + count + 7) >> 3;
    const uint4 *__restrict__ w = (const uint4 *)a0;
    for (int i = t; i < nwords; i += 256)
    {
        const uint4 v = w[i];
        const unsigned u[4] = {v.x, v.y, v.z, v.w};
        const int i0 = i * 8 - lead;
#pragma unroll
        for (int e = 0; e < 8; e++)
        {
            const int idx = i0 + e;
            if (idx >= 0 && idx < count) dst[idx] = (int16_t)(u[e >> 1] >> (16 * (e & 1)));
        }
    }
}

// pend [nch][4096]: the partial segment in front of this write (`fill` samples a row); pcm [nch][n]: the write; nseg = (fill + n) / 4096 > 0
__global__ __launch_bounds__(RATE_THREADS) void k_rate_lines(const int16_t *__restrict__ pend, int fill, const int16_t *__restrict__ pcm, int n,
                                                             int nch, int nseg, const double2 *__restrict__ tw, double *__restrict__ R)
{
    constexpr int NC = RATE_NC;
    extern __shared__ double rt_xch[]; // NC channels x 4096 doubles; the staging area and the partial sums lie in it before the transform
    int16_t *stg = (int16_t *)rt_xch;
    unsigned long long *part = (unsigned long long *)(rt_xch + NC * RATE_STG / 4); // behind the staging area: [4 NC wavefronts][NC channels]
    for (int j = 0; j < nseg; j++)
    {
        // what a thread derives from its index is formed anew in every segment, and once more behind the transform: held across the
        // transform instead, those registers are the ones it lacks
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int c = tid % NC, T = tid / NC;
        // ---- stage
        {
            const int lc = tid >> 8, lt = tid & 255, lch = blockIdx.x * NC + lc; // the staging's channel and thread
            int16_t *dst = stg + lc * RATE_STG;
            if (lch < nch)
            {
                const int p0 = j * RATE_L;                       // first sample of the segment in (pending, write)
                const int npend = fill > p0 ? fill - p0 : 0;     // of it, from the pending buffer (only in segment 0)
                rate_stage_run(pend + (size_t)lch * RATE_L + p0, npend, dst, lt);
                rate_stage_run(pcm + (size_t)lch * n + (p0 + npend - fill), RATE_L - npend, dst + npend, lt);
            }
            else
                for (int i = lt; i < RATE_L; i += 256) dst[i] = 0;
        }
        jd_lds_barrier();
        // ---- square, sum, subtract the mean
        int sq[16];
        unsigned long long sum = 0;
#pragma unroll
        for (int s = 0; s < 16; s++)
        {
            const int y = stg[c * RATE_STG + T + 256 * s];
            sq[s] = y * y;
            sum += (unsigned long long)sq[s];
        }
#pragma unroll
        for (int m = NC; m < 64; m <<= 1) sum += __shfl_xor(sum, m); // the 64 / NC T of this wavefront: lanes NC (T mod (64 / NC)) + c
        if ((tid & 63) < NC) part[(tid >> 6) * NC + c] = sum;
        jd_lds_barrier();
        sum = 0;
#pragma unroll
        for (int w = 0; w < 4 * NC; w++) sum += part[w * NC + c];
        jd_lds_barrier(); // the transform's exchanges overwrite the staging area and the partial sums
        const double mean = (double)(long long)sum * (1.0 / RATE_L);
        CV<16> d;
#pragma unroll
        for (int s = 0; s < 16; s++) { d.r[s] = (double)sq[s] - mean; d.i[s] = 0.0; }
        // ---- Z
        pf_fft4096<NC>(d, rt_xch, tw, T, c);
        // ---- Hann, plane by plane: Z[k] of channel c at rt_xch[NC k + c].  k - 1 and k + 1 stay inside 0 .. 4095 but for k = 0 (slot 0 of T = 0)
        int tid2 = threadIdx.x;
        asm volatile("" : "+v"(tid2));
        const int c2 = tid2 % NC, T2 = tid2 / NC, ch = blockIdx.x * NC + c2;
        const int ns = T2 == 0 ? 9 : 8;
        double *zc = rt_xch + T2 * NC + c2;
        const double *zm = rt_xch + ((T2 - 1) & (RATE_L - 1)) * NC + c2;
        double hr[9], hi[9];
#pragma unroll
        for (int s = 0; s < 16; s++) zc[256 * NC * s] = d.r[s];
        jd_lds_barrier();
        hr[0] = 0.5 * d.r[0] - 0.25 * (zm[0] + zc[NC]);
#pragma unroll
        for (int s = 1; s < 9; s++)
            if (s < ns) hr[s] = 0.5 * d.r[s] - 0.25 * (zc[256 * NC * s - NC] + zc[256 * NC * s + NC]);
        jd_lds_barrier();
#pragma unroll
        for (int s = 0; s < 16; s++) zc[256 * NC * s] = d.i[s];
        jd_lds_barrier();
        hi[0] = 0.5 * d.i[0] - 0.25 * (zm[0] + zc[NC]);
#pragma unroll
        for (int s = 1; s < 9; s++)
            if (s < ns) hi[s] = 0.5 * d.i[s] - 0.25 * (zc[256 * NC * s - NC] + zc[256 * NC * s + NC]);
        jd_lds_barrier(); // the next segment's staging overwrites the plane
        // ---- R += |H|^2
        if (ch < nch)
        {
            double *__restrict__ Rk = R + (size_t)ch * RATE_BINS + T2;
#pragma unroll
            for (int s = 0; s < 9; s++)
                if (s < ns)
                {
                    const double t = hr[s] * hr[s] + hi[s] * hi[s];
                    Rk[256 * s] = Rk[256 * s] + t;
                }
        }
    }
}
