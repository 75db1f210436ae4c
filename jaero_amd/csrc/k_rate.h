// k_rate.h -- the rate meter's line kernels (include/jaero_hip.h, "rate lines" and "gated rate lines"; DESIGN 18, "Rate lines"): the
// Hann-windowed power spectrum of the SQUARED int16 signal of every channel, one 4096-point fp64 transform per channel and segment, summed
// over segments.  The body of all three kernels is k_rate_body.h.
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
//
//   k_rate_lines_gated (a handle switched over by jaero_gate_enable launches it in place of k_rate_lines) differs in four places:
//     decision    where the partial sums meet in LDS every thread adds up the sum E of EVERY channel of the workgroup, not only its own, and
//                 compares each with the channel's gate: channel cc joins iff it lies below nch and E >= gate.  The result is a bit mask in
//                 one scalar register, the same in every thread.
//     statistics  thread cc < NC keeps emax, emin, njoin, ejoin of channel cc in registers over the launch's segments: plain 64-bit loads
//                 in front of the first segment, plain stores behind the last, no atomics (a workgroup owns its channels).
//     skip        nobody joins: the workgroup goes on to the next segment behind the barrier that ends the reading of the partial sums
//                 -- no transform, no Hann step, no access to R.
//     R           somebody joins: transform and Hann step run for the whole workgroup (the exchanges are shared), and only a joining
//                 channel's threads do the read-modify-write.  The others do not touch their rows; they do not add zero.
//
//   k_rate_lines_auto (launched in place of the other two while the handle's mode has JAERO_GATE_AUTO or JAERO_GATE_HIST; include/jaero_hip.h,
//   "one-pass gates") follows k_rate_lines_gated in every respect but three:
//     decision    under AUTO the rule of the one-pass gates: emax, e2, emin are brought up to date with E, the gate becomes (e2 + emin) / 2 or
//                 0, and the segment joins iff E reaches the NEW gate; a channel whose gate rises from 0 on a segment that joins RESTARTS.
//                 Under MANUAL | HIST the plain comparison with the given gate.  E goes through readfirstlane, so the state of both
//                 channels (7 numbers each) is uniform and sits in scalar registers over the launch's segments: loaded in front of the
//                 first, stored behind the last by thread cc < NC with vector stores -- the gate too, under AUTO.
//     R           a restarting channel's threads store |H|^2 where a joining one's add it.
//     histogram   thread cc < NC does the read-modify-write of the one counter of channel cc's row that E falls into, every segment, joined
//                 or not (hist == nullptr: no histogram).  The workgroup owns its channels: no atomics.
#pragma once
#include "wg_fft.h" // pf_fft4096

#define RATE_L 4096
#define RATE_BINS 2049
#define RATE_NC 2                // channels per workgroup
#define RATE_THREADS (256 * RATE_NC)
#define RATE_HBINS 321           // bins of a channel's histogram of E (one-pass gates)
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

// x, the same in every lane, as a value the compiler knows to be uniform: it then lives in a pair of scalar registers
__device__ __forceinline__ unsigned long long rate_uniform(unsigned long long x)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)x), hi = __builtin_amdgcn_readfirstlane((unsigned)(x >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// pend [nch][4096]: the partial segment in front of this write (`fill` samples a row); pcm [nch][n]: the write; nseg = (fill + n) / 4096 > 0
__global__ __launch_bounds__(RATE_THREADS) void k_rate_lines(const int16_t *__restrict__ pend, int fill, const int16_t *__restrict__ pcm, int n,
                                                             int nch, int nseg, const double2 *__restrict__ tw, double *__restrict__ R)
{
#define RATE_GATED 0
#include "k_rate_body.h"
#undef RATE_GATED
}

// the same, gated: gate [nch]; stats [nch][4] = emax, emin, njoin, ejoin
__global__ __launch_bounds__(RATE_THREADS) void k_rate_lines_gated(const int16_t *__restrict__ pend, int fill, const int16_t *__restrict__ pcm, int n,
                                                                   int nch, int nseg, const double2 *__restrict__ tw, double *__restrict__ R,
                                                                   const unsigned long long *__restrict__ gate, unsigned long long *__restrict__ stats)
{
#define RATE_GATED 1
#include "k_rate_body.h"
#undef RATE_GATED
}

// the one-pass gates: gate [nch] (written back under autom); stats [nch][4] as above; stats2 [nch][2] = e2, start; hist [nch][321] or null;
// autom != 0: the device chooses the gates; seg0 = the segments completed since the last reset in front of this launch
__global__ __launch_bounds__(RATE_THREADS) void k_rate_lines_auto(const int16_t *__restrict__ pend, int fill, const int16_t *__restrict__ pcm, int n,
                                                                  int nch, int nseg, const double2 *__restrict__ tw, double *__restrict__ R,
                                                                  unsigned long long *__restrict__ gate, unsigned long long *__restrict__ stats,
                                                                  unsigned long long *__restrict__ stats2, unsigned *__restrict__ hist, int autom,
                                                                  unsigned long long seg0)
{
#define RATE_GATED 2
#include "k_rate_body.h"
#undef RATE_GATED
}
