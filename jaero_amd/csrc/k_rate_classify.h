// k_rate_classify.h -- the rate meter's decision kernel (include/jaero_hip.h, "rate lines, read on the device"; DESIGN 18, "Rate lines, read
// on the device"): per channel, from its row R[0 .. 2048], the median of R[kmin ..] and, per line distance d, the largest min(P[a], P[a + d])
// with the smallest a that attains it, P the three-bin maximum.  Everything is selection: a non-negative double orders as its 64-bit
// pattern does, so the kernel works on the patterns as unsigned integers throughout and the only floating-point operation is the halving of
// an even count's two middle values.
//
//   grid ceil(nch / 4), 256 threads = 4 wavefronts, one channel each; 4 x (2052 + 64) x 8 B = 67 712 B LDS: two workgroups share a CU.
//   Lane l holds bins l + 64 j, j = 0 .. 31, in registers (one coalesced 8-byte load per j: a row starts at any 8-byte address), lane 0
//   also bin 2048.  A wavefront reads and writes its own LDS alone; the three workgroup barriers order its own writes and reads and
//   nothing else.
//     P       the row goes to LDS with R[0] and R[2048] repeated in front and behind (bin k at entry k + 1), so P[k] is the maximum of entries
//             k, k + 1, k + 2 with no clipping; P then takes the row's place (bin k at entry k).
//     median  the bins below kmin (and bin 2048 in lanes other than 0) become 2^64 - 1 in the registers, above every double.  With n = 2049 -
//             kmin values and r = (n - 1) / 2, the order statistic x_r is the largest x with #{v < x} <= r, found bit by bit from bit 62
//             down; #{v < t} is a sum of 33 wave-wide ballot counts, uniform, in scalar registers.  Beside x the loop keeps how many values
//             lie below x and how many share the bits of x decided so far; x_r is one of the latter, and once they are at most 64 -- on
//             spectra after the bits the values have in common and five or six more; never, on a row of equal values -- they are written
//             to a list in LDS, one lane takes each, and the remaining bits cost one compare each instead of 33.  An even n also needs
//             x_(r + 1): x_r itself if #{v <= x_r} >= r + 2, else the smallest v above x_r (a wave-wide minimum); floor = (x_r +
//             x_(r + 1)) / 2 as doubles.
//     search  per distance, lane l walks a = l + 64 j upwards and keeps (value, a) of its first largest min(P[a], P[a + d]), two
//             conflict-free 8-byte LDS reads each; then six xor-shuffle steps in which the larger value wins and, of equal values, the
//             smaller a.  No barrier: P is only read.
//   The wavefront past nch (the last workgroup's) works on row nch - 1 again and stores nothing.  Lane 0 stores the results.
#pragma once
#include "k_rate.h" // RATE_BINS

#define RCL_NC 4                 // channels (wavefronts) per workgroup
#define RCL_THREADS (64 * RCL_NC)
#define RCL_ROW (RATE_BINS + 3)  // 64-bit entries of a channel's LDS row: the bins and the two repeated ends, rounded up to even
#define RCL_SLOTS 32             // bins l + 64 j a lane; bin 2048 is lane 0's 33rd
#define RCL_MAXD 8

struct rcl_dist { int d[RCL_MAXD]; };

// (v, a) before (bv, ba): the larger value, and of equal values the smaller a
__device__ __forceinline__ bool rcl_better(unsigned long long v, int a, unsigned long long bv, int ba)
{
    return v > bv || (v == bv && a < ba);
}

__device__ __forceinline__ unsigned long long rcl_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long rcl_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// R [nch][2049] as 64-bit patterns; kmin in 1 .. 2047; nd in 1 .. 8 distances dd.d[i] >= 1; floor_out [nch], score [nch][nd] (patterns),
// where [nch][nd]
__global__ __launch_bounds__(RCL_THREADS) void k_rate_classify(const unsigned long long *__restrict__ R, int nch, int kmin, int nd, rcl_dist dd,
                                                               double *__restrict__ floor_out, unsigned long long *__restrict__ score,
                                                               int *__restrict__ where)
{
    __shared__ unsigned long long lds[RCL_NC * (RCL_ROW + 64)];
    const int lane = (int)(threadIdx.x & 63u);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c0 = (int)blockIdx.x * RCL_NC + w;
    const bool live = c0 < nch;
    const int c = live ? c0 : nch - 1;
    const unsigned long long *__restrict__ row = R + (size_t)c * RATE_BINS;
    unsigned long long *p = lds + w * RCL_ROW;                  // the row, then P
    unsigned long long *list = lds + RCL_NC * RCL_ROW + w * 64; // the median's last candidates
    const unsigned long long NONE = ~0ull;

    unsigned long long v[RCL_SLOTS + 1];
#pragma unroll
    for (int j = 0; j < RCL_SLOTS; j++) v[j] = row[lane + 64 * j];
    v[RCL_SLOTS] = row[RATE_BINS - 1]; // the same word in every lane

    // ---- P: the row with its ends repeated, then the three-bin maximum in its place
#pragma unroll
    for (int j = 0; j < RCL_SLOTS; j++) p[1 + lane + 64 * j] = v[j];
    if (lane == 0) { p[0] = v[0]; p[RATE_BINS] = v[RCL_SLOTS]; p[RATE_BINS + 1] = v[RCL_SLOTS]; }
    jd_lds_barrier();
    unsigned long long q[RCL_SLOTS + 1];
#pragma unroll
    for (int j = 0; j < RCL_SLOTS; j++) q[j] = rcl_max(rcl_max(p[lane + 64 * j], v[j]), p[lane + 64 * j + 2]);
    q[RCL_SLOTS] = rcl_max(p[RATE_BINS - 1], v[RCL_SLOTS]); // bin 2048: entries 2048, 2049 (itself) and 2050 (itself again)
    jd_lds_barrier();
#pragma unroll
    for (int j = 0; j < RCL_SLOTS; j++) p[lane + 64 * j] = q[j];
    if (lane == 0) p[RATE_BINS - 1] = q[RCL_SLOTS];

    // ---- the median of bins kmin .. 2048
#pragma unroll
    for (int j = 0; j < RCL_SLOTS; j++)
        if (lane + 64 * j < kmin) v[j] = NONE;
    if (lane != 0) v[RCL_SLOTS] = NONE;
    const int n = RATE_BINS - kmin, r = (n - 1) >> 1;
    // x: the bits of x_r above b; below = #{v < x}; inside = #{x <= v < x + 2^(b + 1)}, x_r among them
    unsigned long long x = 0;
    int below = 0, inside = n, b = 62;
#pragma unroll 1
    for (; b >= 0 && inside > 64; b--)
    {
        const unsigned long long t = x | (1ull << b);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j <= RCL_SLOTS; j++) cnt += __popcll(__ballot(v[j] < t));
        if (cnt <= r) { inside -= cnt - below; below = cnt; x = t; }
        else inside = cnt - below;
    }
    // the values that share x's decided bits, in bin order, to the list (at most 64 unless every bit is decided: then nobody reads it)
    {
        const int sh = b + 1; // 0 .. 63; a value of 2^64 - 1 differs from x in bit 63
        const unsigned long long lower = (1ull << lane) - 1ull;
        int base = 0;
#pragma unroll
        for (int j = 0; j <= RCL_SLOTS; j++)
        {
            const bool in = ((v[j] ^ x) >> sh) == 0ull;
            const unsigned long long mask = __ballot(in);
            const int pos = base + __popcll(mask & lower);
            if (in && pos < 64) list[pos] = v[j];
            base += __popcll(mask);
        }
    }
    jd_lds_barrier(); // the list, and P, are in place
    const unsigned long long cand = (b >= 0 && lane < inside) ? list[lane] : NONE;
#pragma unroll 1
    for (; b >= 0; b--) // #{v < t} = below + #{cand < t} for every t inside the candidates' range
    {
        const unsigned long long t = x | (1ull << b);
        if (below + __popcll(__ballot(cand < t)) <= r) x = t;
    }
    unsigned long long xhi = x;
    if ((n & 1) == 0)
    {
        int cle = 0;
        unsigned long long above = NONE;
#pragma unroll
        for (int j = 0; j <= RCL_SLOTS; j++)
        {
            cle += __popcll(__ballot(v[j] <= x));
            if (v[j] > x) above = rcl_min(above, v[j]);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) above = rcl_min(above, __shfl_xor(above, off));
        if (cle < r + 2) xhi = above;
    }
    const double med = (n & 1) ? __longlong_as_double((long long)x)
                               : (__longlong_as_double((long long)x) + __longlong_as_double((long long)xhi)) / 2.0;
    if (live && lane == 0) floor_out[c] = med;

    // ---- per distance: the first largest min(P[a], P[a + d]) over kmin <= a < 2049 - d
#pragma unroll 1
    for (int i = 0; i < nd; i++)
    {
        const int d = dd.d[i];
        if (d >= RATE_BINS - kmin) // no a at all: skipped
        {
            if (live && lane == 0) { score[(size_t)c * nd + i] = 0ull; where[(size_t)c * nd + i] = -1; }
            continue;
        }
        const int aend = RATE_BINS - d;
        unsigned long long bv = 0ull;
        int ba = 0x7fffffff;
#pragma unroll 8
        for (int j = 0; j < RCL_SLOTS; j++)
        {
            const int a = lane + 64 * j;
            const bool ok = a >= kmin && a < aend;
            const int ai = ok ? a : kmin; // kmin + d <= 2048: inside the row
            const unsigned long long m = rcl_min(p[ai], p[ai + d]);
            if (ok && rcl_better(m, a, bv, ba)) { bv = m; ba = a; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
        {
            const unsigned long long ov = __shfl_xor(bv, off);
            const int oa = __shfl_xor(ba, off);
            if (rcl_better(ov, oa, bv, ba)) { bv = ov; ba = oa; }
        }
        if (live && lane == 0) { score[(size_t)c * nd + i] = bv; where[(size_t)c * nd + i] = ba; }
    }
}
