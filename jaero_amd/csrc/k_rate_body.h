// k_rate_body.h -- the body of the three line kernels of k_rate.h, included once by each with RATE_GATED 0 (k_rate_lines), 1
// (k_rate_lines_gated) and 2 (k_rate_lines_auto).  No include guard on purpose.  The stages are shared as text and not as a function: with
// RATE_GATED 0 what the compiler sees is k_rate_lines as it was before the gate existed, token for token, so its code stays the same
// instruction for instruction (as a function inlined into both kernels the same source came out at 158 registers instead of 108); with
// RATE_GATED 1 it sees k_rate_lines_gated as it was before the one-pass gates existed.
// In scope: pend, fill, pcm, n, nch, nseg, tw, R, with RATE_GATED 1 gate and stats, with RATE_GATED 2 also stats2, hist, autom and seg0.
#ifndef RATE_GATED
#error "k_rate_body.h is included by k_rate.h alone"
#endif
    constexpr int NC = RATE_NC;
    extern __shared__ double rt_xch[]; // NC channels x 4096 doubles; the staging area and the partial sums lie in it before the transform
    int16_t *stg = (int16_t *)rt_xch;
    unsigned long long *part = (unsigned long long *)(rt_xch + NC * RATE_STG / 4); // behind the staging area: [4 NC wavefronts][NC channels]
#if RATE_GATED == 2
    // one-pass gates: the whole state of BOTH channels of the workgroup -- the gate, emax, e2, emin, njoin, ejoin, start -- in every thread,
    // and uniform (rate_uniform: through readfirstlane), so it lives in scalar registers and costs the transform no vector register.  E is
    // the same integer in every thread, so every thread takes every step of the rule alike.  Loaded here, stored behind the last segment
    // by thread cc; a channel past nch carries the empty state, never joins and stores nothing.
    unsigned long long g[NC], emax[NC], e2[NC], emin[NC], njoin[NC], ejoin[NC], start[NC];
#pragma unroll
    for (int cc = 0; cc < NC; cc++)
    {
        const int chn = blockIdx.x * NC + cc;
        const bool in = chn < nch;
        g[cc] = in ? rate_uniform(gate[chn]) : 0;
        emax[cc] = in ? rate_uniform(stats[(size_t)chn * 4 + 0]) : 0;
        emin[cc] = in ? rate_uniform(stats[(size_t)chn * 4 + 1]) : ~0ull;
        njoin[cc] = in ? rate_uniform(stats[(size_t)chn * 4 + 2]) : 0;
        ejoin[cc] = in ? rate_uniform(stats[(size_t)chn * 4 + 3]) : 0;
        e2[cc] = in ? rate_uniform(stats2[(size_t)chn * 2 + 0]) : 0;
        start[cc] = in ? rate_uniform(stats2[(size_t)chn * 2 + 1]) : ~0ull;
    }
    const bool keeps = threadIdx.x < NC && blockIdx.x * NC + threadIdx.x < nch; // the thread that stores channel threadIdx.x's state and counts it
#elif RATE_GATED
    // the workgroup's gates (uniform addresses: scalar registers; a channel past nch has none and never joins), and in thread cc < NC the
    // four numbers of channel cc over the launch's segments: loaded here, stored behind the last segment
    unsigned long long g[NC], emax = 0, emin = 0, njoin = 0, ejoin = 0;
#pragma unroll
    for (int cc = 0; cc < NC; cc++) g[cc] = blockIdx.x * NC + cc < nch ? gate[blockIdx.x * NC + cc] : 0;
    const bool keeps = threadIdx.x < NC && blockIdx.x * NC + threadIdx.x < nch;
    if (keeps)
    {
        const unsigned long long *st = stats + (size_t)(blockIdx.x * NC + threadIdx.x) * 4;
        emax = st[0]; emin = st[1]; njoin = st[2]; ejoin = st[3];
    }
#endif
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
#if RATE_GATED == 2
        // ---- decision, one-pass gates (include/jaero_hip.h, "one-pass gates"): E of every channel of the workgroup as in the gated kernel,
        // made uniform, then the rule step by step in scalar arithmetic.  Under JAERO_GATE_AUTO the gate follows (e2 + emin) / 2; without
        // it (MANUAL | HIST) the given gate stays, and then no channel restarts (a restart needs the gate to rise from 0).  Bits cc and
        // NC + cc of `joins` = channel cc joins, channel cc restarts: one scalar register that outlives the transform.
        unsigned joins = 0;
#pragma unroll
        for (int cc = 0; cc < NC; cc++)
        {
            unsigned long long e = 0;
#pragma unroll
            for (int w = 0; w < 4 * NC; w++) e += part[w * NC + cc];
            e = rate_uniform(e);
            if (e > emax[cc]) { e2[cc] = emax[cc]; emax[cc] = e; }
            else if (e > e2[cc]) e2[cc] = e;
            emin[cc] = e < emin[cc] ? e : emin[cc];
            // emin <= e < 2^43 from here on: 3 emin and e2 + emin stay far inside 64 bits
            const unsigned long long gn = !autom ? g[cc] : (e2[cc] > 0 && 2 * e2[cc] >= 3 * emin[cc]) ? (e2[cc] + emin[cc]) / 2 : 0;
            const bool join = blockIdx.x * NC + cc < nch && e >= gn;
            if (join && g[cc] == 0 && gn > 0) // restart: what was summed under gate 0 is thrown away
            {
                njoin[cc] = 1; ejoin[cc] = e; start[cc] = seg0 + (unsigned long long)j;
                joins |= (1u << cc) | (1u << (NC + cc));
            }
            else if (join)
            {
                njoin[cc] += 1; ejoin[cc] += e;
                joins |= 1u << cc;
            }
            g[cc] = gn;
            if (cc == c) sum = e;
        }
        joins = __builtin_amdgcn_readfirstlane(joins);
        // ---- histogram: thread cc < NC has c == cc, so `sum` is E of the channel it keeps; the workgroup owns the row, so a plain
        // read-modify-write of the one counter.  E <= 4096 * 32768^2 = 2^42 lands in bin 320, the last; the bound is kept anyway
        if (hist != nullptr && keeps)
        {
            int b = (int)sum;
            if (sum >= 8)
            {
                const int lg = 63 - __clzll((long long)sum);
                b = 8 * (lg - 2) + (int)((sum >> (lg - 3)) & 7);
            }
            b = b < RATE_HBINS - 1 ? b : RATE_HBINS - 1;
            unsigned *hc = hist + (size_t)(blockIdx.x * NC + threadIdx.x) * RATE_HBINS + b;
            *hc = *hc + 1;
        }
#elif RATE_GATED
        // ---- decision: every thread sums E of EVERY channel of the workgroup (integers: the same E in every thread), so all threads agree
        // on who joins.  bit cc of `joins` = channel cc joins; through readfirstlane it is one scalar register, which outlives the
        // transform -- the sums in LDS do not -- and makes the branches on it uniform for the compiler too
        unsigned joins = 0;
#pragma unroll
        for (int cc = 0; cc < NC; cc++)
        {
            unsigned long long e = 0;
#pragma unroll
            for (int w = 0; w < 4 * NC; w++) e += part[w * NC + cc];
            if (blockIdx.x * NC + cc < nch && e >= g[cc]) joins |= 1u << cc;
            if (cc == c) sum = e;
        }
        joins = __builtin_amdgcn_readfirstlane(joins);
        // ---- statistics: thread cc < NC has c == cc, so `sum` is E of the channel it keeps
        if (keeps)
        {
            emax = sum > emax ? sum : emax;
            emin = sum < emin ? sum : emin;
            if ((joins >> c) & 1) { njoin += 1; ejoin += sum; }
        }
#else
#pragma unroll
        for (int w = 0; w < 4 * NC; w++) sum += part[w * NC + c];
#endif
        jd_lds_barrier(); // the transform's exchanges overwrite the staging area and the partial sums
#if RATE_GATED
        if (joins == 0) continue; // nobody joins: no transform, no Hann step, no access to R.  The whole workgroup takes the branch, behind the
                                  // barrier that keeps the next segment's staging off the partial sums and the staging area
#endif
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
        // ---- R += |H|^2; gated, of the joining channels only (a joining channel lies below nch): one that does not join leaves its row alone
#if RATE_GATED == 2
        // a restarting channel stores where a joining one adds: its row then holds this segment's terms alone, as an ungated meter's
        // first segment does (0 + t == t bit for bit, t being a sum of squares)
        if ((joins >> (NC + c2)) & 1)
        {
            double *__restrict__ Rk = R + (size_t)ch * RATE_BINS + T2;
#pragma unroll
            for (int s = 0; s < 9; s++)
                if (s < ns) Rk[256 * s] = hr[s] * hr[s] + hi[s] * hi[s];
        }
        else
#endif
#if RATE_GATED
        if ((joins >> c2) & 1)
#else
        if (ch < nch)
#endif
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
#if RATE_GATED == 2
#pragma unroll
    for (int cc = 0; cc < NC; cc++)
        if (keeps && threadIdx.x == cc)
        {
            const size_t chn = (size_t)(blockIdx.x * NC + cc);
            if (autom) gate[chn] = g[cc];
            unsigned long long *st = stats + chn * 4, *s2 = stats2 + chn * 2;
            st[0] = emax[cc]; st[1] = emin[cc]; st[2] = njoin[cc]; st[3] = ejoin[cc];
            s2[0] = e2[cc]; s2[1] = start[cc];
        }
#elif RATE_GATED
    if (keeps)
    {
        unsigned long long *st = stats + (size_t)(blockIdx.x * NC + threadIdx.x) * 4;
        st[0] = emax; st[1] = emin; st[2] = njoin; st[3] = ejoin;
    }
#endif
