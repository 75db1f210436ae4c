// k_aerol_sweep.h -- one-call reads of every channel of a bank's per-channel row log (jaero_aerol_read_all, jaero_read_all), and the device wire
// from the Aero-L bank's DataCarrierDetect emissions to the demodulator bank's dcd flag (jaero_aerol_link_dcd).  DESIGN.md sections 19 and 20.
//
// A log is a RowBuf (host_common.h): channel ch's rows at base + ch * cap * rowbytes, its row count in cnt[ch].  With v_c = min(cnt_c, cap)
// - pending_c (a burst bank's soft bits keep a not yet emitted tail; 0 everywhere else), P_c = sum_{k <= c} v_k: channel c is taken iff
// P_c <= caprows; the taken channels' rows go, oldest first, to out + P_{c-1} * rowbytes.
//   k_sweep_sums    : one workgroup per SWEEP_W channels, sum of v over the workgroup
//   k_sweep_offsets : base of the workgroup = sum of the block sums in front of it (every workgroup adds them up itself: at most a few hundred
//                     values, cheaper than a third launch and no workgroup waits for another), exclusive scan inside the workgroup, the
//                     P_c <= caprows rule, offsets / overflow flags / per-workgroup taken counts out
//   k_sweep_gather  : the rows of a workgroup's taken channels are one contiguous output range; thread t moves chunks t, t + 256, .. of it
//                     (the owning channel by binary search over the workgroup's offsets in LDS), then the taken channels' counts are zeroed and
//                     their overflow bit of this class cleared
//   k_sweep_gather_i16 : the same for rows of one int16 (soft bits), whose output offsets are aligned to nothing: 16-byte output words, the
//                     two at the ends of the workgroup's range element by element; a burst bank's pending tail moves to the row's front
// The order is fixed by the channel numbers alone: no atomics, no flags, no look-back.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SWEEP_W 256 // channels per workgroup = threads per workgroup (four wavefronts)

// rows channel ch holds, as the sweep counts them
// (pending: rows at the end of the channel's buffer that stay behind; null = none)
__device__ __forceinline__ int sweep_rows(const int *cnt, int cap, const int *pending, int ch, int nch)
{
    if (ch >= nch) return 0;
    int v = cnt[ch];
    v = v < 0 ? 0 : (v > cap ? cap : v);
    if (pending) v -= pending[ch];
    return v < 0 ? 0 : v;
}

// sum of v over the workgroup's SWEEP_W threads, in every thread (wavefront shuffles, then the four wavefronts through LDS)
__device__ __forceinline__ long long sweep_wg_sum(long long v, long long *s_w /* [4] */)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads(); // s_w may still be read from an earlier use
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(SWEEP_W) void k_sweep_sums(const int *__restrict__ cnt, int cap, const int *__restrict__ pend, int nch,
                                                        long long *__restrict__ blk_sum)
{
    __shared__ long long s_w[4];
    const int ch = blockIdx.x * SWEEP_W + threadIdx.x;
    const long long s = sweep_wg_sum(sweep_rows(cnt, cap, pend, ch, nch), s_w);
    if (threadIdx.x == 0) blk_sum[blockIdx.x] = s;
}

// offsets[ch], ch < nch: P_{ch-1} (saturated at INT_MAX; exact for every taken channel and for the first one not taken, whose value is the
// number of rows taken -- the host copies it over the channels behind it).  offsets[nch] = P_{nch-1}, saturated; *pending the same in 64 bits.
// blk_taken[b]: taken channels of workgroup b (a prefix of it).  ovf[ch] = 1 iff ch is taken and has `ovbit` set in its overflow word.
__global__ __launch_bounds__(SWEEP_W) void k_sweep_offsets(const int *__restrict__ cnt, int cap, const int *__restrict__ pend, int nch,
                                                           const long long *__restrict__ blk_sum, long long caprows, const int *__restrict__ ovword, int ovbit, int *__restrict__ offsets,
                                                           int *__restrict__ blk_taken, long long *__restrict__ pending, unsigned char *__restrict__ ovf)
{
    __shared__ long long s_w[4];
    const int t = threadIdx.x, b = blockIdx.x, ch = b * SWEEP_W + t;
    long long part = 0;
    for (int k = t; k < b; k += SWEEP_W) part += blk_sum[k];
    const long long base = sweep_wg_sum(part, s_w);
    // inclusive scan of v over the workgroup
    const int v = sweep_rows(cnt, cap, pend, ch, nch);
    int incl = v;
    for (int d = 1; d < 64; d <<= 1)
    {
        const int u = __shfl_up(incl, d, 64);
        if ((t & 63) >= d) incl += u;
    }
    __syncthreads();
    if ((t & 63) == 63) s_w[t >> 6] = incl;
    __syncthreads();
    long long wbase = 0;
    for (int w = 0; w < (t >> 6); w++) wbase += s_w[w];
    const long long P = base + wbase + incl, excl = P - v;
    const bool taken = ch < nch && P <= caprows;
    if (ch < nch)
    {
        offsets[ch] = excl > 0x7fffffffll ? 0x7fffffff : (int)excl;
        ovf[ch] = (taken && (ovword[ch] & ovbit)) ? 1 : 0;
        if (ch == nch - 1)
        {
            offsets[nch] = P > 0x7fffffffll ? 0x7fffffff : (int)P;
            *pending = P;
        }
    }
    const long long ntaken = sweep_wg_sum(taken ? 1 : 0, s_w);
    if (t == 0) blk_taken[b] = (int)ntaken;
}

// CH = bytes per chunk (16: uint4, 8: uint2); rowbytes is a multiple of it and every channel's buffer is aligned to it
template <int CH> struct SweepChunk;
template <> struct SweepChunk<16> { using T = uint4; };
template <> struct SweepChunk<8> { using T = uint2; };

template <int CH>
__global__ __launch_bounds__(SWEEP_W) void k_sweep_gather(const char *__restrict__ base, int *__restrict__ cnt, int cap, int rowbytes, int nch,
                                                          const int *__restrict__ offsets, const int *__restrict__ blk_taken, char *__restrict__ out,
                                                          int *__restrict__ ovword, int ovbit)
{
    using T = typename SweepChunk<CH>::T;
    __shared__ int s_off[SWEEP_W + 1];
    const int t = threadIdx.x, ch0 = blockIdx.x * SWEEP_W, ch = ch0 + t;
    const int tk = blk_taken[blockIdx.x]; // <= SWEEP_W and ch0 + tk <= nch (k_sweep_offsets)
    if (tk <= 0) return;                  // the whole workgroup
    if (t < tk)
    {
        const int o = offsets[ch];
        s_off[t] = o;
        if (t == tk - 1) s_off[tk] = o + sweep_rows(cnt, cap, nullptr, ch, nch);
    }
    __syncthreads();
    const int cpr = rowbytes / CH; // chunks per row
    const long long c_first = (long long)s_off[0] * cpr, nchunks = (long long)(s_off[tk] - s_off[0]) * cpr;
    for (long long q = t; q < nchunks; q += SWEEP_W)
    {
        const long long gq = c_first + q;
        const int row = (int)(gq / cpr), part = (int)(gq - (long long)row * cpr);
        // the last i < tk with s_off[i] <= row: channels without rows share their offset with the next one and are passed over
        int lo = 0, hi = tk;
        while (hi - lo > 1)
        {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= row) lo = mid; else hi = mid;
        }
        const char *src = base + ((size_t)(ch0 + lo) * cap + (size_t)(row - s_off[lo])) * rowbytes + (size_t)part * CH;
        *(T *)(out + (size_t)gq * CH) = *(const T *)src;
    }
    __syncthreads();
    if (t < tk)
    {
        cnt[ch] = 0;
        const int ov = ovword[ch];
        if (ov & ovbit) ovword[ch] = ov & ~ovbit;
    }
}

// Rows of one int16.  The workgroup's taken channels own the output elements [e0, e1) = [s_off[0], s_off[tk]); thread t handles the 16-byte
// output words w0 + t, w0 + t + 256, .. that meet the range (word w = elements [8 w, 8 w + 8)).  A word that lies inside the range is
// gathered element by element -- each element's channel is the last i with s_off[i] <= e, so channels without rows between two others are
// passed over and a word may hold several channels' elements -- and stored with one vector store.  The first and the last word of the range
// may hold a neighbouring workgroup's elements as well: those two are stored element by element, this workgroup's elements only, so no two
// workgroups ever store to the same address.  tests/test_bank_read_all_model.py restates this map in numpy and checks that every element
// is written exactly once.  Source loads are 2-byte loads.
// Epilogue: count 0 (pend == null) or the pending tail moved to the front of the row and the count set to its length (a burst bank's soft
// bits, as k_burst_keep_tail); the overflow bit of the class cleared.  `out` is 16-byte aligned.
__device__ __forceinline__ int sweep_owner(const int *s_off, int tk, int e)
{
    int lo = 0, hi = tk;
    while (hi - lo > 1)
    {
        const int mid = (lo + hi) >> 1;
        if (s_off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}
__global__ __launch_bounds__(SWEEP_W) void k_sweep_gather_i16(int16_t *__restrict__ base, int *__restrict__ cnt, int cap, const int *__restrict__ pend, int nch,
                                                              const int *__restrict__ offsets, const int *__restrict__ blk_taken, int16_t *__restrict__ out,
                                                              int *__restrict__ ovword, int ovbit)
{
    __shared__ int s_off[SWEEP_W + 1];
    const int t = threadIdx.x, ch0 = blockIdx.x * SWEEP_W, ch = ch0 + t;
    const int tk = blk_taken[blockIdx.x]; // <= SWEEP_W and ch0 + tk <= nch (k_sweep_offsets)
    if (tk <= 0) return;                  // the whole workgroup
    int v = 0;
    if (t < tk)
    {
        const int o = offsets[ch];
        v = sweep_rows(cnt, cap, pend, ch, nch);
        s_off[t] = o;
        if (t == tk - 1) s_off[tk] = o + v;
    }
    __syncthreads();
    const int e0 = s_off[0], e1 = s_off[tk];
    const int w0 = e0 >> 3, w1 = ((e1 - 1) >> 3) + 1; // (no e + 7: e1 may be INT_MAX)
    for (int w = w0 + t; w < w1; w += SWEEP_W)
    {
        const int lo = max(w << 3, e0), hi = (w << 3) + min(8, e1 - (w << 3));
        if (lo >= hi) continue; // (e0 == e1: nothing to move)
        int i = sweep_owner(s_off, tk, lo);
        if (hi - lo == 8)
        {
            unsigned short h[8];
#pragma unroll
            for (int k = 0; k < 8; k++)
            {
                const int e = lo + k;
                if (e >= s_off[i + 1]) i = sweep_owner(s_off, tk, e);
                h[k] = (unsigned short)base[(size_t)(ch0 + i) * cap + (size_t)(e - s_off[i])];
            }
            uint4 q;
            q.x = h[0] | ((unsigned)h[1] << 16); q.y = h[2] | ((unsigned)h[3] << 16);
            q.z = h[4] | ((unsigned)h[5] << 16); q.w = h[6] | ((unsigned)h[7] << 16);
            *(uint4 *)(out + ((size_t)w << 3)) = q;
        }
        else
            for (int e = lo; e < hi; e++)
            {
                if (e >= s_off[i + 1]) i = sweep_owner(s_off, tk, e);
                out[e] = base[(size_t)(ch0 + i) * cap + (size_t)(e - s_off[i])];
            }
    }
    __syncthreads();
    if (t < tk)
    {
        int left = 0;
        if (pend)
        {
            // the tail behind the v rows taken: at most one group (< 64 entries, k_burst_keep_tail); ascending, the destination never ahead of the source
            int c = cnt[ch];
            c = c < 0 ? 0 : (c > cap ? cap : c);
            left = c - v;
            int16_t *row = base + (size_t)ch * cap;
            if (v > 0) for (int k = 0; k < left; k++) row[k] = row[v + k];
        }
        cnt[ch] = left;
        const int ov = ovword[ch];
        if (ov & ovbit) ovword[ch] = ov & ~ovbit;
    }
}

// The link: mark[ch] = 2 | value of the channel's last DataCarrierDetect emission since the last run (0: none), written by the event helpers
// (aerol_event / cc_event with kind 0).  One lane per channel moves it into the demodulator bank's flag word and clears it.
__global__ void k_dcd_link(int *__restrict__ mark, int *__restrict__ flags, int nch, int dcd_bit)
{
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nch) return;
    const int m = mark[ch];
    if (!m) return;
    flags[ch] = (flags[ch] & ~dcd_bit) | ((m & 1) ? dcd_bit : 0);
    mark[ch] = 0;
}
