// sweep_host.h -- the host side of the one-call reads (k_aerol_sweep.h), shared by the Aero-L bank (jaero_aerol_read_all) and the demodulator bank
// (jaero_read_all); included by aerol_host.h, behind the banks' own kernels.  SweepBufs, the scratch a bank keeps for it, is in host_common.h.
#pragma once
#include "k_aerol_sweep.h"

// whose sweep it is: the bank's scratch, device, stream, allocations, timer and the timer class the sweep's kernels are booked under
struct SweepOwner
{
    const char *who;
    SweepBufs &w;
    int device;
    hipStream_t st;
    DevMem &mem;
    KernelTimer &timer;
    int slot;
    int nch;
};

static int sweep_prepare(const SweepOwner &o)
{
    SweepBufs &w = o.w;
    if (w.d_meta) return 0;
    int rc;
    const int nch = o.nch;
    w.nblk = (nch + SWEEP_W - 1) / SWEEP_W;
    w.off_taken = sizeof(int) * ((size_t)nch + 1);
    w.off_pending = (w.off_taken + sizeof(int) * (size_t)w.nblk + 7) / 8 * 8;
    w.off_ovf = w.off_pending + sizeof(long long);
    w.meta_bytes = w.off_ovf + (size_t)nch;
    DA(o.mem, w.d_blk_sum, w.nblk);
    DA(o.mem, w.d_meta, w.meta_bytes);
    w.h_meta.resize(w.meta_bytes);
    return 0;
}
// One log of every channel in one call.  Two synchronisations: after the offsets, after the rows.  `pending` (a burst demodulator bank's soft
// bits only): rows at the end of each channel's buffer that stay with the channel; rows of one int16 go through k_sweep_gather_i16.
static int sweep_log(const SweepOwner &o, const RowBuf &b, int *ovword, int ovbit, const int *pending, void *rows, int caprows, int *offsets,
                     int *nchannels_taken, long long *rows_pending, unsigned char *overflowed)
{
    int rc;
    HIPCHK(hipSetDevice(o.device));
    if ((rc = sweep_prepare(o))) return rc;
    SweepBufs &w = o.w;
    const int nch = o.nch;
    hipStream_t st = o.st;
    int *d_off = (int *)w.d_meta, *d_taken = (int *)(w.d_meta + w.off_taken);
    int pi = o.timer.begin(o.slot, st);
    hipLaunchKernelGGL(k_sweep_sums, dim3(w.nblk), dim3(SWEEP_W), 0, st, (const int *)b.cnt, b.cap, pending, nch, w.d_blk_sum);
    hipLaunchKernelGGL(k_sweep_offsets, dim3(w.nblk), dim3(SWEEP_W), 0, st, (const int *)b.cnt, b.cap, pending, nch, (const long long *)w.d_blk_sum,
                       (long long)caprows, (const int *)ovword, ovbit, d_off, d_taken, (long long *)(w.d_meta + w.off_pending),
                       (unsigned char *)(w.d_meta + w.off_ovf));
    o.timer.end(pi, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(w.h_meta.data(), w.d_meta, w.meta_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int *h_off = (const int *)w.h_meta.data(), *h_taken = (const int *)(w.h_meta.data() + w.off_taken);
    const unsigned char *h_ovf = (const unsigned char *)(w.h_meta.data() + w.off_ovf);
    int taken = 0;
    for (int k = 0; k < w.nblk; k++) taken += h_taken[k];
    const int total = h_off[taken]; // rows taken: P of the last taken channel (= offsets[nch] when every channel is taken)
    memcpy(offsets, h_off, sizeof(int) * (size_t)taken);
    for (int ch = taken; ch <= nch; ch++) offsets[ch] = total;
    *nchannels_taken = taken;
    if (rows_pending) memcpy(rows_pending, w.h_meta.data() + w.off_pending, sizeof(long long));
    bool any_ov = false;
    for (int ch = 0; ch < nch; ch++) any_ov |= h_ovf[ch] != 0;
    if (overflowed) memcpy(overflowed, h_ovf, (size_t)nch);
    // (a burst channel that hands over nothing keeps its tail where it is, at the front: nothing to launch for it)
    if (total > 0 || any_ov)
    {
        const size_t bytes = (size_t)total * b.rowbytes;
        if (bytes > w.pack_bytes)
        {
            // grown by half at least; the old buffer goes first (nothing is in flight: the stream was synchronised above), the new one is not zeroed
            size_t want = w.pack_bytes + w.pack_bytes / 2;
            if (want < bytes) want = bytes;
            if (w.d_pack)
            {
                for (size_t k = 0; k < o.mem.ptrs.size(); k++) if (o.mem.ptrs[k] == (void *)w.d_pack) { o.mem.ptrs.erase(o.mem.ptrs.begin() + k); break; }
                hipFree(w.d_pack);
                w.d_pack = nullptr; w.pack_bytes = 0;
            }
            if ((rc = dalloc(o.mem, &w.d_pack, want, false))) return rc;
            w.pack_bytes = want;
        }
        pi = o.timer.begin(o.slot, st);
        if (b.rowbytes == sizeof(int16_t))
            hipLaunchKernelGGL(k_sweep_gather_i16, dim3(w.nblk), dim3(SWEEP_W), 0, st, (int16_t *)b.base, b.cnt, b.cap, pending, nch, (const int *)d_off,
                               (const int *)d_taken, (int16_t *)w.d_pack, ovword, ovbit);
        else if (b.rowbytes % 16 == 0)
            hipLaunchKernelGGL(k_sweep_gather<16>, dim3(w.nblk), dim3(SWEEP_W), 0, st, (const char *)b.base, b.cnt, b.cap, (int)b.rowbytes, nch, (const int *)d_off,
                               (const int *)d_taken, w.d_pack, ovword, ovbit);
        else
            hipLaunchKernelGGL(k_sweep_gather<8>, dim3(w.nblk), dim3(SWEEP_W), 0, st, (const char *)b.base, b.cnt, b.cap, (int)b.rowbytes, nch, (const int *)d_off,
                               (const int *)d_taken, w.d_pack, ovword, ovbit);
        o.timer.end(pi, st);
        HIPCHK(hipGetLastError());
        if (bytes) HIPCHK(hipMemcpyAsync(rows, w.d_pack, bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    if (any_ov) return fail(JAERO_EOVERFLOW, "%s: channels overflowed this output buffer (flag %d) since it was last read; rows were dropped", o.who, ovbit);
    return 0;
}
