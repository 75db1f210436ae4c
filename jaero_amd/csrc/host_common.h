// host_common.h -- host plumbing every bank shares (included by jaero_hip.hip after fail / HIPCHK): device memory with one owner, the device
// check, the handle base (stream ordering, quiesce, poison), row drains and overflow reports of the read entry points, HIP-event kernel timing, the carry-over copies of a rate change, and the
// host-built tables the banks upload.
#pragma once

// ------------------------------------------------------------------------------------------ device memory
// The device allocations of one owner (a bank, a C-channel state, a call's scratch), freed when it is destroyed.  Move-only: std::swap of two
// banks swaps what they own.
struct DevMem
{
    std::vector<void *> ptrs;
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    DevMem(DevMem &&o) noexcept { ptrs.swap(o.ptrs); }
    DevMem &operator=(DevMem &&o) noexcept { ptrs.swap(o.ptrs); return *this; }
    ~DevMem() { for (void *q : ptrs) hipFree(q); }
};

template <class T>
static int dalloc(DevMem &m, T **ptr, size_t count, bool zero = true)
{
    void *q = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(JAERO_ENOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    m.ptrs.push_back(q);
    if (zero) { e = hipMemset(q, 0, bytes); if (e != hipSuccess) return fail(JAERO_EHIP, "hipMemset failed: %s", hipGetErrorString(e)); }
    *ptr = (T *)q;
    return 0;
}
// inside a function that returns its rc: the allocation or the reason it failed
#define DA(m, ptr, count) do { if ((rc = dalloc((m), &(ptr), (size_t)(count)))) return rc; } while (0)

// hipSetDevice on a gfx950 device, or ENODEV
static int open_device(int device, hipDeviceProp_t *prop_out = nullptr)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(JAERO_ENODEV, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(JAERO_ENODEV, "device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(JAERO_ENODEV, "device %d is %s; libjaero_hip is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    if (prop_out) *prop_out = prop;
    return 0;
}

// ------------------------------------------------------------------------------------------ device handles
// What every handle that enqueues work keeps (banks, channeliser front ends, rate meters): its device, the stream of its last write, and
// whether a call that advances state failed part-way -- host mirror and device state then disagree, and the handle accepts nothing but its
// destroy: setters would change a state nobody can continue from, readers would hand out half-written outputs without saying so.
struct DevHandle
{
    int device = 0;
    hipStream_t last_stream = nullptr;
    hipEvent_t order_ev = nullptr; // order_behind's, made by the first change of stream
    bool poisoned = false;

    // Work enqueued on `st` is ordered behind everything the handle enqueued before (on last_stream), and `st` becomes last_stream: the rule
    // for every entry point that takes a caller stream and touches device state.  A discard on stream X followed by a call that synchronises
    // last_stream only must not read the counters before the discard lands.
    int order_behind(hipStream_t st)
    {
        if (st != last_stream)
        {
            if (!order_ev) HIPCHK(hipEventCreateWithFlags(&order_ev, hipEventDisableTiming));
            HIPCHK(hipEventRecord(order_ev, last_stream));
            HIPCHK(hipStreamWaitEvent(st, order_ev, 0));
        }
        last_stream = st;
        return 0;
    }
    // everything enqueued so far has run: what control-plane calls and readers wait for
    int quiesce() const
    {
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamSynchronize(last_stream));
        return 0;
    }
    // the destroy functions' prologue: cannot fail, and the owner is deleted behind it
    void teardown()
    {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(last_stream);
        if (order_ev) (void)hipEventDestroy(order_ev);
        order_ev = nullptr;
    }
};
#define QUIESCE(h) do { if (const int rc_ = (h)->quiesce()) return rc_; } while (0)

// Raises `poisoned` where the first step that advances state is about to be enqueued; only commit() lowers it, so every early return in
// between leaves the handle poisoned.  (The test hooks that leave a handle where no write would set the flag and never lower it.)
struct PoisonGuard
{
    DevHandle &h;
    explicit PoisonGuard(DevHandle &handle) : h(handle) { h.poisoned = true; }
    void commit() { h.poisoned = false; }
};

// how the refusal of a poisoned handle words the object: "<who>: an earlier <write> failed part-way; destroy <it> and create a new one"
struct PoisonWords { const char *write, *it; };
static const PoisonWords POISON_BANK = {"jaero_write of this bank", "the bank"}, POISON_LINKED_BANK = {"jaero_write of the bank", "it"},
                         POISON_CHAN = {"write of this channeliser", "it"}, POISON_SPLIT = {"write of this splitter", "it"},
                         POISON_RATE = {"write of this rate meter", "it"};
#define POISONCHK(h, who, words) do { if ((h) && (h)->poisoned) return fail(JAERO_EHIP, "%s: an earlier %s failed part-way; destroy %s and create a new one", who, (words).write, (words).it); } while (0)

// ------------------------------------------------------------------------------------------ outputs
// One channel's rows of a per-channel output buffer: channel ch's rows start at base + ch * cap * rowbytes, its row count is cnt[ch].
struct RowBuf
{
    void *base;
    int *cnt;
    int cap;
    size_t rowbytes;
};

// The read entry points: hands the oldest min(count - pending, caprows) rows of channel ch to the caller and moves the rest (the `pending` ones
// included: burst soft bits not yet emitted) to the front of the channel's buffer, through the host.  Arguments are checked before any copy.
static int drain_rows(const char *who, int device, hipStream_t st, int nch, const RowBuf &b, int ch, void *rows, int caprows, int *nrows,
                      const int *pending = nullptr)
{
    if (!rows || !nrows || ch < 0 || ch >= nch || caprows < 0) return fail(JAERO_EINVAL, "%s: bad arguments", who);
    if (!b.base || !b.cnt) return fail(JAERO_EINVAL, "%s: this output was not enabled at create (or does not exist for this kind)", who);
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize(st));
    int cnt = 0, pend = 0;
    int *dcnt = b.cnt + ch;
    HIPCHK(hipMemcpy(&cnt, dcnt, sizeof(int), hipMemcpyDeviceToHost));
    if (pending) HIPCHK(hipMemcpy(&pend, pending + ch, sizeof(int), hipMemcpyDeviceToHost));
    const int take = cnt - pend < caprows ? cnt - pend : caprows;
    char *src = (char *)b.base + (size_t)ch * b.cap * b.rowbytes;
    if (take > 0) HIPCHK(hipMemcpy(rows, src, b.rowbytes * take, hipMemcpyDeviceToHost));
    if (take < cnt)
    {
        std::vector<char> tmp(b.rowbytes * (size_t)(cnt - take));
        HIPCHK(hipMemcpy(tmp.data(), src + b.rowbytes * take, tmp.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(src, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
    }
    const int rest = cnt - take;
    HIPCHK(hipMemcpy(dcnt, &rest, sizeof(int), hipMemcpyHostToDevice));
    *nrows = take;
    return 0;
}

// Rows the kernels had to drop because the caller fell behind: `bit` of the channel's overflow word, reported once, then cleared.
static int report_overflow(int *dov, int bit, int ch)
{
    int ov = 0;
    HIPCHK(hipMemcpy(&ov, dov, sizeof(int), hipMemcpyDeviceToHost));
    if (!(ov & bit)) return 0;
    const int z = ov & ~bit;
    HIPCHK(hipMemcpy(dov, &z, sizeof(int), hipMemcpyHostToDevice));
    return fail(JAERO_EOVERFLOW, "channel %d overflowed an output buffer (flag %d); rows were dropped", ch, bit);
}

// The peek hooks: one channel's scalars of a [field][nchp] array, each to where the table says ({field, destination}; a copy per field)
template <class T, size_t N>
static int peek_fields(const T *base, size_t nchp, int ch, const std::pair<int, T *> (&table)[N])
{
    for (const auto &[f, dst] : table) HIPCHK(hipMemcpy(dst, base + (size_t)f * nchp + ch, sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------------ kernel timing
// HIP-event timing of a bank's kernel classes (jaero_profile_read, jaero_aerol_profile_read): a pool of event pairs, reused after every collect,
// and one running total per class.  begin returns -1 and records nothing while profiling is off.
struct KernelTimer
{
    struct Slot { double ms = 0; int launches = 0; };
    bool on = false;
    std::vector<Slot> slots;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    std::vector<int> used; // the class of pool[i], i < used.size()

    explicit KernelTimer(int nslots) : slots(nslots) {}
    KernelTimer(const KernelTimer &) = delete;
    KernelTimer &operator=(const KernelTimer &) = delete;
    KernelTimer(KernelTimer &&o) noexcept { swap(o); }
    KernelTimer &operator=(KernelTimer &&o) noexcept { swap(o); return *this; }
    ~KernelTimer() { for (auto &e : pool) { hipEventDestroy(e.first); hipEventDestroy(e.second); } }
    void swap(KernelTimer &o) { std::swap(on, o.on); slots.swap(o.slots); pool.swap(o.pool); used.swap(o.used); }

    int begin(int which, hipStream_t st)
    {
        if (!on) return -1;
        if (used.size() == pool.size())
        {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess) return -1;
            if (hipEventCreate(&b) != hipSuccess) { hipEventDestroy(a); return -1; }
            pool.push_back({a, b});
        }
        const int idx = (int)used.size();
        used.push_back(which);
        hipEventRecord(pool[idx].first, st);
        return idx;
    }
    void end(int idx, hipStream_t st)
    {
        if (idx >= 0) hipEventRecord(pool[idx].second, st);
    }
    void collect()
    {
        for (size_t i = 0; i < used.size(); i++)
        {
            float ms = 0;
            hipEventSynchronize(pool[i].second);
            if (hipEventElapsedTime(&ms, pool[i].first, pool[i].second) == hipSuccess) { slots[used[i]].ms += ms; slots[used[i]].launches++; }
        }
        used.clear();
    }
    int read(int device, int which, double *total_ms, int *launches, int reset)
    {
        HIPCHK(hipSetDevice(device));
        collect();
        if (total_ms) *total_ms = slots[which].ms;
        if (launches) *launches = slots[which].launches;
        if (reset) slots[which] = Slot();
        return 0;
    }
};

// ------------------------------------------------------------------------------------------ rate change
// The carry-over copies of a rate change (jaero_set_settings that re-creates the bank behind the handle): a whole buffer,
static int carry(void *dst, const void *src, size_t bytes)
{
    const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) return fail(JAERO_EHIP, "jaero_set_settings: carry-over copy failed: %s", hipGetErrorString(e));
    return 0;
}
// and the first `rows` rows of every channel into a buffer with another number of rows per channel (outputs not read yet, windows that keep
// their first entries)
static int carry_rows(void *dst, int dcap, const void *src, int scap, size_t rowbytes, int rows, int nchp)
{
    if (rows <= 0) return 0;
    const hipError_t e = hipMemcpy2D(dst, rowbytes * dcap, src, rowbytes * scap, rowbytes * rows, (size_t)nchp, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) return fail(JAERO_EHIP, "jaero_set_settings: carry-over copy failed: %s", hipGetErrorString(e));
    return 0;
}

// ------------------------------------------------------------------------------------------ host-built tables
// TrigLookUp (JAERO/DSP.cpp:11-30): generated on the host so the table bits match the reference's libm
static std::vector<double2> cis_table()
{
    std::vector<double2> cis(JD_WTSIZE);
    for (int i = 0; i < JD_WTSIZE; i++)
    {
        cis[i].y = (sin(2 * M_PI * ((double)i) / JD_WTSIZE));
        cis[i].x = (sin(M_PI_2 + 2 * M_PI * ((double)i) / JD_WTSIZE));
    }
    return cis;
}

// exp(-2 pi i k / n) for k < count
static std::vector<double2> twiddles(int n, int count)
{
    std::vector<double2> tw(count);
    for (int i = 0; i < count; i++) { double a = -2.0 * M_PI * ((double)i) / ((double)n); tw[i].x = cos(a); tw[i].y = sin(a); }
    return tw;
}

// the MSK matched filter: 2 sps taps of a half sine
static std::vector<double> half_sine_taps(int sps)
{
    const double SPS = (double)sps;
    std::vector<double> taps(2 * sps);
    for (int i = 0; i < 2 * SPS; i++) taps[i] = sin(M_PI * i / (2.0 * SPS)) / (2.0 * SPS);
    return taps;
}

// the taps twice in a row (taps2: a filter window that wraps reads on without a modulo)
static std::vector<double> doubled_taps(const std::vector<double> &taps)
{
    const size_t n = taps.size();
    std::vector<double> t2(2 * n);
    for (size_t i = 0; i < 2 * n; i++) t2[i] = taps[i % n];
    return t2;
}

// AeroLScrambler (JAERO/aerol.h:397-420): the first 5000 bits of its sequence, one per byte
static std::vector<uint8_t> scrambler_bits()
{
    std::vector<uint8_t> scr(5000);
    int state[15] = {1, 1, 0, 1, 0, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1};
    for (int k = 0; k < 5000; k++)
    {
        const int val0 = state[0] ^ state[14];
        scr[k] = (uint8_t)val0;
        for (int i = 14; i > 0; i--) state[i] = state[i - 1];
        state[0] = val0;
    }
    return scr;
}

// validate_settings: lockingbw in (0, Fs / 2] and freq_center >= 0.  The estimate's band limit keeps bins below startbin = round(lockingbw /
// hzperbin) and above nfft - startbin: past Fs / 2 the two meet, and the reference's window loop (coarsefreqestimate.cpp:61-74) then
// overwrites its own entries -- not the symmetric window the kernels apply.
static int check_tuning_range(double lockingbw, double freq_center, double Fs)
{
    if (!(lockingbw > 0) || !(freq_center >= 0)) return fail(JAERO_EINVAL, "bad lockingbw/freq_center");
    if (lockingbw > Fs / 2) return fail(JAERO_EINVAL, "lockingbw %g Hz exceeds Fs / 2 = %g Hz", lockingbw, Fs / 2);
    return 0;
}

// ------------------------------------------------------------------------------------------ the dcd link
// What the demodulator banks need to know of jaero_aerol_link_dcd (aerol_host.h keeps the links): a bank that is destroyed ends its link first,
// and a jaero_set_settings that would re-create a linked bank is refused.
struct jaero_ctx;
static void dcd_unlink_bank(jaero_ctx *b);
static bool dcd_bank_linked(const jaero_ctx *b);
#define LINKCHK(c) do { if (dcd_bank_linked(c)) return fail(JAERO_EINVAL, "jaero_set_settings: this change re-creates the bank, which is linked to an Aero-L bank (jaero_aerol_link_dcd): unlink, change, link a matching Aero-L bank"); } while (0)

// ------------------------------------------------------------------------------------------ one-call reads
// A bank's device scratch for the sweep both bank types share (jaero_aerol_read_all, jaero_read_all: sweep_host.h), allocated by its first sweep
struct SweepBufs
{
    int nblk = 0;
    size_t meta_bytes = 0, off_taken = 0, off_pending = 0, off_ovf = 0; // one block, copied to the host in one piece: offsets, taken counts, pending, flags
    char *d_meta = nullptr;
    long long *d_blk_sum = nullptr;
    char *d_pack = nullptr; size_t pack_bytes = 0;
    std::vector<char> h_meta;
    long long bytes() const { return (d_meta ? (long long)meta_bytes + (long long)sizeof(long long) * nblk : 0) + (long long)pack_bytes; }
};
