// lnr_host_util.h -- host-side utilities of lnr_api.hip (included there, after lnr_kernels.hip: one translation unit): owning wrappers of
// device / pinned memory, streams, events and event timers, the kernel-driven small copies, the error text and the error macros.
#pragma once

namespace {

// Counter of the (re)allocations of the thread's current batch: filter_dev points it at its lane's counter, so that with two lanes
// every lane counts its own (an allocation in a timed step is a device-wide stall; LNR_DEBUG_TIMES prints the count)
thread_local std::atomic<unsigned> *t_allocs = nullptr;
struct AllocCount {     // (nests: the capacity re-run calls filter_dev from inside filter_dev)
    std::atomic<unsigned> *prev;
    explicit AllocCount(std::atomic<unsigned> *c) : prev(t_allocs) { t_allocs = c; }
    ~AllocCount() { t_allocs = prev; }
};

struct NoCopy { NoCopy() = default; NoCopy(const NoCopy &) = delete; NoCopy &operator=(const NoCopy &) = delete; };

struct DevBuf : NoCopy {
    void *p = nullptr;
    size_t cap = 0;
    bool ensure(size_t bytes) {
        if (bytes <= cap && p) return true;
        if (t_allocs) ++*t_allocs;
        bool grown = p != nullptr;          // a buffer that had to grow once gets half as much again: batch-dependent sizes creep, and
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }   // re-allocating GBs in the middle of a run costs hundreds of ms
        size_t nc = bytes + (grown ? bytes / 2 : bytes / 8) + 4096;
        if (hipMalloc(&p, nc) != hipSuccess) { p = nullptr; cap = 0; (void)hipGetLastError(); return false; }
        cap = nc;
        return true;
    }
    // pinned host staging for uploads into this buffer: a copy from pageable memory is staged by the runtime and was
    // measured to block the host for ~7 ms now and then; from pinned memory it is a plain asynchronous DMA
    void *hp = nullptr;
    size_t hcap = 0;
    void *host_stage(size_t bytes) {
        if (bytes <= hcap && hp) return hp;
        if (t_allocs) ++*t_allocs;
        if (hp) { (void)hipHostFree(hp); hp = nullptr; hcap = 0; }
        size_t nc = bytes + bytes / 8 + 4096;
        if (hipHostMalloc(&hp, nc, hipHostMallocDefault) != hipSuccess) { hp = nullptr; hcap = 0; (void)hipGetLastError(); return nullptr; }
        hcap = nc;
        return hp;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; if (hp) (void)hipHostFree(hp); hp = nullptr; hcap = 0; }
    ~DevBuf() { release(); }
    template <class T> T *as() const { return (T *)p; }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(hp, o.hp); std::swap(hcap, o.hcap); }
};

// pinned host staging (device-to-host copies from pageable memory run at a fraction of the link rate)
struct PinBuf : NoCopy {
    void *p = nullptr;
    size_t cap = 0;
    bool ensure(size_t bytes) {
        if (bytes <= cap && p) return true;
        bool grown = p != nullptr;
        if (t_allocs) ++*t_allocs;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        size_t nc = bytes + (grown ? bytes / 2 : bytes / 8) + 4096;
        if (hipHostMalloc(&p, nc, hipHostMallocDefault) != hipSuccess) { p = nullptr; cap = 0; (void)hipGetLastError(); return false; }
        cap = nc;
        return true;
    }
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    template <class T> T *as() const { return (T *)p; }
};

// A stream / an event that is destroyed with its owner; both read as the plain handle.  A stream is drained before it goes.
struct Stream : NoCopy {
    hipStream_t s = nullptr;
    bool create(int prio = 0) {     // non-blocking; prio != 0: a priority of its own (see lane_create)
        hipError_t e = prio ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio) : hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (e != hipSuccess) { s = nullptr; (void)hipGetLastError(); }
        return e == hipSuccess;
    }
    void sync() const { if (s) (void)hipStreamSynchronize(s); }
    ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    operator hipStream_t() const { return s; }
};
struct Event : NoCopy {
    hipEvent_t e = nullptr;
    hipError_t create() { hipError_t r = e ? hipSuccess : hipEventCreateWithFlags(&e, hipEventDisableTiming); if (r != hipSuccess) e = nullptr; return r; }   // (no timing: ordering only)
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};
struct Timer : NoCopy {
    hipEvent_t a = nullptr, b = nullptr;
    void init() { if (!a) (void)hipEventCreate(&a); if (!b) (void)hipEventCreate(&b); }
    ~Timer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    void start(hipStream_t s) { (void)hipEventRecord(a, s); }
    void stop(hipStream_t s) { (void)hipEventRecord(b, s); }
    double ms() { float f = 0; if (hipEventSynchronize(b) != hipSuccess) return 0; (void)hipEventElapsedTime(&f, a, b); return f; }
};

// Copy launches of the thread's current batch (LNR_DEBUG_TIMES prints the count: filter_dev resets it)
thread_local unsigned t_copy_launches = 0;

// Up to COPY_SEGS copies of 32-bit words, either side of each pinned host memory, as one single-wave kernel's loads and stores on
// stream st (k_words_out).  add() collects, flush() launches; a ninth add launches the eight before it.
struct CopyBatch {
    lnr::CopySegs S{};
    u32 wgs = 0;
    hipError_t add(void *dst, const void *src, u64 nw, hipStream_t st) {
        if (!nw) return hipSuccess;
        if (S.n == COPY_SEGS) { hipError_t e = flush(st); if (e != hipSuccess) return e; }
        wgs += (u32)std::min<u64>((nw + 63) / 64, 2048);      // (a wave per 64 words, at most 2048 per copy: they loop)
        S.s[S.n] = {(const u32 *)src, (u32 *)dst, nw};
        S.wg_end[S.n++] = wgs;
        return hipSuccess;
    }
    hipError_t flush(hipStream_t st) {
        if (!S.n) return hipSuccess;
        hipLaunchKernelGGL(lnr::k_words_out, dim3(wgs), dim3(64), 0, st, S);
        t_copy_launches++;
        S.n = 0; wgs = 0;
        return hipGetLastError();
    }
};
// one copy, one launch
static inline hipError_t copy_words(void *dst, const void *src, u64 nw, hipStream_t st) {
    CopyBatch cb;
    (void)cb.add(dst, src, nw, st);
    return cb.flush(st);
}

// Device-to-host readbacks of the batch pipeline (counts, flags: a few MB per batch) land in pinned memory and are copied out
// after the stream sync.  They are written there by a kernel's stores, not by a DMA copy: while the copy stream uploads the next
// batch (lnr_filter_submit, 1 GB, 18 ms) a DMA readback on the compute stream was measured to queue behind that upload -- the
// seed stage took 24 ms instead of 6.7 -- and a copy into pageable memory is staged by the runtime on top of that.
// The adds of one round trip go through one launch: flush(st) before the stream sync, finish() after it.
struct Readback {
    struct Item { void *dst; size_t off, bytes; };
    PinBuf *pin = nullptr;
    std::vector<Item> items;
    size_t used = 0;
    CopyBatch cb;
    bool begin(PinBuf &p, size_t total) { pin = &p; items.clear(); used = 0; return p.ensure(total + 64 * 8); }
    hipError_t add(void *dst, const void *dsrc, size_t bytes, hipStream_t st) {   // bytes: a multiple of 4, dsrc 4-byte aligned
        size_t o = (used + 15) & ~(size_t)15;
        used = o + bytes;
        items.push_back({dst, o, bytes});
        return cb.add((char *)pin->p + o, dsrc, bytes / 4, st);
    }
    hipError_t flush(hipStream_t st) { return cb.flush(st); }
    void finish() { for (auto &i : items) if (i.bytes) memcpy(i.dst, (char *)pin->p + i.off, i.bytes); }
};

static const u64 SEQ_PAD = 64;
static inline u64 align_up(u64 v, u64 a) { return (v + a - 1) / a * a; }

// An error text.  The context's is written and read by the caller's thread; a lane's by whoever computes on the lane (a worker, or the
// caller's thread with nothing in flight) and copied out by the caller's thread.  Assignments are serialised, and lnr_last_error hands
// out a copy that only the caller's thread touches.
struct ErrText {
    std::mutex m;
    std::string s, shown;
    ErrText &operator=(const std::string &v) { std::lock_guard<std::mutex> g(m); s = v; return *this; }
    ErrText &operator=(const char *v) { std::lock_guard<std::mutex> g(m); s = v; return *this; }
    std::string get() { std::lock_guard<std::mutex> g(m); return s; }
    const char *show() { std::lock_guard<std::mutex> g(m); shown = s; return shown.c_str(); }
};

// Error macros: the failing function returns a status and leaves the text in `err` -- ctx->err in code that runs for the context
// (HIPCK, ENSURE, KCHECK), L->err in the batch pipeline, which runs on a lane (LCK, LENSURE, LKCHECK).
#define HIPCK_TO(err, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { char b_[256]; snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
                                 (err) = b_; (void)hipGetLastError(); return LNR_ERR_HIP; } } while (0)
#define ENSURE_TO(err, buf, bytes) do { if (!(buf).ensure(bytes)) { char b_[160]; snprintf(b_, sizeof b_, "device allocation of %zu bytes failed (%s:%d)", (size_t)(bytes), __FILE__, __LINE__); \
                                        (err) = b_; return LNR_ERR_NOMEM; } } while (0)
#define HIPCK(call) HIPCK_TO(ctx->err, call)
#define ENSURE(buf, bytes) ENSURE_TO(ctx->err, buf, bytes)
#define KCHECK() HIPCK(hipGetLastError())
#define LCK(call) HIPCK_TO(L->err, call)
#define LENSURE(buf, bytes) ENSURE_TO(L->err, buf, bytes)
#define LKCHECK() LCK(hipGetLastError())
#define HIPCK_CTX(c, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) { (c)->err = std::string(#call) + ": " + hipGetErrorString(e__); return LNR_ERR_HIP; } } while (0)

// v into b through b's pinned staging, as a kernel's loads (same reason as Readback: a DMA copy on the compute stream queues behind the
// copy stream's upload of the next batch): collected in cb, on the stream the caller flushes cb on
template <class T>
lnr_status upload_to(ErrText &err, DevBuf &b, const std::vector<T> &v, CopyBatch &cb, hipStream_t st) {
    ENSURE_TO(err, b, std::max<size_t>(v.size() * sizeof(T), 16));
    if (!v.empty()) {
        void *h = b.host_stage(v.size() * sizeof(T));
        if (!h) { err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
        memcpy(h, v.data(), v.size() * sizeof(T));
        HIPCK_TO(err, cb.add(b.p, h, (v.size() * sizeof(T) + 3) / 4, st));
    }
    return LNR_OK;
}
// (one array, one launch)
template <class T>
lnr_status upload_on(ErrText &err, DevBuf &b, const std::vector<T> &v, hipStream_t st) {
    CopyBatch cb;
    lnr_status s = upload_to(err, b, v, cb, st);
    if (s != LNR_OK) return s;
    HIPCK_TO(err, cb.flush(st));
    return LNR_OK;
}

// host-side lap timer (LNR_DEBUG_TIMES=1 prints where the host thread spends the step)
struct Laps {
    bool on; std::chrono::steady_clock::time_point t0, t; std::string out;
    Laps() : on(getenv("LNR_DEBUG_TIMES") != nullptr) { t0 = t = std::chrono::steady_clock::now(); }
    void lap(const char *name) {
        if (!on) return;
        auto n = std::chrono::steady_clock::now();
        char b[96]; snprintf(b, sizeof b, " %s %.2f", name, std::chrono::duration<double, std::milli>(n - t).count());
        out += b; t = n;
    }
    void done() { if (on) fprintf(stderr, "[lnr] host laps (ms):%s | total %.2f\n", out.c_str(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); }
};

// memcpy of a large block by a few threads (a pageable source is first copied into pinned staging; one thread moves ~10 GB/s)
void par_memcpy(void *dst, const void *src, size_t len) {
    const size_t MIN = 4u << 20;
    unsigned T = (unsigned)std::min<size_t>(4, len / MIN);
    if (T < 2) { memcpy(dst, src, len); return; }
    std::vector<std::thread> th;
    size_t per = ((len + T - 1) / T + 63) & ~(size_t)63;          // (rounded UP before the alignment: T shares of len / T rounded down can end up to T - 1 bytes short of len)
    for (unsigned t = 1; t < T; t++) {
        size_t o = (size_t)t * per, l = o < len ? std::min(per, len - o) : 0;
        if (l) th.emplace_back([=]() { memcpy((char *)dst + o, (const char *)src + o, l); });
    }
    memcpy(dst, src, std::min(per, len));
    for (auto &t : th) t.join();
}

// restores the caller's current device when an entry point returns (a context may live on another device than the one the
// caller's own HIP / torch code is using)
struct DevGuard {
    int prev = -1;
    explicit DevGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); else prev = -1; }
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace
