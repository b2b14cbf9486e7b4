// lnr_api.hip -- C ABI (include/linear_amd.h) of the MI355X filter hot path: context lifecycle, the lanes behind lnr_filter_submit /
// lnr_filter_wait and the entry points.  One translation unit with its headers: lnr_host_util.h (memory / stream / event wrappers, error
// macros), lnr_ctx.h (Index, Tuning, Lane, lnr_ctx), lnr_index.h (index build / adopt / broadcast), lnr_batch.h + lnr_gap_stage.h (the
// per-batch kernel pipeline).  Device code: lnr_kernels.hip + lnr_hd.h.
//
// There is no CPU execution path in this library: every stage runs in a HIP kernel, and every entry
// point fails (LNR_ERR_NO_DEVICE / LNR_ERR_HIP) when no GPU is usable.
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>   // device-wide radix sort of the HIndex build (-i 2, once per index): AMD's native primitives library, no CUB layer
#include "lnr_kernels.hip"
#include "lnr_gap_args.h"
#include "../../include/linear_amd.h"

#include <algorithm>
#include <dlfcn.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace lnr;

#include "lnr_host_util.h"
#include "lnr_ctx.h"
#include "lnr_index.h"
#include "lnr_batch.h"

namespace {

// Upload of one batch into input slot `slot` of lane L, asynchronously on the copy stream; ev_in[slot] marks its end.
// (the copy stream, the staging ring and the error text are the context's)
lnr_status submit_reads(lnr_ctx *ctx, Lane *L, int slot, const u8 *reads, const u64 *off, u32 n) {
    if (!off || (n && !reads)) { ctx->err = "null read buffer"; return LNR_ERR_ARG; }
    for (u32 i = 0; i < n; i++)
        if (off[i + 1] < off[i]) { ctx->err = "read offsets not monotone"; return LNR_ERR_ARG; }   // (before anything is sized by them)
    u64 base = off[0], total = off[n] - off[0];
    DevBuf &dr = L->in_reads[slot], &dof = L->in_off[slot];
    AllocCount count_(&L->allocs);
    ENSURE(dr, std::max<u64>(total, 16));
    ENSURE(dof, ((size_t)n + 1) * 8);
    if (!L->h_off[slot].ensure(((size_t)n + 1) * 8)) { ctx->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
    u64 *o = L->h_off[slot].as<u64>();
    for (u32 i = 0; i <= n; i++) o[i] = off[i] - base;
    hipStream_t sc = ctx->s_copy;
    if (total) {
        hipPointerAttribute_t at;
        bool pinned = hipPointerGetAttributes(&at, reads + base) == hipSuccess && at.type == hipMemoryTypeHost;
        if (!pinned) (void)hipGetLastError();
        if (pinned) {
            // the caller filled memory from lnr_host_alloc (or registered its own): one DMA at link rate, no staging copy
            HIPCK(hipMemcpyAsync(dr.p, reads + base, total, hipMemcpyHostToDevice, sc));
        } else {
            // pageable source: through two pinned staging buffers, so that the host copy of one chunk overlaps the DMA of the last
            const u64 CH = 32ULL << 20;
            for (int k = 0; k < 2; k++) {
                if (!ctx->h_up[k].ensure(CH)) { ctx->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
                HIPCK(ctx->ev_up[k].create());
            }
            // (the staging buffers and their events belong to the context: a second submit right behind the first -- two batches in flight --
            //  must wait for the first one's DMA out of a buffer as well.  An event that was never recorded reads as complete.)
            int k = 0;
            for (u64 o2 = 0; o2 < total; o2 += CH, k ^= 1) {
                u64 len = std::min<u64>(CH, total - o2);
                HIPCK(hipEventSynchronize(ctx->ev_up[k]));                // the last DMA out of this staging buffer has finished
                par_memcpy(ctx->h_up[k].p, reads + base + o2, len);
                HIPCK(hipMemcpyAsync(dr.as<u8>() + o2, ctx->h_up[k].p, len, hipMemcpyHostToDevice, sc));
                HIPCK(hipEventRecord(ctx->ev_up[k], sc));
            }
        }
    }
    HIPCK(hipMemcpyAsync(dof.p, o, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, sc));
    HIPCK(hipEventRecord(L->ev_in[slot], sc));
    L->in_n[slot] = n; L->borrowed[slot] = false;
    return LNR_OK;
}
// The same for a batch that lies on the device already (lnr_filter_submit_dev): the slot records the caller's pointers, nothing is
// uploaded and ev_in[slot] is not used.  h_off (optional): the offsets on the host, copied now; they save prepare_batch its read-back.
lnr_status submit_borrowed(lnr_ctx *ctx, Lane *L, int slot, const u8 *d_reads, const u64 *d_off, const u64 *h_off, u32 n) {
    if (h_off) {
        for (u32 i = 0; i < n; i++)
            if (h_off[i + 1] < h_off[i]) { ctx->err = "read offsets not monotone"; return LNR_ERR_ARG; }
        if (!L->h_off[slot].ensure(((size_t)n + 1) * 8)) { ctx->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
        memcpy(L->h_off[slot].p, h_off, ((size_t)n + 1) * 8);
    }
    L->bor_reads[slot] = d_reads; L->bor_off[slot] = d_off; L->bor_hoff[slot] = h_off != nullptr;
    L->in_n[slot] = n; L->borrowed[slot] = true;
    return LNR_OK;
}

// A lane of ctx (null: it could not be set up).  Stream priority of lane 1: the runtime keeps a pool of hardware queues per priority, so
// kernel streams of another priority than lane 0's do not share a queue with them (two streams on one queue run back to back: lane 1's
// seed lookup would wait behind lane 0's 26 ms bulk kernel and the overlap would be gone).  Measured on the bench workload (ms per step;
// one lane: 43.4): same priority 46.8 -- slower than one lane --, lane 1 high 37.9, lane 1 low 35.2.  Low is the default.
std::unique_ptr<Lane> lane_create(lnr_ctx *ctx, int id) {
    std::unique_ptr<Lane> L(new (std::nothrow) Lane());
    if (!L) return nullptr;
    L->opts = &ctx->opts; L->tun = &ctx->tun; L->ix = &ctx->ix; L->top = ctx; L->id = id;
    if (!L->init(id == 1 ? ctx->tun.lane1_prio : 0)) return nullptr;
    return L;
}

// gives back the large per-batch device buffers of a lane that is switched off (its input slots and result sets stay: batches
// uploaded or computed there are still to be run / handed out)
void lane_release_batch(Lane *L) {
    for (int k = 0; k < 2; k++) { L->js[k].anchors.release(); L->js[k].cap_slots = 0; }
    L->ln.job_scr.release(); L->tb_remap.scr.release(); L->tb_early.scr.release(); L->tb_late.scr.release();
    L->pk.release(); L->nm.release(); L->f1.release(); L->cords.release(); L->out_str.release(); L->out_end.release(); L->gaps.release(); L->gdense.release();
}

// runs the batch in input slot `slot` of lane In on the state of lane C (the same lane, but for a batch lane 1 could not hold); its
// results stay on the device (P) until lnr_filter_wait hands them out
lnr_status compute_slot(Lane *C, Lane *In, int slot, Pre &P) {
    P = Pre();
    P.valid = true; P.tot = 0; P.n = In->in_n[slot];
    const bool bor = In->borrowed[slot];      // (device input of the caller's: complete before it was submitted, no upload to wait for)
    hipError_t e = bor ? hipSuccess : hipStreamWaitEvent(C->stream, In->ev_in[slot], 0);
    const u8 *d_reads = bor ? In->bor_reads[slot] : In->in_reads[slot].as<u8>();
    const u64 *d_off = bor ? In->bor_off[slot] : In->in_off[slot].as<u64>();
    const u64 *h_off = !bor || In->bor_hoff[slot] ? In->h_off[slot].as<u64>() : nullptr;
    P.st = e == hipSuccess ? filter_dev(C, d_reads, d_off, In->in_n[slot], nullptr, h_off) : LNR_ERR_HIP;
    P.err = C->err.get();
    P.stats = C->stats;
    if (P.st == LNR_OK) {
        P.tot = C->last_ncords;
        if (C->h_cord_off.size() != (size_t)P.n + 1) C->h_cord_off.assign((size_t)P.n + 1, 0);
        P.coff = C->h_cord_off;
        P.d_str = C->r_str.p; P.d_end = C->r_end.p;
    }
    return P.st;
}
// (one lane, -g > 0: the oldest submitted batch, computed on the caller's thread from inside lnr_filter_wait)
lnr_status compute_submitted(lnr_ctx *ctx) {
    int slot = ctx->in_head;
    ctx->in_head = (ctx->in_head + 1) % 3; ctx->in_count--;
    return compute_slot(ctx->lane[0].get(), ctx->lane[0].get(), slot, ctx->pre);
}

// One lane's worker: takes the lane's uploaded batches in submission order and runs each to the end (filter_dev is synchronous; the
// thread sleeps in its stream syncs).  A batch that fails parks its status in its ticket; the worker goes on with the next.
void lane_worker(lnr_ctx *top, int li) {
    Lane &Ln = *top->lane[li], &L0 = *top->lane[0];
    (void)hipSetDevice(top->device);
    std::unique_lock<std::mutex> lk(top->mu);
    // (under the lock; R.unhanded < 2, so one of the two is free.)  Into a free one of the lane's two result sets: the batch computed
    // before this one may still be waiting for its download.  The buffers change places under the lock, because lnr_filter_wait_dev takes
    // the buffers of a set that is handed out away from the lane (park_set).  Returns whether the other set has never been sized.
    auto take_set = [](Lane &R, Ticket *T) {
        T->res_set = R.set_used[0] ? 1 : 0;
        R.set_used[T->res_set] = true;
        if (T->res_set != R.set_cur) { R.r_off.swap(R.rB_off); R.r_str.swap(R.rB_str); R.r_end.swap(R.rB_end); R.set_cur = T->res_set; }
        return !R.rB_str.p && !R.set_used[T->res_set ^ 1];   // (an empty batch leaves r_str as it was: its set may hold offsets to hand out)
    };
    auto run = [&](Lane &R, Ticket *T, bool size_other) {     // T on lane R's state, with the lock released; R.busy is set
        compute_slot(&R, &Ln, T->slot, T->pre);
        if (T->pre.st == LNR_OK && size_other) {
            // the lane's first batch: size the other result set now, not in the lane's second batch (with two lanes that one is already
            // past a caller's two warm-up batches, and an allocation stalls the whole device)
            AllocCount count_(&R.allocs);
            (void)R.rB_off.ensure(R.r_off.cap); (void)R.rB_off.host_stage(R.r_off.hcap); (void)R.rB_str.ensure(R.r_str.cap); (void)R.rB_end.ensure(R.r_end.cap);
        }
    };
    for (;;) {
        // (lane 0 leaves its state to a batch that lane 1 could not hold: that batch is older than anything lane 0 has left to do
        //  but one, and lnr_filter_wait hands out in submission order)
        top->cv.wait(lk, [&] { return top->quit || (!Ln.work.empty() && (li == 1 || (Ln.unhanded < 2 && !Ln.busy && !(top->lane1_off && top->lane[1] && top->lane[1]->pending > 0))) && (li == 0 || top->lane1_off || Ln.unhanded < 2)); });
        if (top->quit) return;
        Ticket *T = Ln.work.front();
        Ln.work.pop_front();
        bool on_own = li == 0 || !top->lane1_off;
        if (on_own) {
            Ln.busy = true;
            const bool size_other = take_set(Ln, T);
            lk.unlock();
            if (li == 1 && top->lane1_nomem_test) { top->lane1_nomem_test = false; T->pre = Pre(); T->pre.valid = true; T->pre.st = LNR_ERR_NOMEM; T->pre.err = "LNR_LANE1_NOMEM: allocation failure injected"; }
            else run(Ln, T, size_other);
            lk.lock();
            Ln.busy = false;
            if (li == 1 && T->pre.st == LNR_ERR_NOMEM) {
                Ln.set_used[T->res_set] = false;
                // No room for a second lane's batch state (a workload that fits once, not twice): one lane from now on.  Lane 1's
                // buffers are given back and the batch is run again on lane 0; its input stays where it was uploaded.
                top->lane1_off = true;
                on_own = false;
                lk.unlock();
                Ln.sync();
                lane_release_batch(&Ln);
                if (getenv("LNR_DEBUG_TIMES")) fprintf(stderr, "[lnr] lane 1 out of memory: its batch runs again on lane 0, one lane from now on\n");
                lk.lock();
                top->cv.notify_all();
            }
        }
        if (!on_own) {
            top->cv.wait(lk, [&] { return top->quit || (!L0.busy && L0.unhanded < 2); });
            if (top->quit) return;
            L0.busy = true;
            const bool size_other = take_set(L0, T);
            lk.unlock();
            run(L0, T, size_other);
            lk.lock();
            L0.busy = false;
        }
        Lane &R = on_own ? Ln : L0;
        T->res_lane = on_own ? li : 0;
        T->done = true;
        Ln.slot_busy[T->slot] = false; Ln.pending--; R.unhanded++;
        top->cv.notify_all();
    }
}

// Hands a computed batch to the caller: the next of the two pinned result slots, the download of its `tot` cords (device arrays d_str /
// d_end) on stream st, `out` filled.  `after`: a stream whose work so far the download has to wait for (null: the results are complete).
// Returns with the copies enqueued; when they have finished is the caller's business (a stream sync, an event).
lnr_status hand_out(lnr_ctx *ctx, u32 n, u64 tot, std::vector<u64> &&coff, const void *d_str, const void *d_end, hipStream_t st, hipStream_t after, lnr_cords *out) {
    const int rs = ctx->res_slot;
    ctx->res_slot ^= 1;
    PinBuf &hs_ = ctx->h_cords_str2[rs], &he_ = ctx->h_cords_end2[rs];
    if (!hs_.ensure(std::max<u64>(tot * 8, 16)) || !he_.ensure(std::max<u64>(tot * 8, 16))) { ctx->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
    ctx->h_cord_off2[rs] = std::move(coff);
    if (tot) {
        if (after) { HIPCK(hipEventRecord(ctx->ev_done, after)); HIPCK(hipStreamWaitEvent(st, ctx->ev_done, 0)); }
        HIPCK(hipMemcpyAsync(hs_.p, d_str, tot * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(he_.p, d_end, tot * 8, hipMemcpyDeviceToHost, st));
    }
    out->n_reads = n; out->n_cords = tot;
    out->cord_off = ctx->h_cord_off2[rs].data(); out->cords_str = hs_.as<u64>(); out->cords_end = he_.as<u64>();
    return LNR_OK;
}

// the end of an entry point that computed on lane 0 from the caller's thread: the lane's statistics and, when it failed, its error text
lnr_status lane0_result(lnr_ctx *ctx, lnr_status st) {
    if (st != LNR_OK) ctx->err = ctx->lane[0]->err.get();
    ctx->stats_pub = ctx->lane[0]->stats;
    return st;
}

// The start of every wait, of either kind: the device result handed out by the wait before the last one expires (lnr_ctx::park).
void park_age(lnr_ctx *ctx) {
    lnr_ctx::Parked &a = ctx->park[0], &b = ctx->park[1];
    a.off.swap(b.off); a.str.swap(b.str); a.end.swap(b.end);
}
// lnr_filter_wait_dev's hand-out of a computed batch P whose result lies in (off, str, end) of a lane: those buffers go to park[0], the
// expired ones take their place in the lane (sized for this batch before, so that the lane does not allocate in its next one).
// `mu`: the lock that guards the lane's buffers against its worker (null: the lane computes on the caller's thread).
lnr_status park_set(lnr_ctx *ctx, const Pre &P, std::mutex *mu, Lane &Ln, int set, lnr_cords_dev *out) {
    lnr_ctx::Parked &K = ctx->park[0];
    const size_t nb = ((size_t)P.n + 1) * 8, cb = std::max<u64>(P.tot * 8, 16);
    if (!K.off.ensure(nb) || !K.off.host_stage(nb) || !K.str.ensure(cb) || !K.end.ensure(cb)) { ctx->err = "device allocation failed"; return LNR_ERR_NOMEM; }
    {
        std::unique_lock<std::mutex> lk;
        if (mu) lk = std::unique_lock<std::mutex>(*mu);
        const bool cur = !mu || set == Ln.set_cur;
        (cur ? Ln.r_off : Ln.rB_off).swap(K.off); (cur ? Ln.r_str : Ln.rB_str).swap(K.str); (cur ? Ln.r_end : Ln.rB_end).swap(K.end);
    }
    out->n_reads = P.n; out->n_cords = P.tot;
    out->d_cord_off = K.off.as<u64>(); out->d_cords_str = K.str.as<u64>(); out->d_cords_end = K.end.as<u64>();
    return LNR_OK;
}

// The common half of lnr_filter_submit / lnr_filter_submit_dev: picks the lane and the input slot, has `fill` put the batch there (an
// upload, or the caller's device pointers) and queues it.
template <class Fill> lnr_status submit_batch(lnr_ctx *ctx, Fill fill) {
    DevGuard dg_(ctx->device);
    if (!ctx->ix.has_index) { ctx->err = "no index"; return LNR_ERR_NO_INDEX; }
    if (ctx->in_count + (ctx->pre.valid ? 1 : 0) + ctx->tickets.size() >= 3) { ctx->err = "three batches already in flight: call lnr_filter_wait or lnr_filter_wait_dev first"; return LNR_ERR_ARG; }
    if (two_lanes(ctx)) {
        // the lanes take the batches in turn; an idle context starts with lane 0, so one batch at a time (lnr_filter_batch) never touches lane 1
        int li = (ctx->tickets.empty() || ctx->lane1_off) ? 0 : (ctx->tickets.back()->lane ^ 1);
        if (li == 1 && !ctx->lane[1]) {
            std::unique_ptr<Lane> L1 = lane_create(ctx, 1);
            if (L1) { std::lock_guard<std::mutex> g(ctx->mu); ctx->lane[1] = std::move(L1); }   // (lane 0's worker looks at lane 1's queue)
            else { ctx->lane1_off = true; li = 0; }
        }
        int slot = 0;
        for (;;) {
            Lane &Ln = *ctx->lane[li];
            { std::lock_guard<std::mutex> g(ctx->mu); slot = 0; while (slot < 2 && Ln.slot_busy[slot]) slot++; }
            lnr_status s = fill(&Ln, slot);
            if (s == LNR_ERR_NOMEM && li == 1) { ctx->lane1_off = true; li = 0; continue; }   // no room for a second lane's input: one lane from now on
            if (s != LNR_OK) return s;
            break;
        }
        Lane &Ln = *ctx->lane[li];
        if (!Ln.th.joinable()) {
            try { Ln.th = std::thread(lane_worker, ctx, li); }
            catch (...) { ctx->err = "worker thread could not be started"; return LNR_ERR_INTERNAL; }
        }
        std::unique_ptr<Ticket> T(new Ticket());
        T->lane = li; T->slot = slot;
        {
            std::lock_guard<std::mutex> g(ctx->mu);
            Ln.slot_busy[slot] = true; Ln.pending++;
            Ln.work.push_back(T.get());
        }
        ctx->tickets.push_back(std::move(T));
        ctx->cv.notify_all();
        return LNR_OK;
    }
    int slot = (ctx->in_head + ctx->in_count) % 3;
    lnr_status s = fill(ctx->lane[0].get(), slot);
    if (s != LNR_OK) return s;
    ctx->in_count++;
    return LNR_OK;
}

}  // namespace

// ======================================================================= C ABI ====
extern "C" {

void lnr_opts_default(lnr_opts *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->device = -1; o->index_type = 1; o->feature_type = 2; o->preset = 1; o->gap_len = 0; o->dup = 0; o->scratch_budget = 0;
}

const char *lnr_strerror(lnr_status s) {
    switch (s) {
        case LNR_OK: return "ok";
        case LNR_ERR_ARG: return "invalid argument";
        case LNR_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU path)";
        case LNR_ERR_HIP: return "HIP runtime error";
        case LNR_ERR_NOMEM: return "out of memory";
        case LNR_ERR_NO_INDEX: return "index not built";
        case LNR_ERR_LIMIT: return "input exceeds a format limit";
        case LNR_ERR_UNSUPPORTED: return "option not supported by this build";
        case LNR_ERR_INTERNAL: return "internal capacity overflow";
    }
    return "unknown status";
}
const char *lnr_last_error(const lnr_ctx *ctx) { return ctx ? const_cast<lnr_ctx *>(ctx)->err.show() : "null context"; }

lnr_status lnr_create(const lnr_opts *opts, lnr_ctx **out) {
    if (!out) return LNR_ERR_ARG;
    *out = nullptr;
    lnr_opts o;
    if (opts) o = *opts; else lnr_opts_default(&o);
    if ((o.index_type != 1 && o.index_type != 2) || o.feature_type != 2 || (o.preset != 1 && o.preset != 2) || o.dup > 1) return LNR_ERR_UNSUPPORTED;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return LNR_ERR_NO_DEVICE; }
    int dev = o.device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) return LNR_ERR_NO_DEVICE; }
    if (dev >= ndev) return LNR_ERR_ARG;
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    if (hipSetDevice(dev) != hipSuccess) return LNR_ERR_NO_DEVICE;
    struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore_{prev_dev == dev ? -1 : prev_dev};
    lnr_ctx *ctx = new (std::nothrow) lnr_ctx();
    if (!ctx) return LNR_ERR_NOMEM;
    ctx->opts = o;
    ctx->device = dev;
    ctx->tun = tuning_from_env(dev);
    ctx->lane1_nomem_test = ctx->tun.lane1_nomem;
    if (const char *e = getenv("LNR_DEBUG_OCC")) if (atoi(e)) {
        // what the runtime lets a CU hold of the single-wave job kernel at its launch configuration (registers, static + dynamic LDS)
        size_t lds = (ctx->tun.job_lds_bytes + 15) & ~(size_t)15;
        int nb = -1;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, lnr::k_job, 64, lds) != hipSuccess) { (void)hipGetLastError(); nb = -1; }
        fprintf(stderr, "[lnr] k_job: %d workgroups per CU at %zu B of dynamic LDS\n", nb, lds);
    }
    ctx->lane[0] = lane_create(ctx, 0);
    bool ok = ctx->lane[0] && ctx->s_copy.create() && ctx->s_down.create() && ctx->ev_down.create() == hipSuccess && ctx->ev_done.create() == hipSuccess;
    if (!ok) { (void)hipGetLastError(); lnr_destroy(ctx); return LNR_ERR_HIP; }
    *out = ctx;
    return LNR_OK;
}

void lnr_destroy(lnr_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    // batches still in flight are given up: a worker finishes the batch it is in (tens of ms) and leaves the rest
    { std::lock_guard<std::mutex> g(ctx->mu); ctx->quit = true; }
    ctx->cv.notify_all();
    for (auto &L : ctx->lane) if (L && L->th.joinable()) L->th.join();
    // (an upload into a lane's input slot, or a download out of its result set, may still be queued on the copy streams)
    ctx->s_copy.sync(); ctx->s_down.sync();
    delete ctx;       // the lanes first (each drains its streams), then the copy streams, then the index
}

lnr_status lnr_filter_batch_dev(lnr_ctx *ctx, const uint8_t *d_reads, const uint64_t *d_off, uint32_t n, lnr_cords_dev *out) {
    if (!ctx || !d_off || (n && !d_reads)) return LNR_ERR_ARG;
    DevGuard dg_(ctx->device);
    if (in_flight(ctx)) { ctx->err = "batches submitted with lnr_filter_submit are still in flight"; return LNR_ERR_ARG; }
    return lane0_result(ctx, filter_dev(ctx->lane[0].get(), d_reads, d_off, n, out));
}
lnr_status lnr_last_gaps(lnr_ctx *ctx, lnr_gaps *out) {
    if (!ctx || !out) return LNR_ERR_ARG;
    DevGuard dg_(ctx->device);
    if (!ctx->tickets.empty()) { ctx->err = "lnr_last_gaps: batches are in flight (a worker is writing the per-read arrays)"; return LNR_ERR_ARG; }
    Lane *L = ctx->lane[0].get();
    u32 n = L->last_n;
    out->n_reads = n; out->n_gaps = 0; out->gap_off = nullptr; out->gaps = nullptr;
    ctx->h_gap_off.assign((size_t)n + 1, 0);
    ctx->h_gap_pairs.clear();
    if (n && L->last_gaps_off.size() == n) {
        std::vector<u32> ng(n);
        HIPCK(hipStreamSynchronize(L->stream));
        HIPCK(hipMemcpy(ng.data(), L->ngaps.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (u32 i = 0; i < n; i++) ctx->h_gap_off[i + 1] = ctx->h_gap_off[i] + ng[i];
        ctx->h_gap_pairs.resize(2 * ctx->h_gap_off[n]);
        // the device keeps the gaps of a read at its capacity offset; gather them densely (not on the hot path)
        u64 last = L->last_gaps_off[n - 1];
        std::vector<UP> all;
        {
            // capacity of the last read: L / 1000 + 4 for reads longer than 200 (prepare_batch); copy a safe upper bound
            u64 total_cap = last + 4 + (1u << 10);
            if (total_cap * sizeof(UP) > L->gaps.cap) total_cap = L->gaps.cap / sizeof(UP);
            all.resize(total_cap);
            if (total_cap) HIPCK(hipMemcpy(all.data(), L->gaps.p, total_cap * sizeof(UP), hipMemcpyDeviceToHost));
        }
        for (u32 i = 0; i < n; i++)
            for (u32 k = 0; k < ng[i]; k++) {
                const UP &g = all[L->last_gaps_off[i] + k];
                ctx->h_gap_pairs[2 * (ctx->h_gap_off[i] + k)] = g.first; ctx->h_gap_pairs[2 * (ctx->h_gap_off[i] + k) + 1] = g.second;
            }
    }
    out->n_gaps = ctx->h_gap_off[n];
    out->gap_off = ctx->h_gap_off.data(); out->gaps = ctx->h_gap_pairs.data();
    return LNR_OK;
}
lnr_status lnr_cords_to_host(lnr_ctx *ctx, lnr_cords *out) {
    if (!ctx || !out) return LNR_ERR_ARG;
    DevGuard dg_(ctx->device);
    if (!ctx->tickets.empty()) { ctx->err = "lnr_cords_to_host: batches are in flight"; return LNR_ERR_ARG; }
    Lane *L = ctx->lane[0].get();
    u64 tot = L->last_ncords;
    if (L->h_cord_off.size() != (size_t)L->last_n + 1) L->h_cord_off.assign((size_t)L->last_n + 1, 0);
    // (lnr_filter_wait_dev took the last batch's buffers out of the lane: what stands in their place may be smaller)
    if (tot * 8 > L->r_str.cap || tot * 8 > L->r_end.cap) { ctx->err = "lnr_cords_to_host: the last batch was handed out by lnr_filter_wait_dev"; return LNR_ERR_ARG; }
    lnr_status s = hand_out(ctx, L->last_n, tot, std::vector<u64>(L->h_cord_off), L->r_str.p, L->r_end.p, L->stream, nullptr, out);
    if (s != LNR_OK) return s;
    if (tot) HIPCK(hipStreamSynchronize(L->stream));
    return LNR_OK;
}
void *lnr_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void lnr_host_free(void *p) { if (p) (void)hipHostFree(p); }

lnr_status lnr_filter_submit(lnr_ctx *ctx, const uint8_t *reads, const uint64_t *off, uint32_t n) {
    if (!ctx) return LNR_ERR_ARG;
    return submit_batch(ctx, [&](Lane *L, int slot) { return submit_reads(ctx, L, slot, reads, off, n); });
}
lnr_status lnr_filter_submit_dev(lnr_ctx *ctx, const uint8_t *d_reads, const uint64_t *d_off, const uint64_t *h_off, uint32_t n) {
    if (!ctx) return LNR_ERR_ARG;
    if (!d_off || (n && !d_reads)) { ctx->err = "null read buffer"; return LNR_ERR_ARG; }
    return submit_batch(ctx, [&](Lane *L, int slot) { return submit_borrowed(ctx, L, slot, d_reads, d_off, h_off, n); });
}
lnr_status lnr_filter_wait(lnr_ctx *ctx, lnr_cords *out) {
    if (!ctx || !out) return LNR_ERR_ARG;
    DevGuard dg_(ctx->device);
    park_age(ctx);
    if (!ctx->tickets.empty()) {
        // two lanes: the oldest batch in flight is being computed (or was) by its lane's worker; wait for it, download, hand out
        Ticket *T = ctx->tickets.front().get();
        { std::unique_lock<std::mutex> lk(ctx->mu); ctx->cv.wait(lk, [&] { return T->done; }); }
        Pre P = std::move(T->pre);
        Lane &Ln = *ctx->lane[T->res_lane];
        const int T_set = T->res_set;
        ctx->tickets.pop_front();
        // (the lane's result set is free again once the download has finished, or at once when there is nothing to download)
        struct Free { lnr_ctx *c; Lane &l; int set; ~Free() { { std::lock_guard<std::mutex> g(c->mu); l.unhanded--; l.set_used[set] = false; } c->cv.notify_all(); } } free_{ctx, Ln, T_set};
        if (P.st != LNR_OK) { ctx->err = P.err; return P.st; }
        // (filter_dev returned with the lane's streams idle: the result is complete)
        lnr_status s = hand_out(ctx, P.n, P.tot, std::move(P.coff), P.d_str, P.d_end, ctx->s_down, nullptr, out);
        if (s != LNR_OK) return s;
        if (P.tot) HIPCK(hipStreamSynchronize(ctx->s_down));
        ctx->stats_pub = P.stats;
        return LNR_OK;
    }
    if (!ctx->pre.valid) {
        if (ctx->in_count == 0) { ctx->err = "no batch in flight"; return LNR_ERR_ARG; }
        compute_submitted(ctx);
    }
    // the batch to hand out: its download starts now, on the download stream, behind what lane 0's main stream holds ...
    Pre P = std::move(ctx->pre);
    ctx->pre = Pre();
    if (P.st != LNR_OK) { ctx->err = P.err; return P.st; }
    Lane *L = ctx->lane[0].get();
    lnr_status s = hand_out(ctx, P.n, P.tot, std::move(P.coff), P.d_str, P.d_end, ctx->s_down, L->stream, out);
    if (s != LNR_OK) return s;
    HIPCK(hipEventRecord(ctx->ev_down, ctx->s_down));
    // ... and the next submitted batch is computed meanwhile, into the other set of device result buffers
    if (ctx->in_count > 0) {
        L->r_off.swap(L->rB_off); L->r_str.swap(L->rB_str); L->r_end.swap(L->rB_end);
        compute_submitted(ctx);
    }
    HIPCK(hipEventSynchronize(ctx->ev_down));
    ctx->stats_pub = P.stats;
    return LNR_OK;
}
lnr_status lnr_filter_wait_dev(lnr_ctx *ctx, lnr_cords_dev *out) {
    if (!ctx || !out) return LNR_ERR_ARG;
    DevGuard dg_(ctx->device);
    park_age(ctx);
    out->n_reads = 0; out->n_cords = 0; out->d_cord_off = nullptr; out->d_cords_str = nullptr; out->d_cords_end = nullptr;
    if (!ctx->tickets.empty()) {
        // two lanes: as lnr_filter_wait, but for the download -- the set's buffers are taken out of the lane instead (park_set), so the set is
        // free when this call returns, as it is there
        Ticket *T = ctx->tickets.front().get();
        { std::unique_lock<std::mutex> lk(ctx->mu); ctx->cv.wait(lk, [&] { return T->done; }); }
        Pre P = std::move(T->pre);
        Lane &Ln = *ctx->lane[T->res_lane];
        const int T_set = T->res_set;
        ctx->tickets.pop_front();
        struct Free { lnr_ctx *c; Lane &l; int set; ~Free() { { std::lock_guard<std::mutex> g(c->mu); l.unhanded--; l.set_used[set] = false; } c->cv.notify_all(); } } free_{ctx, Ln, T_set};
        if (P.st != LNR_OK) { ctx->err = P.err; return P.st; }
        lnr_status s = park_set(ctx, P, &ctx->mu, Ln, T_set, out);
        if (s != LNR_OK) return s;
        ctx->stats_pub = P.stats;
        return LNR_OK;
    }
    // one lane: the oldest submitted batch is computed now, unless a lnr_filter_wait before this call computed it ahead.  Nothing is
    // computed ahead here: there is no download to hide it under, and batch k + 1 is computed inside wait(k + 1) at the same cost.
    if (!ctx->pre.valid) {
        if (ctx->in_count == 0) { ctx->err = "no batch in flight"; return LNR_ERR_ARG; }
        compute_submitted(ctx);
    }
    Pre P = std::move(ctx->pre);
    ctx->pre = Pre();
    if (P.st != LNR_OK) { ctx->err = P.err; return P.st; }
    lnr_status s = park_set(ctx, P, nullptr, *ctx->lane[0], 0, out);   // (filter_dev returned with the lane's streams idle: the result in r_* is complete)
    if (s != LNR_OK) return s;
    ctx->stats_pub = P.stats;
    return LNR_OK;
}
lnr_status lnr_filter_batch(lnr_ctx *ctx, const uint8_t *reads, const uint64_t *off, uint32_t n, lnr_cords *out) {
    if (!ctx || !out) return LNR_ERR_ARG;
    if (in_flight(ctx)) { ctx->err = "batches submitted with lnr_filter_submit are still in flight"; return LNR_ERR_ARG; }
    lnr_status s = lnr_filter_submit(ctx, reads, off, n);
    if (s != LNR_OK) return s;
    return lnr_filter_wait(ctx, out);
}

lnr_status lnr_seed_lookup_batch_dev(lnr_ctx *ctx, const uint8_t *d_reads, const uint64_t *d_off, uint32_t n) {
    if (!ctx || !d_off || (n && !d_reads)) return LNR_ERR_ARG;
    DevGuard dg_(ctx->device);
    if (in_flight(ctx)) { ctx->err = "batches submitted with lnr_filter_submit are still in flight"; return LNR_ERR_ARG; }
    return lane0_result(ctx, seed_dev(ctx->lane[0].get(), d_reads, d_off, n, false, ctx->h_anchor_off, ctx->h_anchors));
}
lnr_status lnr_seed_lookup_batch(lnr_ctx *ctx, const uint8_t *reads, const uint64_t *off, uint32_t n, lnr_anchors *out) {
    if (!ctx || !out) return LNR_ERR_ARG;
    DevGuard dg_(ctx->device);
    if (!ctx->ix.has_index) { ctx->err = "no index"; return LNR_ERR_NO_INDEX; }
    if (in_flight(ctx)) { ctx->err = "batches submitted with lnr_filter_submit are still in flight"; return LNR_ERR_ARG; }
    Lane *L = ctx->lane[0].get();
    lnr_status s = submit_reads(ctx, L, 0, reads, off, n);
    if (s != LNR_OK) return s;
    HIPCK(hipStreamWaitEvent(L->stream, L->ev_in[0], 0));
    if ((s = seed_dev(L, L->in_reads[0].as<u8>(), L->in_off[0].as<u64>(), n, true, ctx->h_anchor_off, ctx->h_anchors)) != LNR_OK) { ctx->err = L->err.get(); return s; }
    ctx->stats_pub = L->stats;
    out->n_reads = n; out->n_anchors = ctx->h_anchor_off[n];
    out->anchor_off = ctx->h_anchor_off.data(); out->anchors = ctx->h_anchors.data();
    return LNR_OK;
}

#ifdef LNR_PROF
// diagnostic build only: cumulative per-phase cycle sums of k_job's lane 0 (16 counters)
// diagnostic build: timeline of launch `round` (4 x u64 per launch position); returns positions, *n_heavy = size of the heavy prefix
long long lnr_prof_timeline(lnr_ctx *ctx, unsigned round, unsigned long long *out, unsigned long long cap_positions, unsigned *n_heavy) {
    if (!ctx || round >= 4 || !ctx->lane[0]->tl.p) return -1;
    Lane *L = ctx->lane[0].get();
    unsigned long long n = L->tl_n[round] < cap_positions ? L->tl_n[round] : cap_positions;
    if (hipSetDevice(ctx->device) != hipSuccess) return -1;
    if (hipMemcpy(out, L->tl.as<unsigned long long>() + (size_t)round * (1u << 20) * 4, n * 32, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (n_heavy) *n_heavy = L->tl_nh[round];
    return (long long)n;
}
lnr_status lnr_prof_read(lnr_ctx *ctx, unsigned long long *out16) {
    if (!ctx || !out16 || !ctx->lane[0]->prof.p) return LNR_ERR_ARG;
    HIPCK(hipStreamSynchronize(ctx->stream()));
    HIPCK(hipMemcpy(out16, ctx->lane[0]->prof.p, 192 * 8, hipMemcpyDeviceToHost));
    return LNR_OK;
}
#endif

lnr_status lnr_gap_stream(lnr_ctx *ctx, int set, int *state) {
    if (!ctx || set > 1) return LNR_ERR_ARG;
    if (set >= 0 && in_flight(ctx)) { ctx->err = "lnr_gap_stream: batches are in flight (the next one may have been computed already)"; return LNR_ERR_ARG; }
    if (set >= 0) ctx->lane[0]->gap_ext = set;
    if (state) *state = ctx->lane[0]->gap_ext;
    return LNR_OK;
}

lnr_status lnr_set_gap(lnr_ctx *ctx, uint32_t gap_len, uint32_t dup) {
    if (!ctx || dup > 1) return LNR_ERR_ARG;
    if (in_flight(ctx)) { ctx->err = "lnr_set_gap: batches are in flight"; return LNR_ERR_ARG; }
    ctx->opts.gap_len = gap_len; ctx->opts.dup = dup; ctx->lane[0]->gap_ext = 0;
    return LNR_OK;
}

lnr_status lnr_last_stats(const lnr_ctx *ctx, lnr_stats *st) {
    if (!ctx || !st) return LNR_ERR_ARG;
    *st = ctx->stats_pub;
    return LNR_OK;
}

}  // extern "C"
