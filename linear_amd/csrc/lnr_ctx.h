// lnr_ctx.h -- who owns what behind a lnr_ctx (included by lnr_api.hip):
//   Index   the reference index, made by lnr_index_build / _alloc / _adopt with nothing in flight; the context has one, every lane reads it
//   Tuning  the LNR_* environment knobs, read once in lnr_create; never written afterwards
//   Lane    everything one filter_dev / seed_dev call works on, plus the lane's queue (guarded by lnr_ctx::mu)
//   lnr_ctx what only the caller's thread and the scheduler touch, and the two lanes
#pragma once
#include "lnr_handover.h"

struct lnr_ctx;

namespace {

struct Index {
    bool has_index = false;
    lnr_index_info info{};
    std::vector<u64> seq_len, seq_off, f2_off;
    u32 nbins = 0;
    DevBuf g, dir, hs, f2, d_seq_off, d_f2_off, d_seq_len;
    DevBuf bm, bl, ov;      // derived from dir / hs on every GPU: bm = bucket-non-empty bitmap, bl = bucket lines, ov = their aligned overflow lines (k_ix_lines)
    DevBuf hx_nkeys, hx_nvals; u32 hx_nnodes = 0; u64 hx_empty_dir = 0;   // HIndex (-i 2): dir = hdir[2^18] (head of the block of X, -1: none), hs = ysa, nodes of the large blocks
};

struct Tuning {
    size_t job_lds_bytes = 4 * 1024;    // LDS half of k_job's two-level arena (LNR_JOB_LDS_KB overrides, for tuning).  At five waves per SIMD a CU holds 20 workgroups while 2.6 KB static + the arena stay within 8 KB each (the runtime's answer: LNR_DEBUG_OCC=1); measured at five waves (profiles/r18): 6 KB = 18 workgroups, 5 KB and 4 KB = 20, and 4 KB is the fastest of them
    u32 heavy_lds_kb = 48;              // LDS arena of k_job_heavy (LNR_HEAVY_LDS_KB)
    u32 mid_cap = 6144, mid_lds_kb = 24;   // reads with at least this many anchors run on 4 waves (k_job_mid: the DP is dealt over the waves); LNR_MID_CAP, LNR_MID_LDS_KB
    u32 heavy_cap = 0xffffffffu;        // reads with at least this many anchors (after the Y filter) take the 16-wave path (LNR_HEAVY_CAP overrides)
    u32 heavy_cap_r1 = 7000, mid_cap_r1 = 3000;   // the same cuts for the re-map round (LNR_HEAVY_CAP_R1, LNR_MID_CAP_R1)
    u32 stop_after = 0;                  // diagnostic: LNR_STOP_AFTER (see JobArgs)
    u32 mid_waves = 0;                   // waves per read of the middle class (LNR_MID_WAVES=2|4; 0 = 2 in round 0 on a populated table, else 4)
    bool mid_cap_env = false;            // LNR_MID_CAP given: no density-dependent default
    int seed_bm = -1;                    // bucket bitmap in the seed kernel: -1 = by table density, 0 / 1 forced (LNR_SEED_BM)
    u32 prep_threads = 256;             // workgroup size of k_prep (LNR_PREP_THREADS: 64, 128 or 256)
    u32 prep_grid = 4096;               // workgroups of k_prep (LNR_PREP_GRID): they loop over the reads
    u32 bulk_delay_ticks = 10000;       // head start (100 MHz ticks) of the multi-wave kernels over the bulk kernel (LNR_BULK_DELAY_US)
    u32 cap_shrink = 1;     // diagnostic (LNR_CAP_SHRINK): per-read capacities / this, to exercise the capacity re-run
    u32 seed_lds_pad = 0;   // diagnostic (LNR_SEED_LDS_PAD): dynamic LDS the seed kernel does not use, to lower its waves per CU
    u32 gap_arena2_mb = 64;    // arena of a team of the first stage of the gap re-mapper (LNR_GAP_ARENA2_MB)
    u32 gap_teams = 96, ncu = 0;   // team workgroups of the first stage (k_gap_all; LNR_GAP_TEAMS); compute units of the device
    u32 gap_heavy_w = 60000;   // weight (k_gap_weight) from which a read is expected to need a team (LNR_GAP_HEAVY_W)
    u64 gap_work_cap = 3000000;   // LNR_GAP_WORK_CAP: passed to the kernels, but without effect there -- GapCtx::work is counted only by the serial host loop of gap_chain_anchors, and the kernels always take its coop branch
    u32 nlanes = 2;                     // LNR_LANES=1|2
    int lane1_prio = 1;                 // stream priority of lane 1's kernel streams: 1 = low (diagnostic: LNR_LANE1_PRIO=-1|0|1; see lane_create)
    bool lane1_nomem = false;           // diagnostic (LNR_LANE1_NOMEM=1): lane 1's first batch fails as if the device were full, to exercise that fallback
    bool handover_gate = true;          // the order of the two lanes' job launches (lnr_handover.h); LNR_HANDOVER_GATE=0 switches it off, for profiling only
    u64 gaps_spec = 0;                  // diagnostic (LNR_GAPS_SPEC=<entries>): fixes how many gap entries travel with the tail-A flags (0: the lane's sticky capacity)
};

Tuning tuning_from_env(int device) {
    Tuning t;
    if (const char *e = getenv("LNR_LANES")) { long v = atol(e); if (v == 1 || v == 2) t.nlanes = (u32)v; }
    if (const char *e = getenv("LNR_LANE1_NOMEM")) t.lane1_nomem = atoi(e) != 0;
    if (const char *e = getenv("LNR_HANDOVER_GATE")) t.handover_gate = atoi(e) != 0;
    if (const char *e = getenv("LNR_GAPS_SPEC")) { long long v = atoll(e); if (v >= 1) t.gaps_spec = (u64)v; }
    if (const char *e = getenv("LNR_LANE1_PRIO")) { long v = atol(e); if (v >= -1 && v <= 1) t.lane1_prio = (int)v; }
    if (const char *e = getenv("LNR_CAP_SHRINK")) { long v = atol(e); if (v >= 1 && v <= 4096) t.cap_shrink = (u32)v; }
    if (const char *e = getenv("LNR_GAP_TEAMS")) { long v = atol(e); if (v >= 1 && v <= 4096) t.gap_teams = (u32)v; }
    { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess) t.ncu = (u32)pr.multiProcessorCount; else (void)hipGetLastError(); }
    if (const char *e = getenv("LNR_GAP_HEAVY_W")) { long v = atol(e); if (v >= 1) t.gap_heavy_w = (u32)v; }
    if (const char *e = getenv("LNR_GAP_ARENA2_MB")) { long v = atol(e); if (v >= 1 && v <= 1024) t.gap_arena2_mb = (u32)v; }
    if (const char *e = getenv("LNR_GAP_WORK_CAP")) { long long v = atoll(e); if (v >= 0) t.gap_work_cap = (u64)v; }
    if (const char *e = getenv("LNR_SEED_LDS_PAD")) { long v = atol(e); if (v >= 0 && v <= 100000) t.seed_lds_pad = (u32)v; }
    if (const char *e = getenv("LNR_JOB_LDS_KB")) { long kb = atol(e); if (kb >= 1 && kb <= 156) t.job_lds_bytes = (size_t)kb * 1024; }
    if (const char *e = getenv("LNR_HEAVY_CAP")) { long v = atol(e); if (v >= 64) { t.heavy_cap = (u32)std::min<long>(v, 0xffffffffL); t.heavy_cap_r1 = t.heavy_cap; } }
    if (const char *e = getenv("LNR_HEAVY_LDS_KB")) { long v = atol(e); if (v >= 1 && v <= 56) t.heavy_lds_kb = (u32)v; }
    if (const char *e = getenv("LNR_MID_CAP")) { long v = atol(e); if (v >= 64) { t.mid_cap_env = true; t.mid_cap = (u32)std::min<long>(v, 0xffffffffL); t.mid_cap_r1 = t.mid_cap; } }
    if (const char *e = getenv("LNR_MID_LDS_KB")) { long v = atol(e); if (v >= 1 && v <= 56) t.mid_lds_kb = (u32)v; }
    if (const char *e = getenv("LNR_HEAVY_CAP_R1")) { long v = atol(e); if (v >= 64) t.heavy_cap_r1 = (u32)std::min<long>(v, 0xffffffffL); }
    if (const char *e = getenv("LNR_MID_CAP_R1")) { long v = atol(e); if (v >= 64) t.mid_cap_r1 = (u32)std::min<long>(v, 0xffffffffL); }
    if (const char *e = getenv("LNR_MID_WAVES")) t.mid_waves = atoi(e) == 2 ? 2 : 4;
    if (const char *e = getenv("LNR_SEED_BM")) t.seed_bm = atoi(e) ? 1 : 0;
    if (const char *e = getenv("LNR_STOP_AFTER")) { long v = atol(e); if (v >= 0 && v < 16) t.stop_after = (u32)v; }
    if (const char *e = getenv("LNR_PREP_GRID")) { long v = atol(e); if (v > 0) t.prep_grid = (u32)v; }
    if (const char *e = getenv("LNR_PREP_THREADS")) { long v = atol(e); if (v == 64 || v == 128 || v == 256) t.prep_threads = (u32)v; }
    if (const char *e = getenv("LNR_BULK_DELAY_US")) { long v = atol(e); if (v >= 0 && v <= 5000) t.bulk_delay_ticks = (u32)v * 100; }
    return t;
}

// ---- jobs: a JobSet is one seeded job list (device arrays + host mirrors), js[0] round 0 and js[1] the re-map round (each learns its
// own segment estimate and keeps its own capacities); a Launch is the per-launch state of the job kernels (order, scratch); a TailBuf
// the per-launch state of a tail kernel: tail A of the re-map round, the early and the late tail B.
struct JobSet {
    DevBuf j_read, j_str, j_end, j_mode, j_cap, j_look, j_anc_off, j_nanc, grp_beg, anchors, seed_ctl;
    std::vector<u32> cap, look, nanc;
    std::vector<u64> anc_off;
    u32 est_x16 = 64;               // anchors per sample x 16 the seed kernel sizes a job's first segment with (learned from the last batch)
    u64 cap_slots = 0;              // anchor buffer capacity (u64 slots), sticky
    Timer t_seed;
    PinBuf h_rb;
};
// (host vectors that feed asynchronous uploads live here, not on the stack: the launch functions return before the copy ran)
struct Launch { DevBuf grp_order, j_scr_off, job_scr; std::vector<u32> h_order; std::vector<u64> h_scr_off; };
struct TailBuf { DevBuf off, cap, scr, list; std::vector<u64> h_off; std::vector<u32> h_cap, h_list; };

// A batch that has been computed but not handed out yet: its status, and where its results lie on the device
struct Pre { bool valid = false; lnr_status st = LNR_OK; u32 n = 0; u64 tot = 0; lnr_stats stats; std::vector<u64> coff; const void *d_str = nullptr, *d_end = nullptr; std::string err; };
// A batch in flight on the lanes.  lnr_ctx::mu guards `done`; the other fields belong to the worker from push to `done`.
struct Ticket { int lane = 0, slot = 0, res_lane = 0, res_set = 0; bool done = false; Pre pre; };   // lane: whose input slot; res_lane: whose result set (differs after a fallback)

// One lane: everything per batch -- streams, events, input slots, job sets, scratch, result buffers, stats -- so that two lanes compute
// side by side on one index.  filter_dev / seed_dev run on a lane and reach the options, the knobs and the index through it.
struct Lane {
    const lnr_opts *opts = nullptr;     // the context's (lnr_set_gap changes them with nothing in flight)
    const Tuning *tun = nullptr;
    const Index *ix = nullptr;
    struct ::lnr_ctx *top = nullptr;    // the context: its mutex, condition variable and hand-over state (filter_dev's gate)
    int id = 0;
    ErrText err;                         // of the lane's last batch; copied into the context's when the batch is handed out
    // Kernel streams: `stream` carries seeds, tails and the 16-wave job kernel; s_spare the 4/2-wave job kernel when the 16-wave kernel is
    // in the same launch, s_bulk the single-wave job kernel (and k_f1), s_tail the early tail B of the reads that skip the re-map round.
    // With the context's copy and download streams, six per lane in use: the runtime multiplexes streams onto a few hardware queues (4 by
    // default) and two streams on one queue run their kernels back to back (measured: the bulk kernel waited for the 4-wave kernel).
    Stream stream, s_spare, s_bulk, s_tail;
    Event ev_fork, ev_join_spare, ev_join_bulk, ev_start, ev_prep, ev_f1;
    // ---- batch inputs: three input slots (one batch computed ahead + two uploads pending; lnr_filter_submit / lnr_filter_wait), filled on
    // the context's copy stream; ev_in[k] marks the end of slot k's upload
    DevBuf in_reads[3], in_off[3];
    PinBuf h_off[3];
    Event ev_in[3];
    u32 in_n[3] = {0, 0, 0};
    // a slot filled by lnr_filter_submit_dev borrows the caller's device buffers instead: nothing is uploaded, in_reads / in_off / ev_in of
    // the slot stay unused, and h_off holds the caller's host copy of the offsets when there is one (bor_hoff)
    bool borrowed[3] = {false, false, false}, bor_hoff[3] = {false, false, false};
    const u8 *bor_reads[3] = {nullptr, nullptr, nullptr};
    const u64 *bor_off[3] = {nullptr, nullptr, nullptr};
    // ---- per-read arrays
    DevBuf rlen, rks, nf, f1_off, f1, pk, nm, pk_off;
    DevBuf cords, out_str, out_end, cords_off, cords_cap, ncords, nout, read_err;
    DevBuf gaps, gaps_off, gaps_cap, ngaps, remap, gdense, gcursor, gpos;
    PinBuf h_gaps, h_flags;             // pinned staging of the tail-A results
    u64 gaps_spec_cap = 0;              // gap entries copied in the same round trip as the flags: sticky, grown by half when a batch wrote more
    JobSet js[2];
    Launch ln;
    TailBuf tb_remap, tb_early, tb_late;
    PinBuf h_rb[2];                     // pinned landing zones of the small readbacks: [0] batch offsets and the final counts, [1] the cord counts that size the tails
    DevBuf prof, tl; u32 tl_round = 0, tl_n[4] = {0, 0, 0, 0}; u32 tl_nh[4] = {0, 0, 0, 0};   // LNR_PROF builds
    // ---- the gap re-mapper (-g > 0): arenas of its workers, per-read retry flags, the work counters
    DevBuf gap_arena, gap_flag, gap_next, gap_prof, gap_first, gap_list, gap_rank, gap_weight;
    int gap_ext = 0;        // the read stream's state: 1 once a read of the stream went through mapExtend / mapExtends (lnr_gap_stream)
    // ---- results: two sets of device buffers (r_*: the one the next batch is computed into), so that a batch is computed while the one
    // before it travels to the host
    DevBuf r_off, r_str, r_end, rB_off, rB_str, rB_end;
    std::vector<u64> h_cord_off;
    std::vector<u64> last_gaps_off;      // per-read offsets into `gaps` of the last batch (capacity layout)
    u32 last_n = 0;
    u64 last_ncords = 0;
    u32 cap_scale = 1;      // per-read capacities (cords, gaps) x this: raised for the re-run of a batch in which a read overflowed
    u32 overflow_reruns = 0;
    lnr_stats stats{};
    Timer t_prep, t_job, t_tail, t_total, t_gap;
    std::atomic<unsigned> allocs{0};    // device / pinned (re)allocations made for this lane's batches
    // ---- the lane's queue (lnr_ctx::mu).  One worker thread per lane runs the synchronous filter_dev as soon as the lane has an uploaded
    // batch and a free result set; lnr_filter_wait only waits, downloads and hands out.
    std::thread th;
    std::deque<Ticket *> work;      // uploaded, not computed yet (submission order)
    bool slot_busy[3] = {false, false, false};
    u32 pending = 0;                // submitted and not computed to the end
    u32 unhanded = 0;               // computed and not handed out: each holds one of the lane's two result sets
    bool busy = false;              // a worker is inside filter_dev on this lane's state
    bool set_used[2] = {false, false};   // result sets that hold a batch not handed out yet; set_cur: the one r_off / r_str / r_end are now
    int set_cur = 0;

    bool init(int stream_prio) {
        bool ok = stream.create(stream_prio) && s_spare.create(stream_prio) && s_bulk.create(stream_prio) && s_tail.create(stream_prio);
        for (Event *e : {&ev_fork, &ev_join_spare, &ev_join_bulk, &ev_start, &ev_prep, &ev_f1, &ev_in[0], &ev_in[1], &ev_in[2]}) ok = ok && e->create() == hipSuccess;
        if (!ok) { (void)hipGetLastError(); return false; }
        t_prep.init(); t_job.init(); t_tail.init(); t_total.init(); t_gap.init();
        return true;
    }
    void sync() const { stream.sync(); s_spare.sync(); s_bulk.sync(); s_tail.sync(); }
    ~Lane() { sync(); }             // (events and buffers go before the streams do)
};

}  // namespace

struct lnr_ctx {
    lnr_opts opts;
    int device = 0;
    ErrText err;
    Index ix;
    Tuning tun;
    Stream s_copy, s_down;              // uploads / result downloads of every lane, each on a stream of its own
    Event ev_down, ev_done;
    PinBuf h_up[2]; Event ev_up[2];     // upload staging ring (pageable sources)
    // results land in pinned memory (DMA at link rate, no page faults), two result slots taken in turn: the arrays handed out stay valid
    // until the SECOND next result (a writer thread formats batch k while k + 1 runs)
    PinBuf h_cords_str2[2], h_cords_end2[2];
    std::vector<u64> h_cord_off2[2]; int res_slot = 0;
    // device results handed out by lnr_filter_wait_dev stay valid until the SECOND next wait is called, as the host arrays do.  The wait
    // takes the three buffers of the batch's result set out of the lane and puts the oldest parked ones in their place (pointer swaps: no
    // copy, no allocation once all are grown), so the lane's set is free at once -- as after a download -- and no worker ever waits for a
    // set the caller still reads.  Every wait starts by swapping the two entries: park[0] is then the expired one, park[1] the last handed out.
    struct Parked { DevBuf off, str, end; } park[2];
    std::vector<u64> h_anchor_off, h_anchors, h_gap_off, h_gap_pairs;
    lnr_stats stats_pub{};               // statistics of the batch handed out last (what lnr_last_stats reports)
    // ---- one lane at a time (-g > 0, LNR_LANES=1): batches wait in lane 0's input slots [in_head, in_head + in_count) and are computed on
    // the caller's thread; `pre` is the batch computed ahead (lnr_filter_wait computes the NEXT submitted batch while the results of the
    // one it returns travel to the host)
    Pre pre;
    int in_head = 0, in_count = 0;
    // ---- two lanes: with gap_len == 0 the batches of lnr_filter_submit are dealt in turn to two lanes that compute side by side (the
    // re-map round of batch k leaves the chip almost empty; seed lookup and round 0 of batch k + 1 fill it).  Lane 1 is made on first use.
    // `mu` guards tickets' `done`, the lanes' queues and counters.
    std::deque<std::unique_ptr<Ticket>> tickets;   // in flight, submission order (caller's thread only)
    std::mutex mu;
    std::condition_variable cv;
    bool quit = false;
    std::atomic<bool> lane1_off{false}; // lane 1 could not be set up or ran out of memory: everything is computed on lane 0 from now on
    lnr_ho::Handover ho;                // which lane is in its hand-over (mu; lnr_handover.h)
    bool lane1_nomem_test = false;      // Tuning::lane1_nomem, until lane 1's first batch has consumed it
    std::unique_ptr<Lane> lane[2];      // (last: the lanes go first, while the copy streams are still there)

    hipStream_t stream() const { return lane[0]->stream; }   // where everything outside a batch runs (index build, exports)
};

namespace {
bool in_flight(const lnr_ctx *ctx) { return ctx->in_count || ctx->pre.valid || !ctx->tickets.empty(); }
bool two_lanes(const lnr_ctx *ctx) { return ctx->tun.nlanes == 2 && ctx->opts.gap_len == 0; }
}  // namespace
