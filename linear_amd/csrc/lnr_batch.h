// lnr_batch.h -- the per-batch pipeline on one lane (included by lnr_api.hip): host tables and k_prep, seed lookup, the job kernels of
// round 0 and of the re-map round, the tails, the gap stage (lnr_gap_stage.h) and the result gather.  filter_dev is the pipeline.
#pragma once
#include "lnr_gap_stage.h"

namespace {

// ------------------------------------------------------------------ jobs ----
struct HostJobs {
    std::vector<u32> read, str, end, mode, grp_beg;
    u64 nsamp = 0;
    void add(u32 r, u32 s, u32 e, u32 m) {
        read.push_back(r); str.push_back(s); end.push_back(e); mode.push_back(m);
        nsamp += seed_num_samples(s, e, (u32)job_parm((int)m).alpha);
    }
    u32 size() const { return (u32)read.size(); }
};

struct BatchHost {
    u32 n = 0;
    std::vector<u64> off;
    std::vector<u32> len, nf, cords_cap, gaps_cap;
    std::vector<u64> f1_off, cords_off, gaps_off, pk_off;
};

JobArrays job_arrays(JobSet &S) {
    JobArrays J;
    J.read = S.j_read.as<u32>(); J.str = S.j_str.as<u32>(); J.end = S.j_end.as<u32>(); J.mode = S.j_mode.as<u32>();
    return J;
}
ReadArrays read_arrays(Lane *L) {
    ReadArrays R;
    R.len = L->rlen.as<u32>(); R.ks = L->rks.as<i32>();
    R.pk = L->pk.as<u64>(); R.nm = L->nm.as<u32>(); R.pk_off = L->pk_off.as<u64>();
    return R;
}

// Read features of the whole batch on the side stream, ordered behind whatever the main stream holds right now.  They are
// not needed before the job kernels, so filter_dev issues this right behind the round-0 seed kernel: k_f1 then runs while
// the host reads the seed counts back and prepares the launch order (the GPU would idle there), not beside the seed kernel.
lnr_status launch_f1(Lane *L, u32 n) {
    LCK(hipEventRecord(L->ev_prep, L->stream));
    LCK(hipStreamWaitEvent(L->s_bulk, L->ev_prep, 0));
    hipLaunchKernelGGL(k_f1, dim3(n), dim3(256), 0, L->s_bulk, L->pk.as<u64>(), L->nm.as<u32>(), L->pk_off.as<u64>(), L->rlen.as<u32>(), L->nf.as<u32>(), L->f1_off.as<u64>(), n,
                       L->f1.as<F96>()); LKCHECK();
    LCK(hipEventRecord(L->ev_f1, L->s_bulk));
    return LNR_OK;
}

// Seed lookup (k_seed_fused) of the job list `hj` into the job set S, on stream st.  Returns with the stream idle and the
// per-job counts (bucket entries, lookups, anchors, anchor offsets) mirrored on the host.
lnr_status seed_jobs(Lane *L, JobSet &S, const HostJobs &hj, hipStream_t st, u32 f1_reads = 0) {
    const Index &ix = *L->ix; const Tuning &tun = *L->tun;
    u32 nj = hj.size();
    S.cap.assign(nj, 0); S.look.assign(nj, 0); S.nanc.assign(nj, 0); S.anc_off.assign(nj, 0);
    if (nj == 0) return f1_reads ? launch_f1(L, f1_reads) : LNR_OK;
    lnr_status s;
    CopyBatch up;     // the five job arrays: one launch
    if ((s = upload_to(L->err, S.j_read, hj.read, up, st)) != LNR_OK) return s;
    if ((s = upload_to(L->err, S.j_str, hj.str, up, st)) != LNR_OK) return s;
    if ((s = upload_to(L->err, S.j_end, hj.end, up, st)) != LNR_OK) return s;
    if ((s = upload_to(L->err, S.j_mode, hj.mode, up, st)) != LNR_OK) return s;
    if ((s = upload_to(L->err, S.grp_beg, hj.grp_beg, up, st)) != LNR_OK) return s;
    LCK(up.flush(st));
    LENSURE(S.j_cap, (size_t)nj * 4);
    LENSURE(S.j_look, (size_t)nj * 4);
    LENSURE(S.j_nanc, (size_t)nj * 4);
    LENSURE(S.j_anc_off, (size_t)nj * 8);
    LENSURE(S.seed_ctl, 64);
    if (!S.t_seed.a) S.t_seed.init();
    JobArrays J = job_arrays(S);
    ReadArrays R = read_arrays(L);
    // anchor buffer: every job starts with a segment of est x samples slots and moves to one of twice the size when that fills
    // up, so the buffer holds the first segments plus room for the moves; a launch that runs out is repeated with twice the room
    // The capacity is sticky and generous (grown by half when a batch needs more, never shrunk): re-allocating a buffer of a few GB
    // costs ~300 ms, which one step of a benchmark paid when the estimate crept over the old allocation's slack.
    u64 first_segs = ((hj.nsamp * S.est_x16) >> 4) + (u64)nj * 194;
    u64 need_slots = first_segs * 2 + (1u << 20);
    if (need_slots > S.cap_slots) S.cap_slots = need_slots + need_slots / 2;
    u64 anc_slots = S.cap_slots;
    bool use_bm = tun.seed_bm < 0 ? ix.info.hs_len < (1ULL << 25) : tun.seed_bm != 0;
    for (int attempt = 0; ; attempt++) {
        LENSURE(S.anchors, anc_slots * 8);
        LCK(hipMemsetAsync(S.seed_ctl.p, 0, 64, st));
        SeedOutArrays O;
        O.cursor = S.seed_ctl.as<unsigned long long>(); O.overflow = (int *)(S.seed_ctl.as<char>() + 16); O.capacity = anc_slots;
        O.anchors = S.anchors.as<u64>(); O.anc_off = S.j_anc_off.as<u64>(); O.job_cap = S.j_cap.as<u32>(); O.job_look = S.j_look.as<u32>();
        O.n_anchors = S.j_nanc.as<u32>();
        S.t_seed.start(st);
        // the bucket bitmap answers lookups of empty buckets without touching the bucket lines; once most buckets hold entries
        // (human scale: 328 M entries in 67 M buckets) it is one more dependent load in front of every lookup and is skipped
        if (L->opts->index_type == 2)
            hipLaunchKernelGGL(k_seed_hindex, dim3(nj), dim3(64), 0, st, J, R, ix.hs.as<u64>(), ix.info.hs_len, ix.hx_empty_dir, ix.dir.as<i32>(), ix.hx_nkeys.as<u64>(), ix.hx_nvals.as<u32>(), ix.hx_nnodes, nj, O,
                               S.est_x16);
        else
        hipLaunchKernelGGL(k_seed_fused, dim3(nj), dim3(64), tun.seed_lds_pad, st, J, R, ix.bl.as<ulonglong2>(), use_bm ? ix.bm.as<u32>() : (const u32 *)nullptr, ix.ov.as<u64>(), nj, O, S.est_x16); LKCHECK();
        S.t_seed.stop(st);
        if (f1_reads && attempt == 0) { lnr_status fs = launch_f1(L, f1_reads); if (fs != LNR_OK) return fs; }   // (beside the seed kernel instead: measured no faster)
        int ovf = 0;
        Readback rb;
        if (!rb.begin(S.h_rb, (size_t)nj * 20 + 256)) { L->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
        LCK(rb.add(S.cap.data(), S.j_cap.p, (size_t)nj * 4, st));
        LCK(rb.add(S.look.data(), S.j_look.p, (size_t)nj * 4, st));
        LCK(rb.add(S.nanc.data(), S.j_nanc.p, (size_t)nj * 4, st));
        LCK(rb.add(S.anc_off.data(), S.j_anc_off.p, (size_t)nj * 8, st));
        LCK(rb.add(&ovf, S.seed_ctl.as<char>() + 16, 4, st));
        LCK(rb.flush(st));
        LCK(hipStreamSynchronize(st));
        rb.finish();
        if (!ovf) {                                   // only the successful launch is the stage's time
            L->stats.seed_count_ms += S.t_seed.ms();
            L->stats.seed_count_launches++;
            break;
        }
        if (attempt == 5) { L->err = "anchor buffer overflow after five resizes"; return LNR_ERR_INTERNAL; }
        anc_slots *= 2;
        S.cap_slots = anc_slots;
    }
    {   // learn the segment estimate for the next batch: 1.5 x the mean anchors per sample of this one
        u64 tot = 0;
        for (u32 j = 0; j < nj; j++) tot += S.nanc[j];
        if (hj.nsamp) {
            S.est_x16 = (u32)std::min<u64>(std::max<u64>((tot * 24) / hj.nsamp + 8, 32), 400 * 16);
        }
    }
    L->stats.jobs += nj;
    L->stats.samples += hj.nsamp;
    for (u32 j = 0; j < nj; j++) { L->stats.lookups += S.look[j]; L->stats.bucket_entries += S.cap[j] - 1; L->stats.anchors += S.nanc[j] - 1; }
    return LNR_OK;
}

// copy the raw anchors of a seeded job set to the host arrays (CSR by job)
lnr_status export_anchors(Lane *L, JobSet &S, u32 nj, std::vector<u64> &a_off, std::vector<u64> &a_vals) {
    a_off.assign((size_t)nj + 1, 0);
    for (u32 j = 0; j < nj; j++) a_off[j + 1] = a_off[j] + S.nanc[j];
    a_vals.resize(a_off[nj]);
    u64 used = 0;
    for (u32 j = 0; j < nj; j++) used = std::max<u64>(used, S.anc_off[j] + S.nanc[j]);
    std::vector<u64> all(used);
    if (used) LCK(hipMemcpy(all.data(), S.anchors.p, used * 8, hipMemcpyDeviceToHost));
    for (u32 j = 0; j < nj; j++) memcpy(a_vals.data() + a_off[j], all.data() + S.anc_off[j], (size_t)S.nanc[j] * 8);
    return LNR_OK;
}

// A lane's place in the order of the job launches (lnr_handover.h) for one filter_dev call: enter() in front of the round-0 launch, leave()
// once the round-1 launch is enqueued or known to be empty -- and on every other way out, by the destructor.  Bypassed with one lane
// (LNR_LANES=1, -g > 0, lane 1 switched off) and by LNR_HANDOVER_GATE=0.  LNR_DEBUG_TIMES=1 prints a host stamp (ms) at every phase change.
struct HandoverScope : NoCopy {
    Lane *L; lnr_ctx *c; bool on, held = false;
    explicit HandoverScope(Lane *l) : L(l), c(l->top) { on = c && c->tun.handover_gate && two_lanes(c) && !c->lane1_off; }
    void stamp(const char *what) const {
        if (held && getenv("LNR_DEBUG_TIMES")) fprintf(stderr, "[lnr] handover lane %d %s %.3f\n", L->id, what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count());
    }
    bool enter() {      // true: the lane had to wait for the other lane's hand-over to end
        if (!on || held) return false;
        lnr_ctx *cc = c;
        bool waited = lnr_ho::handover_enter(c->ho, c->mu, c->cv, L->id, [cc] { return cc->quit; });
        held = true;
        stamp(waited ? "gate-passed-after-wait" : "gate-passed");
        return waited;
    }
    void leave() {
        if (!held) return;
        stamp("handover-end");      // (before the other lane can pass)
        held = false;
        (void)lnr_ho::handover_leave(c->ho, c->mu, c->cv, L->id);
    }
    ~HandoverScope() { leave(); }
};

// Per-read job kernels for all groups of the seeded job set S (hj = its host list).  Heaviest group first (anchors that
// passed the Y filter are the work proxy), so the long tail of repeat-rich reads starts at once.  The multi-wave kernels
// are launched first: a multi-wave workgroup only finds a CU with enough free wave slots while the single-wave kernel has
// not flooded the chip (it refills every slot a finished wave frees -- a late heavy launch was measured to start only
// when the bulk kernel drained, 47 ms late).  The bulk kernel follows on s_bulk.  On return everything is enqueued and
// the main stream waits for the side streams; nothing is synchronised unless the scratch budget forces several slices.
lnr_status launch_jobs(Lane *L, JobSet &S, const HostJobs &hj, HandoverScope *gate = nullptr) {
    const Index &ix = *L->ix; const Tuning &tun = *L->tun;
    u32 ngrp = (u32)hj.grp_beg.size() - 1;
    if (ngrp == 0) return LNR_OK;
    Laps laps;
    u32 nj = hj.size();
    Launch &Lx = L->ln;
    hipStream_t sm = L->stream, sb = L->s_bulk;
    u64 budget = L->opts->scratch_budget ? L->opts->scratch_budget : (64ULL << 30);
    const std::vector<u32> &nanc = S.nanc;
    std::vector<u64> w(ngrp, 0);
    for (u32 k = 0; k < ngrp; k++) for (u32 j = hj.grp_beg[k]; j < hj.grp_beg[k + 1]; j++) w[k] += nanc[j];
    std::vector<u32> order(ngrp);   // groups, heaviest first
    {
        // counting sort by weight class (1/8-octave steps: "descending up to 9 %" is all the scheduler needs) in O(n),
        // then the small multi-wave prefix in exact order (the size-class cut below walks it)
        auto cls = [](u64 v) -> u32 {
            if (v < 8) return (u32)v;
            int lg = 63 - __builtin_clzll(v);
            return (u32)(8 * (lg - 2) + ((v >> (lg - 3)) & 7));
        };
        const u32 NCLS = 8 * 64;
        std::vector<u32> cnt(NCLS + 1, 0), gc(ngrp);
        for (u32 k = 0; k < ngrp; k++) { gc[k] = NCLS - 1 - std::min<u32>(cls(w[k]), NCLS - 1); cnt[gc[k] + 1]++; }
        for (u32 c = 0; c < NCLS; c++) cnt[c + 1] += cnt[c];
        for (u32 k = 0; k < ngrp; k++) order[cnt[gc[k]]++] = k;
        u32 nh = 0;
        while (nh < ngrp && w[order[nh]] >= std::min(std::min(tun.heavy_cap, tun.mid_cap), std::min(tun.heavy_cap_r1, tun.mid_cap_r1)) / 2) nh++;
        // (exact order only for a short prefix: at human scale every read carries > 1500 mostly random anchors, the prefix was
        // 60 % of the batch and its sort 2.3 ms of host time per step with the GPU idle; without it the class cuts are exact
        // to the 1/8 octave, which only moves a few reads between kernels)
        if (nh <= 4096) std::stable_sort(order.begin(), order.begin() + nh, [&w](u32 a, u32 b) { return w[a] > w[b]; });
    }
    Lx.h_order = order;
    laps.lap("order");
    lnr_status s;
    CopyBatch up;     // the order travels with the first slice's scratch offsets
    if ((s = upload_to(L->err, Lx.grp_order, Lx.h_order, up, sm)) != LNR_OK) return s;
    laps.lap("upload-order");
    LENSURE(Lx.j_scr_off, (size_t)nj * 8);
    std::vector<u64> &scr_off = Lx.h_scr_off;
    scr_off.assign(nj, 0);
    auto grp_scr = [&](u32 g) { u64 b = 0; for (u32 j = hj.grp_beg[g]; j < hj.grp_beg[g + 1]; j++) b += align_up(job_scratch_bytes((u64)nanc[j] + 2), 256); return b; };
    u32 g0 = 0;
    while (g0 < ngrp) {
        u64 scr = 0;
        u32 g1 = g0;
        while (g1 < ngrp) {
            u64 s2 = scr + grp_scr(order[g1]);
            if (g1 > g0 && s2 > budget) break;
            scr = s2; g1++;
        }
        u64 so = 0;
        for (u32 k = g0; k < g1; k++)
            for (u32 j = hj.grp_beg[order[k]]; j < hj.grp_beg[order[k] + 1]; j++) { scr_off[j] = so; so += align_up(job_scratch_bytes((u64)nanc[j] + 2), 256); }
        laps.lap("scr-layout");
        LENSURE(Lx.job_scr, std::max<u64>(so, 16));
        laps.lap("ensure-scr");
        {
            void *h = Lx.j_scr_off.host_stage((size_t)nj * 8);
            if (!h) { L->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
            memcpy(h, scr_off.data(), (size_t)nj * 8);
            LCK(up.add(Lx.j_scr_off.p, h, (u64)nj * 2, sm));
            LCK(up.flush(sm));
        }
        laps.lap("upload-scr");
        JobArgs A;
        A.grp_order = Lx.grp_order.as<u32>(); A.grp_beg = S.grp_beg.as<u32>(); A.J = job_arrays(S);
        A.anc_off = S.j_anc_off.as<u64>(); A.job_cap = S.j_cap.as<u32>(); A.n_anchors = S.j_nanc.as<u32>(); A.scr_off = Lx.j_scr_off.as<u64>();
        A.anchors = S.anchors.as<u64>(); A.scratch = Lx.job_scr.as<char>();
        A.read_len = L->rlen.as<u32>(); A.f1_off = L->f1_off.as<u64>(); A.nf = L->nf.as<u32>(); A.f1 = L->f1.as<F96>();
        A.g.base = ix.f2.as<F96>(); A.g.off = ix.d_f2_off.as<u64>(); A.g.nseq = ix.info.nseq;
        A.cords = L->cords.as<u64>(); A.cords_off = L->cords_off.as<u64>(); A.cords_cap = L->cords_cap.as<u32>(); A.ncords = L->ncords.as<u32>();
        A.read_err = L->read_err.as<i32>();
        A.nbins = ix.nbins; A.grp_lo = g0; A.grp_hi = g1;
        A.prof = nullptr; A.tl = nullptr; A.stop_after = tun.stop_after;
        // dynamic LDS = the job arena; the binning histogram borrows it first and sweeps the bin range in passes of that many
        // bins, so the LDS per workgroup (hence the residency of the bulk kernel) does not depend on the reference's length
        size_t lds = (tun.job_lds_bytes + 15) & ~(size_t)15;
        A.lds_bytes = (u32)lds;
        A.arena_lds = (u32)lds;
        // size classes along the (weight-descending) slice: heavy = 16 waves per read, mid = 4 waves, rest = 1 wave
        // (the re-map round leaves most of the chip idle, so it can afford wider workgroups for more of its reads)
        bool remap_round_ = nj && hj.mode[0] != 0;
        u64 hcap = remap_round_ ? tun.heavy_cap_r1 : tun.heavy_cap, mcap = remap_round_ ? tun.mid_cap_r1 : tun.mid_cap;
        // a populated table (human scale) adds ~1 500 chance anchors to every read's weight, and the 4-wave kernel holds 14 of a CU's 16
        // wave slots while it runs: fewer reads go there (measured on the GRCh38 stand-in: 6144 -> 40.0 ms, 9000 -> 38.6, 12000 -> 38.5, 20000 -> 45)
        if (!remap_round_ && !tun.mid_cap_env && ix.info.hs_len >= (1ULL << 25)) mcap = 9000;
        u32 gh = g0;                                    // [g0, gh): 16 waves per read
        while (gh < g1 && w[order[gh]] >= hcap) gh++;
        u32 gm = gh;                                    // [gh, gm): 4 (or 2) waves per read
        while (gm < g1 && w[order[gm]] >= mcap) gm++;
#ifdef LNR_PROF
        if (!L->prof.p) { if (!L->prof.ensure(192 * 8)) return LNR_ERR_NOMEM; (void)hipMemsetAsync(L->prof.p, 0, 192 * 8, sm); }
        A.prof = L->prof.as<unsigned long long>();
        // timeline: up to 4 launches of up to 2^20 positions
        if (!L->tl.p) { if (!L->tl.ensure(4ULL * (1u << 20) * 32)) return LNR_ERR_NOMEM; (void)hipMemsetAsync(L->tl.p, 0, 4ULL * (1u << 20) * 32, sm); }
        if (L->tl_round < 4 && g1 <= (1u << 20)) { A.tl = L->tl.as<unsigned long long>() + (size_t)L->tl_round * (1u << 20) * 4; L->tl_n[L->tl_round] = g1; L->tl_nh[L->tl_round] = gm; }
        L->tl_round++;
#endif
        // streams: kernels on one stream run back to back.  The 16-wave kernel stays on the main stream (no event wait, it reaches
        // the GPU first); the 4/2-wave kernel takes the spare stream when the 16-wave class is present, else the main stream; the
        // single-wave kernel goes to the bulk stream when a multi-wave class is present, else the main stream.
        // The gate of the two lanes' order (HandoverScope), for round 0: in front of the first kernel and behind the host work and the small
        // uploads above, which need no order.  A lane that had to wait launches right behind the other lane's round-1 kernels: its bulk
        // kernel then gets the head start below even without a multi-wave class of its own.
        bool head_start = gate && g0 == 0 && gate->enter();
        if (gate && g0 == 0) laps.lap("gate");
        hipStream_t smid = gh > g0 ? L->s_spare : sm;
        bool fork_m = gm > gh && gh > g0, fork_b = g1 > gm && gm > g0;
        if (fork_m || fork_b) LCK(hipEventRecord(L->ev_fork, sm));    // before any launch: nobody waits for another kernel
        if (gh > g0) {
            JobArgs H = A;
            size_t hl = (size_t)tun.heavy_lds_kb * 1024;
            H.grp_lo = g0; H.grp_hi = gh; H.lds_bytes = (u32)hl; H.arena_lds = (u32)hl;
            hipLaunchKernelGGL(k_job_heavy, dim3(gh - g0), dim3(1024), hl, sm, H); LKCHECK();
        }
        if (gm > gh) {
            if (fork_m) LCK(hipStreamWaitEvent(smid, L->ev_fork, 0));
            JobArgs M = A;
            size_t ml = (size_t)tun.mid_lds_kb * 1024;
            M.grp_lo = gh; M.grp_hi = gm; M.lds_bytes = (u32)ml; M.arena_lds = (u32)ml;
            if (tun.mid_waves == 2 || (tun.mid_waves == 0 && !remap_round_ && ix.info.hs_len >= (1ULL << 25)))
                // round 0 at human scale is bound by wave slots (16 per CU at 128 VGPRs): two waves per read of this class hold half the slots of
                // four for a little longer (GRCh38 stand-in: 45.2 vs 47.0 ms per step)
                hipLaunchKernelGGL(k_job_mid2, dim3(gm - gh), dim3(128), ml, smid, M);
            else hipLaunchKernelGGL(k_job_mid, dim3(gm - gh), dim3(256), ml, smid, M); LKCHECK();
            if (fork_m) LCK(hipEventRecord(L->ev_join_spare, smid));
        }
        if (g1 > gm) {
            hipStream_t bulk = fork_b ? sb : sm;
            if (fork_b) LCK(hipStreamWaitEvent(sb, L->ev_fork, 0));
            // (head_start: the other lane's round-1 launch has only just been enqueued, and its wide workgroups take their CUs first)
            if (fork_b || head_start) { hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, bulk, tun.bulk_delay_ticks); LKCHECK(); }
            JobArgs K = A;
            K.grp_lo = gm; K.grp_hi = g1;
            hipLaunchKernelGGL(k_job, dim3(g1 - gm), dim3(64), lds, bulk, K); LKCHECK();
        }
        if (fork_b) { LCK(hipEventRecord(L->ev_join_bulk, sb)); LCK(hipStreamWaitEvent(sm, L->ev_join_bulk, 0)); }
        if (fork_m) LCK(hipStreamWaitEvent(sm, L->ev_join_spare, 0));
        laps.lap("launches");
        L->stats.job_launches++;
        L->stats.groups_heavy += gh - g0; L->stats.groups_mid += gm - gh; L->stats.groups_wave1 += g1 - gm;
        g0 = g1;
        if (g0 < ngrp) LCK(hipStreamSynchronize(sm));   // next slice reuses the scratch
    }
    if (laps.on && std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - laps.t0).count() > 1.5) laps.done();
    return LNR_OK;
}

// per-batch host tables + prep / feature kernels.  d_reads/d_off are device pointers.
lnr_status prepare_batch(Lane *L, const u8 *d_reads, const u64 *d_off, u32 n, BatchHost &B, const u64 *h_off = nullptr) {
    const Tuning &tun = *L->tun;
    B.n = n;
    B.off.resize((size_t)n + 1);
    if (h_off) memcpy(B.off.data(), h_off, ((size_t)n + 1) * 8);     // the host-buffer entry points know the offsets already
    else {
        Readback rb;
        if (!rb.begin(L->h_rb[0], ((size_t)n + 1) * 8)) { L->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
        LCK(rb.add(B.off.data(), d_off, ((size_t)n + 1) * 8, L->stream));
        LCK(rb.flush(L->stream));
        LCK(hipStreamSynchronize(L->stream));
        rb.finish();
    }
    B.len.resize(n); B.nf.resize(n); B.cords_cap.resize(n); B.gaps_cap.resize(n);
    B.f1_off.resize(n); B.cords_off.resize(n); B.gaps_off.resize(n); B.pk_off.resize(n);
    u64 fo = 0, co = 0, go = 0, po = 0;
    for (u32 i = 0; i < n; i++) {
        if (B.off[i + 1] < B.off[i]) { L->err = "read offsets not monotone"; return LNR_ERR_ARG; }
        u64 len = B.off[i + 1] - B.off[i];
        if (len >= (1ULL << 20)) { L->err = "read longer than 2^20-1 bases (cord y field, cords.cpp:15)"; return LNR_ERR_LIMIT; }
        B.len[i] = (u32)len;
        B.pk_off[i] = po; po += 2 * packed_words(len);   // forward + reverse-complement strand
        B.nf[i] = len > 200 ? read_feature_count(len) : 0;
        B.f1_off[i] = fo; fo += 2ULL * B.nf[i];
        B.cords_cap[i] = len > 200 ? (u32)std::min<u64>(std::max<u64>((16 * (len / 64) + 256) / tun.cap_shrink, 8) * L->cap_scale, 1u << 24) : 0;
        B.cords_off[i] = co; co += B.cords_cap[i];
        B.gaps_cap[i] = len > 200 ? (u32)((len / 1000 + 4) * L->cap_scale) : 0;
        B.gaps_off[i] = go; go += B.gaps_cap[i];
    }
    lnr_status s;
    CopyBatch up;     // the eight per-read tables: one launch
    if ((s = upload_to(L->err, L->rlen, B.len, up, L->stream)) != LNR_OK) return s;
    if ((s = upload_to(L->err, L->pk_off, B.pk_off, up, L->stream)) != LNR_OK) return s;
    LENSURE(L->pk, std::max<u64>(po * 8, 16));
    LENSURE(L->nm, std::max<u64>(po * 4, 16));
    if ((s = upload_to(L->err, L->nf, B.nf, up, L->stream)) != LNR_OK) return s;
    if ((s = upload_to(L->err, L->f1_off, B.f1_off, up, L->stream)) != LNR_OK) return s;
    if ((s = upload_to(L->err, L->cords_cap, B.cords_cap, up, L->stream)) != LNR_OK) return s;
    if ((s = upload_to(L->err, L->cords_off, B.cords_off, up, L->stream)) != LNR_OK) return s;
    if ((s = upload_to(L->err, L->gaps_cap, B.gaps_cap, up, L->stream)) != LNR_OK) return s;
    if ((s = upload_to(L->err, L->gaps_off, B.gaps_off, up, L->stream)) != LNR_OK) return s;
    LCK(up.flush(L->stream));
    LENSURE(L->rks, (size_t)n * 4);
    LENSURE(L->f1, std::max<u64>(fo * sizeof(F96), 16));
    LENSURE(L->cords, std::max<u64>(co * 8, 16));
    LENSURE(L->out_str, std::max<u64>(co * 8, 16));
    LENSURE(L->out_end, std::max<u64>(co * 8, 16));
    LENSURE(L->gaps, std::max<u64>(go * sizeof(UP), 16));
    LENSURE(L->gdense, std::max<u64>(go * sizeof(UP), 16));
    LENSURE(L->gcursor, 16);
    LENSURE(L->gpos, (size_t)n * 4);
    LENSURE(L->ncords, (size_t)n * 4);
    LENSURE(L->nout, (size_t)n * 4);
    LENSURE(L->read_err, (size_t)n * 4);
    LENSURE(L->ngaps, (size_t)n * 4);
    LENSURE(L->remap, (size_t)n * 4);
    LCK(hipMemsetAsync(L->ncords.p, 0, (size_t)n * 4, L->stream));
    LCK(hipMemsetAsync(L->read_err.p, 0, (size_t)n * 4, L->stream));
    L->t_prep.start(L->stream);
    hipLaunchKernelGGL(k_prep, dim3(n < tun.prep_grid ? n : tun.prep_grid), dim3(tun.prep_threads), 0, L->stream, d_reads, d_off, L->pk_off.as<u64>(), n, L->pk.as<u64>(), L->nm.as<u32>(), L->rks.as<i32>()); LKCHECK();
    L->t_prep.stop(L->stream);
    L->stats.reads = n;
    L->stats.bases = B.off[n] - B.off[0];
    return LNR_OK;
}

// The reads' current cord counts on their way to the host, on stream st: they size a tail's scratch (tail_prepare).  The caller issues this
// in front of a sync it needs anyway -- the end of round 0, the end of the re-map round -- so the counts cost no round trip of their own.
lnr_status counts_out(Lane *L, u32 n, Readback &rb, std::vector<u32> &ncords, hipStream_t st) {
    ncords.resize(n);
    if (!rb.begin(L->h_rb[1], (size_t)n * 4)) { L->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
    LCK(rb.add(ncords.data(), L->ncords.p, (size_t)n * 4, st));
    LCK(rb.flush(st));
    return LNR_OK;
}

// Scratch layout + launch arguments of a tail kernel over the reads in `list` (null = all reads), on stream st; ncords: the cord counts
// the kernel will meet (counts of reads outside `list` are not used).  Returns with the tables' upload enqueued.
lnr_status tail_prepare(Lane *L, const BatchHost &B, TailBuf &tb, const std::vector<u32> *list, hipStream_t st, TailArgs &T, const u32 *ncords) {
    u32 n = B.n;
    tb.h_off.assign(n, 0); tb.h_cap.assign(n, 0);
    u64 o = 0;
    u32 cnt = list ? (u32)list->size() : n;
    for (u32 k = 0; k < cnt; k++) {
        u32 i = list ? (*list)[k] : k;
        tb.h_cap[i] = ncords[i] + 4; tb.h_off[i] = o; o += align_up(tail_scratch_bytes(tb.h_cap[i]), 256);
    }
    lnr_status s;
    CopyBatch up;     // off / cap / list: one launch
    if ((s = upload_to(L->err, tb.off, tb.h_off, up, st)) != LNR_OK) return s;
    if ((s = upload_to(L->err, tb.cap, tb.h_cap, up, st)) != LNR_OK) return s;
    LENSURE(tb.scr, std::max<u64>(o, 16));
    T.read_len = L->rlen.as<u32>(); T.n = cnt; T.list = nullptr;
    if (list) {
        tb.h_list = *list;
        if ((s = upload_to(L->err, tb.list, tb.h_list, up, st)) != LNR_OK) return s;
        T.list = tb.list.as<u32>();
    }
    LCK(up.flush(st));
    T.cords = L->cords.as<u64>(); T.cords_off = L->cords_off.as<u64>(); T.cords_cap = L->cords_cap.as<u32>(); T.ncords = L->ncords.as<u32>();
    T.read_err = L->read_err.as<i32>();
    T.scratch = tb.scr.as<char>(); T.scr_off = tb.off.as<u64>(); T.scr_cap = tb.cap.as<u32>();
    T.gaps = L->gaps.as<UP>(); T.gaps_off = L->gaps_off.as<u64>(); T.gaps_cap = L->gaps_cap.as<u32>(); T.ngaps = L->ngaps.as<u32>(); T.remap = L->remap.as<u32>();
    T.gdense = L->gdense.as<UP>(); T.gcursor = L->gcursor.as<u32>(); T.gpos = L->gpos.as<u32>();
    T.out_str = L->out_str.as<u64>(); T.out_end = L->out_end.as<u64>(); T.nout = L->nout.as<u32>();
    return LNR_OK;
}

void reset_stats(Lane *L) { memset(&L->stats, 0, sizeof L->stats); }
void finish_stats(Lane *L, const BatchHost &B) {
    u64 rb = 0;
    for (u32 i = 0; i < B.n; i++) if (B.len[i] > 200) rb += (B.len[i] + 3) / 4;
    L->stats.seed_bytes = rb + L->stats.lookups * 8 + L->stats.bucket_entries * 8 + L->stats.anchors * 8;
}

// Tail A + re-map round of every read (round 0 has completed on the main stream; nc0: the cord counts it left): clean / gather / gaps
// decide the remap loop (pmpfinder.cpp:2744-2749); every gap of a poorly covered read is then re-seeded with step 7 / score0
// (pmpfinder.cpp:2749-2767) into job set 1 (j1).  Returns with the launches enqueued and nc_a = the cord counts after tail A.
lnr_status remap_round(Lane *L, const BatchHost &B, HostJobs &j1, const std::vector<u32> &nc0, std::vector<u32> &nc_a) {
    hipStream_t st = L->stream;
    JobSet &S = L->js[1];
    u32 n = B.n;
    TailArgs T;
    lnr_status s;
    if ((s = tail_prepare(L, B, L->tb_remap, nullptr, st, T, nc0.data())) != LNR_OK) return s;
    Laps laps;
    laps.lap("tail_prepare");
    LCK(hipMemsetAsync(L->gcursor.p, 0, 4, st));
    hipLaunchKernelGGL(k_tail_a, dim3((T.n + 63) / 64), dim3(64), 0, st, T); LKCHECK();
    // One round trip for everything tail A decided: the flags, the cord counts (final for the reads that skip the re-map round: they size
    // the early tail B) and the dense gap list up to a sticky capacity.  A second trip only when tail A wrote more gaps than that.
    if (!L->h_flags.ensure((size_t)n * 16 + 16)) { L->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
    u32 *remap = L->h_flags.as<u32>(), *ngaps = remap + n, *gpos = ngaps + n, *nca = gpos + n, *gtot_p = nca + n;
    u64 spec = std::min<u64>(L->tun->gaps_spec ? L->tun->gaps_spec : L->gaps_spec_cap, L->gdense.cap / sizeof(UP));
    if (!L->h_gaps.ensure(std::max<u64>(spec, 1) * sizeof(UP))) { L->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
    CopyBatch cb;
    LCK(cb.add(remap, L->remap.p, n, st));
    LCK(cb.add(ngaps, L->ngaps.p, n, st));
    LCK(cb.add(gpos, L->gpos.p, n, st));
    LCK(cb.add(nca, L->ncords.p, n, st));
    LCK(cb.add(gtot_p, L->gcursor.p, 1, st));
    LCK(cb.add(L->h_gaps.p, L->gdense.p, spec * sizeof(UP) / 4, st));
    LCK(cb.flush(st));
    LCK(hipStreamSynchronize(st));
    laps.lap("tail_a+flags");
    nc_a.assign(nca, nca + n);
    u64 gtot = *gtot_p;
    if (gtot == 0) return LNR_OK;
    if (gtot > spec) {
        if (!L->h_gaps.ensure(gtot * sizeof(UP))) { L->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }   // (may move: all of the list again)
        LCK(copy_words(L->h_gaps.p, L->gdense.p, gtot * sizeof(UP) / 4, st));
        LCK(hipStreamSynchronize(st));
        L->gaps_spec_cap = gtot + gtot / 2;
    }
    UP *gaps = L->h_gaps.as<UP>();
    for (u32 i = 0; i < n; i++) {
        if (!(remap[i] && ngaps[i])) continue;
        L->stats.remap_reads++;
        j1.grp_beg.push_back(j1.size());
        for (u32 k = 0; k < ngaps[i]; k++) {
            UP y = forward_y(gaps[gpos[i] + k], B.len[i]);
            j1.add(i, (u32)y.first, (u32)y.second, 1);
        }
    }
    j1.grp_beg.push_back(j1.size());
    laps.lap("gaps-copy+build");
    if ((s = seed_jobs(L, S, j1, st)) != LNR_OK) return s;
    laps.lap("seed1(sync)");
    s = launch_jobs(L, S, j1);
    laps.lap("launch1");
    laps.done();
    return s;
}

lnr_status filter_dev(Lane *L, const u8 *d_reads, const u64 *d_off, u32 n, lnr_cords_dev *out, const u64 *h_off = nullptr, int attempt = 0) {
    const Index &ix = *L->ix;
    if (!ix.has_index) { L->err = "no index: call lnr_index_build or lnr_index_adopt first"; return LNR_ERR_NO_INDEX; }
    reset_stats(L);
    AllocCount count_(&L->allocs);
    HandoverScope gate(L);     // (its own in the re-run after an overflow: the outer call's hand-over ended with its round-1 launch)
    if (attempt == 0) t_copy_launches = 0;
    L->last_n = n; L->last_ncords = 0;
    if (out) { out->n_reads = n; out->n_cords = 0; out->d_cord_off = nullptr; out->d_cords_str = nullptr; out->d_cords_end = nullptr; }
    LENSURE(L->r_off, ((size_t)n + 1) * 8);
    if (n == 0) {
        LCK(hipMemsetAsync(L->r_off.p, 0, 8, L->stream));
        LCK(hipStreamSynchronize(L->stream));
        if (out) out->d_cord_off = L->r_off.as<u64>();
        return LNR_OK;
    }
    Laps laps;
    L->t_total.start(L->stream);
    BatchHost B;
    lnr_status s = prepare_batch(L, d_reads, d_off, n, B, h_off);
    if (s != LNR_OK) return s;
    L->last_gaps_off = B.gaps_off;
    laps.lap("prepare");
    // round 0: one job per read longer than 200 bases (mapper.cpp:430,440), whole read, default parameters
    HostJobs j0;
    for (u32 i = 0; i < n; i++) {
        if (B.len[i] > 200) { j0.grp_beg.push_back(j0.size()); j0.add(i, 0, B.len[i], 0); }
    }
    j0.grp_beg.push_back(j0.size());
    if ((s = seed_jobs(L, L->js[0], j0, L->stream, n)) != LNR_OK) return s;
    laps.lap("seed0(sync)");
    LCK(hipStreamWaitEvent(L->stream, L->ev_f1, 0));   // read features ready (k_f1 ran beside the seed kernel)
    L->t_job.start(L->stream);
    LCK(hipEventRecord(L->ev_start, L->stream));
    LCK(hipStreamWaitEvent(L->s_spare, L->ev_start, 0));
    LCK(hipStreamWaitEvent(L->s_bulk, L->ev_start, 0));
    laps.lap("events");
    if ((s = launch_jobs(L, L->js[0], j0, &gate)) != LNR_OK) return s;
    gate.stamp("round0-enqueued");
    laps.lap("launch0");
    std::vector<u32> nc0, nc_a, nc1;
    {   // the cord counts of round 0 (they size tail A's scratch) come back with the sync that ends round 0
        Readback rb;
        if ((s = counts_out(L, n, rb, nc0, L->stream)) != LNR_OK) return s;
        LCK(hipStreamSynchronize(L->stream));
        rb.finish();
    }
    HostJobs j1;
    if ((s = remap_round(L, B, j1, nc0, nc_a)) != LNR_OK) return s;
    gate.leave();
    laps.lap("tailA+seed1+launch1");
    // Tail B (block chaining on both strands, flags, cords_end; pmpfinder.cpp:2764-2801) of the reads that do not go through
    // the re-map round is final after tail A: it runs on its own stream while the re-map jobs (a few long reads) are busy.
    std::vector<u32> late_list, early_list;
    bool early = j1.size() > 0;
    if (early) {
        std::vector<char> in_r1(n, 0);
        for (u32 q = 0; q < j1.size(); q++) in_r1[j1.read[q]] = 1;
        for (u32 i = 0; i < n; i++) (in_r1[i] ? late_list : early_list).push_back(i);
        TailArgs TE;
        if ((s = tail_prepare(L, B, L->tb_early, &early_list, L->s_tail, TE, nc_a.data())) != LNR_OK) return s;
        if (TE.n) { hipLaunchKernelGGL(k_tail_b, dim3((TE.n + 63) / 64), dim3(64), 0, L->s_tail, TE); LKCHECK(); }   // (every read may be in the re-map round)
        LCK(hipEventRecord(L->ev_prep, L->s_tail));
    }
    L->t_job.stop(L->stream);
    {   // the final cord counts of the late tail's reads come back with the sync that ends the re-map round
        Readback rb;
        if ((s = counts_out(L, n, rb, nc1, L->stream)) != LNR_OK) return s;
        LCK(hipStreamSynchronize(L->stream));
        rb.finish();
    }
    L->stats.job_ms += L->t_job.ms();
    laps.lap("wait-r1");
    TailArgs T;
    if ((s = tail_prepare(L, B, L->tb_late, early ? &late_list : nullptr, L->stream, T, nc1.data())) != LNR_OK) return s;
    L->t_tail.start(L->stream);
    if (T.n) { hipLaunchKernelGGL(k_tail_b, dim3((T.n + 63) / 64), dim3(64), 0, L->stream, T); LKCHECK(); }
    L->t_tail.stop(L->stream);
    if (early) LCK(hipStreamWaitEvent(L->stream, L->ev_prep, 0));
    int ext_state_out = L->gap_ext;
    if (L->opts->gap_len) {
        u32 maxlen = 0;
        for (u32 i = 0; i < n; i++) maxlen = std::max(maxlen, B.len[i]);
        if ((s = gap_stage(L, d_reads, d_off, n, maxlen, &ext_state_out)) != LNR_OK) return s;
    }
    std::vector<u32> nout(n);
    std::vector<i32> rerr(n);
    u32 gap_second = 0, gap_last = 0;
    {
        Readback rb;
        if (!rb.begin(L->h_rb[0], (size_t)n * 8 + 256)) { L->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
        LCK(rb.add(nout.data(), L->nout.p, (size_t)n * 4, L->stream));
        LCK(rb.add(rerr.data(), L->read_err.p, (size_t)n * 4, L->stream));
        if (L->opts->gap_len) LCK(rb.add(&gap_second, L->gap_next.as<u32>() + 16, 4, L->stream));
        if (L->opts->gap_len) LCK(rb.add(&gap_last, L->gap_next.as<u32>() + 24 + 8, 4, L->stream));   // (k_gap_team's count of the reads it did)
        LCK(rb.flush(L->stream));
        LCK(hipStreamSynchronize(L->stream));
        rb.finish();
    }
    L->stats.tail_ms += L->t_tail.ms();
    if (L->opts->gap_len) { L->stats.gap_ms += L->t_gap.ms(); L->stats.gap_second_pass += gap_second; L->stats.gap_last_launch += gap_last; }
    for (u32 i = 0; i < n; i++)
        if (rerr[i]) {
            // A read outgrew a per-read capacity (cords: 16 per 64 bases + 256; gaps: one per 1000 bases + 4 -- heuristics, generous by an
            // order of magnitude).  Nothing of the batch is handed out; the batch is run again with 4x, then 16x the capacities.
            if (attempt < 2) {
                L->t_total.stop(L->stream);
                LCK(hipStreamSynchronize(L->stream));
                L->cap_scale = attempt == 0 ? 4 : 16;
                L->overflow_reruns++;
                lnr_status rs = filter_dev(L, d_reads, d_off, n, out, h_off, attempt + 1);
                L->cap_scale = 1;
                return rs;
            }
            char b[160];
            snprintf(b, sizeof b, "device capacity overflow on read %u (stage code %d, length %u) with 16x capacities", i, rerr[i], B.len[i]);
            L->err = b;
            return LNR_ERR_INTERNAL;
        }
    L->gap_ext = ext_state_out;        // (only a batch that went through: a re-run after an overflow starts from the state the batch met)
    L->h_cord_off.assign((size_t)n + 1, 0);
    for (u32 i = 0; i < n; i++) L->h_cord_off[i + 1] = L->h_cord_off[i] + nout[i];
    u64 tot = L->h_cord_off[n];
    LENSURE(L->r_str, std::max<u64>(tot * 8, 16));
    LENSURE(L->r_end, std::max<u64>(tot * 8, 16));
    {
        void *h = L->r_off.host_stage(((size_t)n + 1) * 8);
        if (!h) { L->err = "pinned host allocation failed"; return LNR_ERR_NOMEM; }
        memcpy(h, L->h_cord_off.data(), ((size_t)n + 1) * 8);
        LCK(copy_words(L->r_off.p, h, ((u64)n + 1) * 2, L->stream));
    }
    hipLaunchKernelGGL(k_gather_out, dim3(n), dim3(64), 0, L->stream, L->out_str.as<u64>(), L->out_end.as<u64>(), L->cords_off.as<u64>(), L->nout.as<u32>(),
                       L->r_off.as<u64>(), n, L->r_str.as<u64>(), L->r_end.as<u64>()); LKCHECK();
    L->t_total.stop(L->stream);
    LCK(hipStreamSynchronize(L->stream));
    laps.lap("tailB+gather");
    if (laps.on) { char b[96]; snprintf(b, sizeof b, " | lane %d allocations so far %u, copy launches of this batch %u", L->id, L->allocs.load(), t_copy_launches); laps.out += b; }
    laps.done();
    L->stats.prep_ms = L->t_prep.ms();
    L->stats.total_ms = L->t_total.ms();
    L->stats.cords = tot;
    finish_stats(L, B);
    L->last_ncords = tot;
    if (out) { out->n_cords = tot; out->d_cord_off = L->r_off.as<u64>(); out->d_cords_str = L->r_str.as<u64>(); out->d_cords_end = L->r_end.as<u64>(); }
    return LNR_OK;
}

// (a_off / a_vals: the anchors by read, CSR, filled when to_host)
lnr_status seed_dev(Lane *L, const u8 *d_reads, const u64 *d_off, u32 n, bool to_host, std::vector<u64> &a_off, std::vector<u64> &a_vals) {
    const Index &ix = *L->ix;
    if (!ix.has_index) { L->err = "no index: call lnr_index_build or lnr_index_adopt first"; return LNR_ERR_NO_INDEX; }
    reset_stats(L);
    a_off.assign((size_t)n + 1, 0);
    a_vals.clear();
    if (n == 0) return LNR_OK;
    L->t_total.start(L->stream);
    BatchHost B;
    lnr_status s = prepare_batch(L, d_reads, d_off, n, B);
    if (s != LNR_OK) return s;
    HostJobs j0;
    std::vector<u32> job_of(n, 0xffffffffu);
    for (u32 i = 0; i < n; i++) {
        if (B.len[i] >= 43) { job_of[i] = j0.size(); j0.grp_beg.push_back(j0.size()); j0.add(i, 0, B.len[i], 0); }
    }
    j0.grp_beg.push_back(j0.size());
    if ((s = seed_jobs(L, L->js[0], j0, L->stream, n)) != LNR_OK) return s;
    if (to_host && (s = export_anchors(L, L->js[0], j0.size(), a_off, a_vals)) != LNR_OK) return s;
    LCK(hipStreamWaitEvent(L->stream, L->ev_f1, 0));
    L->t_total.stop(L->stream);
    LCK(hipStreamSynchronize(L->stream));
    L->stats.prep_ms = L->t_prep.ms();
    L->stats.total_ms = L->t_total.ms();
    // stats.seed_bytes with every read counted
    u64 rb = 0;
    for (u32 i = 0; i < n; i++) if (job_of[i] != 0xffffffffu) rb += (B.len[i] + 3) / 4;
    L->stats.seed_bytes = rb + L->stats.lookups * 8 + L->stats.bucket_entries * 8 + L->stats.anchors * 8;
    if (to_host) {
        // re-index the per-job CSR by read (reads without a job get the bare dummy)
        std::vector<u64> off((size_t)n + 1, 0), vals;
        for (u32 i = 0; i < n; i++) {
            u64 c = job_of[i] == 0xffffffffu ? 1 : a_off[job_of[i] + 1] - a_off[job_of[i]];
            off[i + 1] = off[i] + c;
        }
        vals.assign(off[n], 0);
        for (u32 i = 0; i < n; i++)
            if (job_of[i] != 0xffffffffu) {
                u64 a = a_off[job_of[i]], c = a_off[job_of[i] + 1] - a;
                memcpy(vals.data() + off[i], a_vals.data() + a, c * 8);
            }
        a_off.swap(off);
        a_vals.swap(vals);
    }
    return LNR_OK;
}

}  // namespace
