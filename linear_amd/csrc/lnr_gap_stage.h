// lnr_gap_stage.h -- host side of the gap re-mapper (-g > 0) behind tail B, on one lane's main stream (included by lnr_batch.h; the kernels
// and their launch functions are lnr_gap_kernels.hip, a translation unit of its own, behind lnr_gap_args.h).
#pragma once

namespace {

#ifdef LNR_GAP_DEVPROF
// diagnostic build: what the device counters of the batch's gap stage say (stderr)
lnr_status gap_devprof_report(Lane *L, u32 n) {
    unsigned long long hp[96];
    LCK(hipMemcpyAsync(hp, L->gap_prof.p, sizeof hp, hipMemcpyDeviceToHost, L->stream));
    LCK(hipStreamSynchronize(L->stream));
    static const char *nm[10] = {"sort k-mers", "join", "k-mer stream", "sort anchors", "chain DP", "traceback", "chain tiles", "map along chain (incl.)", "tiles from chain", "filter anchors (sorts)"};
    for (int la = 0; la < 3; la++) {
        const unsigned long long *q = hp + 16 * la;
        fprintf(stderr, "[gap prof] launch %d: reads %llu, lane/wave time %.1f ms in total, slowest read %.1f ms\n", la, q[12], q[11] / 1e5, q[15] / 1e5);
        const unsigned long long *w = hp + 48 + 16 * la;
        fprintf(stderr, "[gap prof]    slowest read: index %llu, length %llu, cords in %llu, arena high-water %llu bytes; its longest chain DP: %.1f ms, %llu anchors, score fn %llu, %s\n", w[10], w[11], w[12], w[13],
                (double)(w[14] & ((1ULL << 56) - 1)) / 1e5, hp[90 + la], (w[14] >> 56) & 15, (w[14] >> 60) ? "by columns" : "single wave");
        for (int k = 0; k < 10; k++) fprintf(stderr, "[gap prof]    %-26s %10.1f ms  %5.1f %%   slowest read: %8.1f ms\n", nm[k], q[k] / 1e5, q[11] ? 100.0 * q[k] / q[11] : 0.0, w[k] / 1e5);
    }
    fprintf(stderr, "[gap prof] map along chain, all launches: streams + join + anchor sort %.1f ms, chain DP + traceback + tiles %.1f ms\n", hp[63] / 1e5, hp[79] / 1e5);
    fprintf(stderr, "[gap prof] first launch: at most %llu workers (waves) alive at once\n", hp[95]);
    {   // how well the weight predicts: weights of the reads the team launch did, and of the slowest / all reads of the first launch
        std::vector<u32> wt(n); std::vector<unsigned long long> pr0(n);
        LCK(hipMemcpy(wt.data(), L->gap_weight.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        LCK(hipMemcpy(pr0.data(), (char *)L->gap_prof.p + 96 * 8, (size_t)n * 8, hipMemcpyDeviceToHost));
        std::vector<u32> wh, wl; std::vector<std::pair<double, u32> > slow;
        for (u32 i = 0; i < n; i++) { if (!pr0[i]) continue; if ((pr0[i] >> 56) >= 1) wh.push_back(wt[i]); else { wl.push_back(wt[i]); slow.push_back({(double)(pr0[i] & ((1ULL << 56) - 1)) / 1e5, wt[i]}); } }
        std::sort(wh.begin(), wh.end()); std::sort(wl.begin(), wl.end()); std::sort(slow.begin(), slow.end());
        if (!wh.empty() && !wl.empty()) {
            fprintf(stderr, "[gap prof] weight of team-launch reads: min %u p10 %u p50 %u p90 %u max %u | of first-launch reads: p50 %u p90 %u p99 %u p99.9 %u max %u\n", wh[0], wh[wh.size() / 10], wh[wh.size() / 2], wh[wh.size() * 9 / 10], wh.back(),
                    wl[wl.size() / 2], wl[wl.size() * 9 / 10], wl[wl.size() * 99 / 100], wl[(size_t)(wl.size() * 0.999)], wl.back());
            fprintf(stderr, "[gap prof] slowest first-launch reads (ms : weight):");
            for (size_t k = 0; k < 16 && k < slow.size(); k++) fprintf(stderr, " %.0f:%u", slow[slow.size() - 1 - k].first, slow[slow.size() - 1 - k].second);
            fprintf(stderr, "\n");
        }
    }
    {   // reads in flight over the first launch's duration (start / end ticks of every read, 10 ns)
        std::vector<unsigned long long> se(2 * (size_t)n);
        LCK(hipMemcpy(se.data(), (char *)L->gap_prof.p + (96 + (size_t)n) * 8, 2 * (size_t)n * 8, hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ULL, t1 = 0;
        for (u32 i = 0; i < n; i++) if (se[i]) { t0 = std::min(t0, se[i]); t1 = std::max(t1, se[n + i]); }
        if (t1 > t0) {
            const int NBK = 20;
            std::vector<double> busy(NBK, 0.0);
            double span = (double)(t1 - t0), bw = span / NBK;
            for (u32 i = 0; i < n; i++) if (se[i]) {
                double a = (double)(se[i] - t0), b = (double)(se[n + i] - t0);
                for (int k = (int)(a / bw); k < NBK && k * bw < b; k++) busy[k] += std::min(b, (k + 1) * bw) - std::max(a, k * bw);
            }
            fprintf(stderr, "[gap prof] first launch: %.1f ms from the first read's start to the last read's end; mean reads in flight per twentieth:", span / 1e5);
            for (int k = 0; k < NBK; k++) fprintf(stderr, " %.0f", busy[k] / bw);
            fprintf(stderr, "\n");
        }
    }
    std::vector<unsigned long long> pr(n);
    LCK(hipMemcpy(pr.data(), (char *)L->gap_prof.p + 96 * 8, (size_t)n * 8, hipMemcpyDeviceToHost));
    for (int la = 0; la < 3; la++) {
        std::vector<double> t;
        for (u32 i = 0; i < n; i++) if (pr[i] && (int)(pr[i] >> 56) == la) t.push_back((double)(pr[i] & ((1ULL << 56) - 1)) / 1e5);
        if (t.empty()) continue;
        std::sort(t.begin(), t.end());
        double sum = 0; for (double v : t) sum += v;
        fprintf(stderr, "[gap prof] launch %d per-read ms: n %zu sum %.1f p50 %.3f p90 %.3f p99 %.3f p99.9 %.3f max %.3f | top:", la, t.size(), sum, t[t.size() / 2], t[t.size() * 9 / 10], t[t.size() * 99 / 100], t[(size_t)(t.size() * 0.999)], t.back());
        for (size_t k = 0; k < 12 && k < t.size(); k++) fprintf(stderr, " %.1f", t[t.size() - 1 - k]);
        fprintf(stderr, "\n");
    }
    return LNR_OK;
}
#endif

// The gap re-mapper on the final cords of the batch (reads of at most maxlen bases): every read in the fused first stage (k_gap_all), then
// the flagged reads with the largest arena (k_gap_team).  Returns with the launches enqueued; *ext_out is the read stream's state behind
// the batch, which the caller commits to L->gap_ext only for a batch that went through.
lnr_status gap_stage(Lane *L, const u8 *d_reads, const u64 *d_off, u32 n, u32 maxlen, int *ext_out) {
    const Index &ix = *L->ix; const Tuning &tun = *L->tun;
    // arena budget of the gap re-mapper's workers: 48 GiB of the 288, never more than lnr_opts.scratch_budget (when given) nor than 80 % of what
    // is free on the device beside the arena already held -- a second context on the GPU gets fewer workers instead of LNR_ERR_NOMEM
    u64 budget = (u64)48 << 30;
    if (L->opts->scratch_budget && L->opts->scratch_budget < budget) budget = L->opts->scratch_budget;
    { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess) { u64 avail = (u64)(((double)fr + (double)L->gap_arena.cap) * 0.8); if (avail < budget) budget = avail; } else (void)hipGetLastError(); }
    if (budget < ((u64)1 << 30)) budget = (u64)1 << 30;
    // (tests/host_shim.cpp hs_gap_arena1 restates this formula at cap_scale 1: change both)
    u64 arena1 = align_up(((u64)512 << 10) * L->cap_scale + 16ULL * maxlen + sizeof(LeaderScratch) + 65536, 256);
    u64 arena2 = std::max<u64>(((u64)tun.gap_arena2_mb << 20) * L->cap_scale, arena1 * 2);
    u64 arena3 = std::max<u64>(((u64)64 << 20) * L->cap_scale, arena2 * 2);
    u32 w3 = (u32)std::min<u64>(n, std::max<u64>(1, (budget / 2) / arena3));   // workgroups of the last launch
    const u32 ncu = tun.ncu ? tun.ncu : 256, nteams = std::min<u32>(tun.gap_teams, ncu / 2);
    u64 fused_bytes = (u64)nteams * arena2 + (u64)ncu * K_GAP_TEAM * arena1;     // (a small chunk runs fewer teams and more single waves: bounded by every CU full of single waves)
    LENSURE(L->gap_arena, std::max((u64)w3 * arena3, fused_bytes));
    LENSURE(L->gap_flag, (size_t)n * 4);
    LENSURE(L->gap_next, 256);
    LCK(hipMemsetAsync(L->gap_next.p, 0, 256, L->stream));
    GapArgs G;
    G.g = ix.g.as<u8>(); G.seq_off = ix.d_seq_off.as<u64>(); G.seq_len = ix.d_seq_len.as<u64>();
    G.gf.base = ix.f2.as<F96>(); G.gf.off = ix.d_f2_off.as<u64>(); G.gf.nseq = ix.info.nseq;
    G.reads = d_reads; G.off = d_off; G.n = n;
    G.nf = L->nf.as<u32>(); G.f1_off = L->f1_off.as<u64>(); G.f1 = L->f1.as<F96>();
    G.out_str = L->out_str.as<u64>(); G.out_end = L->out_end.as<u64>(); G.cords_off = L->cords_off.as<u64>(); G.cords_cap = L->cords_cap.as<u32>();
    G.nout = L->nout.as<u32>(); G.read_err = L->read_err.as<i32>(); G.gap_flag = L->gap_flag.as<u32>();
    G.arena = (char *)L->gap_arena.p;
    G.prof = nullptr;
#ifdef LNR_GAP_DEVPROF
    LENSURE(L->gap_prof, (96 + 3 * (size_t)n) * 8);
    LCK(hipMemsetAsync(L->gap_prof.p, 0, (96 + 3 * (size_t)n) * 8, L->stream));
    G.prof = L->gap_prof.as<unsigned long long>();
#endif
    G.gap_len_min = L->opts->gap_len == 1 ? 50 : (L->opts->gap_len < 10 ? 10 : L->opts->gap_len);   // mapper.cpp:438-453
    G.f_dup = (int)L->opts->dup;
    L->t_gap.start(L->stream);
    LENSURE(L->gap_first, 64);
    G.first_ext = L->gap_first.as<u32>();
    LENSURE(L->gap_rank, ((size_t)n + 16) * 4);
    LENSURE(L->gap_weight, ((size_t)n + 16) * 4);
    // list / hand-over queue: n entries + one per team.  A team of k_gap_all looks at queue entry k before it knows whether the single waves
    // are through, for k up to (reads handed over) + (teams) - 1; every entry it can look at is zeroed before the launch.  (With n entries
    // only, a batch of one read that was handed over had its team read entry 1: stale words of an earlier batch, taken for a read index.)
    const size_t list_words = (size_t)n + 16 + nteams + 16;
    LENSURE(L->gap_list, list_words * 4);
    G.list = L->gap_list.as<u32>() + 16; G.list_n = L->gap_list.as<u32>();
    // one "ladder" over the reads of [lo, hi): the fused first stage, then the reads it flagged with the largest arena
    auto ladder = [&](u32 lo, u32 hi, u32 ext_from, int probe) -> hipError_t {
        hipError_t e = hipMemsetAsync(L->gap_next.p, 0, 256, L->stream);
        if (e != hipSuccess) return e;
        u32 m = hi - lo;
        G.lo = lo; G.n = hi; G.ext_from = ext_from; G.probe = probe;
        G.work_cap = tun.gap_work_cap;
        if ((e = launch_gap_weight(G.reads, G.off, G.out_str, G.cords_off, G.nout, lo, hi, L->gap_weight.as<u32>(), L->stream)) != hipSuccess) return e;
        if ((e = launch_gap_rank(L->gap_weight.as<u32>(), lo, hi, L->gap_rank.as<u32>() + 16, L->gap_rank.as<u32>(), tun.gap_heavy_w, L->stream)) != hipSuccess) return e;
        G.order = L->gap_rank.as<u32>() + 16;
        G.next = L->gap_next.as<u32>(); G.last = 0;
        // one launch: teams on the reads expected to be heavy + on what the single waves hand over, single waves on the rest
        if ((e = hipMemsetAsync(L->gap_list.p, 0, list_words * 4, L->stream)) != hipSuccess) return e;
        G.nteams = std::min<u32>(nteams, std::max<u32>(1, m / 8));
        u32 bulk_wg = std::min<u32>(ncu > G.nteams ? ncu - G.nteams : 1, (m + K_GAP_TEAM - 1) / K_GAP_TEAM);
        G.nbulk_waves = bulk_wg * K_GAP_TEAM; G.arena_bytes = arena1; G.arena2_bytes = arena2;
        G.n_heavy = L->gap_rank.as<u32>(); G.q = L->gap_list.as<u32>() + 16;
        if ((e = launch_gap_all(G, G.nteams + bulk_wg, L->stream)) != hipSuccess) return e;
        G.work_cap = ~0ULL;
        if ((e = launch_gap_order(G.gap_flag, lo, hi, L->gap_list.as<u32>() + 16, L->gap_list.as<u32>(), L->stream)) != hipSuccess) return e;
        G.arena_bytes = arena3; G.next = L->gap_next.as<u32>() + 24; G.last = 1;
        return launch_gap_team(G, std::min(w3, m), L->stream);
    };
    // The stream state (GapArgs): once a read of the stream has extended, every later read starts "extended" -- one ladder over the batch.
    // Until then the batch is taken in growing chunks: a probe ladder finds the chunk's first extending read r* (all reads started "not
    // extended", nothing written), then the chunk is done for good with the reads behind r* started "extended".  The state is kept in
    // the context across batches (one context = one read stream in file order, the reference's `-t 1`; lnr_gap_stream).
    int ext_state = L->gap_ext;
    u32 lo = 0;
    for (u32 chunk = 256; lo < n && !ext_state; chunk = chunk < (1u << 20) ? chunk * 4 : chunk) {
        u32 hi = (u32)std::min<u64>(n, (u64)lo + chunk), first = 0xffffffffu;
        LCK(hipMemsetAsync(L->gap_first.p, 0xff, 64, L->stream));
        LCK(ladder(lo, hi, 0xffffffffu, 1));
        LCK(hipMemcpyAsync(&first, L->gap_first.p, 4, hipMemcpyDeviceToHost, L->stream));
        LCK(hipStreamSynchronize(L->stream));
        LCK(ladder(lo, hi, first == 0xffffffffu ? first : first + 1, 0));
        if (first != 0xffffffffu) ext_state = 1;
        lo = hi;
    }
    if (lo < n) LCK(ladder(lo, n, 0, 0));
    *ext_out = ext_state;
    L->t_gap.stop(L->stream);
#ifdef LNR_GAP_DEVPROF
    return gap_devprof_report(L, n);
#else
    return LNR_OK;
#endif
}

}  // namespace

