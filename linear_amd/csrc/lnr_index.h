// lnr_index.h -- the index behind a context (included by lnr_api.hip): DIndex / HIndex build orchestration, the views derived from a
// received index, and the lnr_index_* entry points (build, export, alloc / blob / adopt, broadcast between GPUs).  Everything here runs
// with nothing in flight, on lane 0's main stream, and writes lnr_ctx::ix.
#pragma once

namespace {

// exclusive scan of n int32 on the device (in -> out), tmp = block sums
lnr_status dev_scan_i32(lnr_ctx *ctx, const i32 *in, i32 *out, u64 n, DevBuf &tmp) {
    hipStream_t sm = ctx->stream();
    u32 nblk = (u32)((n + SCAN_BLK - 1) / SCAN_BLK);
    ENSURE(tmp, (size_t)nblk * 4 + 16);
    hipLaunchKernelGGL(k_scan_blk, dim3(nblk), dim3(SCAN_TPB), 0, sm, in, out, n, tmp.as<i32>()); KCHECK();
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, sm, tmp.as<i32>(), nblk); KCHECK();
    hipLaunchKernelGGL(k_scan_add, dim3(nblk), dim3(SCAN_TPB), 0, sm, out, n, tmp.as<i32>()); KCHECK();
    return LNR_OK;
}

// The seed kernel's view of the DIndex, derived from dir / hs on this GPU: bucket bitmap, bucket lines and their overflow lines.
lnr_status build_seed_view(lnr_ctx *ctx) {
    Index &ix = ctx->ix; hipStream_t sm = ctx->stream();
    u64 nb = ix.info.dir_len - 1, nwords = (((nb + (1u << BM_GROUP_LOG2) - 1) >> BM_GROUP_LOG2) + 31) / 32;
    ENSURE(ix.bm, nwords * 4 + 16);
    hipLaunchKernelGGL(k_ix_bitmap, dim3((u32)((nwords + 255) / 256)), dim3(256), 0, sm, ix.dir.as<i32>(), nb, ix.bm.as<u32>()); KCHECK();
    DevBuf ovoff, tmp;                                        // overflow lines per bucket -> first overflow line of every bucket
    ENSURE(ovoff, (nb + 1) * 4 + 16);
    hipLaunchKernelGGL(k_ix_ovcount, dim3((u32)((nb + 1 + 255) / 256)), dim3(256), 0, sm, ix.dir.as<i32>(), nb, ovoff.as<i32>()); KCHECK();
    lnr_status st = dev_scan_i32(ctx, ovoff.as<i32>(), ovoff.as<i32>(), nb + 1, tmp);
    if (st != LNR_OK) return st;
    i32 nov = 0;
    HIPCK(hipMemcpyAsync(&nov, ovoff.as<i32>() + nb, 4, hipMemcpyDeviceToHost, sm));
    HIPCK(hipStreamSynchronize(sm));
    if (nov < 0) { ctx->err = "overflow lines of the bucket view exceed 2^31"; return LNR_ERR_LIMIT; }
    ENSURE(ix.ov, ((u64)nov + 1) * 128);
    ENSURE(ix.bl, nb * 128);
    hipLaunchKernelGGL(k_ix_lines, dim3((u32)((nb * 8 + 255) / 256)), dim3(256), 0, sm, ix.dir.as<i32>(), ix.hs.as<u64>(), ovoff.as<i32>(), nb, ix.bl.as<ulonglong2>(),
                       ix.ov.as<u64>()); KCHECK();
    HIPCK(hipStreamSynchronize(sm));                 // ovoff / tmp go out of scope
    return LNR_OK;
}

// ---- HIndex (-i 2): lookup tables from ysa (ctx->ix.hs), at build and at adopt
lnr_status hx_derive(lnr_ctx *ctx) {
    Index &ix = ctx->ix; hipStream_t sm = ctx->stream();
    u64 n = ix.info.hs_len;
    if (n < 2) { ctx->err = "empty HIndex"; return LNR_ERR_ARG; }
    {   // emptyDir: the first zero word (heads and bodies are not zero) -- the last two words, or, where the reference gave up its last block
        // (build_hindex), the two words in front of what it left of that block: at most six words from the end
        u64 tn = std::min<u64>(n, 6), tw[6];
        HIPCK(hipMemcpyAsync(tw, ix.hs.as<u64>() + (n - tn), tn * 8, hipMemcpyDeviceToHost, sm));
        HIPCK(hipStreamSynchronize(sm));
        ix.hx_empty_dir = n - 2;
        for (u64 q = 0; q < tn; q++) if (!tw[q]) { ix.hx_empty_dir = n - tn + q; break; }
    }
    ENSURE(ix.dir, ix.info.dir_len * 4);
    HIPCK(hipMemsetAsync(ix.dir.p, 0xff, ix.info.dir_len * 4, sm));
    DevBuf flag, tmp;
    ENSURE(flag, (n + 1) * 4 + 16);
    hipLaunchKernelGGL(k_hx_derive, dim3((u32)((n + 255) / 256)), dim3(256), 0, sm, ix.hs.as<u64>(), n, ix.hx_empty_dir, ix.dir.as<i32>(), flag.as<i32>()); KCHECK();
    HIPCK(hipMemsetAsync(flag.as<i32>() + n, 0, 4, sm));
    hipLaunchKernelGGL(k_hx_nodes_mark, dim3(1u << HX_XBITS), dim3(256), 0, sm, ix.hs.as<u64>(), ix.dir.as<i32>(), flag.as<i32>()); KCHECK();
    DevBuf excl;
    ENSURE(excl, (n + 1) * 4 + 16);
    lnr_status st = dev_scan_i32(ctx, flag.as<i32>(), excl.as<i32>(), n + 1, tmp);
    if (st != LNR_OK) return st;
    i32 nn = 0;
    HIPCK(hipMemcpyAsync(&nn, excl.as<i32>() + n, 4, hipMemcpyDeviceToHost, sm));
    HIPCK(hipStreamSynchronize(sm));
    ix.hx_nnodes = (u32)nn;
    ENSURE(ix.hx_nkeys, (size_t)std::max(nn, 1) * 8);
    ENSURE(ix.hx_nvals, (size_t)std::max(nn, 1) * 4);
    if (nn) {
        DevBuf k_in, v_in, cub;
        ENSURE(k_in, (size_t)nn * 8); ENSURE(v_in, (size_t)nn * 4);
        hipLaunchKernelGGL(k_hx_nodes_fill_blk, dim3(1u << HX_XBITS), dim3(256), 0, sm, ix.hs.as<u64>(), ix.dir.as<i32>(), flag.as<i32>(), excl.as<i32>(), k_in.as<u64>(), v_in.as<u32>()); KCHECK();
        size_t tb = 0;   // stable sort by (X, Y20): equal keys keep ysa order, the lookup takes the first
        HIPCK(rocprim::radix_sort_pairs(nullptr, tb, k_in.as<u64>(), ix.hx_nkeys.as<u64>(), v_in.as<u32>(), ix.hx_nvals.as<u32>(), (size_t)nn, 0u, (unsigned)(20 + HX_XBITS), sm));
        ENSURE(cub, tb + 16);
        HIPCK(rocprim::radix_sort_pairs(cub.p, tb, k_in.as<u64>(), ix.hx_nkeys.as<u64>(), v_in.as<u32>(), ix.hx_nvals.as<u32>(), (size_t)nn, 0u, (unsigned)(20 + HX_XBITS), sm));
        HIPCK(hipStreamSynchronize(sm));
    }
    HIPCK(hipStreamSynchronize(sm));
    return LNR_OK;
}
// ---- HIndex build (createHIndex, index_util.cpp:1463-1476): samples per -t chunk, blocks by X, bodies descending, ysa
lnr_status build_hindex(lnr_ctx *ctx, const u64 *len, u32 nseq, u32 T) {
    Index &ix = ctx->ix; hipStream_t sm = ctx->stream();
    std::vector<HxPiece> pieces;
    std::vector<u32> chunk_first;                                        // index of every chunk's first piece (+ end sentinel)
    u64 stage = 0;
    for (u32 j = 0; j < nseq; j++) {
        if (len[j] < HX_SPAN) { ctx->err = "sequence shorter than the HIndex shape (17 bases)"; return LNR_ERR_LIMIT; }
        u64 npos = len[j] - HX_SPAN + 1, size2 = npos / T;
        for (u32 t = 0; t < T; t++) {                                    // __createHsArray :745-760
            u64 chunk, start;
            if (t < npos - size2 * T) { chunk = size2 + 1; start = (size2 + 1) * t; }
            else { chunk = size2; start = len[j] + 1 - HX_SPAN - size2 * (T - t); }
            chunk_first.push_back((u32)pieces.size());
            u64 u = start;
            do {                                                         // (a chunk of no positions still has its hashInit: one empty piece)
                HxPiece c; c.seq_off = ix.seq_off[j]; c.seq_id = j; c.start = start; c.chunk = chunk;
                c.u = u; c.v = std::min(u + HX_PIECE, start + chunk); if (c.v < c.u) c.v = c.u;
                if (start + chunk - c.v < 64) c.v = start + chunk;       // no sliver at the end: the last piece holds the chunk's end rule
                c.first = u == start ? 1 : 0; c.out_base = stage; c.kt0 = ~0ULL; c.kinit = start; c.nc = ~0ULL; c.slen = len[j];
                stage += (c.v - c.u) / HX_STEP + 4;
                pieces.push_back(c);
                u = c.v;
            } while (u < start + chunk);
        }
    }
    chunk_first.push_back((u32)pieces.size());
    u32 npc = (u32)pieces.size(), nchk = (u32)chunk_first.size() - 1;
    DevBuf d_pc, fileX, body, d_po, d_cp, d_fn, d_fc, d_tc, Xs, bodies, Xs2, bodies2, cub, flag, cntX, tmp;
    lnr_status s;
    if ((s = upload_on(ctx->err, d_pc, pieces, sm)) != LNR_OK) return s;
    ENSURE(d_fn, (size_t)npc * 8 + 16); ENSURE(d_fc, (size_t)npc * 8 + 16); ENSURE(d_tc, (size_t)npc * 8 + 16);
    hipLaunchKernelGGL(k_hx_pre, dim3((npc + 63) / 64), dim3(64), 0, sm, ix.g.as<u8>(), d_pc.as<HxPiece>(), npc, d_fn.as<u64>(), d_fc.as<u64>(), d_tc.as<u64>()); KCHECK();
    {   // what a piece needs from its neighbours: where a jump over an N cluster lands behind it (nc), the chunk's first clean window
        // (kinit: the state its hashInit leaves) and where the first N enters a window of the chunk (kt0)
        std::vector<u64> fn(npc), fc(npc), tc(npc);
        HIPCK(hipMemcpyAsync(fn.data(), d_fn.p, (size_t)npc * 8, hipMemcpyDeviceToHost, sm));
        HIPCK(hipMemcpyAsync(fc.data(), d_fc.p, (size_t)npc * 8, hipMemcpyDeviceToHost, sm));
        HIPCK(hipMemcpyAsync(tc.data(), d_tc.p, (size_t)npc * 8, hipMemcpyDeviceToHost, sm));
        HIPCK(hipStreamSynchronize(sm));
        u64 carried = ~0ULL;
        for (i64 q = (i64)npc - 1; q >= 0; q--) {                                // pieces are in sequence order, positions ascending
            bool seq_last = q == (i64)npc - 1 || pieces[q + 1].seq_id != pieces[q].seq_id;
            if (seq_last) carried = tc[q];                                        // (position len is always clean: padding)
            pieces[q].nc = carried;
            if (fc[q] != ~0ULL) carried = fc[q];
        }
        for (u32 c = 0; c < nchk; c++) {
            u32 p0 = chunk_first[c], p1 = chunk_first[c + 1];
            u64 kt0 = ~0ULL;
            for (u32 q = p0; q < p1; q++) if (fn[q] != ~0ULL) { kt0 = fn[q] - 16; break; }
            u64 kinit = fc[p0] != ~0ULL ? fc[p0] : pieces[p0].nc;
            for (u32 q = p0; q < p1; q++) { pieces[q].kt0 = kt0; pieces[q].kinit = kinit; }
        }
        if ((s = upload_on(ctx->err, d_pc, pieces, sm)) != LNR_OK) return s;
    }
    ENSURE(fileX, stage * 4 + 16); ENSURE(body, stage * 8 + 16); ENSURE(d_po, (size_t)npc * sizeof(HxPieceOut) + 16);
    hipLaunchKernelGGL(k_hx_piece, dim3((npc + 63) / 64), dim3(64), 0, sm, ix.g.as<u8>(), d_pc.as<HxPiece>(), npc, fileX.as<u32>(), body.as<u64>(), d_po.as<HxPieceOut>()); KCHECK();
    std::vector<HxPieceOut> po(npc);
    HIPCK(hipMemcpyAsync(po.data(), d_po.p, (size_t)npc * sizeof(HxPieceOut), hipMemcpyDeviceToHost, sm));
    HIPCK(hipStreamSynchronize(sm));
    std::vector<HxCopy> cp(npc);
    u64 n = 0;
    for (u32 c = 0; c < nchk; c++) {
        u32 p0 = chunk_first[c], p1 = chunk_first[c + 1];
        bool have_prev = false; u32 prevX = 0, endX = 0; bool any_hashed = false; i64 last_emit = -1;
        for (u32 q = p0; q < p1; q++) {
            HxCopy k; k.src = pieces[q].out_base; k.n = po[q].cnt; k.patch = 0; k.patchX = 0; k.pad = 0;
            if (po[q].cnt) {
                if (q != p0 && have_prev && po[q].firstX == prevX) { k.src++; k.n--; }   // first sample of the piece repeats the X of the sample before it
                have_prev = true; prevX = po[q].lastX;
            }
            k.dst = n; n += k.n;
            if (k.n) last_emit = q;
            if (po[q].hashed) { any_hashed = true; endX = po[q].endX; }
            cp[q] = k;
        }
        if (last_emit >= 0 && any_hashed) { cp[(u32)last_emit].patch = 1; cp[(u32)last_emit].patchX = endX; }   // :801
    }
    if (n >= (1ULL << 31) - 4) { ctx->err = "too many HIndex samples"; return LNR_ERR_LIMIT; }
    if (n == 0) { ctx->err = "no HIndex samples"; return LNR_ERR_ARG; }
    ix.info.n_samples = n;
    if ((s = upload_on(ctx->err, d_cp, cp, sm)) != LNR_OK) return s;
    ENSURE(Xs, n * 4 + 16); ENSURE(bodies, n * 8 + 16); ENSURE(Xs2, n * 4 + 16); ENSURE(bodies2, n * 8 + 16);
    hipLaunchKernelGGL(k_hx_compact, dim3(npc), dim3(256), 0, sm, d_cp.as<HxCopy>(), npc, fileX.as<u32>(), body.as<u64>(), Xs.as<u32>(), bodies.as<u64>()); KCHECK();
    // blocks by X ascending, bodies of a block descending (_sort_YSA_Block :600-611): sort by body descending, then stable by X.
    // (The reference's block sort is stable in file order, but the bodies of a block are re-sorted as whole words afterwards.)
    size_t tb1 = 0, tb2 = 0;
    HIPCK(rocprim::radix_sort_pairs_desc(nullptr, tb1, bodies.as<u64>(), bodies2.as<u64>(), Xs.as<u32>(), Xs2.as<u32>(), (size_t)n, 0u, 64u, sm));
    HIPCK(rocprim::radix_sort_pairs(nullptr, tb2, Xs2.as<u32>(), Xs.as<u32>(), bodies2.as<u64>(), bodies.as<u64>(), (size_t)n, 0u, (unsigned)HX_XBITS, sm));
    ENSURE(cub, std::max(tb1, tb2) + 16);
    HIPCK(rocprim::radix_sort_pairs_desc(cub.p, tb1, bodies.as<u64>(), bodies2.as<u64>(), Xs.as<u32>(), Xs2.as<u32>(), (size_t)n, 0u, 64u, sm));
    HIPCK(rocprim::radix_sort_pairs(cub.p, tb2, Xs2.as<u32>(), Xs.as<u32>(), bodies2.as<u64>(), bodies.as<u64>(), (size_t)n, 0u, (unsigned)HX_XBITS, sm));
    ENSURE(flag, (n + 1) * 4 + 16); ENSURE(cntX, ((size_t)1 << HX_XBITS) * 4);
    HIPCK(hipMemsetAsync(cntX.p, 0, ((size_t)1 << HX_XBITS) * 4, sm));
    HIPCK(hipMemsetAsync(flag.as<i32>() + n, 0, 4, sm));
    hipLaunchKernelGGL(k_hx_flags, dim3((u32)((n + 255) / 256)), dim3(256), 0, sm, Xs.as<u32>(), n, flag.as<i32>(), cntX.as<u32>()); KCHECK();
    if ((s = dev_scan_i32(ctx, flag.as<i32>(), flag.as<i32>(), n + 1, tmp)) != LNR_OK) return s;
    i32 ndist = 0;
    HIPCK(hipMemcpyAsync(&ndist, flag.as<i32>() + n, 4, hipMemcpyDeviceToHost, sm));
    HIPCK(hipStreamSynchronize(sm));
    u64 ysa_len = n + (u64)ndist + 2;
    ix.info.hs_len = ysa_len;
    ENSURE(ix.hs, ysa_len * 8 + 64);
    hipLaunchKernelGGL(k_hx_assemble, dim3((u32)((n + 255) / 256)), dim3(256), 0, sm, Xs.as<u32>(), bodies.as<u64>(), n, flag.as<i32>(), cntX.as<u32>(), ix.hs.as<u64>(), ysa_len); KCHECK();
    if (n - (u64)ndist <= 2) {
        // _createYSA :1336-1352, "abort the last block": with fewer than three merges (every sample is a block of its own before the blocks of
        // one X are merged: merges = n - ndist) the reference ends ysa in front of its last block -- two zero heads there, emptyDir on them --
        // and leaves behind what its compaction had put after them: the block's other bodies, unsorted (file order) and with their Y, and
        // in the last two words what the moves by `merges` places did not overwrite.  A reference of a few dozen samples; a few words, patched here.
        u32 merges = (u32)(n - (u64)ndist), take = (u32)std::min<u64>(n, 3);
        u32 hx[3]; u64 hb[3];
        HIPCK(hipMemcpyAsync(hx, Xs.as<u32>() + (n - take), take * 4, hipMemcpyDeviceToHost, sm));
        HIPCK(hipMemcpyAsync(hb, bodies.as<u64>() + (n - take), take * 8, hipMemcpyDeviceToHost, sm));
        HIPCK(hipStreamSynchronize(sm));
        u32 xl = hx[take - 1], m = 0;
        std::vector<u64> fb;                                                  // the last block's bodies in file order: (sequence, position) ascending
        for (u32 q = take; q-- > 0 && hx[q] == xl;) { fb.push_back(hb[q]); m++; }
        std::sort(fb.begin(), fb.end(), [](u64 a, u64 b) { return (a & HS_MASK40) < (b & HS_MASK40); });
        std::vector<u64> w(m + 3, 0);                                         // from the block's head on: 0, 0, bodies 2 .. m, then the two last words
        for (u32 r = 1; r < m; r++) w[1 + r] = fb[r];
        if (merges == 1) w[m + 1] = fb[m - 1];
        if (merges == 2) { w[m + 1] = hs_head(2, xl); w[m + 2] = fb[m - 1]; }
        HIPCK(hipMemcpyAsync(ix.hs.as<u64>() + (ysa_len - 2 - (m + 1)), w.data(), w.size() * 8, hipMemcpyHostToDevice, sm));
    }
    HIPCK(hipStreamSynchronize(sm));
    return hx_derive(ctx);
}

void set_index_layout(lnr_ctx *ctx, const u64 *len, u32 nseq, u32 T) {
    Index &ix = ctx->ix;
    ix.seq_len.assign(len, len + nseq);
    ix.seq_off.assign(nseq, 0);
    ix.f2_off.assign(nseq + 1, 0);
    u64 o = 0, maxlen = 0;
    for (u32 i = 0; i < nseq; i++) {
        ix.seq_off[i] = o;
        o += align_up(len[i] + SEQ_PAD, 64);
        ix.f2_off[i + 1] = ix.f2_off[i] + genome_feature_count(len[i], T);
        maxlen = std::max(maxlen, len[i]);
    }
    ix.info.nseq = nseq;
    ix.info.genome_bytes = o;
    ix.info.dir_len = ctx->opts.index_type == 2 ? ((u64)1 << HX_XBITS) + 1 : ((u64)1 << 26) + 1;
    ix.info.f2_len = ix.f2_off[nseq];
    ix.nbins = (u32)((maxlen + (2ULL << 20)) / 30000 + 2);
}

lnr_status upload_index_layout(lnr_ctx *ctx) {
    Index &ix = ctx->ix; hipStream_t sm = ctx->stream();
    lnr_status s;
    if ((s = upload_on(ctx->err, ix.d_seq_off, ix.seq_off, sm)) != LNR_OK) return s;
    if ((s = upload_on(ctx->err, ix.d_f2_off, ix.f2_off, sm)) != LNR_OK) return s;
    if ((s = upload_on(ctx->err, ix.d_seq_len, ix.seq_len, sm)) != LNR_OK) return s;
    return LNR_OK;
}
}  // namespace

extern "C" {

lnr_status lnr_index_build(lnr_ctx *ctx, const uint8_t *const *seq, const uint64_t *len, uint32_t nseq, uint32_t T) {
    if (!ctx) return LNR_ERR_ARG;
    if (!seq || !len || nseq == 0) { ctx->err = "null/empty sequence set"; return LNR_ERR_ARG; }
    if (nseq >= 1024) { ctx->err = "at most 1023 reference sequences (cord id field; linear.cpp:107)"; return LNR_ERR_LIMIT; }
    if (T == 0) T = 1;
    for (u32 i = 0; i < nseq; i++) {
        if (!seq[i]) { ctx->err = "null sequence pointer"; return LNR_ERR_ARG; }
        if (len[i] >= (1ULL << 30) - (1ULL << 20)) { ctx->err = "sequence too long for the 30-bit x field (cords.cpp:13-14)"; return LNR_ERR_LIMIT; }
    }
    if (in_flight(ctx)) { ctx->err = "lnr_index_build: batches are in flight"; return LNR_ERR_ARG; }
    DevGuard dg_(ctx->device);
    Index &ix = ctx->ix; hipStream_t sm = ctx->stream();
    ix.has_index = false;
    set_index_layout(ctx, len, nseq, T);
    ix.info.layout_threads = T;
    lnr_status s;
    if ((s = upload_index_layout(ctx)) != LNR_OK) return s;
    // genome: padded device copy (zero padding pins the reference's out-of-range reads to 'A')
    ENSURE(ix.g, ix.info.genome_bytes + 64);
    HIPCK(hipMemsetAsync(ix.g.p, 0, ix.info.genome_bytes + 64, sm));
    for (u32 i = 0; i < nseq; i++)
        if (len[i]) HIPCK(hipMemcpyAsync(ix.g.as<u8>() + ix.seq_off[i], seq[i], len[i], hipMemcpyDefault, sm));   // host or device source
    Timer tm; tm.init();
    tm.start(sm);
    {   // ordinals above 4 -> N
        u64 n16 = (ix.info.genome_bytes + 64) / 16;
        hipLaunchKernelGGL(k_clamp_bases, dim3((u32)((n16 + 255) / 256)), dim3(256), 0, sm, ix.g.as<u8>(), n16);
    }
    if (ctx->opts.index_type == 2) {   // HIndex: own build; genome features as for the DIndex
        lnr_status hst = build_hindex(ctx, len, nseq, T);
        if (hst != LNR_OK) return hst;
        ENSURE(ix.f2, std::max<u64>(ix.info.f2_len * sizeof(F96), 16));
        if (ix.info.f2_len)
            hipLaunchKernelGGL(k_f2, dim3((u32)((ix.info.f2_len + 255) / 256)), dim3(256), 0, sm, ix.g.as<u8>(), ix.d_seq_off.as<u64>(), ix.d_f2_off.as<u64>(), nseq,
                               ix.info.f2_len, ix.f2.as<F96>());
        tm.stop(sm);
        hipError_t he = hipStreamSynchronize(sm);
        if (he == hipSuccess) he = hipGetLastError();
        if (he != hipSuccess) { ctx->err = std::string("HIndex build: ") + hipGetErrorString(he); return LNR_ERR_HIP; }
        ix.info.build_ms = tm.ms();
        ix.has_index = true;
        return LNR_OK;
    }
    // chunks of the T-thread layout (index_util.cpp:1654-1666)
    std::vector<ChunkDesc> chunks;
    u64 nsamp = 0;
    for (u32 i = 0; i < nseq; i++)
        for (u32 t = 0; t < T; t++) {
            i64 ts, te;
            chunk_bounds(len[i], T, t, ts, te);
            if (ts >= te) continue;
            u64 ns = chunk_num_samples(ts, te);
            if (!ns) continue;
            ChunkDesc c; c.seq_off = ix.seq_off[i]; c.t_str = ts; c.samp_base = nsamp; c.nsamp = (u32)ns; c.seq_id = i; c.ks = 0; c.C = 0;
            chunks.push_back(c);
            nsamp += ns;
        }
    if (nsamp >= (1ULL << 32) - 2) { ctx->err = "too many genome samples"; return LNR_ERR_LIMIT; }
    ix.info.n_samples = nsamp;
    u64 dir_len = ix.info.dir_len;
    ENSURE(ix.dir, dir_len * 4);
    DevBuf d_chunks, Xs, vals, cnt, blk, scan_tmp, big, nbig;
    ENSURE(cnt, dir_len * 4);
    HIPCK(hipMemsetAsync(cnt.p, 0, dir_len * 4, sm));
    u64 hs_len = 0;
    if (nsamp) {
        if ((s = upload_on(ctx->err, d_chunks, chunks, sm)) != LNR_OK) return s;
        ENSURE(Xs, nsamp * 4);
        ENSURE(vals, nsamp * 8);
        u32 nch = (u32)chunks.size();
        hipLaunchKernelGGL(k_ix_chunk_const, dim3(nch), dim3(256), 0, sm, ix.g.as<u8>(), (u64)(ix.info.genome_bytes + 64), d_chunks.as<ChunkDesc>(), nch); KCHECK();
        hipLaunchKernelGGL(k_ix_sample, dim3((u32)((nsamp + 255) / 256)), dim3(256), 0, sm, ix.g.as<u8>(), d_chunks.as<ChunkDesc>(), nch, nsamp, Xs.as<u32>(), vals.as<u64>()); KCHECK();
        u32 nrb = (u32)((nsamp + REC_BLK - 1) / REC_BLK);
        ENSURE(blk, (size_t)nrb * 4);
        hipLaunchKernelGGL(k_ix_start_blk, dim3(nrb), dim3(REC_TPB), 0, sm, Xs.as<u32>(), nsamp, blk.as<u32>()); KCHECK();
        hipLaunchKernelGGL(k_max_top, dim3(1), dim3(1024), 0, sm, blk.as<u32>(), nrb); KCHECK();
        hipLaunchKernelGGL(k_ix_rec, dim3(nrb), dim3(REC_TPB), 0, sm, Xs.as<u32>(), nsamp, blk.as<u32>(), cnt.as<i32>()); KCHECK();
        hipLaunchKernelGGL(k_ix_omit, dim3((u32)((dir_len + 255) / 256)), dim3(256), 0, sm, cnt.as<i32>(), dir_len); KCHECK();
    }
    if ((s = dev_scan_i32(ctx, cnt.as<i32>(), ix.dir.as<i32>(), dir_len, scan_tmp)) != LNR_OK) return s;
    i32 total = 0;
    HIPCK(hipMemcpyAsync(&total, ix.dir.as<i32>() + (dir_len - 1), 4, hipMemcpyDeviceToHost, sm));
    HIPCK(hipStreamSynchronize(sm));
    hs_len = (u64)total;
    ENSURE(ix.hs, std::max<u64>(hs_len * 8, 16));
    if (nsamp && hs_len) {
        HIPCK(hipMemsetAsync(cnt.p, 0, dir_len * 4, sm));
        hipLaunchKernelGGL(k_ix_scatter, dim3((u32)((nsamp + 255) / 256)), dim3(256), 0, sm, Xs.as<u32>(), vals.as<u64>(), nsamp, ix.dir.as<i32>(), cnt.as<i32>(), ix.hs.as<u64>()); KCHECK();
        ENSURE(big, (hs_len / 33 + 2) * 4);
        ENSURE(nbig, 16);
        HIPCK(hipMemsetAsync(nbig.p, 0, 4, sm));
        u64 nb = dir_len - 1;
        hipLaunchKernelGGL(k_ix_sort_small, dim3((u32)((nb + 255) / 256)), dim3(256), 0, sm, ix.dir.as<i32>(), nb, ix.hs.as<u64>(), big.as<u32>(), nbig.as<u32>()); KCHECK();
        u32 hb = 0;
        HIPCK(hipMemcpyAsync(&hb, nbig.p, 4, hipMemcpyDeviceToHost, sm));
        HIPCK(hipStreamSynchronize(sm));
        if (hb) {
            hipLaunchKernelGGL(k_ix_sort_big, dim3(hb), dim3(64), 0, sm, ix.dir.as<i32>(), ix.hs.as<u64>(), big.as<u32>(), hb); KCHECK();
        }
    }
    if ((s = build_seed_view(ctx)) != LNR_OK) return s;   // bucket bitmap, bucket lines, overflow lines for the seed kernel
    // genome window features
    ENSURE(ix.f2, std::max<u64>(ix.info.f2_len * sizeof(F96), 16));
    if (ix.info.f2_len) {
        hipLaunchKernelGGL(k_f2, dim3((u32)((ix.info.f2_len + 255) / 256)), dim3(256), 0, sm, ix.g.as<u8>(), ix.d_seq_off.as<u64>(), ix.d_f2_off.as<u64>(), nseq,
                           ix.info.f2_len, ix.f2.as<F96>()); KCHECK();
    }
    tm.stop(sm);
    HIPCK(hipStreamSynchronize(sm));
    ix.info.build_ms = tm.ms();
    ix.info.hs_len = hs_len;
    ix.has_index = true;
    return LNR_OK;
}

lnr_status lnr_index_info_get(const lnr_ctx *ctx, lnr_index_info *info) {
    if (!ctx || !info) return LNR_ERR_ARG;
    if (!ctx->ix.has_index) return LNR_ERR_NO_INDEX;
    *info = ctx->ix.info;
    return LNR_OK;
}

lnr_status lnr_index_export(lnr_ctx *ctx, int32_t *dir, uint64_t *hs, int32_t *f2, uint64_t *f2_off) {
    if (!ctx) return LNR_ERR_ARG;
    if (!ctx->ix.has_index) return LNR_ERR_NO_INDEX;
    DevGuard dg_(ctx->device);
    Index &ix = ctx->ix; hipStream_t sm = ctx->stream();
    HIPCK(hipStreamSynchronize(sm));
    if (dir) HIPCK(hipMemcpy(dir, ix.dir.p, ix.info.dir_len * 4, hipMemcpyDeviceToHost));
    if (hs && ix.info.hs_len) HIPCK(hipMemcpy(hs, ix.hs.p, ix.info.hs_len * 8, hipMemcpyDeviceToHost));
    if (f2 && ix.info.f2_len) {
        std::vector<F96> tmp(ix.info.f2_len);
        HIPCK(hipMemcpy(tmp.data(), ix.f2.p, ix.info.f2_len * sizeof(F96), hipMemcpyDeviceToHost));
        for (u64 i = 0; i < ix.info.f2_len; i++) { f2[3 * i] = tmp[i].v0; f2[3 * i + 1] = tmp[i].v1; f2[3 * i + 2] = tmp[i].v2; }
    }
    if (f2_off) memcpy(f2_off, ix.f2_off.data(), ix.f2_off.size() * 8);
    return LNR_OK;
}

lnr_status lnr_index_alloc(lnr_ctx *ctx, const lnr_index_info *info, const uint64_t *seq_len) {
    if (!ctx || !info || !seq_len || info->nseq == 0 || info->nseq >= 1024) return LNR_ERR_ARG;
    if (in_flight(ctx)) { ctx->err = "lnr_index_alloc: batches are in flight"; return LNR_ERR_ARG; }
    DevGuard dg_(ctx->device);
    Index &ix = ctx->ix; hipStream_t sm = ctx->stream();
    ix.has_index = false;
    set_index_layout(ctx, seq_len, info->nseq, info->layout_threads ? info->layout_threads : 1);
    if (ix.info.genome_bytes != info->genome_bytes || ix.info.f2_len != info->f2_len || ix.info.dir_len != info->dir_len) {
        ctx->err = "index info does not match the sequence lengths";
        return LNR_ERR_ARG;
    }
    ix.info = *info;
    lnr_status s;
    if ((s = upload_index_layout(ctx)) != LNR_OK) return s;
    ENSURE(ix.g, ix.info.genome_bytes + 64);
    ENSURE(ix.dir, ix.info.dir_len * 4);
    ENSURE(ix.hs, std::max<u64>(ix.info.hs_len * 8, 16));
    ENSURE(ix.f2, std::max<u64>(ix.info.f2_len * sizeof(F96), 16));
    HIPCK(hipStreamSynchronize(sm));
    return LNR_OK;
}
lnr_status lnr_index_blob(lnr_ctx *ctx, uint32_t which, void **d_ptr, uint64_t *bytes) {
    if (!ctx || !d_ptr || !bytes) return LNR_ERR_ARG;
    switch (which) {
        case 0: *d_ptr = ctx->ix.g.p; *bytes = ctx->ix.info.genome_bytes; break;
        case 1: *d_ptr = ctx->ix.dir.p; *bytes = ctx->ix.info.dir_len * 4; break;
        case 2: *d_ptr = ctx->ix.hs.p; *bytes = ctx->ix.info.hs_len * 8; break;
        case 3: *d_ptr = ctx->ix.f2.p; *bytes = ctx->ix.info.f2_len * sizeof(F96); break;
        default: return LNR_ERR_ARG;
    }
    if (!*d_ptr) return LNR_ERR_NO_INDEX;
    return LNR_OK;
}
lnr_status lnr_index_adopt(lnr_ctx *ctx) {
    if (!ctx) return LNR_ERR_ARG;
    if (!ctx->ix.g.p || !ctx->ix.dir.p || !ctx->ix.hs.p || !ctx->ix.f2.p) return LNR_ERR_NO_INDEX;
    if (in_flight(ctx)) { ctx->err = "lnr_index_adopt: batches are in flight"; return LNR_ERR_ARG; }
    DevGuard dg_(ctx->device);
    Index &ix = ctx->ix; hipStream_t sm = ctx->stream();
    { lnr_status st_ = ctx->opts.index_type == 2 ? hx_derive(ctx) : build_seed_view(ctx); if (st_ != LNR_OK) return st_; }   // derived structures: rebuilt from the received dir / hs (ysa)
    HIPCK(hipStreamSynchronize(sm));
    ix.has_index = true;
    return LNR_OK;
}

// ---- one process, several GPUs: the index of ctxs[root] into the other contexts (RCCL between devices, device copies inside one)
namespace {
struct Rccl {
    void *lib = nullptr;
    int (*CommInitAll)(void **, int, const int *) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*Broadcast)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool load() {
        if (lib) return true;
        for (const char *nm : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) { lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL); if (lib) break; }
        if (!lib) return false;
        CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll"); CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        Broadcast = (decltype(Broadcast))dlsym(lib, "ncclBroadcast"); GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd"); GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        return CommInitAll && CommDestroy && Broadcast && GroupStart && GroupEnd;
    }
};
Rccl g_rccl;
}  // namespace

lnr_status lnr_index_broadcast(lnr_ctx *const *ctxs, uint32_t n, uint32_t root, double *seconds) {
    if (!ctxs || n == 0 || root >= n) return LNR_ERR_ARG;
    for (uint32_t i = 0; i < n; i++) if (!ctxs[i]) return LNR_ERR_ARG;
    lnr_ctx *src = ctxs[root];
    if (!src->ix.has_index) { src->err = "lnr_index_broadcast: the root context has no index"; return LNR_ERR_NO_INDEX; }
    auto t0 = std::chrono::steady_clock::now();
    lnr_status s;
    for (uint32_t i = 0; i < n; i++) {
        if (i == root) continue;
        if (ctxs[i]->opts.index_type != src->opts.index_type) { ctxs[i]->err = "lnr_index_broadcast: contexts with different index types"; return LNR_ERR_ARG; }
        if ((s = lnr_index_alloc(ctxs[i], &src->ix.info, src->ix.seq_len.data())) != LNR_OK) return s;
    }
    // one representative context per device (the root for its own); RCCL between the representatives
    std::vector<uint32_t> rep;
    rep.push_back(root);
    for (uint32_t i = 0; i < n; i++) {
        bool seen = false;
        for (uint32_t r : rep) seen = seen || ctxs[r]->device == ctxs[i]->device;
        if (!seen) rep.push_back(i);
    }
    { DevGuard dg_(src->device); HIPCK_CTX(src, hipStreamSynchronize(src->stream())); }
    if (rep.size() > 1) {
        if (!g_rccl.load()) { src->err = "lnr_index_broadcast: librccl could not be loaded"; return LNR_ERR_HIP; }
        std::vector<int> devs;
        for (uint32_t r : rep) devs.push_back(ctxs[r]->device);
        std::vector<void *> comms(rep.size(), nullptr);
        int rc = g_rccl.CommInitAll(comms.data(), (int)rep.size(), devs.data());
        if (rc != 0) { src->err = std::string("ncclCommInitAll: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error"); return LNR_ERR_HIP; }
        for (uint32_t which = 0; which < 4 && rc == 0; which++) {
            g_rccl.GroupStart();
            for (size_t k = 0; k < rep.size() && rc == 0; k++) {
                lnr_ctx *c = ctxs[rep[k]];
                void *p = nullptr; uint64_t bytes = 0;
                if (lnr_index_blob(c, which, &p, &bytes) != LNR_OK) { rc = -1; break; }
                (void)hipSetDevice(c->device);
                rc = g_rccl.Broadcast(p, p, (size_t)bytes, /* ncclUint8 */ 1, /* root = rep[0] */ 0, comms[k], c->stream());
            }
            int rc2 = g_rccl.GroupEnd();
            if (rc == 0) rc = rc2;
        }
        for (size_t k = 0; k < rep.size(); k++) { lnr_ctx *c = ctxs[rep[k]]; (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream()); }
        for (void *cm : comms) if (cm) g_rccl.CommDestroy(cm);
        (void)hipSetDevice(src->device);
        if (rc != 0) { src->err = std::string("ncclBroadcast: ") + (rc > 0 && g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error"); return LNR_ERR_HIP; }
    }
    // contexts that share a device with a representative: device-to-device copies from it
    for (uint32_t i = 0; i < n; i++) {
        if (i == root) continue;
        bool is_rep = false; uint32_t from = root;
        for (uint32_t r : rep) { if (r == i) is_rep = true; if (ctxs[r]->device == ctxs[i]->device) from = r; }
        if (!is_rep) {
            DevGuard dg_(ctxs[i]->device);
            for (uint32_t which = 0; which < 4; which++) {
                void *ps = nullptr, *pd = nullptr; uint64_t b1 = 0, b2 = 0;
                if (lnr_index_blob(ctxs[from], which, &ps, &b1) != LNR_OK || lnr_index_blob(ctxs[i], which, &pd, &b2) != LNR_OK || b1 != b2) return LNR_ERR_INTERNAL;
                HIPCK_CTX(ctxs[i], hipMemcpyAsync(pd, ps, b1, hipMemcpyDeviceToDevice, ctxs[i]->stream()));
            }
            HIPCK_CTX(ctxs[i], hipStreamSynchronize(ctxs[i]->stream()));
        }
    }
    for (uint32_t i = 0; i < n; i++) if (i != root && (s = lnr_index_adopt(ctxs[i])) != LNR_OK) return s;
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return LNR_OK;
}
}  // extern "C"
