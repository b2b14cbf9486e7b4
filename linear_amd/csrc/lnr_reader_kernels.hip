// lnr_reader_kernels.hip -- the GPU side of the reader (lnr_reader_next_dev): FASTA / FASTQ text -> Dna5 ordinals back to back + read
// offsets in HBM.  gfx950, wave64.  Every decision comes from lnr_reader_hd.h, the same text the CPU test pins.  BAM records (further
// down: k_bam_find and its siblings) come from the same device text; their decisions are lnr_bam_hd.h's.
//
// Three steps per window of text, on the reader's own stream:
//   k_rd_measure   one workgroup = one wave per tile of RD_TILE bytes: the tile goes to LDS by 16-byte loads, the wave walks it in groups
//                  of 64 bytes, lane = byte; the byte classes are wave ballots, the counts popcounts of them; one Sum per tile
//   k_rd_scan      one workgroup: every thread folds its share of the tile summaries, the shares are scanned, every tile gets the state at
//                  its first byte (Carry); then the take is decided on the device (lnr_rd::plan_of / take_group / result_of): the wave
//                  looks once more at the one tile that holds the last record start within the limits
//   k_rd_emit      the walk again with the carried state: a base lane stores its ordinal at (bases before it) -- position by ballot and
//                  prefix popcount, guarded by the number of bases the scan chose; a record-start lane stores off[k] and the header begin,
//                  the lane of a header's '\n' the header end.  No atomics; the only divergence is on lanes that hold a record boundary.
// The text of a mapped file is pageable: it goes up through two pinned staging buffers that host threads fill in turn, and the tiles of a
// chunk are measured while the next chunk is copied.  A gzip file is inflated straight into ONE pinned buffer by the caller, the whole window
// before its copy starts: the inflate is serial and takes over 95 % of such a call, so a second buffer would hide next to nothing.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "lnr_reader_hd.h"
#include "lnr_reader_hook.h"
#if defined(__HIP_DEVICE_COMPILE__)
#define LNR_INFLATE_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))      // the decoder's state is the same in every lane
#endif
#include "lnr_inflate_hd.h"
#include "lnr_bam_hd.h"
#include "lnr_gunzip_hd.h"

namespace {

using namespace lnr_rd;

constexpr u32 RD_TILE = 4096;                  // bytes of text per workgroup
constexpr u32 SCAN_THREADS = 256;
constexpr u64 RD_CHUNK = 16ULL << 20;          // bytes per staging buffer (a multiple of RD_TILE)

__device__ __forceinline__ void load_tile(const u8 *text, u64 t0, u8 *lds) {        // the buffer is padded to whole tiles
    const uint4 *src = reinterpret_cast<const uint4 *>(text + t0);
    for (u32 i = threadIdx.x & 63; i < RD_TILE / 16; i += 64) reinterpret_cast<uint4 *>(lds)[i] = src[i];
    __syncthreads();
}
__device__ __forceinline__ Masks group_masks(int fmt, u32 bits) {
    Masks m;
    m.valid = __ballot(bits & 1u); m.nl = __ballot(bits & 2u); m.keep = __ballot(bits & 8u);
    m.gt = 0; m.wsbad = 0; m.notat = 0; m.notplus = 0;
    if (fmt == FASTA) m.gt = __ballot(bits & 4u);
    else { m.wsbad = __ballot(bits & 16u); m.notat = __ballot(bits & 32u); m.notplus = __ballot(bits & 64u); }
    return m;
}

__global__ __launch_bounds__(64) void k_rd_measure(const u8 *text, u64 len, int fmt, u32 tile0, Sum *sums) {
    __shared__ __attribute__((aligned(16))) u8 lds[RD_TILE];
    const u32 lane = threadIdx.x, tile = tile0 + blockIdx.x;
    const u64 t0 = (u64)tile * RD_TILE, tend = t0 + RD_TILE < len ? t0 + RD_TILE : len;
    load_tile(text, t0, lds);
    u8 prevc = t0 ? text[t0 - 1] : (u8)'\n';
    FaState fa = fa_begin(prevc == '\n', 2, 0, 0);
    FqState fq = fq_begin(prevc == '\n');
    for (u64 g = t0; g < tend; g += 64) {
        const u32 o = (u32)(g - t0) + lane;
        const u8 c = lds[o], p = lane ? lds[o - 1] : prevc;
        const Masks m = group_masks(fmt, g + lane < tend ? byte_bits(fmt, c, p) : 0u);
        if (fmt == FASTA) { Out out; fa_step(fa, m, g, out); }
        else fq_measure_step(fq, m, g);
        prevc = lds[(u32)(g - t0) + 63];
    }
    if (lane == 0) sums[tile] = fmt == FASTA ? fa_sum(fa) : fq.s;
}

struct ScanArgs { const u8 *text; const Sum *sums; Carry *carry; u32 nt; Limits L; Result *res; u64 *d_off; u64 rec_base, base_base; };

// record starts of tile `tile` against the limits (one wave)
__device__ void take_tile(const ScanArgs &A, const Plan &P, u32 tile, const Carry &c, const u8 *lds, Take &t) {
    const u32 lane = threadIdx.x & 63;
    const u64 t0 = (u64)tile * RD_TILE, tend = t0 + RD_TILE < A.L.len ? t0 + RD_TILE : A.L.len;
    const u8 prevc = t0 ? A.text[t0 - 1] : (u8)'\n';
    FaState fa = fa_begin(prevc == '\n', c.st, c.kept, c.rec);
    FqEmit fq{c.kept, c.nl, prevc == '\n' ? 1u : 0u};
    for (u64 g = t0; g < tend; g += 64) {
        const u8 ch = lds[(u32)(g - t0) + lane];
        const Masks m = group_masks(A.L.fmt, g + lane < tend ? byte_bits(A.L.fmt, ch, 0) & 15u : 0u);
        const u64 kept0 = A.L.fmt == FASTA ? fa.kept : fq.kept, rec0 = fa.recs;
        const u32 line0 = fq.l;
        Out o;
        if (A.L.fmt == FASTA) fa_step(fa, m, g, o); else fq_emit_step(fq, m, o);
        take_group(A.L, P, o, m, rec0, line0, kept0, t);
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void k_rd_scan(ScanArgs A) {
    __shared__ Sum part[SCAN_THREADS];
    __shared__ Sum total;
    __shared__ u32 best[SCAN_THREADS][2];
    __shared__ u32 sel[2];
    __shared__ __attribute__((aligned(16))) u8 lds[RD_TILE];
    const u32 t = threadIdx.x, chunk = (A.nt + SCAN_THREADS - 1) / SCAN_THREADS;
    const u32 lo = (u64)t * chunk < A.nt ? t * chunk : A.nt, hi = lo + chunk < A.nt ? lo + chunk : A.nt;
    Sum S = sum_identity();
    for (u32 i = lo; i < hi; i++) S = sum_combine(S, A.sums[i]);
    part[t] = S;
    __syncthreads();
    if (t == 0) {
        Sum run = sum_identity();
        for (u32 i = 0; i < SCAN_THREADS; i++) { const Sum v = part[i]; part[i] = run; run = sum_combine(run, v); }
        total = run;
    }
    __syncthreads();
    const Plan P = plan_of(A.L, total);
    S = part[t];
    u32 b1 = NONE, b2 = NONE;
    for (u32 i = lo; i < hi; i++) {
        const Sum T = A.sums[i];
        Carry c = carry_of(S);
        if (A.L.fmt != FASTA) c.kept = S.cnt[1];
        A.carry[i] = c;
        if (tile_candidate(A.L, P, S, T)) { b2 = b1; b1 = i; }
        S = sum_combine(S, T);
    }
    best[t][0] = b1; best[t][1] = b2;
    __syncthreads();
    if (t == 0) {                                    // the last two candidate tiles (shares are in tile order)
        u32 s0 = NONE, s1 = NONE;
        for (int i = SCAN_THREADS - 1; i >= 0 && s1 == NONE; i--)
            for (int k = 0; k < 2; k++) {
                const u32 v = best[i][k];
                if (v == NONE) continue;
                if (s0 == NONE) s0 = v; else if (s1 == NONE) s1 = v;
            }
        sel[0] = s0; sel[1] = s1;
    }
    __syncthreads();
    Take tk; tk.n = 0; tk.bases = 0; tk.found = 0;
    for (int k = 0; k < 2; k++) {                    // one wave looks at the text of the chosen tile (every wave keeps to the barriers)
        const u32 tile = sel[k];
        if (tile == NONE) break;
        load_tile(A.text, (u64)tile * RD_TILE, lds);
        if (t < 64 && !tk.found) take_tile(A, P, tile, A.carry[tile], lds, tk);
        __syncthreads();
    }
    if (t == 0) {
        const Result r = result_of(A.L, P, tk);
        *A.res = r;
        A.d_off[A.rec_base + r.n] = A.base_base + r.bases;
    }
}

struct EmitArgs { const u8 *text; u64 len; int fmt; const Carry *carry; Result *res; u64 rec_base, base_base; u8 *out; u64 *d_off; u64 *hdr; };

__global__ __launch_bounds__(64) void k_rd_emit(EmitArgs A) {
    __shared__ __attribute__((aligned(16))) u8 lds[RD_TILE];
    const u32 lane = threadIdx.x, tile = blockIdx.x;
    const u64 t0 = (u64)tile * RD_TILE, tend = t0 + RD_TILE < A.len ? t0 + RD_TILE : A.len;
    const u64 n = A.res->n, bases = A.res->bases;
    const Carry c = A.carry[tile];
    if (c.kept >= bases && (A.fmt == FASTA ? c.rec : c.nl / 4) > n) return;      // the whole tile lies behind the take
    load_tile(A.text, t0, lds);
    const u8 prevc = t0 ? A.text[t0 - 1] : (u8)'\n';
    FaState fa = fa_begin(prevc == '\n', c.st, c.kept, c.rec);
    FqEmit fq{c.kept, c.nl, prevc == '\n' ? 1u : 0u};
    const u64 bit = 1ULL << lane;
    for (u64 g = t0; g < tend; g += 64) {
        const u8 ch = lds[(u32)(g - t0) + lane];
        const u64 pos = g + lane;
        const Masks m = group_masks(A.fmt, pos < tend ? byte_bits(A.fmt, ch, 0) & 15u : 0u);
        const u64 kept0 = A.fmt == FASTA ? fa.kept : fq.kept, rec0 = fa.recs;
        const u32 line0 = fq.l;
        Out o;
        if (A.fmt == FASTA) fa_step(fa, m, g, o); else fq_emit_step(fq, m, o);
        const u64 idx = kept0 + popc(o.base & below(lane));
        if ((o.base & bit) && idx < bases) A.out[A.base_base + idx] = ordinal(ch);
        if ((o.rs | o.hdr) & bit) {                                              // lanes on a record boundary or in a header
            const u64 k = A.fmt == FASTA ? rec0 + popc(o.rs & (below(lane) | bit)) - 1 : (u64)(line0 + popc(m.nl & below(lane))) / 4;
            if (o.rs & bit) {
                if (k < n) { A.d_off[A.rec_base + k] = A.base_base + idx; A.hdr[2 * k] = pos + 1; }
                else if (k == n) A.res->consumed = pos;
            }
            if (k < n) {
                if (m.nl & bit) A.hdr[2 * k + 1] = pos;
                else if (pos + 1 == A.len) A.hdr[2 * k + 1] = A.len;
            }
        }
    }
}

// ---- BGZF: one wave inflates one block (lnr_inflate_hd.h) straight into the window's text in global memory.  Every lane runs the decoder
// with the same values (bit buffer, code tables in LDS); lane 0 stores literals, all lanes copy a match: byte i of it comes from byte
// (i mod distance) of the source, all of which the wave has stored before.  A workgroup-scope fence stands between those stores and the
// loads: on gfx950 it needs no vmcnt wait (a CU performs one wave's vector memory operations in issue order through its one L1, so the
// load sees the store), and it keeps the compiler from reordering them.  Then 64 slices of the text are CRC'd, one per lane, and combined.
struct WaveSink {
    u8 *out; u32 lane;
    __device__ void lit(u32 pos, u8 b) { if (lane == 0) out[pos] = b; }
    __device__ void match(u32 pos, u32 len, u32 dist) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        const u8 *src = out + (pos - dist);
        for (u32 i = lane; i < len; i += 64) out[pos + i] = src[dist >= len ? i : i % dist];
    }
    __device__ void stored(u32 pos, const u8 *src, u32 n) { for (u32 i = lane; i < n; i += 64) out[pos + i] = src[i]; }
};

__global__ __launch_bounds__(64) void k_bgzf_inflate(const u8 *comp, u64 comp_len, const lnr_rdgpu_bgzf_blk *tab, u32 nblk, u8 *text, u64 text_cap, u32 *status) {
    __shared__ lnr_inf::Tables T;
    const u32 b = blockIdx.x, lane = threadIdx.x;
    if (b >= nblk) return;
    const lnr_rdgpu_bgzf_blk B = tab[b];
    u32 st;
    if (B.coff > comp_len || B.clen > comp_len - B.coff || B.ooff > text_cap || B.isize > text_cap - B.ooff) st = lnr_inf::E_TABLE;
    else {
        WaveSink o{text + B.ooff, lane};
        st = lnr_inf::inflate_block(comp + B.coff, B.clen, o, B.isize, T);
        if (st == lnr_inf::OK) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            const u32 S = (B.isize + 63) / 64, a = lane * S < B.isize ? lane * S : B.isize, e = a + S < B.isize ? a + S : B.isize;
            u32 x = lnr_inf::crc_shift(lnr_inf::crc_of(o.out + a, e - a), B.isize - e);
            for (int d = 32; d; d >>= 1) x ^= (u32)__shfl_xor((int)x, d, 64);
            if (x != B.crc) st = lnr_inf::E_CRC;
        }
    }
    if (lane == 0) status[b] = st;
}

// header bytes (BAM: names) of the taken records -> one run of bytes the host reads (one wave per record).  STRIP_CR: trailing '\r' dropped
// as the host parser does for a header line; a BAM name is taken byte for byte
template <bool STRIP_CR>
__global__ __launch_bounds__(64) void k_rd_gather(const u8 *text, u64 len, const u64 *hdr, const u64 *dst_off, u64 n, u8 *dst, u64 dst_cap, u32 *lens) {
    const u64 k = blockIdx.x;
    if (k >= n) return;
    const u32 lane = threadIdx.x;
    const u64 hb = hdr[2 * k], o = dst_off[k];
    u64 he = hdr[2 * k + 1];
    if (hb > he || he > len || o > dst_cap || he - hb > dst_cap - o) { if (lane == 0) lens[k] = ~0u; return; }
    if (STRIP_CR) while (he > hb && text[he - 1] == '\r') he--;
    for (u64 i = lane; i < he - hb; i += 64) dst[o + i] = text[hb + i];
    if (lane == 0) lens[k] = (u32)(he - hb);
}

// ---- BAM input: the window's bytes are length-prefixed records, so record starts form a serial chain.  Every decision comes
// from lnr_bam_hd.h.  Separate launches on the reader's stream, no kernel waits for another workgroup:
//   k_bam_find     one wave per tile of BAM_TILE bytes GUESSES the tile's first record start -- 64 offsets at a time, lane = offset, the bytes
//                  staged through LDS by 16-byte loads, the first lane that passes rec_plausible wins -- and walks the chain from there to
//                  the tile's end, storing the starts in the tile's slice of a list
//   k_bam_stitch   one wave carries the TRUE position through the tiles in order (summaries loaded 64 at a time, stepped through by
//                  shuffles; serial in the number of tiles, and a repair walk is run by all lanes alike, as in k_bam_find): a tile whose guess is the true position is accepted whole, any other is walked again from the true position
//                  and its slice rewritten; then the prefix sum of the tiles' counts numbers the records
//   k_bam_meta     per record 16 bytes (offset, l_seq, flag, name length, CIGAR length) in record order: all the host sees of the records;
//                  the take (lnr_bam::take) runs there
//   k_bam_emit     the packed SEQ of every taken record -> ordinals at off[k], 16 bases per lane and store, a reverse-strand record
//                  mirrored and complemented; qualities, CIGAR and aux bytes are never read
//   k_rd_gather<false>  the names of the taken records, byte for byte (a header line loses its trailing '\r': not a name)
#ifndef LNR_BAM_TILE
#define LNR_BAM_TILE 131072                    // a multiple of BAM_STAGE; variant builds for the tile-size comparison set it (tools/measure/reader_bam_ab.py)
#endif
constexpr u32 BAM_TILE = LNR_BAM_TILE;                // bytes of records per wave of k_bam_find (32 KiB, 64 KiB and 128 KiB compared in profiles/r12)
constexpr u32 BAM_SLICE = BAM_TILE / lnr_bam::MIN_REC + 2;
constexpr u32 BAM_STAGE = 1024;                // offsets tested per LDS fill; a candidate's 36 bytes reach at most 35 bytes past them
constexpr u32 BAM_CHUNK = 4096;                // bases of one record per wave of k_bam_emit
u64 bam_text_cap(u64 tlen) { return ((tlen + BAM_TILE - 1) / BAM_TILE) * BAM_TILE + BAM_STAGE; }      // every LDS fill stays inside the buffer

struct BamStitch { u64 consumed, nrec, bad_off; u32 flag, repaired; };

__global__ __launch_bounds__(64) void k_bam_find(const u8 *text, u64 len, int n_ref, u32 *list, lnr_bam::Tile *tiles) {
    __shared__ __attribute__((aligned(16))) u8 lds[BAM_STAGE + 64];
    const u32 lane = threadIdx.x, tile = blockIdx.x;
    const u64 t0 = (u64)tile * BAM_TILE, tend = t0 + BAM_TILE < len ? t0 + BAM_TILE : len;
    u32 first = lnr_bam::NONE;
    for (u64 c = t0; c < tend && first == lnr_bam::NONE; c += BAM_STAGE) {
        __syncthreads();
        const uint4 *src = reinterpret_cast<const uint4 *>(text + c);             // c is a multiple of 16; the buffer holds bam_text_cap bytes
        for (u32 i = lane; i < (BAM_STAGE + 64) / 16; i += 64) reinterpret_cast<uint4 *>(lds)[i] = src[i];
        __syncthreads();
        for (u32 g = 0; g < BAM_STAGE && c + g < tend; g += 64) {
            const u64 p = c + g + lane;
            bool ok = p < tend && p + lnr_bam::HEAD <= len;
            if (ok) ok = lnr_bam::rec_plausible(lnr_bam::rec_fields(lds + g + lane), n_ref, text + p, len - p);      // (the name's NUL from global memory)
            const u64 m = __ballot(ok);
            if (m) { first = (u32)(c + g - t0) + ctz(m); break; }
        }
    }
    // the walk is serial and wave-uniform: all 64 lanes run it with the same values (the loads are one request per step, lane 0 stores);
    // nothing is gained over one lane, nothing lost either -- a cooperative walk would have to know the chain it is looking for
    const lnr_bam::Tile T = lnr_bam::speculate(text, len, n_ref, t0, tend, first, list + (u64)tile * BAM_SLICE, BAM_SLICE, lane == 0);
    if (lane == 0) tiles[tile] = T;
}

__global__ __launch_bounds__(64) void k_bam_stitch(const u8 *text, u64 len, int n_ref, u32 nt, u32 *list, const lnr_bam::Tile *tiles, u32 *cnt, u64 *prefix, BamStitch *out) {
    const u32 lane = threadIdx.x;
    u64 p = 0, nrec = 0;
    u32 flag = lnr_bam::CH_OK, repaired = 0, next = 0, base = lnr_bam::NONE;
    lnr_bam::Tile mine; mine.exit = 0; mine.first = lnr_bam::NONE; mine.count = 0; mine.flag = 0; mine.pad = 0;
    while (p < len && flag == lnr_bam::CH_OK) {
        const u32 t = (u32)(p / BAM_TILE);                                        // the tile that holds the true position (t < nt, t >= next)
        for (u32 i = next + lane; i < t; i += 64) cnt[i] = 0;                     // tiles that lie inside a record: no start, whatever they guessed
        repaired += t - next;
        if (base == lnr_bam::NONE || t >= base + 64) { base = t & ~63u; if (base + lane < nt) mine = tiles[base + lane]; }
        lnr_bam::Tile T;
        const int srcl = (int)(t - base);
        T.exit = (u64)(u32)__shfl((int)(u32)mine.exit, srcl, 64) | ((u64)(u32)__shfl((int)(u32)(mine.exit >> 32), srcl, 64) << 32);
        T.first = (u32)__shfl((int)mine.first, srcl, 64); T.count = (u32)__shfl((int)mine.count, srcl, 64); T.flag = (u32)__shfl((int)mine.flag, srcl, 64); T.pad = 0;
        const u64 t0 = (u64)t * BAM_TILE, tend = t0 + BAM_TILE < len ? t0 + BAM_TILE : len;
        u32 count = 0;
        flag = lnr_bam::stitch_tile(text, len, n_ref, p, t0, tend, T, list + (u64)t * BAM_SLICE, BAM_SLICE, count, repaired, lane == 0);
        if (count > BAM_SLICE) count = BAM_SLICE;                                 // (cannot happen: a valid record is MIN_REC bytes or more)
        if (lane == 0) cnt[t] = count;
        nrec += count;
        next = t + 1;
        if (flag == lnr_bam::CH_OK && p < tend) break;                             // (cannot happen: a walk that is not stopped leaves its tile)
    }
    for (u32 i = next + lane; i < nt; i += 64) cnt[i] = 0;                        // tiles behind the stop hold no record of this window
    __syncthreads();
    u64 run = 0;
    for (u32 b = 0; b < nt; b += 64) {                                            // record numbering: exclusive prefix sum of the counts
        const u32 v = b + lane < nt ? cnt[b + lane] : 0;
        u32 inc = v;
        for (int d = 1; d < 64; d <<= 1) { const u32 o = (u32)__shfl_up((int)inc, d, 64); if ((int)lane >= d) inc += o; }
        if (b + lane < nt) prefix[b + lane] = run + inc - v;
        run += (u32)__shfl((int)inc, 63, 64);
    }
    if (lane == 0) {
        prefix[nt] = run;
        BamStitch o; o.consumed = p; o.nrec = nrec; o.bad_off = p; o.flag = flag; o.repaired = repaired;
        *out = o;
    }
}

__global__ __launch_bounds__(64) void k_bam_meta(const u8 *text, u64 len, const u32 *list, const u32 *cnt, const u64 *prefix, u64 nrec, lnr_bam::Meta *meta) {
    const u32 tile = blockIdx.x, c = cnt[tile];
    const u64 k0 = prefix[tile];
    for (u32 j = threadIdx.x; j < c && j < BAM_SLICE; j += 64) {
        const u32 p = list[(u64)tile * BAM_SLICE + j];
        if (k0 + j < nrec && (u64)p + lnr_bam::HEAD <= len) meta[k0 + j] = lnr_bam::meta_of(p, lnr_bam::rec_fields(text + p));
    }
}

// one taken record: its packed SEQ in the window, its bases, where they go in the block, reverse strand; chunk = BAM_CHUNK bases of one record
struct BamJob { u64 dst; u32 seq, l_seq, rev, pad; };
struct BamChunk { u32 rec, start; };

__global__ __launch_bounds__(64) void k_bam_emit(const u8 *text, u64 len, const BamJob *jobs, const BamChunk *chunks, u32 nchunk, u8 *out, u64 out_cap) {
    if (blockIdx.x >= nchunk) return;
    const BamChunk C = chunks[blockIdx.x];
    const BamJob J = jobs[C.rec];
    const u64 l = J.l_seq;
    if ((u64)J.seq + (l + 1) / 2 > len || J.dst + l > out_cap) return;             // (checked on the host too)
    const u8 *seq = text + J.seq;
    // lnr_bam::base_at with the packed byte kept between the two bases it holds: a lane's run loads every byte once
    u64 held = ~0ULL; u8 cur = 0;
    const bool rev = J.rev != 0;
    auto base = [&](u64 j) -> u8 {
        const u64 s = rev ? l - 1 - j : j;
        if ((s >> 1) != held) { held = s >> 1; cur = seq[held]; }
        const u8 o = lnr_bam::nib2ord((s & 1) ? (cur & 15u) : (u32)(cur >> 4));
        return rev ? lnr_bam::ord_complement(o) : o;
    };
    // the wave's share of the record, in block coordinates; lanes take the 16-byte aligned segments that meet it
    const u64 a = J.dst + C.start, e = J.dst + (C.start + BAM_CHUNK < l ? C.start + BAM_CHUNK : l);
    for (u64 s0 = (a & ~15ULL) + 16ULL * threadIdx.x; s0 < e; s0 += 16ULL * 64) {
        if (s0 >= a && s0 + 16 <= e) {
            uint32_t wds[4];
            for (u32 q = 0; q < 4; q++) {
                u32 v = 0;
                for (u32 i = 0; i < 4; i++) v |= (u32)base(s0 + 4 * q + i - J.dst) << (8 * i);
                wds[q] = v;
            }
            *reinterpret_cast<uint4 *>(out + s0) = make_uint4(wds[0], wds[1], wds[2], wds[3]);
        } else {
            for (u64 x = s0 < a ? a : s0; x < e && x < s0 + 16; x++) out[x] = base(x - J.dst);
        }
    }
}

double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Buf { void *p = nullptr; u64 cap = 0; };
struct Pin { void *p = nullptr; u64 cap = 0; };
struct Block { Buf reads, off; Pin h_off; };
struct GzDev;
void gz_free(GzDev *G);

}  // namespace

struct lnr_rdgpu {
    int device = 0;
    u32 slots = 0;
    hipStream_t st = nullptr, s_copy = nullptr;
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> ev_m;               // pairs around the measure launches of a window
    Buf text, sums, carry, hdr, res;
    Pin up[2], stage, h_res, h_hdr;
    Block blk[8];
    double ms[5] = {0, 0, 0, 0, 0};
    // BGZF: compressed bytes, block table, status per block, a buffer for moves that overlap, the gathered headers
    Buf comp, btab, bstat, move, idoff, idbytes, idlen;
    Pin h_btab, h_bstat, h_head, h_idoff, h_idbytes, h_idlen;
    // BAM: the list of record starts (a slice per tile), the tiles' speculation, their counts and prefix sums, the stitch's result, the
    // per-record metadata, the emit's jobs and chunks
    Buf blist, btiles, bcnt, bprefix, bstitch, bmeta, bjobs, bchunks;
    Pin h_bstitch, h_bmeta, h_bjobs, h_bchunks;
    hipEvent_t ev_b[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_i[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms_inf[2] = {0, 0};
    GzDev *gz = nullptr;                        // plain gzip rounds (lnr_rdgpu_gzip_round): buffers and the window, on g->st
};

namespace {

struct DeviceGuard {                            // every entry works on its device (none given: the caller's) and leaves the caller's current device as it found it
    int prev = -1;
    hipError_t set = hipSuccess;
    explicit DeviceGuard(int device = -1) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (device >= 0) set = hipSetDevice(device); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define RD_CK(call, status)                                                                                              \
    do { hipError_t e_ = (call); if (e_ != hipSuccess) { snprintf(err, err_cap, "%s: %s", #call, hipGetErrorString(e_)); return (status); } } while (0)
#define RD_ON_DEVICE(g)                                                                                                  \
    DeviceGuard dg((g)->device);                                                                                         \
    if (dg.set != hipSuccess) { snprintf(err, err_cap, "hipSetDevice(g->device): %s", hipGetErrorString(dg.set)); return -3; }

int dev_need(Buf &b, u64 bytes, char *err, size_t err_cap) {
    if (bytes <= b.cap) return 0;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    const u64 want = bytes + bytes / 4 + 256;
    RD_CK(hipMalloc(&b.p, want), -4);
    b.cap = want;
    return 0;
}
bool pin_need(Pin &b, u64 bytes) {
    if (bytes <= b.cap) return true;
    if (b.p) { (void)hipHostFree(b.p); b.p = nullptr; b.cap = 0; }
    const u64 want = bytes + bytes / 4 + 4096;
    if (hipHostMalloc(&b.p, want, hipHostMallocDefault) != hipSuccess) { b.p = nullptr; return false; }
    b.cap = want;
    return true;
}
void par_copy(void *dst, const void *src, u64 n, u32 threads) {
    if (threads < 2 || n < (1u << 20)) { memcpy(dst, src, n); return; }
    std::vector<std::thread> th;
    const u64 share = (n + threads - 1) / threads;
    for (u32 t = 1; t < threads; t++) {
        const u64 a = share * t < n ? share * t : n, b = a + share < n ? a + share : n;
        if (b > a) th.emplace_back([=] { memcpy((char *)dst + a, (const char *)src + a, b - a); });
    }
    memcpy(dst, src, share < n ? share : n);
    for (auto &x : th) x.join();
}
void free_all(lnr_rdgpu *g) {
    for (Buf *b : {&g->text, &g->sums, &g->carry, &g->hdr, &g->res, &g->comp, &g->btab, &g->bstat, &g->move, &g->idoff, &g->idbytes, &g->idlen,
                   &g->blist, &g->btiles, &g->bcnt, &g->bprefix, &g->bstitch, &g->bmeta, &g->bjobs, &g->bchunks}) if (b->p) (void)hipFree(b->p);
    for (Pin *b : {&g->up[0], &g->up[1], &g->stage, &g->h_res, &g->h_hdr, &g->h_btab, &g->h_bstat, &g->h_head, &g->h_idoff, &g->h_idbytes, &g->h_idlen,
                   &g->h_bstitch, &g->h_bmeta, &g->h_bjobs, &g->h_bchunks}) if (b->p) (void)hipHostFree(b->p);
    for (hipEvent_t e : g->ev_b) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->ev_i) if (e) (void)hipEventDestroy(e);
    for (Block &b : g->blk) { if (b.reads.p) (void)hipFree(b.reads.p); if (b.off.p) (void)hipFree(b.off.p); if (b.h_off.p) (void)hipHostFree(b.h_off.p); }
    for (hipEvent_t e : g->ev_up) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->ev_m) if (e) (void)hipEventDestroy(e);
    if (g->gz) gz_free(g->gz);
    if (g->st) (void)hipStreamDestroy(g->st);
    if (g->s_copy) (void)hipStreamDestroy(g->s_copy);
}

// scan + emit over the window's text in g->text (measured already: nchunk pairs of events), results and header spans to the host
int scan_emit(lnr_rdgpu *g, const lnr_rdgpu_window *w, u32 nt, u64 nchunk, u64 max_rec, lnr_rdgpu_result *r, char *err, size_t err_cap) {
    Block &b = g->blk[w->slot];
    u8 *d_text = (u8 *)g->text.p;
    double t0;
    // ---- scan + emit
    ScanArgs SA;
    SA.text = d_text; SA.sums = (const Sum *)g->sums.p; SA.carry = (Carry *)g->carry.p; SA.nt = nt;
    SA.L.fmt = w->fmt; SA.L.eof = w->eof ? 1u : 0u; SA.L.len = w->len; SA.L.allowed = w->allowed; SA.L.free = w->free;
    SA.res = (Result *)g->res.p; SA.d_off = (u64 *)b.off.p; SA.rec_base = w->rec_base; SA.base_base = w->base_base;
    EmitArgs EA;
    EA.text = d_text; EA.len = w->len; EA.fmt = w->fmt; EA.carry = (const Carry *)g->carry.p; EA.res = (Result *)g->res.p;
    EA.rec_base = w->rec_base; EA.base_base = w->base_base; EA.out = (u8 *)b.reads.p; EA.d_off = (u64 *)b.off.p; EA.hdr = (u64 *)g->hdr.p;
    RD_CK(hipEventRecord(g->ev[0], g->st), -3);
    hipLaunchKernelGGL(k_rd_scan, dim3(1), dim3(SCAN_THREADS), 0, g->st, SA);
    RD_CK(hipEventRecord(g->ev[1], g->st), -3);
    hipLaunchKernelGGL(k_rd_emit, dim3(nt), dim3(64), 0, g->st, EA);
    RD_CK(hipEventRecord(g->ev[2], g->st), -3);
    RD_CK(hipMemcpyAsync(g->h_res.p, g->res.p, sizeof(Result), hipMemcpyDeviceToHost, g->st), -3);
    RD_CK(hipStreamSynchronize(g->st), -3);
    RD_CK(hipGetLastError(), -3);
    t0 = wall_ms();
    const Result R = *(const Result *)g->h_res.p;
    if (R.n > max_rec || R.bases > w->free) { snprintf(err, err_cap, "internal: the scan took %llu records", (unsigned long long)R.n); return -8; }
    u64 *h_off = (u64 *)b.h_off.p;
    RD_CK(hipMemcpyAsync(h_off + w->rec_base, (u64 *)b.off.p + w->rec_base, 8 * (R.n + 1), hipMemcpyDeviceToHost, g->st), -3);
    if (R.n) RD_CK(hipMemcpyAsync(g->h_hdr.p, g->hdr.p, 16 * R.n, hipMemcpyDeviceToHost, g->st), -3);
    RD_CK(hipStreamSynchronize(g->st), -3);
    g->ms[4] += wall_ms() - t0;
    float f = 0;
    for (u64 k = 0; k < nchunk; k++) { RD_CK(hipEventElapsedTime(&f, g->ev_m[2 * k], g->ev_m[2 * k + 1]), -3); g->ms[1] += f; }
    RD_CK(hipEventElapsedTime(&f, g->ev[0], g->ev[1]), -3); g->ms[2] += f;
    RD_CK(hipEventElapsedTime(&f, g->ev[1], g->ev[2]), -3); g->ms[3] += f;
    r->n = R.n; r->bases = R.bases; r->consumed = R.consumed == ~0ULL ? w->len : R.consumed;
    r->handover = R.handover; r->full = R.full; r->too_big = R.too_big;
    r->hdr = (const uint64_t *)g->h_hdr.p;
    return 0;
}

// measure / scan / emit over the w->len bytes of a window's text.  Host text (w->text) goes up first, chunk by chunk through the pinned
// staging buffers (or as it is: w->pinned), every chunk measured behind its copy; w->text == null: the text lies in g->text already
int parse_text(lnr_rdgpu *g, const lnr_rdgpu_window *w, lnr_rdgpu_result *r, char *err, size_t err_cap) {
    Block &b = g->blk[w->slot];
    const bool up = w->text != nullptr;
    const u32 nt = (u32)((w->len + RD_TILE - 1) / RD_TILE);
    const u64 max_rec = w->allowed < w->len / 2 + 1 ? w->allowed : w->len / 2 + 1;
    int s = 0;
    if ((up && (s = dev_need(g->text, (u64)nt * RD_TILE + 16, err, err_cap))) || (s = dev_need(g->sums, (u64)nt * sizeof(Sum), err, err_cap)) ||
        (s = dev_need(g->carry, (u64)nt * sizeof(Carry), err, err_cap)) || (s = dev_need(g->hdr, 16 * max_rec + 16, err, err_cap))) return s;
    if (!pin_need(g->h_hdr, 16 * max_rec + 16)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    if (w->base_base + w->free + 16 > b.reads.cap || 8 * (w->rec_base + w->allowed + 1) > b.off.cap) { snprintf(err, err_cap, "internal: block accounting"); return -8; }
    u8 *d_text = (u8 *)g->text.p;
    const double t0 = wall_ms();
    const u64 nchunk = !up || w->pinned ? 1 : (w->len + RD_CHUNK - 1) / RD_CHUNK;
    while (g->ev_m.size() < 2 * nchunk) { hipEvent_t e; RD_CK(hipEventCreate(&e), -3); g->ev_m.push_back(e); }
    if (up && !w->pinned) for (Pin &p : g->up) if (!pin_need(p, RD_CHUNK)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    for (u64 k = 0; k < nchunk; k++) {
        const u64 o = k * RD_CHUNK, len = nchunk == 1 ? w->len : (w->len - o < RD_CHUNK ? w->len - o : RD_CHUNK);
        if (up) {
            const void *src = w->text + o;
            if (!w->pinned) {
                RD_CK(hipEventSynchronize(g->ev_up[k & 1]), -3);                  // the last copy out of this staging buffer has finished
                par_copy(g->up[k & 1].p, w->text + o, len, w->threads);
                src = g->up[k & 1].p;
            }
            RD_CK(hipMemcpyAsync(d_text + o, src, len, hipMemcpyHostToDevice, g->s_copy), -3);
            RD_CK(hipEventRecord(g->ev_up[k & 1], g->s_copy), -3);
            RD_CK(hipStreamWaitEvent(g->st, g->ev_up[k & 1], 0), -3);
        }
        const u32 tile0 = (u32)(o / RD_TILE), tiles = (u32)((len + RD_TILE - 1) / RD_TILE);
        RD_CK(hipEventRecord(g->ev_m[2 * k], g->st), -3);
        hipLaunchKernelGGL(k_rd_measure, dim3(tiles), dim3(64), 0, g->st, (const u8 *)d_text, (u64)w->len, w->fmt, tile0, (Sum *)g->sums.p);
        RD_CK(hipEventRecord(g->ev_m[2 * k + 1], g->st), -3);
    }
    if (up) { RD_CK(hipStreamSynchronize(g->s_copy), -3); g->ms[0] += wall_ms() - t0; }
    return scan_emit(g, w, nt, nchunk, max_rec, r, err, err_cap);
}

// the bytes of the n spans at g->hdr (the same on the host at g->h_hdr: begin, end in the device text of tlen bytes) -> one run of bytes on
// the host, one wave per span: the header lines of a text window (strip_cr: without trailing '\r'), the names of a BAM window (`what`, for
// the messages).  n > 0: returns with the stream synchronised
int gather_names(lnr_rdgpu *g, bool strip_cr, u64 n, u64 tlen, const char *what, lnr_rdgpu_names *out, char *err, size_t err_cap) {
    int s;
    if (!pin_need(g->h_idoff, 8 * n + 8) || !pin_need(g->h_idlen, 4 * n + 4)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    const u64 *span = (const u64 *)g->h_hdr.p; const u32 *lens = (const u32 *)g->h_idlen.p;
    u64 *ido = (u64 *)g->h_idoff.p, total = 0;
    for (u64 k = 0; k < n; k++) {
        if (span[2 * k] > span[2 * k + 1] || span[2 * k + 1] > tlen) { snprintf(err, err_cap, "internal: header span of record %llu", (unsigned long long)k); return -8; }
        ido[k] = total; total += span[2 * k + 1] - span[2 * k];
    }
    if (!pin_need(g->h_idbytes, total + 1)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    out->ids = (const char *)g->h_idbytes.p; out->id_off = ido; out->id_len = lens;
    if (!n) return 0;
    if ((s = dev_need(g->idoff, 8 * n, err, err_cap)) || (s = dev_need(g->idlen, 4 * n, err, err_cap)) || (s = dev_need(g->idbytes, total + 1, err, err_cap))) return s;
    RD_CK(hipMemcpyAsync(g->idoff.p, ido, 8 * n, hipMemcpyHostToDevice, g->st), -3);
    RD_CK(hipEventRecord(g->ev_i[2], g->st), -3);
    hipLaunchKernelGGL(strip_cr ? k_rd_gather<true> : k_rd_gather<false>, dim3((u32)n), dim3(64), 0, g->st, (const u8 *)g->text.p, tlen, (const u64 *)g->hdr.p,
                       (const u64 *)g->idoff.p, n, (u8 *)g->idbytes.p, total, (u32 *)g->idlen.p);
    RD_CK(hipEventRecord(g->ev_i[3], g->st), -3);
    RD_CK(hipMemcpyAsync(g->h_idlen.p, g->idlen.p, 4 * n, hipMemcpyDeviceToHost, g->st), -3);
    if (total) RD_CK(hipMemcpyAsync(g->h_idbytes.p, g->idbytes.p, total, hipMemcpyDeviceToHost, g->st), -3);
    RD_CK(hipStreamSynchronize(g->st), -3);
    RD_CK(hipGetLastError(), -3);
    float f = 0; RD_CK(hipEventElapsedTime(&f, g->ev_i[2], g->ev_i[3]), -3); g->ms_inf[1] += f;
    for (u64 k = 0; k < n; k++) {                                          // (a span the kernel refused has the length ~0)
        const u64 l = span[2 * k + 1] - span[2 * k];
        if (strip_cr ? lens[k] > l : lens[k] != l) { snprintf(err, err_cap, "internal: gathered %s of record %llu", what, (unsigned long long)k); return -8; }
    }
    return 0;
}

}  // namespace

extern "C" {

uint32_t lnr_rdgpu_tile(void) { return RD_TILE; }
uint32_t lnr_rdgpu_bam_tile(void) { return BAM_TILE; }

int lnr_rdgpu_open(int32_t device, uint32_t slots, lnr_rdgpu **out, char *err, size_t err_cap) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) { snprintf(err, err_cap, "no usable HIP device for the GPU reader"); return -2; }
    DeviceGuard dg;
    if (device < 0) device = dg.prev < 0 ? 0 : dg.prev;
    if (device >= count) { snprintf(err, err_cap, "no usable HIP device %d for the GPU reader (%d present)", (int)device, count); return -2; }
    lnr_rdgpu *g = new (std::nothrow) lnr_rdgpu();
    if (!g) return -4;
    g->device = device; g->slots = slots;
    auto fail = [&](int s) { free_all(g); delete g; return s; };
    if (hipSetDevice(device) != hipSuccess) { snprintf(err, err_cap, "hipSetDevice(%d) failed", (int)device); return fail(-2); }
    auto step = [&]() -> int {
        RD_CK(hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking), -3);
        RD_CK(hipStreamCreateWithFlags(&g->s_copy, hipStreamNonBlocking), -3);
        for (hipEvent_t &e : g->ev_up) RD_CK(hipEventCreate(&e), -3);
        for (hipEvent_t &e : g->ev) RD_CK(hipEventCreate(&e), -3);
        for (hipEvent_t &e : g->ev_i) RD_CK(hipEventCreate(&e), -3);
        for (hipEvent_t &e : g->ev_b) RD_CK(hipEventCreate(&e), -3);
        if (!pin_need(g->h_res, sizeof(Result))) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
        return dev_need(g->res, sizeof(Result), err, err_cap);
    };
    if (int s = step()) return fail(s);
    *out = g;
    return 0;
}

int lnr_rdgpu_block(lnr_rdgpu *g, uint32_t slot, uint64_t dst_cap, uint32_t max_reads, uint8_t **d_reads, uint64_t **d_off, uint64_t **h_off,
                    char *err, size_t err_cap) {
    RD_ON_DEVICE(g);
    Block &b = g->blk[slot];
    int s;
    // 16 spare bytes behind the bases: lnr_filter_batch_dev reads none, the context's own upload keeps the same floor
    if ((s = dev_need(b.reads, dst_cap + 16, err, err_cap)) || (s = dev_need(b.off, 8ULL * (max_reads + 1ULL), err, err_cap))) return s;
    if (!pin_need(b.h_off, 8ULL * (max_reads + 1ULL))) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    *d_reads = (uint8_t *)b.reads.p; *d_off = (uint64_t *)b.off.p; *h_off = (uint64_t *)b.h_off.p;
    (*h_off)[0] = 0;
    RD_CK(hipMemsetAsync(b.off.p, 0, 8, g->st), -3);
    RD_CK(hipStreamSynchronize(g->st), -3);
    return 0;
}

uint8_t *lnr_rdgpu_stage(lnr_rdgpu *g, uint64_t bytes) {
    DeviceGuard dg(g->device);
    if (dg.set != hipSuccess) return nullptr;
    return pin_need(g->stage, bytes) ? (uint8_t *)g->stage.p : nullptr;
}

int lnr_rdgpu_parse(lnr_rdgpu *g, const lnr_rdgpu_window *w, lnr_rdgpu_result *r, char *err, size_t err_cap) {
    if (!w->len || w->len > (1ULL << 30) || w->slot >= g->slots) { snprintf(err, err_cap, "internal: window of %llu bytes", (unsigned long long)w->len); return -8; }
    RD_ON_DEVICE(g);
    return parse_text(g, w, r, err, err_cap);
}

// pageable host bytes -> device, through the two pinned staging buffers that host threads fill in turn; g->st waits for the last copy
static int upload_pageable(lnr_rdgpu *g, u8 *dst, const u8 *src, u64 len, u32 threads, char *err, size_t err_cap) {
    for (Pin &p : g->up) if (!pin_need(p, RD_CHUNK)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    u64 k = 0;
    for (u64 o = 0; o < len; o += RD_CHUNK, k++) {
        const u64 n = len - o < RD_CHUNK ? len - o : RD_CHUNK;
        RD_CK(hipEventSynchronize(g->ev_up[k & 1]), -3);
        par_copy(g->up[k & 1].p, src + o, n, threads);
        RD_CK(hipMemcpyAsync(dst + o, g->up[k & 1].p, n, hipMemcpyHostToDevice, g->s_copy), -3);
        RD_CK(hipEventRecord(g->ev_up[k & 1], g->s_copy), -3);
    }
    if (k) RD_CK(hipStreamWaitEvent(g->st, g->ev_up[(k - 1) & 1], 0), -3);
    return 0;
}

// device text [from, from + n) -> [to, to + n) on g->st, to < from; through g->move where the two overlap
static int move_text(lnr_rdgpu *g, u8 *text, u64 to, u64 from, u64 n, char *err, size_t err_cap) {
    if (!n || to == from) return 0;
    if (to + n <= from) { RD_CK(hipMemcpyAsync(text + to, text + from, n, hipMemcpyDeviceToDevice, g->st), -3); return 0; }
    if (int s = dev_need(g->move, n, err, err_cap)) return s;
    RD_CK(hipMemcpyAsync(g->move.p, text + from, n, hipMemcpyDeviceToDevice, g->st), -3);
    RD_CK(hipMemcpyAsync(text + to, g->move.p, n, hipMemcpyDeviceToDevice, g->st), -3);
    return 0;
}

// g->text holds `need` bytes (whole tiles) and the text the last window left, [keep_from, keep_from + carry), stands at its front: moved
// there, or into a new buffer where this one is too small
static int text_front(lnr_rdgpu *g, u64 need, u64 keep_from, u64 carry, char *err, size_t err_cap) {
    if (need <= g->text.cap) return move_text(g, (u8 *)g->text.p, 0, keep_from, carry, err, err_cap);
    Buf nb;
    if (int s = dev_need(nb, need, err, err_cap)) return s;
    if (carry) {
        hipError_t e = hipMemcpyAsync(nb.p, (u8 *)g->text.p + keep_from, carry, hipMemcpyDeviceToDevice, g->st);
        if (e == hipSuccess) e = hipStreamSynchronize(g->st);
        if (e != hipSuccess) { (void)hipFree(nb.p); snprintf(err, err_cap, "moving the carried text: %s", hipGetErrorString(e)); return -3; }
    }
    if (g->text.p) (void)hipFree(g->text.p);
    g->text = nb;
    return 0;
}

// the inflate step of a BGZF window: the carried text to the front, the blocks inflated behind it, the first bytes of the text (up to 64 KiB)
// and the blocks' status words on the host.  bad->status != 0: block bad->blk did not inflate.  The caller has set the device.
static int inflate_window(lnr_rdgpu *g, const lnr_rdgpu_bgzf *job, const lnr_rdgpu_window *w, lnr_rdgpu_badblk *bad, u64 *hl_out, char *err, size_t err_cap) {
    const u64 tlen = job->carry + job->new_text;
    if (!tlen || tlen > (1ULL << 30) || w->slot >= g->slots || job->comp_len > (1ULL << 31)) { snprintf(err, err_cap, "internal: window of %llu bytes", (unsigned long long)tlen); return -8; }
    if (job->keep_from + job->carry > g->text.cap) { snprintf(err, err_cap, "internal: carried text outside the buffer"); return -8; }
    int s;
    if ((s = text_front(g, w->fmt == 3 ? bam_text_cap(tlen) : ((tlen + RD_TILE - 1) / RD_TILE) * RD_TILE + 16, job->keep_from, job->carry, err, err_cap))) return s;
    u8 *d_text = (u8 *)g->text.p;
    // ---- compressed bytes and the block table up, one wave per block
    double t0 = wall_ms();
    const u32 nblk = job->nblk;
    if (nblk) {
        const u64 tb = (u64)nblk * sizeof(lnr_rdgpu_bgzf_blk);
        if ((s = dev_need(g->comp, job->comp_len + 16, err, err_cap)) || (s = dev_need(g->btab, tb, err, err_cap)) || (s = dev_need(g->bstat, 4ULL * nblk, err, err_cap))) return s;
        if (!pin_need(g->h_btab, tb) || !pin_need(g->h_bstat, 4ULL * nblk)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
        memcpy(g->h_btab.p, job->blk, tb);
        RD_CK(hipMemcpyAsync(g->btab.p, g->h_btab.p, tb, hipMemcpyHostToDevice, g->st), -3);
        RD_CK(hipMemsetAsync(g->bstat.p, 0xff, 4ULL * nblk, g->st), -3);
        if ((s = upload_pageable(g, (u8 *)g->comp.p, job->comp, job->comp_len, w->threads, err, err_cap))) return s;
        RD_CK(hipEventRecord(g->ev_i[0], g->st), -3);
        hipLaunchKernelGGL(k_bgzf_inflate, dim3(nblk), dim3(64), 0, g->st, (const u8 *)g->comp.p, (u64)job->comp_len, (const lnr_rdgpu_bgzf_blk *)g->btab.p, nblk,
                           d_text + job->carry, (u64)job->new_text, (u32 *)g->bstat.p);
        RD_CK(hipEventRecord(g->ev_i[1], g->st), -3);
        RD_CK(hipMemcpyAsync(g->h_bstat.p, g->bstat.p, 4ULL * nblk, hipMemcpyDeviceToHost, g->st), -3);
    }
    constexpr u64 HEAD = 65536;                                            // (blanks in front of the first record are used up this many per pass)
    if (!pin_need(g->h_head, HEAD)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    const u64 hl = tlen < HEAD ? tlen : HEAD;
    RD_CK(hipMemcpyAsync(g->h_head.p, d_text, hl, hipMemcpyDeviceToHost, g->st), -3);
    RD_CK(hipStreamSynchronize(g->st), -3);
    RD_CK(hipGetLastError(), -3);
    g->ms[0] += wall_ms() - t0;
    float f = 0;
    if (nblk) {
        RD_CK(hipEventElapsedTime(&f, g->ev_i[0], g->ev_i[1]), -3); g->ms_inf[0] += f;
        const u32 *stt = (const u32 *)g->h_bstat.p;
        for (u32 k = 0; k < nblk; k++) if (stt[k]) { bad->blk = k; bad->status = stt[k]; return 0; }
    }
    *hl_out = hl;
    return 0;
}

// measure / scan / emit over the tlen bytes of text at g->text (its first hl bytes lie at g->h_head), the header bytes of the taken records
// gathered: what follows the inflate of a BGZF window, and the rounds of a plain gzip file.  The caller has set the device.
static int parse_device_text(lnr_rdgpu *g, lnr_rdgpu_window *w, lnr_rdgpu_result *r, lnr_rdgpu_bgzf_result *br, u64 tlen, u64 hl, char *err, size_t err_cap) {
    int s;
    if (w->fmt == 0 && lnr_bam::is_magic((const u8 *)g->h_head.p, hl)) { w->fmt = 3; br->first = 'B'; return 0; }     // BAM: lnr_rdgpu_parse_bam reads this text
    // ---- a window starts at a record start: white space in front of it (the start of the file) is skipped
    const u8 *head = (const u8 *)g->h_head.p;
    u64 lead = 0;
    while (lead < hl && is_ws(head[lead])) lead++;
    br->lead = lead;
    if (lead == hl) return 0;                                              // nothing but blanks so far: the caller uses them up
    br->first = head[lead];
    if (w->fmt == 0) w->fmt = head[lead] == '>' ? FASTA : head[lead] == '@' ? FASTQ : -1;
    if (w->fmt < 0 || head[lead] != (w->fmt == FASTA ? '>' : '@')) return 0;
    if (lead) {
        if ((s = move_text(g, (u8 *)g->text.p, 0, lead, tlen - lead, err, err_cap))) return s;
        tlen -= lead;
    }
    w->len = tlen; w->text = nullptr; w->pinned = 1;
    if ((s = parse_text(g, w, r, err, err_cap))) return s;
    br->parsed = 1;
    return gather_names(g, true, r->n, tlen, "header", &br->names, err, err_cap);
}

int lnr_rdgpu_parse_bgzf(lnr_rdgpu *g, const lnr_rdgpu_bgzf *job, lnr_rdgpu_window *w, lnr_rdgpu_result *r, lnr_rdgpu_bgzf_result *br,
                         char *err, size_t err_cap) {
    *br = lnr_rdgpu_bgzf_result{};
    br->first = -1;
    *r = lnr_rdgpu_result{};
    RD_ON_DEVICE(g);
    int s;
    u64 tlen = job->carry + job->new_text, hl = 0;
    if ((s = inflate_window(g, job, w, &br->bad_block, &hl, err, err_cap)) || br->bad_block.status) return s;
    return parse_device_text(g, w, r, br, tlen, hl, err, err_cap);
}

int lnr_rdgpu_parse_bam(lnr_rdgpu *g, const lnr_rdgpu_bgzf *job, lnr_rdgpu_window *w, const lnr_rdgpu_bam_in *in, lnr_rdgpu_result *r,
                        lnr_rdgpu_bam_result *br, char *err, size_t err_cap) {
    using namespace lnr_bam;
    *br = lnr_rdgpu_bam_result{};
    *r = lnr_rdgpu_result{};
    RD_ON_DEVICE(g);
    int s;
    u64 tlen;
    int n_ref = in->n_ref;
    w->fmt = 3;
    if (job) {
        // ---- inflate behind the carried text, then pass the header where it still stands in front
        tlen = job->carry + job->new_text;
        u64 hl = 0;
        if ((s = inflate_window(g, job, w, &br->bad_block, &hl, err, err_cap)) || br->bad_block.status) return s;
        if (!in->hdr_done) {
            Header h = header_span((const u8 *)g->h_head.p, hl);
            while (h.status == 1 && h.need <= tlen) {                          // a header longer than the head: the head is downloaded again, larger
                hl = h.need + 65536 < tlen ? h.need + 65536 : tlen;
                if (!pin_need(g->h_head, hl)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
                RD_CK(hipMemcpyAsync(g->h_head.p, g->text.p, hl, hipMemcpyDeviceToHost, g->st), -3);
                RD_CK(hipStreamSynchronize(g->st), -3);
                h = header_span((const u8 *)g->h_head.p, hl);
            }
            if (h.status) { br->hdr_state = h.status < 0 ? 2 : 1; return 0; }
            br->lead = h.first; br->n_ref = n_ref = h.n_ref;
            if (h.first) {
                if ((s = move_text(g, (u8 *)g->text.p, 0, h.first, tlen - h.first, err, err_cap))) return s;
                tlen -= h.first;
            }
        }
    } else {
        tlen = w->len;
        if (!tlen || tlen > (1ULL << 30) || w->slot >= g->slots) { snprintf(err, err_cap, "internal: window of %llu bytes", (unsigned long long)tlen); return -8; }
        if ((s = dev_need(g->text, bam_text_cap(tlen), err, err_cap))) return s;
        const double t0 = wall_ms();
        RD_CK(hipMemcpyAsync(g->text.p, w->text, tlen, hipMemcpyHostToDevice, g->st), -3);
        RD_CK(hipStreamSynchronize(g->st), -3);
        g->ms[0] += wall_ms() - t0;
    }
    w->len = tlen;
    if (!tlen) return 0;
    if (g->text.cap < bam_text_cap(tlen)) { snprintf(err, err_cap, "internal: text buffer of %llu bytes", (unsigned long long)g->text.cap); return -8; }
    Block &b = g->blk[w->slot];
    if (w->base_base + w->free + 16 > b.reads.cap || 8 * (w->rec_base + w->allowed + 1) > b.off.cap) { snprintf(err, err_cap, "internal: block accounting"); return -8; }
    const u8 *d_text = (const u8 *)g->text.p;
    const u32 nt = (u32)((tlen + BAM_TILE - 1) / BAM_TILE);
    // ---- find, stitch: the record starts of the window
    if ((s = dev_need(g->blist, 4ULL * nt * BAM_SLICE, err, err_cap)) || (s = dev_need(g->btiles, (u64)nt * sizeof(Tile), err, err_cap)) ||
        (s = dev_need(g->bcnt, 4ULL * nt, err, err_cap)) || (s = dev_need(g->bprefix, 8ULL * (nt + 1), err, err_cap)) || (s = dev_need(g->bstitch, sizeof(BamStitch), err, err_cap))) return s;
    if (!pin_need(g->h_bstitch, sizeof(BamStitch))) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    RD_CK(hipEventRecord(g->ev_b[0], g->st), -3);
    hipLaunchKernelGGL(k_bam_find, dim3(nt), dim3(64), 0, g->st, d_text, tlen, n_ref, (u32 *)g->blist.p, (Tile *)g->btiles.p);
    RD_CK(hipEventRecord(g->ev_b[1], g->st), -3);
    hipLaunchKernelGGL(k_bam_stitch, dim3(1), dim3(64), 0, g->st, d_text, tlen, n_ref, nt, (u32 *)g->blist.p, (const Tile *)g->btiles.p, (u32 *)g->bcnt.p, (u64 *)g->bprefix.p,
                       (BamStitch *)g->bstitch.p);
    RD_CK(hipMemcpyAsync(g->h_bstitch.p, g->bstitch.p, sizeof(BamStitch), hipMemcpyDeviceToHost, g->st), -3);
    RD_CK(hipStreamSynchronize(g->st), -3);
    RD_CK(hipGetLastError(), -3);
    const BamStitch S = *(const BamStitch *)g->h_bstitch.p;
    const u64 nrec = S.nrec;
    if (S.consumed > tlen || nrec > tlen / MIN_REC + 1 || S.flag > CH_CUT) { snprintf(err, err_cap, "internal: the stitch found %llu records", (unsigned long long)nrec); return -8; }
    // ---- per-record metadata to the host (never a base)
    const Meta *M = nullptr;
    if (nrec) {
        if ((s = dev_need(g->bmeta, nrec * sizeof(Meta), err, err_cap))) return s;
        if (!pin_need(g->h_bmeta, nrec * sizeof(Meta))) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
        RD_CK(hipMemsetAsync(g->bmeta.p, 0xff, nrec * sizeof(Meta), g->st), -3);
        hipLaunchKernelGGL(k_bam_meta, dim3(nt), dim3(64), 0, g->st, d_text, tlen, (const u32 *)g->blist.p, (const u32 *)g->bcnt.p, (const u64 *)g->bprefix.p, nrec, (Meta *)g->bmeta.p);
    }
    RD_CK(hipEventRecord(g->ev_b[2], g->st), -3);
    double t0 = wall_ms();
    if (nrec) {
        RD_CK(hipMemcpyAsync(g->h_bmeta.p, g->bmeta.p, nrec * sizeof(Meta), hipMemcpyDeviceToHost, g->st), -3);
        RD_CK(hipStreamSynchronize(g->st), -3);
        RD_CK(hipGetLastError(), -3);
        M = (const Meta *)g->h_bmeta.p;
    }
    // ---- the take, on the host: the delivered records' lengths in order against the limits
    std::vector<u32> lens; std::vector<u64> which;
    for (u64 k = 0; k < nrec; k++) {
        const u32 flag = M[k].flag_name & 0xffffu, lname = M[k].flag_name >> 16;
        const u64 end = (u64)M[k].off + HEAD + lname + 4ULL * M[k].n_cigar + ((u64)M[k].l_seq + 1) / 2;
        if (lname < 1 || end > S.consumed || (k && M[k].off <= M[k - 1].off)) { snprintf(err, err_cap, "internal: metadata of record %llu", (unsigned long long)k); return -8; }
        if (delivered(flag)) { lens.push_back(M[k].l_seq); which.push_back(k); }
    }
    const lnr_bam::Take T = lnr_bam::take(lens.data(), lens.size(), w->free, w->allowed, w->rec_base == 0);
    // the host reader meets a refused record (or the end of the file inside one) when it has taken every delivered record in front of it
    // and may read on: then this call is the one that fails
    const bool at_end = !T.full && T.n < w->allowed;
    if (at_end && (S.flag == CH_BAD || (S.flag == CH_CUT && w->eof))) { br->bad = S.flag == CH_BAD ? 1 : 2; br->bad_ord = nrec; br->bad_off = S.bad_off; return 0; }
    // what is used up: everything in front of the first delivered record that was not taken
    const u64 stop = T.n < which.size() ? which[T.n] : nrec;
    r->n = T.n; r->bases = T.bases; r->full = T.full; r->too_big = T.too_big; r->handover = 0;
    r->consumed = stop < nrec ? M[stop].off : S.consumed;
    br->passed = stop; br->skipped = stop - T.n; br->tiles = nt; br->repaired = S.repaired;
    // ---- emit: jobs and chunks up, ordinals and offsets into the block
    u64 *h_off = (u64 *)b.h_off.p;
    const u64 n = T.n;
    if (!pin_need(g->h_bjobs, (n + 1) * sizeof(BamJob)) || !pin_need(g->h_hdr, 16 * n + 16)) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    BamJob *J = (BamJob *)g->h_bjobs.p;
    u64 *span = (u64 *)g->h_hdr.p, at = w->base_base, nchunk = 0;
    for (u64 i = 0; i < n; i++) {
        const Meta &m = M[which[i]];
        const u32 flag = m.flag_name & 0xffffu, lname = m.flag_name >> 16;
        J[i].dst = at; J[i].seq = m.off + HEAD + lname + 4 * m.n_cigar; J[i].l_seq = m.l_seq; J[i].rev = reversed(flag) ? 1u : 0u; J[i].pad = 0;
        br->reverse += J[i].rev;
        h_off[w->rec_base + i] = at;
        at += m.l_seq;
        nchunk += ((u64)m.l_seq + BAM_CHUNK - 1) / BAM_CHUNK;
        span[2 * i] = (u64)m.off + HEAD; span[2 * i + 1] = (u64)m.off + HEAD + lname - 1;
    }
    h_off[w->rec_base + n] = at;
    if (at != w->base_base + T.bases || nchunk > 0xffffffffULL) { snprintf(err, err_cap, "internal: block accounting"); return -8; }
    if (!pin_need(g->h_bchunks, (nchunk + 1) * sizeof(BamChunk))) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    BamChunk *C = (BamChunk *)g->h_bchunks.p;
    for (u64 i = 0, c = 0; i < n; i++) for (u32 st = 0; st < J[i].l_seq; st += BAM_CHUNK) { C[c].rec = (u32)i; C[c].start = st; c++; }
    g->ms[4] += wall_ms() - t0;
    RD_CK(hipMemcpyAsync((u64 *)b.off.p + w->rec_base, h_off + w->rec_base, 8 * (n + 1), hipMemcpyHostToDevice, g->st), -3);
    RD_CK(hipEventRecord(g->ev_b[3], g->st), -3);
    if (n) {
        if ((s = dev_need(g->bjobs, n * sizeof(BamJob), err, err_cap)) || (s = dev_need(g->bchunks, (nchunk + 1) * sizeof(BamChunk), err, err_cap)) ||
            (s = dev_need(g->hdr, 16 * n, err, err_cap))) return s;
        RD_CK(hipMemcpyAsync(g->bjobs.p, J, n * sizeof(BamJob), hipMemcpyHostToDevice, g->st), -3);
        if (nchunk) RD_CK(hipMemcpyAsync(g->bchunks.p, C, nchunk * sizeof(BamChunk), hipMemcpyHostToDevice, g->st), -3);
        RD_CK(hipMemcpyAsync(g->hdr.p, span, 16 * n, hipMemcpyHostToDevice, g->st), -3);
        RD_CK(hipEventRecord(g->ev_b[3], g->st), -3);
        if (nchunk) hipLaunchKernelGGL(k_bam_emit, dim3((u32)nchunk), dim3(64), 0, g->st, d_text, tlen, (const BamJob *)g->bjobs.p, (const BamChunk *)g->bchunks.p, (u32)nchunk,
                                       (u8 *)b.reads.p, (u64)(w->base_base + w->free));
        RD_CK(hipEventRecord(g->ev_b[4], g->st), -3);
    } else RD_CK(hipEventRecord(g->ev_b[4], g->st), -3);
    if ((s = gather_names(g, false, n, tlen, "name", &br->names, err, err_cap))) return s;      // (ends with the stream synchronised where there are names)
    if (!n) { RD_CK(hipStreamSynchronize(g->st), -3); RD_CK(hipGetLastError(), -3); }
    float f = 0;
    RD_CK(hipEventElapsedTime(&f, g->ev_b[0], g->ev_b[1]), -3); br->find_ms = f; g->ms[1] += f;
    RD_CK(hipEventElapsedTime(&f, g->ev_b[1], g->ev_b[2]), -3); br->stitch_ms = f; g->ms[2] += f;
    RD_CK(hipEventElapsedTime(&f, g->ev_b[3], g->ev_b[4]), -3); br->emit_ms = f; g->ms[3] += f;
    return 0;
}

void lnr_rdgpu_inflate_times(const lnr_rdgpu *g, double *ms2) { ms2[0] = g->ms_inf[0]; ms2[1] = g->ms_inf[1]; }

int lnr_rdgpu_append(lnr_rdgpu *g, uint32_t slot, uint64_t base_base, const uint8_t *bases, uint64_t nb, uint64_t rec_base, const uint64_t *off, uint64_t n,
                     char *err, size_t err_cap) {
    RD_ON_DEVICE(g);
    Block &b = g->blk[slot];
    if (base_base + nb + 16 > b.reads.cap || 8 * (rec_base + n + 1) > b.off.cap) { snprintf(err, err_cap, "internal: block accounting"); return -8; }
    if (nb) RD_CK(hipMemcpy((u8 *)b.reads.p + base_base, bases, nb, hipMemcpyHostToDevice), -3);
    RD_CK(hipMemcpy((u64 *)b.off.p + rec_base, off, 8 * (n + 1), hipMemcpyHostToDevice), -3);
    return 0;
}

void lnr_rdgpu_times(const lnr_rdgpu *g, double *ms5) { for (int i = 0; i < 5; i++) ms5[i] = g->ms[i]; }
void lnr_rdgpu_times_reset(lnr_rdgpu *g) { for (double &m : g->ms) m = 0; g->ms_inf[0] = g->ms_inf[1] = 0; }

// ---- a genome held on the device: a delivered block moves into an allocation of its own, on the reader's stream, no host hop
int32_t lnr_rdgpu_device(const lnr_rdgpu *g) { return g->device; }

int lnr_rdgpu_keep(lnr_rdgpu *g, const uint8_t *d_src, uint64_t bytes, uint8_t **d_out, char *err, size_t err_cap) {
    RD_ON_DEVICE(g);
    void *p = nullptr;
    RD_CK(hipMalloc(&p, bytes + 16), -4);
    hipError_t e = bytes ? hipMemcpyAsync(p, d_src, bytes, hipMemcpyDeviceToDevice, g->st) : hipSuccess;
    if (e == hipSuccess) e = hipMemsetAsync((u8 *)p + bytes, 0, 16, g->st);
    if (e == hipSuccess) e = hipStreamSynchronize(g->st);
    if (e != hipSuccess) { (void)hipFree(p); snprintf(err, err_cap, "copy of a genome block on the device: %s", hipGetErrorString(e)); return -3; }
    *d_out = (uint8_t *)p;
    return 0;
}

int lnr_rdgpu_keep_download(int32_t device, const uint8_t *d_src, uint8_t *dst, uint64_t bytes, char *err, size_t err_cap) {
    DeviceGuard dg(device);
    if (dg.set != hipSuccess) { snprintf(err, err_cap, "hipSetDevice(%d): %s", (int)device, hipGetErrorString(dg.set)); return -3; }
    if (bytes) RD_CK(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost), -3);
    return 0;
}

void lnr_rdgpu_keep_free(int32_t device, uint8_t *d) {
    if (!d) return;
    DeviceGuard dg(device);
    if (dg.set == hipSuccess) (void)hipFree(d);
}

void lnr_rdgpu_close(lnr_rdgpu *g) {
    if (!g) return;
    DeviceGuard dg(g->device);
    (void)hipDeviceSynchronize();
    free_all(g);
    delete g;
}

}  // extern "C"

// ---- plain gzip: one member inflated in parallel from DEFLATE block starts.  Every decision comes from lnr_gunzip_hd.h.
// A round = a run of compressed bytes with a known start bit and the 32 KiB of text in front of it, cut into chunks.  Separate launches on
// one stream, no kernel waits for another workgroup:
//   k_gz_find      one wave per chunk (not chunk 0: it holds the round's start), lane = bit offset: the first offset that passes
//                  lnr_gz::is_dynamic_start, by ballot and first lane; a chunk without one ends at its last bit
//   k_gz_measure   one wave per chunk that has a candidate (and chunk 0): the counting decode up to the first boundary at or past the next candidate
//   k_gz_stitch    one wave, in order (lnr_gz::stitch_round): which candidates a true piece's decode lands on exactly, counting on where it
//                  overshoots; the true pieces with their text offsets, the round's end bit and text, cut at the text cap
//   k_gz_emit      one wave per true piece: the decode again, into one u16 per text byte (lane 0 stores literals, all lanes copy a match or
//                  a stored run: the store / fence / load pattern of WaveSink)
//   k_gz_chain     one wave, pieces in order: the last 32 Ki symbols in front of every piece start resolved in place, 64 lanes side by side
//   k_gz_resolve   one wave per tile of text: every symbol through its piece's window into bytes; the tile's CRC32 from 64 slices
//   k_gz_keep      the last 32 KiB of (old window, round text): the next round's window
namespace {

using lnr_gz::u16;
constexpr u32 GZ_TILE = 16384;                 // text bytes per wave of k_gz_resolve (64 CRC slices of 256 bytes)

__device__ __forceinline__ u64 gz_uniform(u64 v) {
    return (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)v) | ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32)) << 32);
}

__global__ __launch_bounds__(64) void k_gz_find(const u8 *comp, u64 clen, u64 start_bit, u64 chunk, u32 nchunk, u64 *cand) {
    const u32 c = blockIdx.x, lane = threadIdx.x;
    if (c >= nchunk) return;
    u64 found = lnr_gz::NONE;
    if (c) {
        u64 lo, hi;
        lnr_gz::chunk_bits(start_bit, clen, chunk, c, lo, hi);
        for (u64 g = lo; g < hi; g += 64) {
            const u64 b = g + lane;
            const u64 m = __ballot(b < hi && lnr_gz::is_dynamic_start(comp, clen, b));
            if (m) { found = g + ctz(m); break; }
        }
    }
    if (lane == 0) cand[c] = found;
}

__global__ __launch_bounds__(64) void k_gz_measure(const u8 *comp, u64 clen, u64 start_bit, const u64 *cand, u32 nchunk, lnr_gz::Meas *meas) {
    __shared__ lnr_inf::Tables T;
    const u32 c = blockIdx.x;
    if (c >= nchunk || (c && cand[c] == lnr_gz::NONE)) return;
    const u32 nc = lnr_gz::next_cand(cand, nchunk, c + 1);
    const u64 from = gz_uniform(c ? cand[c] : start_bit), stop = gz_uniform(nc < nchunk ? cand[nc] : lnr_gz::NONE);
    lnr_gz::CountSink cs;
    const lnr_gz::Meas m = lnr_gz::decode_chunk(comp, clen, from, stop, lnr_gz::NONE, cs, T);
    if (threadIdx.x == 0) meas[c] = m;
}

__global__ __launch_bounds__(64) void k_gz_stitch(const u8 *comp, u64 clen, u64 start_bit, const u64 *cand, const lnr_gz::Meas *meas, u32 nchunk, u64 text_cap,
                                                  lnr_gz::Piece *pieces, lnr_gz::Round *out) {
    __shared__ lnr_inf::Tables T;
    const lnr_gz::Round R = lnr_gz::stitch_round(comp, clen, start_bit, cand, meas, nchunk, text_cap, T, pieces, threadIdx.x == 0);
    if (threadIdx.x == 0) *out = R;
}

struct WaveSymSink {
    u16 *sym; u32 lane;
    __device__ void lit(u64 pos, u8 b) { if (lane == 0) sym[pos] = b; }
    __device__ void match(u64 pos, u32 len, u32 dist) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        for (u32 i = lane; i < len; i += 64) sym[pos + i] = lnr_gz::sym_copy(sym, pos, dist, i);
    }
    __device__ void stored(u64 pos, const u8 *src, u32 n) { for (u32 i = lane; i < n; i += 64) sym[pos + i] = src[i]; }
};

// bad[p] != 0: the second decode of piece p did not end where the first one did (cannot happen: both are the same function of the same bytes)
__global__ __launch_bounds__(64) void k_gz_emit(const u8 *comp, u64 clen, const lnr_gz::Piece *pieces, u32 npieces, u16 *sym, u64 text, u32 *bad) {
    __shared__ lnr_inf::Tables T;
    const u32 p = blockIdx.x;
    if (p >= npieces) return;
    lnr_gz::Piece P = pieces[p];
    P.start_bit = gz_uniform(P.start_bit); P.end_bit = gz_uniform(P.end_bit); P.text_off = gz_uniform(P.text_off); P.text = gz_uniform(P.text);
    u32 b = 1;
    if (P.text_off <= text && P.text <= text - P.text_off) {
        WaveSymSink o{sym + P.text_off, threadIdx.x};
        const lnr_gz::Meas E = lnr_gz::decode_chunk(comp, clen, P.start_bit, P.end_bit, P.text, o, T);
        b = (E.end_bit != P.end_bit || E.text != P.text) ? 1u : 0u;
    }
    if (threadIdx.x == 0) bad[p] = b;
}

struct GzChain { u64 win_syms; u32 bad_piece, status; };

__global__ __launch_bounds__(64) void k_gz_chain(const lnr_gz::Piece *pieces, u32 npieces, u16 *sym, u64 text, const u8 *win, u32 hist, const u32 *bad, GzChain *out) {
    const u32 lane = threadIdx.x;
    u64 refs = 0;
    u32 status = lnr_inf::OK, bad_piece = 0;
    for (u32 p = 0; p < npieces && status == lnr_inf::OK; p++) {
        lnr_gz::Piece P = pieces[p];
        P.text_off = gz_uniform(P.text_off); P.text = gz_uniform(P.text);
        if (bad[p] || P.text_off > text || P.text > text - P.text_off) { status = lnr_inf::E_TABLE; bad_piece = p; break; }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");             // what other lanes resolved in the pieces before
        u32 fail = 0;
        for (u64 t = lnr_gz::chain_from(P) + lane; t < P.text_off + P.text; t += 64) {
            const u32 was = sym[t];
            const int v = lnr_gz::resolve_sym(sym, P.text_off, t, win, hist);
            if (v < 0) fail = 1; else { sym[t] = (u16)v; refs += was >= 256; }
        }
        if (__ballot(fail)) { status = lnr_inf::E_DISTANCE; bad_piece = p; }
    }
    for (int d = 32; d; d >>= 1) refs += (u64)(u32)__shfl_xor((int)(u32)refs, d, 64) | ((u64)(u32)__shfl_xor((int)(u32)(refs >> 32), d, 64) << 32);
    if (lane == 0) { GzChain o; o.win_syms = refs; o.bad_piece = bad_piece; o.status = status; *out = o; }
}

struct GzTile { u32 crc, refs, bad, pad; };

__global__ __launch_bounds__(64) void k_gz_resolve(const lnr_gz::Piece *pieces, u32 npieces, const u16 *sym, u64 text, const u8 *win, u32 hist, u8 *out, GzTile *tiles) {
    const u32 lane = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * GZ_TILE, t1 = t0 + GZ_TILE < text ? t0 + GZ_TILE : text;
    if (t0 >= text || !npieces) return;
    u32 lo = 0, hi = npieces - 1;                                           // the last piece whose text starts at or in front of t0
    while (lo < hi) { const u32 mid = (lo + hi + 1) / 2; if (pieces[mid].text_off <= t0) lo = mid; else hi = mid - 1; }
    u32 p = lo, refs = 0, fail = 0;
    for (u64 g = t0; g < t1; g += 64) {
        while (p + 1 < npieces && pieces[p + 1].text_off <= g) p++;
        const u64 t = g + lane;
        if (t < t1) {
            u32 q = p;
            while (q + 1 < npieces && pieces[q + 1].text_off <= t) q++;
            const u32 was = sym[t];
            const int v = lnr_gz::resolve_sym(sym, pieces[q].text_off, t, win, hist);
            if (v < 0) fail = 1; else out[t] = (u8)v;
            refs += was >= 256;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");                 // the CRC slices read what other lanes stored
    const u64 n = t1 - t0, S = (n + 63) / 64, a = lane * S < n ? lane * S : n, e = a + S < n ? a + S : n;
    u32 x = lnr_inf::crc_shift(lnr_inf::crc_of(out + t0 + a, e - a), n - e);
    for (int d = 32; d; d >>= 1) { x ^= (u32)__shfl_xor((int)x, d, 64); refs += (u32)__shfl_xor((int)refs, d, 64); }
    const u64 anyfail = __ballot(fail);
    if (lane == 0) { GzTile o; o.crc = x; o.refs = refs; o.bad = anyfail ? 1u : 0u; o.pad = 0; tiles[blockIdx.x] = o; }
}

__global__ __launch_bounds__(256) void k_gz_keep(const u8 *old_win, const u8 *text, u64 n, u8 *new_win) {
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= lnr_gz::WIN) return;
    new_win[j] = n >= lnr_gz::WIN ? text[n - lnr_gz::WIN + j] : j + n < lnr_gz::WIN ? old_win[j + n] : text[j + n - lnr_gz::WIN];
}

// the buffers and the stream of the gzip rounds
struct GzDev {
    hipStream_t st = nullptr;
    bool own_stream = true;                    // (the reader's rounds run on the reader's stream)
    hipEvent_t ev[8] = {};
    Buf comp, cand, meas, pieces, round, sym, bad, chain, tiles, text, win[2];
    Pin h_round, h_chain, h_tiles;
    u32 cur_win = 0;
    ~GzDev() {
        for (Buf *b : {&comp, &cand, &meas, &pieces, &round, &sym, &bad, &chain, &tiles, &text, &win[0], &win[1]}) if (b->p) (void)hipFree(b->p);
        for (Pin *b : {&h_round, &h_chain, &h_tiles}) if (b->p) (void)hipHostFree(b->p);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (st && own_stream) (void)hipStreamDestroy(st);
    }
};

// One round on the device, in two steps; compressed bytes [0, clen) lie at G.comp, the window in G.win[G.cur_win].
// gz_plan: find, measure, stitch -> *R (ms6[0..2] +=).  gz_fill, where R has pieces and no status: emit, chain, resolve -> R->text bytes at
// `out` (device), the window moved on, *crc = CRC32 of the round's text (ms6[3..5] +=); a reference before the member's first byte sets R->status.
int gz_plan(GzDev &G, u64 clen, u64 start_bit, u64 chunk, u64 text_cap, lnr_gz::Round *R, u32 *nchunk_out, double *ms6, char *err, size_t err_cap) {
    using namespace lnr_gz;
    const u32 nchunk = chunks_of(start_bit, clen, chunk);
    *nchunk_out = nchunk;
    if (!nchunk) { *R = empty_round(start_bit); return 0; }               // not a byte: AT_INPUT, nothing is launched
    int s;
    if ((s = dev_need(G.cand, 8ULL * nchunk, err, err_cap)) || (s = dev_need(G.meas, (u64)nchunk * sizeof(Meas), err, err_cap)) ||
        (s = dev_need(G.pieces, (u64)nchunk * sizeof(Piece), err, err_cap)) || (s = dev_need(G.round, sizeof(Round), err, err_cap)) ||
        (s = dev_need(G.bad, 4ULL * nchunk, err, err_cap)) || (s = dev_need(G.chain, sizeof(GzChain), err, err_cap))) return s;
    if (!pin_need(G.h_round, sizeof(Round)) || !pin_need(G.h_chain, sizeof(GzChain))) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    const u8 *comp = (const u8 *)G.comp.p;
    RD_CK(hipEventRecord(G.ev[0], G.st), -3);
    hipLaunchKernelGGL(k_gz_find, dim3(nchunk), dim3(64), 0, G.st, comp, clen, start_bit, chunk, nchunk, (u64 *)G.cand.p);
    RD_CK(hipEventRecord(G.ev[1], G.st), -3);
    hipLaunchKernelGGL(k_gz_measure, dim3(nchunk), dim3(64), 0, G.st, comp, clen, start_bit, (const u64 *)G.cand.p, nchunk, (Meas *)G.meas.p);
    RD_CK(hipEventRecord(G.ev[2], G.st), -3);
    hipLaunchKernelGGL(k_gz_stitch, dim3(1), dim3(64), 0, G.st, comp, clen, start_bit, (const u64 *)G.cand.p, (const Meas *)G.meas.p, nchunk, text_cap,
                       (Piece *)G.pieces.p, (Round *)G.round.p);
    RD_CK(hipEventRecord(G.ev[3], G.st), -3);
    RD_CK(hipMemcpyAsync(G.h_round.p, G.round.p, sizeof(Round), hipMemcpyDeviceToHost, G.st), -3);
    RD_CK(hipStreamSynchronize(G.st), -3);
    RD_CK(hipGetLastError(), -3);
    *R = *(const Round *)G.h_round.p;
    float f = 0;
    for (int k = 0; k < 3; k++) { RD_CK(hipEventElapsedTime(&f, G.ev[k], G.ev[k + 1]), -3); ms6[k] += f; }
    if (R->pieces > nchunk || R->text > text_cap) { snprintf(err, err_cap, "internal: the stitch found %u pieces", R->pieces); return -8; }
    return 0;
}
int gz_fill(GzDev &G, u64 clen, u64 start_bit, u32 hist, lnr_gz::Round *R, u8 *out, u32 *crc, u64 *win_syms, double *ms6, char *err, size_t err_cap) {
    using namespace lnr_gz;
    int s;
    float f = 0;
    const u8 *comp = (const u8 *)G.comp.p;
    *crc = 0; *win_syms = 0;
    const u32 ntile = (u32)((R->text + GZ_TILE - 1) / GZ_TILE);
    if ((s = dev_need(G.sym, 2 * R->text + 16, err, err_cap)) ||
        (s = dev_need(G.tiles, (u64)(ntile + 1) * sizeof(GzTile), err, err_cap))) return s;
    if (!pin_need(G.h_tiles, (u64)(ntile + 1) * sizeof(GzTile))) { snprintf(err, err_cap, "pinned host allocation failed"); return -4; }
    const u8 *win = (const u8 *)G.win[G.cur_win].p;
    RD_CK(hipEventRecord(G.ev[4], G.st), -3);
    hipLaunchKernelGGL(k_gz_emit, dim3(R->pieces), dim3(64), 0, G.st, comp, clen, (const Piece *)G.pieces.p, R->pieces, (u16 *)G.sym.p, R->text, (u32 *)G.bad.p);
    RD_CK(hipEventRecord(G.ev[5], G.st), -3);
    hipLaunchKernelGGL(k_gz_chain, dim3(1), dim3(64), 0, G.st, (const Piece *)G.pieces.p, R->pieces, (u16 *)G.sym.p, R->text, win, hist, (const u32 *)G.bad.p, (GzChain *)G.chain.p);
    RD_CK(hipEventRecord(G.ev[6], G.st), -3);
    if (ntile) hipLaunchKernelGGL(k_gz_resolve, dim3(ntile), dim3(64), 0, G.st, (const Piece *)G.pieces.p, R->pieces, (const u16 *)G.sym.p, R->text, win, hist, out, (GzTile *)G.tiles.p);
    RD_CK(hipEventRecord(G.ev[7], G.st), -3);
    hipLaunchKernelGGL(k_gz_keep, dim3(WIN / 256), dim3(256), 0, G.st, win, (const u8 *)out, R->text, (u8 *)G.win[G.cur_win ^ 1].p);
    RD_CK(hipMemcpyAsync(G.h_chain.p, G.chain.p, sizeof(GzChain), hipMemcpyDeviceToHost, G.st), -3);
    if (ntile) RD_CK(hipMemcpyAsync(G.h_tiles.p, G.tiles.p, (u64)ntile * sizeof(GzTile), hipMemcpyDeviceToHost, G.st), -3);
    RD_CK(hipStreamSynchronize(G.st), -3);
    RD_CK(hipGetLastError(), -3);
    G.cur_win ^= 1;
    for (int k = 3; k < 6; k++) { RD_CK(hipEventElapsedTime(&f, G.ev[k + 1], G.ev[k + 2]), -3); ms6[k] += f; }
    const GzChain C = *(const GzChain *)G.h_chain.p;
    if (C.status) { R->status = C.status; R->bad_bit = start_bit; return 0; }
    *win_syms = C.win_syms;
    const GzTile *T = (const GzTile *)G.h_tiles.p;
    u32 c = 0;
    for (u32 k = 0; k < ntile; k++) {                                      // the tiles' CRCs folded in order
        if (T[k].bad) { R->status = lnr_inf::E_DISTANCE; R->bad_bit = start_bit; return 0; }
        const u64 n = (u64)k * GZ_TILE + GZ_TILE < R->text ? GZ_TILE : R->text - (u64)k * GZ_TILE;
        c = lnr_inf::crc_combine(c, T[k].crc, n);
        *win_syms += T[k].refs;
    }
    *crc = c;
    return 0;
}

void gz_free(GzDev *G) { delete G; }

}  // namespace

// One round of a plain gzip member for the reader: the round's compressed bytes up, find / measure / stitch; where it has pieces, the carried
// text to the front of g->text and the round's text resolved behind it.  Afterwards the device text is [0, carry + out->text).
extern "C" int lnr_rdgpu_gzip_round(lnr_rdgpu *g, const lnr_rdgpu_gzip *job, lnr_rdgpu_gzip_result *out, char *err, size_t err_cap) {
    using namespace lnr_gz;
    *out = lnr_rdgpu_gzip_result{};
    if (!job->comp_len || job->comp_len > (1ULL << 31) || job->start_bit > 7 || job->hist > WIN || job->carry > (1ULL << 30) || job->text_cap > (1ULL << 30) - job->carry ||
        job->keep_from + job->carry > g->text.cap) { snprintf(err, err_cap, "internal: gzip round of %llu bytes", (unsigned long long)job->comp_len); return -8; }
    RD_ON_DEVICE(g);
    int s;
    if (!g->gz) {
        g->gz = new (std::nothrow) GzDev();
        if (!g->gz) return -4;
        g->gz->st = g->st; g->gz->own_stream = false;
        for (hipEvent_t &e : g->gz->ev) RD_CK(hipEventCreate(&e), -3);
        if ((s = dev_need(g->gz->win[0], WIN, err, err_cap)) || (s = dev_need(g->gz->win[1], WIN, err, err_cap))) return s;
    }
    GzDev &G = *g->gz;
    lnr_rdgpu_gz_counts &C = out->counts;
    if ((s = dev_need(G.comp, job->comp_len + 16, err, err_cap))) return s;
    double t0 = wall_ms();
    if ((s = upload_pageable(g, (u8 *)G.comp.p, job->comp, job->comp_len, job->threads, err, err_cap))) return s;
    RD_CK(hipStreamSynchronize(g->s_copy), -3);
    C.upload_ms = wall_ms() - t0;
    Round R;
    u32 nchunk = 0, crc = 0;
    u64 refs = 0;
    double ms6[6] = {0, 0, 0, 0, 0, 0};
    if ((s = gz_plan(G, job->comp_len, job->start_bit, job->chunk, job->text_cap, &R, &nchunk, ms6, err, err_cap))) return s;
    if (!R.status && R.pieces) {
        if ((s = text_front(g, bam_text_cap(job->carry + R.text) + 16, job->keep_from, job->carry, err, err_cap))) return s;
        if ((s = gz_fill(G, job->comp_len, job->start_bit, job->hist, &R, (u8 *)g->text.p + job->carry, &crc, &refs, ms6, err, err_cap))) return s;
        out->moved = 1;
    }
    out->status = R.status; out->stop = R.stop; out->pieces = R.pieces; out->crc = crc;
    out->bad_off = R.bad_bit >> 3; out->end_bit = R.end_bit; out->text = R.text;
    C.find_ms = ms6[0]; C.measure_ms = ms6[1]; C.stitch_ms = ms6[2]; C.emit_ms = ms6[3]; C.chain_ms = ms6[4]; C.resolve_ms = ms6[5];
    if (!R.status && R.pieces) {
        C.rounds = 1; C.chunks = nchunk; C.true_pieces = R.pieces; C.false_candidates = R.falses; C.candidates = R.cands;
        C.deflate_blocks = R.blocks; C.compressed_bytes = (R.end_bit + 7) >> 3; C.text_bytes = R.text; C.window_symbols = refs;
    }
    return 0;
}

extern "C" int lnr_rdgpu_gunzip(int32_t device, const uint8_t *gz, uint64_t size, uint8_t *text, uint64_t text_cap, uint64_t *text_size, lnr_rdgpu_gz_counts *last,
                                lnr_rdgpu_gz_counts *total, uint64_t *bad_off, uint32_t *bad_status, char *err, size_t err_cap) {
    using namespace lnr_gz;
    *text_size = 0; *bad_off = 0; *bad_status = 0;
    *last = lnr_rdgpu_gz_counts{}; *total = lnr_rdgpu_gz_counts{};
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) { snprintf(err, err_cap, "no usable HIP device for the GPU inflate"); return -2; }
    DeviceGuard dg;
    if (device < 0) device = dg.prev < 0 ? 0 : dg.prev;
    if (device >= count) { snprintf(err, err_cap, "no usable HIP device %d for the GPU inflate (%d present)", (int)device, count); return -2; }
    if (size > (1ULL << 31)) { snprintf(err, err_cap, "%llu compressed bytes: beyond the staging limit of 2^31", (unsigned long long)size); return -6; }
    RD_CK(hipSetDevice(device), -2);
    const u64 chunk = lnr_gz::env_bytes("LNR_READER_GZ_CHUNK", 128ULL << 10, 1024, 1ULL << 30), round = lnr_gz::env_bytes("LNR_READER_GZ_ROUND", 64ULL << 20, 1024, 1ULL << 31);
    GzDev G;
    int s;
    RD_CK(hipStreamCreateWithFlags(&G.st, hipStreamNonBlocking), -3);
    for (hipEvent_t &e : G.ev) RD_CK(hipEventCreate(&e), -3);
    if ((s = dev_need(G.comp, size + 16, err, err_cap)) || (s = dev_need(G.win[0], WIN, err, err_cap)) || (s = dev_need(G.win[1], WIN, err, err_cap))) return s;
    double t0 = wall_ms();
    if (size) RD_CK(hipMemcpyAsync(G.comp.p, gz, size, hipMemcpyHostToDevice, G.st), -3);
    RD_CK(hipStreamSynchronize(G.st), -3);
    total->upload_ms += wall_ms() - t0;
    u64 done = 0, bad = 0;
    auto fail = [&](u32 status, u64 at) { *bad_status = status; *bad_off = at; *text_size = done; return 0; };
    Member m;
    for (;;) {
        u32 st = member_enter(m, gz, size);
        if (st) return fail(st, m.pos);
        if (m.end) break;
        const u64 rsize = member_round_size(m, round), rb = m.start_bit >> 3, clen = size - rb < rsize ? size : rb + rsize;
        const u64 cap = text_cap - done < (1ULL << 30) ? text_cap - done : 1ULL << 30;
        Round R;
        u32 nchunk = 0, rcrc = 0;
        u64 refs = 0;
        lnr_rdgpu_gz_counts L{};
        double ms6[6] = {0, 0, 0, 0, 0, 0};
        if ((s = gz_plan(G, clen, m.start_bit, chunk, cap, &R, &nchunk, ms6, err, err_cap))) return s;
        if (!R.status && R.pieces) {
            if ((s = dev_need(G.text, R.text + 16, err, err_cap)) || (s = gz_fill(G, clen, m.start_bit, m.hist, &R, (u8 *)G.text.p, &rcrc, &refs, ms6, err, err_cap))) return s;
        }
        bool grown, final = false;
        st = round_verdict(m, R, clen, size, rsize, grown, &bad);
        if (st == E_TEXT_CAP && R.pieces && cap < text_cap - done) st = 0;          // cut at the 1 GiB a round may hold, not at the caller's buffer
        L.find_ms = ms6[0]; L.measure_ms = ms6[1]; L.stitch_ms = ms6[2]; L.emit_ms = ms6[3]; L.chain_ms = ms6[4]; L.resolve_ms = ms6[5];
        if (!st && !grown) {
            t0 = wall_ms();
            if (R.text) RD_CK(hipMemcpy(text + done, G.text.p, R.text, hipMemcpyDeviceToHost), -3);
            L.download_ms = wall_ms() - t0;
            L.rounds = 1; L.chunks = nchunk; L.true_pieces = R.pieces; L.false_candidates = R.falses; L.candidates = R.cands;
            L.deflate_blocks = R.blocks; L.compressed_bytes = ((R.end_bit + 7) >> 3) - rb; L.text_bytes = R.text; L.window_symbols = refs;
        } else if (grown) L.grown_rounds = 1;
        *last = L;
        lnr_rdgpu_gz_add(total, &L);
        if (st) return fail(st, bad);
        if (grown) continue;
        done += R.text;
        if ((st = member_fold(m, gz, size, R, rcrc, &final, &bad))) return fail(st, bad);
        total->members += final;
    }
    *text_size = done;
    return 0;
}
