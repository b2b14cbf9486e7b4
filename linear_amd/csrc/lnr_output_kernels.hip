// lnr_output_kernels.hip -- the GPU side of the writer (lnr_writer_format_gpu / _dev): the cords of a batch -> SAM records or APF text in
// HBM, then one copy into pinned host memory.  gfx950, wave64.  Every byte comes from lnr_output_hd.h, the same text the CPU test pins.
//
// Three steps on the writer's own stream:
//   k_out_measure<Fmt>  bytes of text per read                  (one wave per read)
//   k_out_scan          exclusive scan -> 64-bit text offsets, total read back through pinned memory
//   k_out_emit<Fmt>     every read writes its text at its offset (one wave per read; placement by the scan alone, no atomics)
// Both kernels are format_read<Fmt, EMIT>, the one skeleton of a read.  Tiling: workgroup = one wave = one read, lane = item (cord j of the
// read, lnr_output_hd.h) in tiles of 64 cords.  An item is head, body, tail.  Per tile the lanes size their items with the counting sink, a
// wave scan turns sizes into positions, the lanes format head and tail again into an LDS window that mirrors the 4-byte-aligned
// destination, and the wave copies byte ranges of the window out: the whole tile where no item has a body (consecutive items touch), else
// per record its head range and its tail range.  Text longer than the window takes more rounds: a lane formats once per window its head or
// tail touches and the sink drops what lies outside.  The body of a record -- its SEQ -- is 10-20 kB where head and tail are some hundred
// bytes, and is written by the whole wave, record after record of the tile: the owning lane walks its record once more and streams the
// SEGMENTS of the SEQ (lnr_output_hd.h) into an LDS table, SEG_CAP at a time, then every lane produces destination-aligned dwords -- finds
// its segment by bisection over the table's SEQ positions (SegCursor), loads the source bytes (genome forward; read forward, or backward and
// complemented for flag 16).  The block header of an APF item and the record of a SAM item look ahead along the read inside one lane; read
// index, pointers, counts and the read's text offset are wave-uniform (blockIdx), so the compiler keeps them scalar.
//
// The formats are small policy structs that answer only what differs (see the comment above them):
//   Text    SAM without SEQ, and APF (lnr_writer_format_gpu / _dev): an item is its head alone
//   SamSeq  SAM with SEQ (lnr_writer_format_seq_gpu / _dev): head, the letters mapped through ACGTN, tail; measuring sums element counts and
//           touches no base
//   Paf     PAF lines (lnr_writer_format_paf_gpu / _dev): one per SAM record, head alone; a lane walks its record twice (sums, then the cg tag)
//   Bam     BAM records without SEQ and with it (lnr_writer_format_bam_gpu / _dev): head (block_size, core, QNAME, CIGAR words), SEQ packed
//           two bases to a byte (a lane's dword is 8 bases) plus the 0xff run, tag
//
// Every store of a byte range that is not a lane's own -- the window copies, the SEQ letters and nibbles, the 0xff runs, the copies of the
// sort and the BGZF pack -- is lnr_span_hd.h's span_store with another word source: whole dwords where the dword lies inside the range,
// single bytes in the first and the last dword, which neighbouring ranges share.  The CPU test pins that routine under the sanitizers.
//
// BGZF output (lnr_writer_set_bgzf): the text stays in HBM and is compressed there, every 0xff00 bytes of it into one BGZF member by
// lnr_deflate_hd.h -- the same text the CPU test pins against zlib.
//   k_bgzf_deflate  one workgroup of 512 lanes per block (a grid of at most one workgroup per CU walks the blocks): the block's text and
//                   the hash table in LDS, the member image built in the table's place, then copied to the block's 65536-byte slot
//   k_out_scan      member sizes -> offsets
//   k_bgzf_pack     the slots -> one contiguous run (span_copy), the only bytes that are downloaded
//
// Coordinate sort (lnr_writer_sort_*): the BAM records of every batch are held until the sort -- without their quality spans (l_seq bytes of
// 0xff: bam_qual_span), in device segments or, with lnr_writer_sort_spill, in pinned host segments --, the order is computed on keys alone
// and the records move once more, straight into the buffer the deflate kernel reads.
//   k_sort_index    per batch, one lane per read: walks the read's full records at g->text by block_size (byte loads: records start anywhere);
//                   first pass: counts them and sizes the read's held bytes (k_out_scan places the reads); second pass: appends
//                   key = (u32)refID << 32 | (u32)pos, flag, stream offset, address of the held bytes, full size, reference end and the
//                   quality span per record.  The append is atomic; the stream offset is part of the order, so the result does not depend on
//                   the append order.
//   k_sort_keep     per batch, one wave per read: copies the records into the segment (or the staging buffer of a spilled batch, which one
//                   device-to-host copy then moves) and leaves the quality spans out (span_copy)
//   the sort        rocPRIM's stable radix sort twice: by (reverse bit, stream offset), then by key; k_sort_apply gathers the per-record
//                   arrays into that order and a scan of the sorted sizes places every record in the sorted stream S
//   k_sort_gather   per piece: one workgroup per 0xff00 bytes of S (= one BGZF member); bisection finds the first record that reaches into
//                   the tile, waves copy record after record (span_copy: destination-aligned dwords put together from two aligned source
//                   dwords; a piece of 8 KiB or more is copied by the whole workgroup): held bytes, the 0xff run of the quality span
//                   (span_fill), held bytes again.  Spilled records are read straight out of the pinned memory.  No atomics.
//   per piece       k_bgzf_deflate / k_out_scan / k_bgzf_pack as for any text
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>   // AMD's native primitives library: the stable radix sort and the scan of the coordinate sort
#include <rocprim/device/device_scan.hpp>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "lnr_deflate_hd.h"
#include "lnr_output_hd.h"
#include "lnr_output_hook.h"
#include "lnr_span_hd.h"

namespace {

using namespace lnr_out;

constexpr u32 OUT_WIN = 8192;                 // bytes of LDS window per wave (a tile of 64 APF lines is about 2 KiB)

struct LdsSink {                              // writes the bytes that fall into the window, counts on past the others
    char *lds; u64 rel;                       // position relative to the window start (wraps below it: "negative" is huge)
    __device__ void put(char c) { if (rel < OUT_WIN) lds[rel] = c; rel++; }
};

__device__ __forceinline__ u64 wave_incl_scan_u64(u64 v) {
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) { u64 t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
    return v;
}

// the wave copies staged positions [a, b) that fall into the window at wlo (4-byte aligned) from lds to dst; staged position p <-> dst[p]
__device__ __forceinline__ void window_out(const char *lds, u64 wlo, uint8_t *dst, u64 a, u64 b, u32 lane) {
    const u64 lo = a > wlo ? a : wlo, hi = b < wlo + OUT_WIN ? b : wlo + OUT_WIN;
    if (lo >= hi) return;
    const u32 *w = reinterpret_cast<const u32 *>(lds) + (((lo & ~3ULL) - wlo) >> 2);
    span_store(dst + lo, (u32)(hi - lo), lane, 64u, [=](u32 q, bool) { return w[q >> 2]; });
}

// ---- the SEQ of a record, written by the whole wave off a table of its segments (lnr_output_hd.h)
constexpr u32 SEG_CAP = 256;                   // segments of a record in LDS at a time
struct SeqArgs { const uint8_t *genome; const u64 *gstart; const uint8_t *reads; };       // (A.len holds read offsets here: read k = reads + len[k])
struct SegTable { u64 pos[SEG_CAP + 1], x[SEG_CAP], y[SEG_CAP]; u32 kind[SEG_CAP]; };       // pos: SEQ position of segment i, pos[i + 1] its end
struct SegFill {                               // keeps segments skip .. skip + SEG_CAP - 1 of the walk, counts on past the others
    SegTable *t; u32 skip;
    __device__ void seg(u32 k, u32 kind, u64 p, u64 x, u64 y, u32 c) {
        const u32 i = k - skip;
        if (i < SEG_CAP) { t->pos[i] = p; t->pos[i + 1] = p + c; t->x[i] = x; t->y[i] = y; t->kind[i] = kind; }
    }
};
struct SegCursor {                             // the last segment that starts at or before SEQ position `first` (bisection), then a forward walk
    const SegTable *tab; u32 s = 0; u64 s_lo, s_hi;
    __device__ SegCursor(const SegTable *t, u32 cnt, u64 first) : tab(t) {
        for (u32 hi = cnt; hi - s > 1;) { const u32 mid = (s + hi) >> 1; if (tab->pos[mid] <= first) s = mid; else hi = mid; }
        s_lo = tab->pos[s]; s_hi = tab->pos[s + 1];
    }
    __device__ u64 to(u64 sp) {                // moves on to the segment of sp; returns sp's offset in it
        while (sp >= s_hi) { s++; s_lo = s_hi; s_hi = tab->pos[s + 1]; }
        return sp - s_lo;
    }
};
// letters: SEQ positions [tab.pos[0], tab.pos[cnt]) of one record; staged position of SEQ position p = q0 + p.  A lane's dword is 4 bases.
__device__ __forceinline__ void seq_copy(const SegTable *tab, u32 cnt, const RecSrc &r, uint8_t *dst, u64 q0, u32 lane) {
    const u64 e0 = q0 + tab->pos[0], e1 = q0 + tab->pos[cnt];
    span_store(dst + e0, (u32)(e1 - e0), lane, 64u, [&](u32 q, bool) {
        const u64 p = (e0 & ~3ULL) + q;
        SegCursor c(tab, cnt, (p > e0 ? p : e0) - q0);
        u32 word = 0;
        for (u32 b = 0; b < 4; b++) {
            const u64 pb = p + b;
            if (pb < e0 || pb >= e1) continue;
            const u64 o = c.to(pb - q0);
            word |= (u32)(uint8_t)seq_char(r, tab->kind[c.s], tab->x[c.s] + o, tab->y[c.s] + o) << (8 * b);
        }
        return word;
    });
}
// nibbles: the packed bytes of SEQ bases [tab.pos[0], tab.pos[cnt]) of one record; staged position of packed byte j = q0 + j.  A lane's
// dword is 8 bases.  A first base at an odd position shares its byte with `carry`, the nibble of the base before it; a last base at an even
// position is left to the next round unless this round is the record's last (then its byte's low nibble is 0).
__device__ __forceinline__ void seq_pack_copy(const SegTable *tab, u32 cnt, const RecSrc &r, uint8_t *dst, u64 q0, u32 carry, bool last_round, u32 lane) {
    const u64 b0 = tab->pos[0], b1 = tab->pos[cnt];
    const u64 e0 = q0 + (b0 >> 1), e1 = q0 + (last_round ? (b1 + 1) >> 1 : b1 >> 1);
    span_store(dst + e0, (u32)(e1 - e0), lane, 64u, [&](u32 q, bool) {
        const u64 p = (e0 & ~3ULL) + q;
        u64 first = 2 * ((p > e0 ? p : e0) - q0);
        if (first < b0) first = b0;
        SegCursor c(tab, cnt, first);
        u32 word = 0;
        for (u32 b = 0; b < 4; b++) {
            const u64 pb = p + b;
            if (pb < e0 || pb >= e1) continue;
            u32 byte = 0;
            for (u32 h = 0; h < 2; h++) {
                const u64 sp = 2 * (pb - q0) + h;
                u32 nb;
                if (sp < b0) nb = carry;
                else if (sp >= b1) nb = 0;
                else { const u64 o = c.to(sp); nb = seq_nib(r, tab->kind[c.s], tab->x[c.s] + o, tab->y[c.s] + o); }
                byte |= h ? nb : nb << 4;
            }
            word |= byte << (8 * b);
        }
        return word;
    });
}

// ---- one read, one wave
struct ReadArgs {
    Params P;
    const u64 *coff, *cs, *ce, *len; int len_is_off;
    const char *ids; const u64 *idoff;
    int what, seq;                             // seq: records carry SEQ (Q holds the genome and the reads, len read offsets)
    SeqArgs Q;
};
struct Read { const u64 *cs, *ce; u64 nc, L; const char *id; bool blank; u64 n_rec; };      // read k's slice of the batch: wave-uniform
struct Sizes { u64 head = 0, body = 0, tail = 0; };       // an item's bytes: head and tail are formatted by its lane through the LDS window, the body between them is written by the wave

// The formats.  A format answers what differs between them: whether cord j is an item, the item's three sizes, "format head / tail into
// this sink", whether consecutive items touch (no body anywhere: the tile is one byte range), and "write the body of a record for this round
// of its segment table".  Everything else is format_read's.
// (All of it is inlined into the kernel, by force: the formats hold references to the kernel's by-value arguments, and one call left out of
// line would make the compiler copy those into scratch memory.)
struct Text {                                  // SAM without SEQ, and APF: an item is its head alone
    static constexpr bool BODY = false;
    using Item = Sizes;
    const ReadArgs &A; const Read &R;
    __device__ __forceinline__ bool item(u64 j) const { return A.what == 2 || rec_first(R.cs, R.ce, j, A.P.thd_large_X); }
    __device__ __forceinline__ bool touch() const { return true; }
    __device__ __forceinline__ void size(Item &z, u64 j, u64 it) const { CountSink c; head(c, z, j, it); z.head = c.n; }
    template <class S> __device__ __forceinline__ void head(S &s, const Item &, u64 j, u64 it) const {
        if (A.what == 2) apf_item(s, A.P, R.cs, R.nc, j, R.L, R.id, R.blank);
        else sam_item(s, A.P, R.cs, R.ce, R.nc, j, R.L, R.id, it, R.n_rec);
    }
    template <class S> __device__ __forceinline__ void tail(S &, u64) const {}
};
struct SamSeq {                                // head (with the '*' of an empty SEQ), letters, tail
    static constexpr bool BODY = true;
    using Item = Sizes;
    const ReadArgs &A; const Read &R;
    __device__ __forceinline__ bool item(u64 j) const { return rec_first(R.cs, R.ce, j, A.P.thd_large_X); }
    __device__ __forceinline__ bool touch() const { return false; }
    __device__ __forceinline__ void size(Item &z, u64 j, u64 it) const {
        CountSink h; z.body = sam_head(h, A.P, R.cs, R.ce, R.nc, j, R.L, R.id); z.head = h.n + (z.body == 0);
        CountSink t; tail(t, it); z.tail = t.n;
    }
    template <class S> __device__ __forceinline__ void head(S &s, const Item &, u64 j, u64) const { if (sam_head(s, A.P, R.cs, R.ce, R.nc, j, R.L, R.id) == 0) s.put('*'); }
    template <class S> __device__ __forceinline__ void tail(S &s, u64 it) const { sam_tail(s, A.P, R.cs, R.ce, R.nc, R.L, it, R.n_rec); }
    __device__ __forceinline__ void body(const SegTable *tab, u32 cnt, const RecSrc &r, uint8_t *dst, u64 q0, bool, u32 &, u32 lane) const { seq_copy(tab, cnt, r, dst, q0, lane); }
};
struct Paf {                                   // PAF: one line per SAM record, an item is its head alone (paf_item)
    static constexpr bool BODY = false;
    using Item = Sizes;
    const ReadArgs &A; const Read &R;
    __device__ __forceinline__ bool item(u64 j) const { return rec_first(R.cs, R.ce, j, A.P.thd_large_X); }
    __device__ __forceinline__ bool touch() const { return true; }
    __device__ __forceinline__ void size(Item &z, u64 j, u64 it) const { CountSink c; head(c, z, j, it); z.head = c.n; }
    template <class S> __device__ __forceinline__ void head(S &s, const Item &, u64 j, u64) const { paf_item(s, A.P, R.cs, R.ce, R.nc, j, R.L, R.id); }
    template <class S> __device__ __forceinline__ void tail(S &, u64) const {}
};
// BAM records, with SEQ and without: head (block_size, core, QNAME, CIGAR words), packed SEQ plus the 0xff run, tag (lnr_output_hd.h).  A
// table round that ends on an odd base hands the high nibble on (`carry`) and leaves the byte to the next round; the record's last round
// also fills the 0xff run behind the packed bytes.
struct Bam {
    static constexpr bool BODY = true;
    struct Item : Sizes { BamCount c; u64 bases = 0; };
    const ReadArgs &A; const Read &R; u64 qlen;
    __device__ __forceinline__ Bam(const ReadArgs &a, const Read &r) : A(a), R(r), qlen(str_len(r.id)) {}
    __device__ __forceinline__ bool item(u64 j) const { return rec_first(R.cs, R.ce, j, A.P.thd_large_X); }
    __device__ __forceinline__ bool touch() const { return !A.seq; }      // without SEQ head and tag of consecutive records touch
    __device__ __forceinline__ void size(Item &z, u64 j, u64 it) const {
        record_ops(z.c, A.P, R.cs, R.ce, R.nc, j, R.L);
        z.head = bam_head_size(qlen, z.c.k);
        z.bases = A.seq ? z.c.seq : 0; z.body = bam_packed(z.bases) + z.bases;
        CountSink t; tail(t, it); z.tail = t.n;
    }
    template <class S> __device__ __forceinline__ void head(S &s, const Item &z, u64 j, u64) const { bam_head(s, A.P, R.cs, R.ce, R.nc, j, R.L, R.id, z.c, z.bases, z.tail); }
    template <class S> __device__ __forceinline__ void tail(S &s, u64 it) const { bam_tail(s, A.P, R.cs, R.ce, R.nc, R.L, it, R.n_rec); }
    __device__ __forceinline__ void body(const SegTable *tab, u32 cnt, const RecSrc &r, uint8_t *dst, u64 q0, bool last_round, u32 &carry, u32 lane) const {
        seq_pack_copy(tab, cnt, r, dst, q0, carry, last_round, lane);
        const u64 o = tab->pos[cnt] - 1 - tab->pos[cnt - 1];                // the round's last base: the next round's carry
        carry = seq_nib(r, tab->kind[cnt - 1], tab->x[cnt - 1] + o, tab->y[cnt - 1] + o);
        if (last_round) { const u64 nb = tab->pos[cnt]; span_fill(dst + q0 + bam_packed(nb), 0xff, (u32)nb, lane, 64u); }
    }
};

// one wave = read k.  EMIT false: returns the bytes of its text.  EMIT true: writes them to text + toff.
template <class Fmt, bool EMIT> __device__ __forceinline__ u64 format_read(const ReadArgs &A, u32 k, char *text, u64 toff, char *lds, SegTable *tab) {
    const u32 lane = threadIdx.x & 63;
    const u64 a = A.coff[k], nc = A.coff[k + 1] - a;
    Read R{A.cs + a, A.ce + a, nc, A.len_is_off ? A.len[k + 1] - A.len[k] : A.len[k], A.ids + A.idoff[k], k > 0, 0};
    const Fmt F{A, R};
    if (A.what != 2)                            // (an APF item does not ask how many there are)
        for (u64 base = 1; base < nc; base += 64) {
            const u64 j = base + lane;
            R.n_rec += (u64)__popcll(__ballot(j < nc && F.item(j)));
        }
    const SeqSrc q{A.Q.genome, A.Q.gstart, A.P.glen, A.P.nseq, A.seq ? A.Q.reads + A.len[k] : nullptr, R.L};      // (used where the format has bodies)
    const u32 mis = (u32)(toff & 3);           // the LDS window mirrors the destination from a 4-byte boundary on
    uint8_t *dst = reinterpret_cast<uint8_t *>(text) + (toff - mis);      // staged position p of the read's text <-> dst[p]
    u64 pos = 0, rec_carry = 0;
    for (u64 base = 1; base < nc; base += 64) {
        const u64 j = base + lane;
        const bool item = j < nc && F.item(j);
        const u64 bal = __ballot(item);
        const u64 it = rec_carry + (u64)__popcll(bal & ((1ULL << lane) - 1ULL));
        typename Fmt::Item z;
        if (item) F.size(z, j, it);
        const u64 sz = z.head + z.body + z.tail;
        const u64 incl = wave_incl_scan_u64(sz);
        const u64 tile_total = __shfl(incl, 63, 64);
        if constexpr (EMIT) {
            const u64 s0 = mis + pos, s1 = s0 + tile_total, mine = s0 + incl - sz, tpos = mine + z.head + z.body;
            for (u64 wlo = s0 & ~3ULL; wlo < s1; wlo += OUT_WIN) {      // text longer than the window takes more rounds
                const bool hin = z.head && mine < wlo + OUT_WIN && mine + z.head > wlo, tin = z.tail && tpos < wlo + OUT_WIN && tpos + z.tail > wlo;
                const u64 in = __ballot(hin || tin);
                if (!in) continue;                                 // a window inside one body
                if (hin) { LdsSink s{lds, mine - wlo}; F.head(s, z, j, it); }
                if (tin) { LdsSink s{lds, tpos - wlo}; F.tail(s, it); }
                __syncthreads();               // (the workgroup is this one wave; all loop bounds here are wave-uniform)
                if (F.touch()) window_out(lds, wlo, dst, s0, s1, lane);
                else
                    for (u64 todo = in; todo; todo &= todo - 1) {  // a body lies between head and tail: two ranges per record
                        const int own = __ffsll((unsigned long long)todo) - 1;
                        const u64 h0 = __shfl(mine, own, 64), h1 = h0 + __shfl(z.head, own, 64), t0 = __shfl(tpos, own, 64), t1 = t0 + __shfl(z.tail, own, 64);
                        window_out(lds, wlo, dst, h0, h1, lane);
                        window_out(lds, wlo, dst, t0, t1, lane);
                    }
                __syncthreads();
            }
            if constexpr (Fmt::BODY) {
                for (u64 todo = __ballot(z.body > 0); todo; todo &= todo - 1) {        // the records of the tile, one after the other
                    const int own = __ffsll((unsigned long long)todo) - 1;
                    const u64 lo = base + (u64)own;                    // its first cord: wave-uniform
                    const u64 q0 = __shfl(mine + z.head, own, 64);
                    const RecSrc r = rec_src(q, R.cs, lo);
                    u32 done = 0, total, carry = 0;
                    do {                                               // the owning lane walks its record again, SEG_CAP segments into the table per round
                        u32 seen = 0;
                        if (lane == (u32)own) { SegFill f{tab, done}; SegOps<SegFill> so(f, cx(R.cs[lo])); record_ops(so, A.P, R.cs, R.ce, nc, lo, R.L); seen = so.k; }
                        __syncthreads();
                        total = (u32)__builtin_amdgcn_readfirstlane((int)__shfl(seen, own, 64));
                        const u32 cnt = total - done < SEG_CAP ? total - done : SEG_CAP;
                        if (cnt) F.body(tab, cnt, r, dst, q0, done + cnt == total, carry, lane);
                        done += cnt;
                        __syncthreads();
                    } while (done < total);
                }
            }
        }
        pos += tile_total;
        rec_carry += (u64)__popcll(bal);
    }
    return pos;
}

template <class Fmt> __global__ __launch_bounds__(64) void k_out_measure(ReadArgs A, u64 *sizes) {
    const u64 s = format_read<Fmt, false>(A, blockIdx.x, nullptr, 0, nullptr, nullptr);
    if (threadIdx.x == 0) sizes[blockIdx.x] = s;
}
template <class Fmt> __global__ __launch_bounds__(64) void k_out_emit(ReadArgs A, const u64 *toff, char *text) {
    __shared__ __attribute__((aligned(16))) char lds[OUT_WIN];
    SegTable *tab = nullptr;
    if constexpr (Fmt::BODY) { __shared__ SegTable t; tab = &t; }
    format_read<Fmt, true>(A, blockIdx.x, text, toff[blockIdx.x], lds, tab);
}
template <class Fmt> void launch_format(bool emit, u32 n, hipStream_t st, const ReadArgs &A, u64 *sizes, char *text) {
    if (emit) hipLaunchKernelGGL(k_out_emit<Fmt>, dim3(n), dim3(64), 0, st, A, (const u64 *)sizes, text);
    else hipLaunchKernelGGL(k_out_measure<Fmt>, dim3(n), dim3(64), 0, st, A, sizes);
}
// in place: a[0 .. n) sizes -> exclusive offsets, a[n] = total.  One workgroup: n is the reads of a batch.
__global__ __launch_bounds__(1024) void k_out_scan(u64 *a, u32 n) {
    __shared__ u64 part[1024];
    const u32 t = threadIdx.x, chunk = (n + 1023) / 1024;
    const u64 lo = (u64)t * chunk < n ? (u64)t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    u64 s = 0;
    for (u64 i = lo; i < hi; i++) s += a[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) { u64 run = 0; for (u32 i = 0; i < 1024; i++) { u64 v = part[i]; part[i] = run; run += v; } a[n] = run; }
    __syncthreads();
    u64 run = part[t];
    for (u64 i = lo; i < hi; i++) { u64 v = a[i]; a[i] = run; run += v; }
}

// ---- BGZF
constexpr u32 DEF_THREADS = 512;
struct DevTeam {                               // the workgroup as lnr_deflate_hd.h's team
    u32 tid, nt;
    __device__ void sync() { __syncthreads(); }
    __device__ void amax(u32 *p, u32 v) { atomicMax(p, v); }
    __device__ void aadd(u32 *p, u32 v) { atomicAdd(p, v); }
    __device__ void aor(u32 *p, u32 v) { atomicOr(p, v); }
    __device__ void axor(u32 *p, u32 v) { atomicXor(p, v); }
    // the greedy walk by wave 0: 64 positions in the lanes, the walker's position is wave-uniform and reads a lane's length with readlane
    __device__ void parse(u32 *tok, u32 n) {
        if (tid >= 64) return;
        u32 p = 0;
        u32 next = tid < n ? tok[tid] : 0;
        for (u32 base = 0; base < n; base += 64) {
            const u32 i = base + tid;
            const u32 len = lnr_def::tok_len(next);
            next = i + 64 < n ? tok[i + 64] : 0;            // (in flight while this tile is walked)
            u64 vis = 0;
            const u32 end = base + 64 < n ? base + 64 : n;
            while (p < end) {
                const u32 at = (u32)__builtin_amdgcn_readfirstlane((int)(p - base));
                const u32 l = (u32)__builtin_amdgcn_readlane((int)len, (int)at);
                vis |= 1ULL << at;
                p += l ? l : 1;
            }
            if (i < n && !((vis >> tid) & 1ULL)) tok[i] = lnr_def::SKIP;
        }
    }
};

// text [k * 0xff00, ...) -> slot k (65536 bytes each), msize[k] = bytes of the member; msize[nblocks + 1] counts the stored members.
// tok: 0xff00 words per workgroup of the grid.  text is 4-byte aligned.
__global__ __launch_bounds__(DEF_THREADS) void k_bgzf_deflate(const uint8_t *text, u64 total, u32 nblocks, uint8_t *slots, u64 *msize, u32 *tok_all) {
    __shared__ __attribute__((aligned(16))) uint8_t txt[lnr_def::BLOCK_TEXT];
    __shared__ __attribute__((aligned(16))) u32 tab[lnr_def::HASH_SIZE];      // the hash table, then the member image (MEMBER_CAP bytes)
    __shared__ lnr_def::Work W;
    static_assert(sizeof(tab) == lnr_def::MEMBER_CAP, "the member image takes the table's place");
    DevTeam T{threadIdx.x, blockDim.x};
    u32 *tok = tok_all + (u64)blockIdx.x * lnr_def::BLOCK_TEXT;
    for (u32 k = blockIdx.x; k < nblocks; k += gridDim.x) {
        const u64 lo = (u64)k * lnr_def::BLOCK_TEXT;
        const u32 n = total - lo < lnr_def::BLOCK_TEXT ? (u32)(total - lo) : lnr_def::BLOCK_TEXT;
        const u32 *src = reinterpret_cast<const u32 *>(text + lo);           // (0xff00 is a multiple of 4)
        for (u32 i = T.tid; i < n / 4; i += T.nt) reinterpret_cast<u32 *>(txt)[i] = src[i];
        for (u32 i = (n & ~3u) + T.tid; i < n; i += T.nt) txt[i] = text[lo + i];
        __syncthreads();
        u32 stored = 0;
        const u32 m = lnr_def::deflate_member(T, W, txt, n, tab, tok, reinterpret_cast<uint8_t *>(tab), &stored);
        u32 *dst = reinterpret_cast<u32 *>(slots + (u64)k * lnr_def::MEMBER_CAP);
        for (u32 i = T.tid; i < (m + 3) / 4; i += T.nt) dst[i] = tab[i];
        if (T.tid == 0) { msize[k] = m; if (stored) atomicAdd((unsigned long long *)&msize[nblocks + 1], 1ULL); }
        __syncthreads();
    }
}
// slot k -> out + off[k], off[k + 1] - off[k] bytes
__global__ __launch_bounds__(256) void k_bgzf_pack(const uint8_t *slots, const u64 *off, uint8_t *out) {
    const u32 k = blockIdx.x;
    const u64 o = off[k];
    span_copy(out + o, slots + (u64)k * lnr_def::MEMBER_CAP, (u32)(off[k + 1] - o), threadIdx.x, 256u);
}

// ---- coordinate sort
struct SortArrays { u64 *key; u32 *flag; u64 *soff; u64 *addr; u32 *size; i64 *end; u32 *qoff, *lseq; };     // per record, in arrival order
// recs: the batch's full records at g->text; roff[n + 1]: the reads' offsets in them (what k_out_scan left).  COUNT: *counter += records and
// cpos[k] = the bytes read k's records take in the hold (without their quality spans); else cpos[k] is where those bytes start (cpos after
// k_out_scan), hold the address of the batch's held bytes, and record number base + (*counter)++ is filled in.  A block_size that does not
// fit its read ends the read's walk in both passes alike (the encoder writes none).
template <bool COUNT> __global__ __launch_bounds__(256) void k_sort_index(const uint8_t *recs, const u64 *roff, u32 n, u64 stream_base, SortArrays A, u64 base, unsigned long long *counter,
                                                                          u64 *cpos, u64 hold) {
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    u64 p = roff[k];
    const u64 e = roff[k + 1];
    u32 cnt = 0;
    u64 c = COUNT ? 0 : cpos[k];
    while (p + 36 <= e) {
        const u64 sz = 4ULL + le32_at(recs + p);
        if (sz < 36 || p + sz > e) break;
        const BamQual q = bam_qual_span(recs + p, sz);
        if (COUNT) cnt++;
        else {
            const BamKey key = bam_key(recs + p, sz);
            const u64 i = base + atomicAdd(counter, 1ULL);
            A.key[i] = bam_sort_key(key); A.flag[i] = key.flag; A.soff[i] = stream_base + p;
            A.addr[i] = hold + c; A.size[i] = (u32)sz; A.end[i] = key.end; A.qoff[i] = q.qoff; A.lseq[i] = q.l_seq;
        }
        c += sz - q.l_seq;
        p += sz;
    }
    if (COUNT) { cpos[k] = c; if (cnt) atomicAdd(counter, (unsigned long long)cnt); }
}
// first pass of the sort: (reverse bit, stream offset) as one key, the record's number as the value
__global__ __launch_bounds__(256) void k_sort_prep(const u32 *flag, const u64 *soff, u64 n, u64 *k1, u32 *v1) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { k1[i] = ((u64)((flag[i] >> 4) & 1u) << 63) | soff[i]; v1[i] = (u32)i; }
}
__global__ __launch_bounds__(256) void k_sort_take(const u64 *key, const u32 *perm, u64 n, u64 *out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = key[perm[i]];
}
// the per-record arrays in sorted order; size64[n] = 0, so that the scan over n + 1 elements leaves the total in off[n]
__global__ __launch_bounds__(256) void k_sort_apply(SortArrays A, const u32 *perm, u64 n, u64 *s_addr, u64 *s_size, u32 *s_flag, i64 *s_end, u32 *s_qoff, u32 *s_lseq) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const u32 r = perm[i];
        s_addr[i] = A.addr[r]; s_size[i] = A.size[r]; s_flag[i] = A.flag[r]; s_end[i] = A.end[r]; s_qoff[i] = A.qoff[r]; s_lseq[i] = A.lseq[r];
    } else if (i == n) s_size[i] = 0;
}
// The batch's records at recs (g->text) -> hold, without their quality spans: one wave per read (four to a workgroup) walks the read's
// records and copies what lies before and after each span; cpos[k]: where read k's held bytes start (k_sort_index<true>, scanned).  All
// of the walk is wave-uniform.  Reads of recs stay inside [0, roff[n] + 3]; writes inside hold[cpos[k], cpos[k + 1]).
__global__ __launch_bounds__(256) void k_sort_keep(const uint8_t *recs, const u64 *roff, const u64 *cpos, u32 n, uint8_t *hold) {
    const u32 k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= n) return;
    u64 p = roff[k];
    const u64 e = roff[k + 1];
    uint8_t *d = hold + cpos[k];
    while (p + 36 <= e) {
        const u64 sz = 4ULL + le32_at(recs + p);
        if (sz < 36 || p + sz > e) break;
        const BamQual q = bam_qual_span(recs + p, sz);
        if (q.l_seq) {
            span_copy(d, recs + p, q.qoff, lane, 64u);
            span_copy(d + q.qoff, recs + p + q.qoff + q.l_seq, (u32)(sz - q.qoff - q.l_seq), lane, 64u);
        } else span_copy(d, recs + p, (u32)sz, lane, 64u);
        d += sz - q.l_seq;
        p += sz;
    }
}
constexpr u32 GATHER_BIG = 8192;               // a piece of a record this long is copied by the whole workgroup, a shorter one by one wave
// S[a, b) -> out (4-byte aligned), one workgroup per BLOCK_TEXT bytes; s_off[n + 1]: the records' offsets in S, s_addr[n] where their held
// bytes lie (device memory or pinned host memory alike), s_qoff / s_lseq[n] the quality span the hold leaves out.  Bytes [x0, x1) of a
// record are held bytes up to qoff, 0xff up to qoff + l_seq, then held bytes again, l_seq further down.
__global__ __launch_bounds__(256) void k_sort_gather(const u64 *s_off, const u64 *s_addr, const u32 *s_qoff, const u32 *s_lseq, u64 n, u64 a, u64 b, uint8_t *out) {
    const u64 t0 = a + (u64)blockIdx.x * lnr_def::BLOCK_TEXT;
    const u64 t1 = t0 + lnr_def::BLOCK_TEXT < b ? t0 + lnr_def::BLOCK_TEXT : b;
    u64 lo = 0, hi = n;                          // the last record that starts at or before t0 (s_off[0] = 0)
    while (hi - lo > 1) { const u64 mid = lo + (hi - lo) / 2; if (s_off[mid] <= t0) lo = mid; else hi = mid; }
    uint8_t *dst = out + (t0 - a);
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int big = 0; big < 2; big++)
        for (u64 r = big ? lo : lo + wave; r < n; r += big ? 1 : 4) {
            const u64 o = s_off[r];
            if (o >= t1) break;
            const u64 e = s_off[r + 1], c0 = o > t0 ? o : t0, c1 = e < t1 ? e : t1;
            if (c1 <= c0) continue;
            const u32 len = (u32)(c1 - c0);
            if ((len >= GATHER_BIG) != (big != 0)) continue;
            const u32 t = big ? threadIdx.x : lane, nt = big ? 256u : 64u;
            const uint8_t *src = reinterpret_cast<const uint8_t *>(s_addr[r]);
            uint8_t *d = dst + (c0 - t0);
            const u64 x0 = c0 - o, x1 = c1 - o, l = s_lseq[r];
            if (l == 0) { span_copy(d, src + x0, len, t, nt); continue; }
            const u64 q0 = s_qoff[r], q1 = q0 + l;
            if (x0 < q0) span_copy(d, src + x0, (u32)((x1 < q0 ? x1 : q0) - x0), t, nt);
            const u64 f0 = x0 > q0 ? x0 : q0, f1 = x1 < q1 ? x1 : q1;
            if (f0 < f1) span_fill(d + (f0 - x0), 0xff, (u32)(f1 - f0), t, nt);
            const u64 p0 = x0 > q1 ? x0 : q1;
            if (p0 < x1) span_copy(d + (p0 - x0), src + (p0 - l), (u32)(x1 - p0), t, nt);
        }
}

double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Buf { void *p = nullptr; u64 cap = 0; };

// cap: bytes for records; the allocation has 8 more (span_copy reads up to 3 bytes past a record's end: lnr_span_hd.h).  A host segment
// (pinned, alloc != nullptr) has HOST_FRONT bytes in front of p as well, and dev is what the kernels read it by.
struct SortSeg { char *p; u64 cap, used; char *alloc = nullptr, *dev = nullptr; };
struct SortState {
    int on = 0;                                 // 0 off, 1 collecting, 2 sorted: pieces go out
    u64 max_bytes = 0, stream = 0, nrec = 0, rec_cap = 0;
    int spill = 0; u64 max_host = 0;            // lnr_outgpu_sort_spill: the host tier and its budget
    std::vector<SortSeg> segs, hsegs;           // the device tier, the host tier
    Buf key, flag, soff, addr, size, end, qoff, lseq;       // per record in arrival order, rec_cap entries
    Buf k1, k2, v1, v2, tmp, s_addr, s_size, s_off, s_flag, s_end, s_qoff, s_lseq, counter;      // the sort's scratch and the arrays in sorted order (keys: k2)
    Buf cpos, stage;                            // per batch: the reads' offsets in the hold; the device staging of a batch on its way to the host tier
    u32 piece_members = 0; u64 members = 0, cursor = 0;
    std::vector<u64> moff;                      // member offsets of the last piece
    lnr_outgpu_sort_info info{};
    lnr_outgpu_hold_info hold{};
};
constexpr u64 SORT_SEG_MIN = 256ULL << 20, SORT_HOST_SEG = 64ULL << 20, HOST_FRONT = 16;

}  // namespace

struct lnr_outgpu {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t bev[4] = {nullptr, nullptr, nullptr, nullptr};       // BGZF: around k_bgzf_deflate, around k_bgzf_pack
    Buf gblob, goff, glen, ids, idoff, coff, cs, ce, len, sizes, text;
    Buf slots, msize, tok, packed;              // BGZF: a slot per block, member sizes / offsets, tokens per workgroup, the contiguous run
    int bgzf = 0; u32 cus = 1;
    lnr_outgpu_bgzf_stats bz{};
    u64 *h_bz = nullptr;                        // pinned: bytes of the run, stored members
    Buf genome, gstart, reads;                  // SEQ: the writer's own copy of the genome (lnr_outgpu_set_genome), the reads of a host-form call
    u32 nseq = 0;
    char *h_text = nullptr; u64 h_cap = 0;      // pinned
    u64 *h_total = nullptr;                     // pinned
    u64 *h_sort = nullptr;                      // pinned: the sort's counts and totals
    double ms[5] = {0, 0, 0, 0, 0};
    SortState sort;
};

namespace {

struct DeviceGuard {                            // every entry leaves the caller's current device as it found it
    int prev = -1;
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define OUT_CK(call, status)                                                                                              \
    do { hipError_t e_ = (call); if (e_ != hipSuccess) { snprintf(err, err_cap, "%s: %s", #call, hipGetErrorString(e_)); return (status); } } while (0)

int dev_need(Buf &b, u64 bytes, char *err, size_t err_cap) {
    if (bytes <= b.cap) return 0;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    u64 want = bytes + bytes / 4 + 256;
    OUT_CK(hipMalloc(&b.p, want), -4);
    b.cap = want;
    return 0;
}
std::vector<Buf *> sort_bufs(SortState &S) {        // every device buffer of the sort but the segments
    return {&S.key, &S.flag, &S.soff, &S.addr, &S.size, &S.end, &S.qoff, &S.lseq, &S.k1, &S.k2, &S.v1, &S.v2, &S.tmp, &S.s_addr, &S.s_size, &S.s_off, &S.s_flag, &S.s_end,
            &S.s_qoff, &S.s_lseq, &S.counter, &S.cpos, &S.stage};
}
void sort_free(lnr_outgpu *g) {
    SortState &S = g->sort;
    for (SortSeg &sg : S.segs) (void)hipFree(sg.p);
    for (SortSeg &sg : S.hsegs) (void)hipHostFree(sg.alloc);
    for (Buf *b : sort_bufs(S))
        if (b->p) { (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
    S = SortState();
}
void free_all(lnr_outgpu *g) {
    sort_free(g);
    for (Buf *b : {&g->gblob, &g->goff, &g->glen, &g->ids, &g->idoff, &g->coff, &g->cs, &g->ce, &g->len, &g->sizes, &g->text, &g->genome, &g->gstart, &g->reads, &g->slots, &g->msize, &g->tok, &g->packed}) if (b->p) (void)hipFree(b->p);
    if (g->h_text) (void)hipHostFree(g->h_text);
    if (g->h_bz) (void)hipHostFree(g->h_bz);
    for (hipEvent_t e : g->bev) if (e) (void)hipEventDestroy(e);
    if (g->h_total) (void)hipHostFree(g->h_total);
    if (g->h_sort) (void)hipHostFree(g->h_sort);
    for (hipEvent_t e : g->ev) if (e) (void)hipEventDestroy(e);
    if (g->st) (void)hipStreamDestroy(g->st);
}

int host_need(lnr_outgpu *g, u64 bytes, char *err, size_t err_cap) {      // the pinned buffer the caller reads
    if (bytes + 8 <= g->h_cap) return 0;
    if (g->h_text) { (void)hipHostFree(g->h_text); g->h_text = nullptr; g->h_cap = 0; }
    u64 want = bytes + bytes / 4 + 4096;
    OUT_CK(hipHostMalloc((void **)&g->h_text, want, hipHostMallocDefault), -4);
    g->h_cap = want;
    return 0;
}

// `total` bytes of text at d_text (device, 4-byte aligned) -> BGZF members in the pinned buffer.  Fills g->bz and g->ms[4].
int bgzf_run(lnr_outgpu *g, const uint8_t *d_text, u64 total, const char **data, uint64_t *size, char *err, size_t err_cap) {
    static const char empty[1] = "";
    g->bz = lnr_outgpu_bgzf_stats{};
    g->bz.text_bytes = total;
    if (total == 0) { *data = empty; *size = 0; return 0; }
    const u64 nb64 = (total + lnr_def::BLOCK_TEXT - 1) / lnr_def::BLOCK_TEXT;
    if (nb64 > 0x7fffffffULL) { snprintf(err, err_cap, "text of %llu bytes is too long for one BGZF call", (unsigned long long)total); return -1; }
    const u32 nb = (u32)nb64, grid = nb < g->cus ? nb : g->cus;
    int s;
    if ((s = dev_need(g->slots, (u64)nb * lnr_def::MEMBER_CAP, err, err_cap)) || (s = dev_need(g->msize, 8ULL * (nb + 2ULL), err, err_cap)) ||
        (s = dev_need(g->tok, 4ULL * grid * lnr_def::BLOCK_TEXT, err, err_cap))) return s;
    u64 *msize = (u64 *)g->msize.p;
    OUT_CK(hipMemsetAsync(msize + nb, 0, 16, g->st), -3);
    OUT_CK(hipEventRecord(g->bev[0], g->st), -3);
    hipLaunchKernelGGL(k_bgzf_deflate, dim3(grid), dim3(DEF_THREADS), 0, g->st, d_text, total, nb, (uint8_t *)g->slots.p, msize, (u32 *)g->tok.p);
    OUT_CK(hipEventRecord(g->bev[1], g->st), -3);
    hipLaunchKernelGGL(k_out_scan, dim3(1), dim3(1024), 0, g->st, msize, nb);
    OUT_CK(hipMemcpyAsync(g->h_bz, msize + nb, 16, hipMemcpyDeviceToHost, g->st), -3);
    OUT_CK(hipStreamSynchronize(g->st), -3);
    OUT_CK(hipGetLastError(), -3);
    const u64 ctotal = g->h_bz[0];
    if (ctotal > (u64)nb * lnr_def::MEMBER_CAP) { snprintf(err, err_cap, "BGZF members of %llu bytes for %u blocks", (unsigned long long)ctotal, nb); return -3; }
    if ((s = dev_need(g->packed, ctotal + 8, err, err_cap)) || (s = host_need(g, ctotal, err, err_cap))) return s;
    OUT_CK(hipEventRecord(g->bev[2], g->st), -3);
    hipLaunchKernelGGL(k_bgzf_pack, dim3(nb), dim3(256), 0, g->st, (const uint8_t *)g->slots.p, (const u64 *)msize, (uint8_t *)g->packed.p);
    OUT_CK(hipEventRecord(g->bev[3], g->st), -3);
    OUT_CK(hipStreamSynchronize(g->st), -3);
    OUT_CK(hipGetLastError(), -3);
    const double t0 = wall_ms();
    OUT_CK(hipMemcpyAsync(g->h_text, g->packed.p, ctotal, hipMemcpyDeviceToHost, g->st), -3);
    OUT_CK(hipStreamSynchronize(g->st), -3);
    g->ms[4] = wall_ms() - t0;
    float f = 0;
    OUT_CK(hipEventElapsedTime(&f, g->bev[0], g->bev[1]), -3); g->bz.deflate_ms = f;
    OUT_CK(hipEventElapsedTime(&f, g->bev[2], g->bev[3]), -3); g->bz.pack_ms = f;
    g->bz.blocks = nb; g->bz.stored_blocks = g->h_bz[1]; g->bz.compressed_bytes = ctotal;
    *data = g->h_text; *size = ctotal;
    return 0;
}

// sort mode: the batch's `total` record bytes at g->text (roff: the reads' offsets, n + 1) into a segment without their quality spans, their
// keys into the arrays.  The tier: the device while the held bytes stay under max_bytes and a segment can be had, else -- with
// lnr_outgpu_sort_spill on -- pinned host memory under its own budget, else -4.  Nothing of the state changes unless everything succeeded.
int sort_add_to(lnr_outgpu *g, u64 total, const u64 *roff, u32 n, SortSeg &fresh, char *err, size_t err_cap) {
    SortState &S = g->sort;
    int s;
    if (!g->h_sort) OUT_CK(hipHostMalloc((void **)&g->h_sort, 2 * sizeof(u64), hipHostMallocDefault), -4);
    if ((s = dev_need(S.counter, 16, err, err_cap)) || (s = dev_need(S.cpos, 8ULL * (n + 1ULL), err, err_cap))) return s;
    unsigned long long *counter = (unsigned long long *)S.counter.p;
    u64 *cpos = (u64 *)S.cpos.p;
    const uint8_t *recs = (const uint8_t *)g->text.p;
    OUT_CK(hipMemsetAsync(counter, 0, 16, g->st), -3);
    SortArrays A{};
    const u32 grid = (n + 255) / 256;
    OUT_CK(hipEventRecord(g->ev[0], g->st), -3);
    hipLaunchKernelGGL(k_sort_index<true>, dim3(grid), dim3(256), 0, g->st, recs, roff, n, S.stream, A, S.nrec, counter, cpos, 0ULL);
    OUT_CK(hipEventRecord(g->ev[1], g->st), -3);
    hipLaunchKernelGGL(k_out_scan, dim3(1), dim3(1024), 0, g->st, cpos, n);
    OUT_CK(hipMemcpyAsync(g->h_sort, counter, 8, hipMemcpyDeviceToHost, g->st), -3);
    OUT_CK(hipMemcpyAsync(g->h_sort + 1, cpos + n, 8, hipMemcpyDeviceToHost, g->st), -3);
    OUT_CK(hipStreamSynchronize(g->st), -3);
    OUT_CK(hipGetLastError(), -3);
    const u64 more = g->h_sort[0], held = g->h_sort[1];
    if (S.nrec + more > 0xffffffffULL) { snprintf(err, err_cap, "sort: more than 2^32 - 1 records"); return -6; }
    if (held > total) { snprintf(err, err_cap, "sort: %llu bytes to hold of a batch of %llu", (unsigned long long)held, (unsigned long long)total); return -8; }
    // the tier and the batch's place in it
    const u64 dev_held = S.hold.held_device_bytes, host_held = S.hold.held_host_bytes;
    SortSeg *sg = nullptr;
    u64 at = 0;
    bool host = false;
    char why[160] = "";
    if (!(S.max_bytes && dev_held + held > S.max_bytes)) {
        sg = S.segs.empty() ? nullptr : &S.segs.back();
        at = sg ? (sg->used + 15) & ~15ULL : 0;
        if (!sg || at + held > sg->cap) {
            u64 want = SORT_SEG_MIN;
            if (S.max_bytes && S.max_bytes - dev_held < want) want = S.max_bytes - dev_held;
            if (want < held) want = held;
            void *p = nullptr;
            if (hipMalloc(&p, want + 8) == hipSuccess) { fresh = SortSeg{(char *)p, want, 0}; sg = &fresh; at = 0; }
            else {
                (void)hipGetLastError();
                sg = nullptr;
                snprintf(why, sizeof why, "a segment of %llu bytes could not be allocated", (unsigned long long)want);
            }
        }
    } else snprintf(why, sizeof why, "max_device_bytes is %llu", (unsigned long long)S.max_bytes);
    if (!sg && !S.spill) {
        if (S.max_bytes && dev_held + held > S.max_bytes)
            snprintf(err, err_cap, "sort: %llu record bytes held on the device, %llu more asked for, max_device_bytes is %llu", (unsigned long long)dev_held, (unsigned long long)held, (unsigned long long)S.max_bytes);
        else snprintf(err, err_cap, "sort: %llu record bytes held on the device, %s for %llu more", (unsigned long long)dev_held, why, (unsigned long long)held);
        return -4;
    }
    if (!sg) {
        host = true;
        bool ok = host_held + held <= S.max_host && host_held + held >= host_held;
        if (ok) {
            sg = S.hsegs.empty() ? nullptr : &S.hsegs.back();
            at = sg ? (sg->used + 15) & ~15ULL : 0;
            if (!sg || at + held > sg->cap) {
                u64 want = SORT_HOST_SEG;
                if (S.max_host - host_held < want) want = S.max_host - host_held;
                if (want < held) want = held;
                void *p = nullptr, *d = nullptr;
                if (hipHostMalloc(&p, HOST_FRONT + want + 8, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&d, p, 0) == hipSuccess) {
                    fresh = SortSeg{(char *)p + HOST_FRONT, want, 0, (char *)p, (char *)d + HOST_FRONT};
                    sg = &fresh; at = 0;
                } else {
                    (void)hipGetLastError();
                    if (p) (void)hipHostFree(p);
                    sg = nullptr; ok = false;
                }
            }
        }
        if (!ok) {
            snprintf(err, err_cap, "sort: %llu record bytes held on the device (%s), %llu in host memory, %llu more asked for, max_host_bytes is %llu%s", (unsigned long long)dev_held, why,
                     (unsigned long long)host_held, (unsigned long long)held, (unsigned long long)S.max_host, host_held + held <= S.max_host ? ": a pinned segment could not be allocated" : "");
            return -4;
        }
        if ((s = dev_need(S.stage, held + 8, err, err_cap))) return s;
    }
    if (S.nrec + more > S.rec_cap) {              // grow: new arrays, the old entries copied over
        const u64 cap = (S.nrec + more) + (S.nrec + more) / 2 + 1024;
        struct { Buf *b; u64 w; } arr[8] = {{&S.key, 8}, {&S.flag, 4}, {&S.soff, 8}, {&S.addr, 8}, {&S.size, 4}, {&S.end, 8}, {&S.qoff, 4}, {&S.lseq, 4}};
        for (auto &x : arr) {
            void *p = nullptr;
            if (hipMalloc(&p, cap * x.w) != hipSuccess) {
                (void)hipGetLastError();
                snprintf(err, err_cap, "sort: %llu record bytes held on the device, the arrays for %llu records could not be allocated", (unsigned long long)dev_held, (unsigned long long)cap);
                return -4;
            }
            if (S.nrec && hipMemcpy(p, x.b->p, S.nrec * x.w, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipFree(p); snprintf(err, err_cap, "sort: copying the record arrays failed"); return -3; }
            if (x.b->p) (void)hipFree(x.b->p);
            x.b->p = p; x.b->cap = cap * x.w;
        }
        S.rec_cap = cap;
    }
    A = SortArrays{(u64 *)S.key.p, (u32 *)S.flag.p, (u64 *)S.soff.p, (u64 *)S.addr.p, (u32 *)S.size.p, (i64 *)S.end.p, (u32 *)S.qoff.p, (u32 *)S.lseq.p};
    uint8_t *hold = host ? (uint8_t *)S.stage.p : (uint8_t *)sg->p + at;           // where k_sort_keep writes
    const u64 addr = (u64)((host ? sg->dev : sg->p) + at);                         // where k_sort_gather will read
    OUT_CK(hipMemsetAsync(counter, 0, 16, g->st), -3);
    OUT_CK(hipEventRecord(g->bev[0], g->st), -3);
    hipLaunchKernelGGL(k_sort_keep, dim3((n + 3) / 4), dim3(256), 0, g->st, recs, roff, (const u64 *)cpos, n, hold);
    OUT_CK(hipEventRecord(g->bev[1], g->st), -3);
    OUT_CK(hipEventRecord(g->bev[2], g->st), -3);
    hipLaunchKernelGGL(k_sort_index<false>, dim3(grid), dim3(256), 0, g->st, recs, roff, n, S.stream, A, S.nrec, counter, cpos, addr);
    OUT_CK(hipEventRecord(g->bev[3], g->st), -3);
    OUT_CK(hipStreamSynchronize(g->st), -3);
    OUT_CK(hipGetLastError(), -3);
    double spill_ms = 0;
    if (host && held) {                           // the batch's way to the host tier: one DMA copy out of the staging buffer
        const double t0 = wall_ms();
        OUT_CK(hipMemcpyAsync(sg->p + at, hold, held, hipMemcpyDeviceToHost, g->st), -3);
        OUT_CK(hipStreamSynchronize(g->st), -3);
        spill_ms = wall_ms() - t0;
    }
    float f0 = 0, f1 = 0, f2 = 0;
    OUT_CK(hipEventElapsedTime(&f0, g->ev[0], g->ev[1]), -3);
    OUT_CK(hipEventElapsedTime(&f1, g->bev[2], g->bev[3]), -3);
    OUT_CK(hipEventElapsedTime(&f2, g->bev[0], g->bev[1]), -3);
    // everything succeeded: the state moves on
    if (sg == &fresh) { std::vector<SortSeg> &v = host ? S.hsegs : S.segs; v.push_back(fresh); sg = &v.back(); fresh = SortSeg{nullptr, 0, 0}; }
    S.info.index_ms += f0 + f1;
    S.hold.keep_ms += f2; S.hold.spill_ms += spill_ms;
    sg->used = at + held; S.stream += total; S.nrec += more;
    if (host) { S.hold.held_host_bytes += held; S.hold.host_batches++; } else { S.hold.held_device_bytes += held; S.hold.device_batches++; }
    S.hold.stream_bytes = S.stream;
    return 0;
}
int sort_add(lnr_outgpu *g, u64 total, const u64 *roff, u32 n, char *err, size_t err_cap) {
    if (total == 0) return 0;
    SortSeg fresh{nullptr, 0, 0};                 // a segment made for this batch: the state's only once the batch is in
    std::vector<SortSeg> &segs = g->sort.segs, &hsegs = g->sort.hsegs;
    if (segs.size() == segs.capacity()) segs.reserve(2 * segs.size() + 4);         // (so that taking the segment in cannot fail)
    if (hsegs.size() == hsegs.capacity()) hsegs.reserve(2 * hsegs.size() + 4);
    const int s = sort_add_to(g, total, roff, n, fresh, err, err_cap);
    if (fresh.alloc) (void)hipHostFree(fresh.alloc);
    else if (fresh.p) (void)hipFree(fresh.p);
    return s;
}

}  // namespace

extern "C" {

int lnr_outgpu_open(int32_t device, const char *gblob, uint64_t gblob_bytes, const uint64_t *goff, const uint64_t *glen, uint32_t nseq,
                    lnr_outgpu **out, char *err, size_t err_cap) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) { snprintf(err, err_cap, "no usable HIP device for the GPU writer"); return -2; }
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    if (device < 0) device = dg.prev < 0 ? 0 : dg.prev;
    if (device >= count) { snprintf(err, err_cap, "no usable HIP device %d for the GPU writer (%d present)", (int)device, count); return -2; }
    lnr_outgpu *g = new (std::nothrow) lnr_outgpu();
    if (!g) return -4;
    g->device = device; g->nseq = nseq;
    auto fail = [&](int s) { free_all(g); delete g; return s; };
    if (hipSetDevice(device) != hipSuccess) { snprintf(err, err_cap, "hipSetDevice(%d) failed", (int)device); return fail(-2); }
    int s = 0;
    auto step = [&]() -> int {
        OUT_CK(hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking), -3);
        for (hipEvent_t &e : g->ev) OUT_CK(hipEventCreate(&e), -3);
        for (hipEvent_t &e : g->bev) OUT_CK(hipEventCreate(&e), -3);
        int cus = 0;
        OUT_CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device), -3);
        g->cus = cus > 0 ? (u32)cus : 1;
        OUT_CK(hipHostMalloc((void **)&g->h_bz, 2 * sizeof(u64), hipHostMallocDefault), -4);
        OUT_CK(hipHostMalloc((void **)&g->h_total, sizeof(u64), hipHostMallocDefault), -4);
        if ((s = dev_need(g->gblob, gblob_bytes + 1, err, err_cap)) || (s = dev_need(g->goff, 8ULL * nseq + 8, err, err_cap)) || (s = dev_need(g->glen, 8ULL * nseq + 8, err, err_cap))) return s;
        if (nseq) {
            OUT_CK(hipMemcpyAsync(g->gblob.p, gblob, gblob_bytes, hipMemcpyHostToDevice, g->st), -3);
            OUT_CK(hipMemcpyAsync(g->goff.p, goff, 8ULL * nseq, hipMemcpyHostToDevice, g->st), -3);
            OUT_CK(hipMemcpyAsync(g->glen.p, glen, 8ULL * nseq, hipMemcpyHostToDevice, g->st), -3);
        }
        OUT_CK(hipStreamSynchronize(g->st), -3);
        return 0;
    };
    if ((s = step())) return fail(s);
    *out = g;
    return 0;
}

static int set_genome_from(lnr_outgpu *g, const uint8_t *const *seq, const uint64_t *glen, uint32_t nseq, hipMemcpyKind kind, char *err, size_t err_cap) {
    if (nseq != g->nseq) { snprintf(err, err_cap, "the genome has %u sequences, the writer was opened with %u", nseq, g->nseq); return -1; }
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    OUT_CK(hipSetDevice(g->device), -3);
    u64 *start = new (std::nothrow) u64[nseq + 1ULL];
    if (!start) return -4;
    start[0] = 0;
    for (u32 i = 0; i < nseq; i++) start[i + 1] = start[i] + glen[i];
    int s = 0;
    auto step = [&]() -> int {
        if ((s = dev_need(g->genome, start[nseq] + 1, err, err_cap)) || (s = dev_need(g->gstart, 8ULL * nseq + 8, err, err_cap))) return s;
        for (u32 i = 0; i < nseq; i++)
            if (glen[i]) OUT_CK(hipMemcpyAsync((char *)g->genome.p + start[i], seq[i], glen[i], kind, g->st), -3);
        OUT_CK(hipMemcpyAsync(g->gstart.p, start, 8ULL * nseq + 8, hipMemcpyHostToDevice, g->st), -3);
        OUT_CK(hipStreamSynchronize(g->st), -3);
        return 0;
    };
    s = step();
    delete[] start;
    return s;
}
int lnr_outgpu_set_genome(lnr_outgpu *g, const uint8_t *const *seq, const uint64_t *glen, uint32_t nseq, char *err, size_t err_cap) {
    return set_genome_from(g, seq, glen, nseq, hipMemcpyHostToDevice, err, err_cap);
}
int lnr_outgpu_set_genome_dev(lnr_outgpu *g, const uint8_t *const *d_seq, const uint64_t *glen, uint32_t nseq, char *err, size_t err_cap) {
    return set_genome_from(g, d_seq, glen, nseq, hipMemcpyDeviceToDevice, err, err_cap);
}

int lnr_outgpu_format(lnr_outgpu *g, const lnr_outgpu_batch *b, const char **text, uint64_t *size, char *err, size_t err_cap) {
    static const char empty[1] = "";
    for (double &m : g->ms) m = 0;
    g->bz = lnr_outgpu_bgzf_stats{};
    const u32 n = b->n_reads;
    if (n == 0) { *text = empty; *size = 0; return 0; }
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    OUT_CK(hipSetDevice(g->device), -3);
    int s;
    ReadArgs A;
    A.P.gblob = (const char *)g->gblob.p; A.P.goff = (const u64 *)g->goff.p; A.P.glen = (const u64 *)g->glen.p; A.P.nseq = g->nseq;
    A.P.thd_large_X = b->thd_large_X; A.P.thd_DI = b->thd_DI; A.P.thd_X = b->thd_X;
    A.what = b->what;
    const bool seq = b->reads != nullptr;      // SAM / BAM with SEQ: b->read_len holds n + 1 offsets in both forms
    A.seq = seq ? 1 : 0;
    A.Q = SeqArgs{(const uint8_t *)g->genome.p, (const u64 *)g->gstart.p, b->reads};
    // read ids: once per call, '\0'-separated blob + offsets
    double t0 = wall_ms();
    const u64 id_bytes = b->id_off[n - 1] + strlen(b->read_ids + b->id_off[n - 1]) + 1;
    if ((s = dev_need(g->ids, id_bytes, err, err_cap)) || (s = dev_need(g->idoff, 8ULL * n, err, err_cap)) || (s = dev_need(g->sizes, 8ULL * (n + 1ULL), err, err_cap))) return s;
    OUT_CK(hipMemcpyAsync(g->ids.p, b->read_ids, id_bytes, hipMemcpyHostToDevice, g->st), -3);
    OUT_CK(hipMemcpyAsync(g->idoff.p, b->id_off, 8ULL * n, hipMemcpyHostToDevice, g->st), -3);
    A.ids = (const char *)g->ids.p; A.idoff = (const u64 *)g->idoff.p;
    if (b->dev_form) {
        A.coff = b->cord_off; A.cs = b->cords_str; A.ce = b->cords_end; A.len = b->read_len; A.len_is_off = 1;
    } else {
        if ((s = dev_need(g->coff, 8ULL * (n + 1ULL), err, err_cap)) || (s = dev_need(g->cs, 8ULL * b->n_cords + 8, err, err_cap)) ||
            (s = dev_need(g->ce, 8ULL * b->n_cords + 8, err, err_cap)) || (s = dev_need(g->len, 8ULL * (n + 1ULL), err, err_cap))) return s;
        OUT_CK(hipMemcpyAsync(g->coff.p, b->cord_off, 8ULL * (n + 1ULL), hipMemcpyHostToDevice, g->st), -3);
        if (b->n_cords) {
            OUT_CK(hipMemcpyAsync(g->cs.p, b->cords_str, 8ULL * b->n_cords, hipMemcpyHostToDevice, g->st), -3);
            OUT_CK(hipMemcpyAsync(g->ce.p, b->cords_end, 8ULL * b->n_cords, hipMemcpyHostToDevice, g->st), -3);
        }
        OUT_CK(hipMemcpyAsync(g->len.p, b->read_len, 8ULL * (n + (seq ? 1ULL : 0ULL)), hipMemcpyHostToDevice, g->st), -3);
        if (seq) {
            const u64 bases = b->read_len[n];
            if ((s = dev_need(g->reads, bases + 1, err, err_cap))) return s;
            if (bases) OUT_CK(hipMemcpyAsync(g->reads.p, b->reads, bases, hipMemcpyHostToDevice, g->st), -3);
            A.Q.reads = (const uint8_t *)g->reads.p;
        }
        A.coff = (const u64 *)g->coff.p; A.cs = (const u64 *)g->cs.p; A.ce = (const u64 *)g->ce.p; A.len = (const u64 *)g->len.p; A.len_is_off = seq ? 1 : 0;
    }
    OUT_CK(hipStreamSynchronize(g->st), -3);
    g->ms[0] = wall_ms() - t0;
    u64 *sizes = (u64 *)g->sizes.p;
    OUT_CK(hipEventRecord(g->ev[0], g->st), -3);
    const bool bam = b->what == 3;
    const auto launch = bam ? launch_format<Bam> : b->what == 4 ? launch_format<Paf> : seq ? launch_format<SamSeq> : launch_format<Text>;
    launch(false, n, g->st, A, sizes, nullptr);
    OUT_CK(hipEventRecord(g->ev[1], g->st), -3);
    hipLaunchKernelGGL(k_out_scan, dim3(1), dim3(1024), 0, g->st, sizes, n);
    OUT_CK(hipEventRecord(g->ev[2], g->st), -3);
    OUT_CK(hipMemcpyAsync(g->h_total, sizes + n, sizeof(u64), hipMemcpyDeviceToHost, g->st), -3);
    OUT_CK(hipStreamSynchronize(g->st), -3);
    OUT_CK(hipGetLastError(), -3);
    const u64 total = *g->h_total;
    if ((s = dev_need(g->text, total + 8, err, err_cap))) return s;
    if (!g->bgzf && (s = host_need(g, total, err, err_cap))) return s;
    OUT_CK(hipEventRecord(g->ev[3], g->st), -3);
    launch(true, n, g->st, A, sizes, (char *)g->text.p);
    OUT_CK(hipEventRecord(g->ev[4], g->st), -3);
    OUT_CK(hipStreamSynchronize(g->st), -3);
    OUT_CK(hipGetLastError(), -3);
    float f = 0;
    OUT_CK(hipEventElapsedTime(&f, g->ev[0], g->ev[1]), -3); g->ms[1] = f;
    OUT_CK(hipEventElapsedTime(&f, g->ev[1], g->ev[2]), -3); g->ms[2] = f;
    OUT_CK(hipEventElapsedTime(&f, g->ev[3], g->ev[4]), -3); g->ms[3] = f;
    if (bam && g->sort.on == 1) { *text = empty; *size = 0; return sort_add(g, total, sizes, n, err, err_cap); }      // sort mode: the records stay
    if (g->bgzf) return bgzf_run(g, (const uint8_t *)g->text.p, total, text, size, err, err_cap);      // the text stays on the device
    t0 = wall_ms();
    if (total) OUT_CK(hipMemcpyAsync(g->h_text, g->text.p, total, hipMemcpyDeviceToHost, g->st), -3);
    OUT_CK(hipStreamSynchronize(g->st), -3);
    g->ms[4] = wall_ms() - t0;
    *text = g->h_text; *size = total;
    return 0;
}

void lnr_outgpu_set_bgzf(lnr_outgpu *g, int on) { g->bgzf = on ? 1 : 0; }

int lnr_outgpu_bgzf_bytes(lnr_outgpu *g, const char *bytes, uint64_t size, const char **data, uint64_t *out_size, char *err, size_t err_cap) {
    for (double &m : g->ms) m = 0;
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    OUT_CK(hipSetDevice(g->device), -3);
    int s;
    if (size) {
        if ((s = dev_need(g->text, size + 8, err, err_cap))) return s;
        const double t0 = wall_ms();
        OUT_CK(hipMemcpyAsync(g->text.p, bytes, size, hipMemcpyHostToDevice, g->st), -3);
        OUT_CK(hipStreamSynchronize(g->st), -3);
        g->ms[0] = wall_ms() - t0;
    }
    return bgzf_run(g, (const uint8_t *)g->text.p, size, data, out_size, err, err_cap);
}

void lnr_outgpu_bgzf_stats_get(const lnr_outgpu *g, lnr_outgpu_bgzf_stats *out) { *out = g->bz; }

// ---- sort mode
int lnr_outgpu_sort_begin(lnr_outgpu *g, uint64_t max_bytes, char *err, size_t err_cap) {
    if (g->sort.on) { snprintf(err, err_cap, "the sort mode is on already"); return -1; }
    g->sort.on = 1; g->sort.max_bytes = max_bytes;
    return 0;
}

int lnr_outgpu_sort_spill(lnr_outgpu *g, uint64_t max_host_bytes, char *err, size_t err_cap) {
    if (g->sort.on != 1) { snprintf(err, err_cap, "the sort mode is not collecting"); return -1; }
    g->sort.spill = max_host_bytes ? 1 : 0; g->sort.max_host = max_host_bytes;
    return 0;
}

void lnr_outgpu_sort_hold_info_get(const lnr_outgpu *g, lnr_outgpu_hold_info *out) { *out = g->sort.hold; }

int lnr_outgpu_sort_finish(lnr_outgpu *g, uint32_t piece_members, char *err, size_t err_cap) {
    SortState &S = g->sort;
    if (S.on != 1) { snprintf(err, err_cap, "the sort mode is not collecting"); return -1; }
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    OUT_CK(hipSetDevice(g->device), -3);
    const u64 n = S.nrec;
    int s;
    if (n) {
        size_t t1 = 0, t2 = 0, t3 = 0;
        OUT_CK(rocprim::radix_sort_pairs(nullptr, t1, (u64 *)nullptr, (u64 *)nullptr, (u32 *)nullptr, (u32 *)nullptr, (size_t)n, 0u, 64u, g->st), -3);
        OUT_CK(rocprim::exclusive_scan(nullptr, t3, (u64 *)nullptr, (u64 *)nullptr, (u64)0, (size_t)(n + 1), rocprim::plus<u64>(), g->st), -3);
        t2 = t1 > t3 ? t1 : t3;
        if ((s = dev_need(S.k1, 8 * n, err, err_cap)) || (s = dev_need(S.k2, 8 * n, err, err_cap)) || (s = dev_need(S.v1, 4 * n, err, err_cap)) || (s = dev_need(S.v2, 4 * n, err, err_cap)) ||
            (s = dev_need(S.tmp, t2 + 16, err, err_cap)) || (s = dev_need(S.s_addr, 8 * n, err, err_cap)) || (s = dev_need(S.s_size, 8 * (n + 1), err, err_cap)) ||
            (s = dev_need(S.s_off, 8 * (n + 1), err, err_cap)) || (s = dev_need(S.s_flag, 4 * n, err, err_cap)) || (s = dev_need(S.s_end, 8 * n, err, err_cap)) ||
            (s = dev_need(S.s_qoff, 4 * n, err, err_cap)) || (s = dev_need(S.s_lseq, 4 * n, err, err_cap))) return s;
        const SortArrays A{(u64 *)S.key.p, (u32 *)S.flag.p, (u64 *)S.soff.p, (u64 *)S.addr.p, (u32 *)S.size.p, (i64 *)S.end.p, (u32 *)S.qoff.p, (u32 *)S.lseq.p};
        u64 *k1 = (u64 *)S.k1.p, *k2 = (u64 *)S.k2.p;
        u32 *v1 = (u32 *)S.v1.p, *v2 = (u32 *)S.v2.p;
        const u32 grid = (u32)((n + 256) / 256);          // (n + 1 lanes: k_sort_apply writes the scan's last input)
        OUT_CK(hipEventRecord(g->bev[0], g->st), -3);
        hipLaunchKernelGGL(k_sort_prep, dim3(grid), dim3(256), 0, g->st, (const u32 *)A.flag, (const u64 *)A.soff, n, k1, v1);
        size_t tb = t2;
        OUT_CK(rocprim::radix_sort_pairs(S.tmp.p, tb, k1, k2, v1, v2, (size_t)n, 0u, 64u, g->st), -3);          // by (reverse bit, stream offset)
        hipLaunchKernelGGL(k_sort_take, dim3(grid), dim3(256), 0, g->st, (const u64 *)A.key, (const u32 *)v2, n, k1);
        tb = t2;
        OUT_CK(rocprim::radix_sort_pairs(S.tmp.p, tb, k1, k2, v2, v1, (size_t)n, 0u, 64u, g->st), -3);          // stably by key: k2 sorted keys, v1 the order
        hipLaunchKernelGGL(k_sort_apply, dim3(grid), dim3(256), 0, g->st, A, (const u32 *)v1, n, (u64 *)S.s_addr.p, (u64 *)S.s_size.p, (u32 *)S.s_flag.p, (i64 *)S.s_end.p, (u32 *)S.s_qoff.p, (u32 *)S.s_lseq.p);
        tb = t2;
        OUT_CK(rocprim::exclusive_scan(S.tmp.p, tb, (u64 *)S.s_size.p, (u64 *)S.s_off.p, (u64)0, (size_t)(n + 1), rocprim::plus<u64>(), g->st), -3);
        OUT_CK(hipEventRecord(g->bev[1], g->st), -3);
        OUT_CK(hipMemcpyAsync(g->h_sort, (u64 *)S.s_off.p + n, 8, hipMemcpyDeviceToHost, g->st), -3);
        OUT_CK(hipStreamSynchronize(g->st), -3);
        OUT_CK(hipGetLastError(), -3);
        float f = 0;
        OUT_CK(hipEventElapsedTime(&f, g->bev[0], g->bev[1]), -3);
        S.info.sort_ms = f;
        if (g->h_sort[0] != S.stream) { snprintf(err, err_cap, "sort: the sorted records have %llu bytes, %llu were kept", (unsigned long long)g->h_sort[0], (unsigned long long)S.stream); return -8; }
    }
    S.members = (S.stream + lnr_def::BLOCK_TEXT - 1) / lnr_def::BLOCK_TEXT;
    S.cursor = 0;
    S.piece_members = piece_members ? (piece_members < 65536u ? piece_members : 65536u) : 4096u;
    S.info.records = n; S.info.record_bytes = S.stream; S.info.members = S.members;
    u64 held = 0;
    for (const SortSeg &sg : S.segs) held += sg.cap + 8;
    for (const Buf *b : sort_bufs(S)) held += b->cap;
    S.info.device_bytes = held;
    S.on = 2;
    return 0;
}

int lnr_outgpu_sort_next(lnr_outgpu *g, const char **data, uint64_t *size, const uint64_t **moff, uint32_t *nb, char *err, size_t err_cap) {
    static const char empty[1] = "";
    SortState &S = g->sort;
    if (S.on != 2) { snprintf(err, err_cap, "the records have not been sorted"); return -1; }
    *data = empty; *size = 0; *moff = nullptr; *nb = 0;
    if (S.cursor >= S.members) return 0;
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    OUT_CK(hipSetDevice(g->device), -3);
    const u64 left = S.members - S.cursor;
    const u32 cnt = left < S.piece_members ? (u32)left : S.piece_members;
    const u64 a = S.cursor * lnr_def::BLOCK_TEXT, b = a + (u64)cnt * lnr_def::BLOCK_TEXT < S.stream ? a + (u64)cnt * lnr_def::BLOCK_TEXT : S.stream;
    int s;
    if ((s = dev_need(g->text, b - a + 8, err, err_cap))) return s;
    OUT_CK(hipEventRecord(g->ev[0], g->st), -3);
    hipLaunchKernelGGL(k_sort_gather, dim3(cnt), dim3(256), 0, g->st, (const u64 *)S.s_off.p, (const u64 *)S.s_addr.p, (const u32 *)S.s_qoff.p, (const u32 *)S.s_lseq.p, S.nrec, a, b, (uint8_t *)g->text.p);
    OUT_CK(hipEventRecord(g->ev[1], g->st), -3);
    if ((s = bgzf_run(g, (const uint8_t *)g->text.p, b - a, data, size, err, err_cap))) return s;
    if (g->bz.blocks != cnt) { snprintf(err, err_cap, "sort: a piece of %u members came back as %llu", cnt, (unsigned long long)g->bz.blocks); return -8; }
    S.moff.resize((size_t)cnt + 1);
    OUT_CK(hipMemcpy(S.moff.data(), g->msize.p, 8ULL * (cnt + 1ULL), hipMemcpyDeviceToHost), -3);      // msize after its scan: the members' offsets
    float f = 0;
    OUT_CK(hipEventElapsedTime(&f, g->ev[0], g->ev[1]), -3);
    S.info.gather_ms += f; S.info.deflate_ms += g->bz.deflate_ms; S.info.pack_ms += g->bz.pack_ms; S.info.download_ms += g->ms[4];
    S.cursor += cnt;
    *moff = S.moff.data(); *nb = cnt;
    return 0;
}

int lnr_outgpu_sort_fetch(lnr_outgpu *g, uint64_t *key, uint32_t *flag, int64_t *end, uint64_t *off, char *err, size_t err_cap) {
    SortState &S = g->sort;
    if (S.on != 2) { snprintf(err, err_cap, "the records have not been sorted"); return -1; }
    const u64 n = S.nrec;
    off[0] = 0;
    if (!n) return 0;
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    OUT_CK(hipSetDevice(g->device), -3);
    OUT_CK(hipMemcpy(key, S.k2.p, 8 * n, hipMemcpyDeviceToHost), -3);
    OUT_CK(hipMemcpy(flag, S.s_flag.p, 4 * n, hipMemcpyDeviceToHost), -3);
    OUT_CK(hipMemcpy(end, S.s_end.p, 8 * n, hipMemcpyDeviceToHost), -3);
    OUT_CK(hipMemcpy(off, S.s_off.p, 8 * (n + 1), hipMemcpyDeviceToHost), -3);
    return 0;
}

void lnr_outgpu_sort_info_get(const lnr_outgpu *g, lnr_outgpu_sort_info *out) { *out = g->sort.info; }

void lnr_outgpu_sort_end(lnr_outgpu *g) {
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    (void)hipSetDevice(g->device);
    (void)hipStreamSynchronize(g->st);
    sort_free(g);
}

void lnr_outgpu_times(const lnr_outgpu *g, double *ms5) { for (int i = 0; i < 5; i++) ms5[i] = g->ms[i]; }

void lnr_outgpu_close(lnr_outgpu *g) {
    if (!g) return;
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    (void)hipSetDevice(g->device);
    free_all(g);
    delete g;
}

}  // extern "C"
