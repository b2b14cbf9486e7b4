// lnr_output_hd.h -- the per-read formatters of lnr_output.cpp (SAM records, APF text, BAM records) as __host__ __device__ code over raw arrays.
//
// PRODUCT code: the kernels of lnr_output_kernels.hip call these functions on the device; tests/output_shim.cpp compiles the same text
// with g++ so that every byte is pinned on a machine without a GPU (tests/test_output_hd_cpu.py).  The host writer lnr_writer_format keeps
// its own std::string form in lnr_output.cpp and is the yardstick this file is compared with.
//
// Unit of work: the ITEM = one cord j (1 <= j < n) of a read.
//   APF  item j = the '@' header when cord j - 1 ends a block, then the '|' line of cord j          (print_cords_apf f_io.cpp:100-207)
//   SAM  item j = the whole record line when cord j starts a record (j == 1 or ifCreateNew_ between j - 1 and j), else nothing
//                                                                                                 (cords2BamLink f_io.cpp:899-1011)
//   PAF  item j = the PAF line of the record that cord j starts, else nothing                      (no counterpart in the reference)
// An item is written through a SINK with put(char): CountSink measures, a byte sink emits, one body serves both, so size and content
// cannot disagree.  No std::string / std::vector: a record's CIGAR is streamed through a one-element merge window (appendCigarShrink
// only ever looks at the last element), the SA:Z summary of a record is a second walk over its cords.
// With SEQ (sam_item_seq) a record line is head, SEQ, tail; the SEQ is a stream of SEGMENTS (bases of the genome, of the read, or the per-base
// comparison of an X element) that comes off the walk that prints the CIGAR: serially through the sink here, dealt to a wave in the kernels.
#pragma once
#include <stdint.h>
#include <math.h>
#include "ref_sort.h"      // LNR_HD

namespace lnr_out {

typedef uint64_t u64;
typedef int64_t i64;
typedef uint32_t u32;

struct Params {                 // plain data: what the writer knows about the genome and the preset
    const char *gblob;          // genome names, '\0'-separated
    const u64 *goff;            // nseq: start of name g in gblob
    const u64 *glen;            // nseq
    u32 nseq;
    u64 thd_large_X;
    i64 thd_DI, thd_X;
};

LNR_HD inline u64 cx(u64 v) { return (v >> 20) & ((1ULL << 30) - 1); }
LNR_HD inline u64 cy(u64 v) { return v & 0xfffffULL; }
LNR_HD inline u64 cid(u64 v) { return (v >> 50) & 1023ULL; }
LNR_HD inline u64 cstrand(u64 v) { return (v >> 61) & 1ULL; }
LNR_HD inline bool cend(u64 v) { return (v >> 60) & 1ULL; }
LNR_HD inline u64 shift_cord(u64 v, i64 x, i64 y) { return (u64)((i64)v + (x << 20) + y); }
LNR_HD inline i64 iabs(i64 v) { return v < 0 ? -v : v; }

// ---- sinks and text primitives
struct CountSink { u64 n = 0; LNR_HD void put(char) { n++; } };
struct ByteSink { char *p; LNR_HD void put(char c) { *p++ = c; } };

template <class S> LNR_HD inline void put_str(S &s, const char *z) { for (; *z; z++) s.put(*z); }
// decimal by hand: digits are taken low to high into 4-bit slots of one register (no array, no scratch) and handed out high to low;
// 16 digits per register, the 4 more a 64-bit value may have go first
template <class S> LNR_HD inline void put_dec16(S &s, u64 v, int min_digits) {
    u64 acc = 0; int k = 0;
    do { acc = (acc << 4) | (v % 10); v /= 10; k++; } while (v || k < min_digits);
    while (k--) { s.put((char)('0' + (acc & 15))); acc >>= 4; }
}
template <class S> LNR_HD inline void put_u(S &s, u64 v) {
    const u64 P16 = 10000000000000000ULL;
    if (v >= P16) { put_dec16(s, v / P16, 1); put_dec16(s, v % P16, 16); }
    else put_dec16(s, v, 1);
}
template <class S> LNR_HD inline void put_i(S &s, i64 v) {
    if (v < 0) { s.put('-'); put_u(s, (u64)0 - (u64)v); }
    else put_u(s, (u64)v);
}
LNR_HD inline const char *gname(const Params &P, u64 g) { return g < P.nseq ? P.gblob + P.goff[g] : "*"; }

// ---- APF
template <class S> LNR_HD inline void apf_item(S &out, const Params &P, const u64 *c, u64 n, u64 j, u64 L, const char *rid, bool blank_before) {
    bool head = cend(c[j - 1]);
    if (head) {
        u64 m = j; int main_cnt = 0, block_len = 0;
        while (m < n && !cend(c[m])) { if (cstrand(c[m])) main_cnt++; block_len++; m++; }
        char main_icon = main_cnt > block_len / 2 ? '-' : (main_cnt == block_len / 2 ? (cstrand(c[j]) ? '-' : '+') : '+');
        u64 e = m < n ? m : n - 1;                    // the block's last cord: its end flag, or the read's last cord
        u64 r_end = cy(c[e]) + 96, s_end = cx(c[e]) + 96;
        if (blank_before) out.put('\n');
        u64 g = cid(c[j]);
        out.put('@'); out.put(' '); put_str(out, rid); out.put(' ');
        put_u(out, L); out.put(' ');
        put_u(out, cy(c[j])); out.put(' ');
        put_u(out, r_end < L ? r_end : L); out.put(' ');
        out.put(main_icon); out.put(' ');
        put_str(out, gname(P, g)); out.put(' ');
        put_u(out, g < P.nseq ? P.glen[g] : 0); out.put(' ');
        put_u(out, cx(c[j])); out.put(' ');
        put_u(out, s_end); out.put('\n');
    }
    i64 d1 = 0, d2 = 0;
    if (!head) { d1 = (i64)(cx(c[j]) - cx(c[j - 1])); d2 = (i64)(cy(c[j]) - cy(c[j - 1])); }
    out.put('|'); out.put(' ');
    put_u(out, cy(c[j])); out.put(' ');
    put_u(out, cx(c[j])); out.put(' ');
    put_i(out, d2); out.put(' ');
    put_i(out, d1); out.put(' ');
    out.put(cstrand(c[j]) ? '-' : '+');
    out.put('\n');
}

// ---- SAM
LNR_HD inline int if_create_new(u64 c1s, u64 c1e, u64 c2s, u64 thd_large_X) {      // ifCreateNew_ f_io.cpp:674-692
    u64 x11 = cx(c1s), y11 = cy(c1s), x12 = cx(c1e), y12 = cy(c1e), x21 = cx(c2s), y21 = cy(c2s);
    return cend(c1s) || x11 > x21 || y11 > y21 || ((i64)(x21 - x12) > (i64)thd_large_X && (i64)(y21 - y12) > (i64)thd_large_X) || cstrand(c1s ^ c2s);
}
// cord i is the last of its record
LNR_HD inline bool rec_last(const u64 *cs, const u64 *ce, u64 n, u64 i, u64 thd_large_X) { return i == n - 1 || if_create_new(cs[i], ce[i], cs[i + 1], thd_large_X); }
// cord j is the first of a record
LNR_HD inline bool rec_first(const u64 *cs, const u64 *ce, u64 j, u64 thd_large_X) { return j == 1 || if_create_new(cs[j - 1], ce[j - 1], cs[j], thd_large_X); }

// (float)|DI| / (float)thd_DI, correctly rounded and never fused: 160 / 80 must stay 2, an approximate reciprocal makes it 2.0000002 -> 3 pieces
LNR_HD inline float div_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// The CIGAR of one record as a stream of merged elements: Ops::op(char, u32 count, index of the element)
template <class Ops> struct Merge {                   // appendCigarShrink f_io.cpp:659-669 with a window of one element
    Ops &ops; char op = 0; u32 cnt = 0; u32 idx = 0; bool have = false;
    LNR_HD explicit Merge(Ops &o) : ops(o) {}
    LNR_HD void flush() { if (have) { ops.op(op, cnt, idx); idx++; have = false; } }
    LNR_HD void push(char o, u32 k) { flush(); op = o; cnt = k; have = true; }               // push_back
    LNR_HD void shrink(char o, u32 k) { if (have && op == o) cnt += k; else push(o, k); }
};
template <class M> LNR_HD inline void rect(M &m, u64 a, u64 b, int f_m) {                     // createRectangleCigarPair f_io.cpp:697-718
    u64 dx = cx(b) - cx(a), dy = cy(b) - cy(a);
    char o1 = f_m ? 'X' : '=', o2; u32 n1, n2;
    if (dx >= dy) { o2 = 'D'; n1 = (u32)dy; n2 = (u32)(dx - dy); }
    else { o2 = 'I'; n1 = (u32)dx; n2 = (u32)(dy - dx); }
    if (n1) m.shrink(o1, n1);
    if (n2) m.shrink(o2, n2);
}
template <class M> LNR_HD inline void cord2cigar(M &m, u64 c1s, u64 c1e, u64 c2s, i64 thd_DI, i64 thd_X) {   // cord2cigar_ f_io.cpp:758-875
    // (its diagonal check against the previous cord's return value cannot fail here: that value IS c1s, by construction of the caller)
    u64 x12 = cx(c1e), y12 = cy(c1e), x21 = cx(c2s), y21 = cy(c2s);
    if (x12 < x21 && y12 < y21) {
        rect(m, c1s, c1e, 0);
        i64 DI = (i64)(x21 - x12 - y21 + y12);
        i64 X = (i64)(x21 - x12 < y21 - y12 ? x21 - x12 : y21 - y12);
        if (iabs(DI) > thd_DI && X > thd_X) {
            i64 split_n = (i64)ceilf(div_rn((float)iabs(DI), (float)thd_DI));
            if (X < split_n) split_n = X;
            i64 split_DI = thd_DI, split_X = X / split_n;
            u64 s = c1e;
            for (i64 i = 0; i < split_n - 1; i++) {
                u64 e = DI < 0 ? shift_cord(s, split_X, split_X + split_DI) : shift_cord(s, split_X + split_DI, split_X);
                rect(m, s, e, 0);
                s = e;
            }
            rect(m, s, c2s, 1);
        } else rect(m, c1e, c2s, 1);
    } else rect(m, c1s, c2s, 0);
}
// every element of the record whose first cord is lo, in order; returns the record's last cord
template <class Ops> LNR_HD inline u64 record_ops(Ops &ops, const Params &P, const u64 *cs, const u64 *ce, u64 n, u64 lo, u64 L) {
    Merge<Ops> m(ops);
    if (cy(cs[lo]) != 0) m.push('S', (u32)cy(cs[lo]));                       // insertNewBamRecord align_util.cpp:325-333
    u64 i = lo;
    for (;; i++) {
        bool last = rec_last(cs, ce, n, i, P.thd_large_X);
        cord2cigar(m, cs[i], ce[i], last ? ce[i] : cs[i + 1], P.thd_DI, P.thd_X);
        if (last) break;
    }
    i64 clipped = (i64)(int)(L - cy(ce[i]));
    if (clipped > 0) m.push('S', (u32)clipped);
    m.flush();
    return i;
}
// prints the elements; `seq` = bases the record's SEQ has (S I = X take one from the read or the genome each, D none)
template <class S> struct TextOps {
    S &out; u32 k = 0; u64 seq = 0;
    LNR_HD explicit TextOps(S &o) : out(o) {}
    LNR_HD void op(char o, u32 c, u32) { put_u(out, c); out.put(o); k++; if (o != 'D') seq += c; }
};
struct SazOps {                                                               // createSAZTagCigar align_util.cpp:452-520
    u64 s0 = 0, cm = 0, nm = 0; i64 ci = 0;
    LNR_HD void op(char o, u32 c, u32 idx) {
        if (idx == 0 && o == 'S') s0 = c;
        else if (o == '=') cm += c;
        else if (o == 'X') { cm += c; nm += c; }
        else if (o == 'I') { ci -= c; nm += c; }
        else if (o == 'D') { ci += c; nm += c; }
    }
};
LNR_HD inline unsigned rec_flag(const u64 *cs, u64 lo) { return (lo == 1 ? 0u : 2048u) | (cstrand(cs[lo]) ? 16u : 0u); }

// the line of record number `it` (of n_rec) whose first cord is lo = head, SEQ, tail
// head: QNAME .. TLEN and the tab before SEQ; returns the bases of the record's SEQ
template <class S> LNR_HD inline u64 sam_head(S &out, const Params &P, const u64 *cs, const u64 *ce, u64 n, u64 lo, u64 L, const char *qname) {
    put_str(out, qname); out.put('\t');
    put_u(out, rec_flag(cs, lo)); out.put('\t');
    put_str(out, gname(P, (u64)(int)cid(cs[lo]))); out.put('\t');
    put_i(out, (i64)cx(cs[lo]) + 1); put_str(out, "\t255\t");
    TextOps<S> t(out);
    record_ops(t, P, cs, ce, n, lo, L);
    if (t.k == 0) out.put('*');
    put_str(out, "\t*\t0\t0\t");
    return t.seq;
}
// the entries of SA:Z: every other record of the read, in record order
template <class S> LNR_HD inline void sa_entries(S &out, const Params &P, const u64 *cs, const u64 *ce, u64 n, u64 L, u64 it) {
    u64 a = 1;
    for (u64 jr = 0; a < n; jr++) {
        SazOps z;
        u64 b = record_ops(z, P, cs, ce, n, a, L);
        if (jr != it) {
            // NM cache (createSAZTagCigarOneChimeric align_util.cpp:642-678): a record's NM is summed the first time any line lists it --
            // line 0 lists all others first, line 1 lists record 0 first; every later listing prints 0
            bool first_visit = it == 0 || (it == 1 && jr == 0);
            put_str(out, gname(P, (u64)(int)cid(cs[a]))); out.put(',');
            put_i(out, (i64)cx(cs[a]) + 1); out.put(',');
            out.put(cstrand(cs[a]) ? '-' : '+'); out.put(',');
            put_u(out, z.s0); out.put('S');
            put_u(out, (unsigned)z.cm); out.put('M');
            put_u(out, (unsigned)iabs(z.ci)); out.put(z.ci < 0 ? 'I' : 'D');
            put_str(out, "0S,255,");
            put_i(out, first_visit ? (int)z.nm : 0); out.put(';');
        }
        a = b + 1;
    }
}
// tail: the tab after SEQ, QUAL, SA:Z, end of line
template <class S> LNR_HD inline void sam_tail(S &out, const Params &P, const u64 *cs, const u64 *ce, u64 n, u64 L, u64 it, u64 n_rec) {
    put_str(out, "\t*");
    if (n_rec > 1) { put_str(out, "\tSA:Z:"); sa_entries(out, P, cs, ce, n, L, it); }
    out.put('\n');
}
template <class S> LNR_HD inline void sam_item(S &out, const Params &P, const u64 *cs, const u64 *ce, u64 n, u64 lo, u64 L, const char *qname, u64 it, u64 n_rec) {
    sam_head(out, P, cs, ce, n, lo, L, qname);
    out.put('*');                                      // SEQ not printed
    sam_tail(out, P, cs, ce, n, L, it, n_rec);
}

// ---- SEQ of a record (-ss 1: fillBamRecordLinkRecords align_util.cpp:745-808 with f_is_align == 0, cigar2SamSeq :1434-1500)
// Two iterators walk the record's CIGAR: the genome from (sequence id, POS), the read from its first base -- for flag 16 from the first base
// of its reverse complement.  S and I take their bases from the read, '=' takes them from the GENOME, X prints the read's base where it
// differs from the genome's and N where it does not, D only moves the genome on.  A source position outside its sequence (undefined in the
// reference) reads as ordinal 0 here; ordinals above 4 read as N.
struct SeqSrc {                 // plain data: where the bases of one read's records come from
    const uint8_t *genome;      // every sequence back to back, one Dna5 ordinal per byte
    const u64 *gstart;          // nseq: first base of sequence g in genome
    const u64 *glen;            // nseq
    u32 nseq;
    const uint8_t *read;        // the read, forward
    u64 L;
    const uint8_t *const *gseq = nullptr;      // host writer: nseq separately held sequences instead of genome + gstart
};
struct RecSrc { const uint8_t *g; u64 gl; const uint8_t *read; u64 L; bool rev; };     // the two sources of ONE record: its genome sequence, the read and its strand
LNR_HD inline RecSrc rec_src(const SeqSrc &q, const u64 *cs, u64 lo) {
    const u64 g = (u64)(int)cid(cs[lo]);
    const bool ok = g < q.nseq;
    return RecSrc{ok ? (q.gseq ? q.gseq[g] : q.genome + q.gstart[g]) : nullptr, ok ? q.glen[g] : 0, q.read, q.L, cstrand(cs[lo]) != 0};
}
enum { SEG_READ = 0, SEG_GENOME = 1, SEG_X = 2 };
LNR_HD inline u32 seq_read_ord(const RecSrc &r, u64 y) {                           // base y of the read, or of its reverse complement
    if (y >= r.L) return 0;
    u32 b = r.rev ? r.read[r.L - 1 - y] : r.read[y];
    return b > 3 ? 4u : (r.rev ? 3u - b : b);
}
LNR_HD inline u32 seq_genome_ord(const RecSrc &r, u64 x) {
    if (x >= r.gl) return 0;
    u32 b = r.g[x];
    return b > 4 ? 4u : b;
}
LNR_HD inline u32 seq_ord(const RecSrc &r, u32 kind, u64 x, u64 y) {               // 0..4 = ACGTN
    if (kind == SEG_GENOME) return seq_genome_ord(r, x);
    u32 o = seq_read_ord(r, y);
    if (kind == SEG_X && o == seq_genome_ord(r, x)) o = 4;
    return o;
}
LNR_HD inline char seq_char(const RecSrc &r, u32 kind, u64 x, u64 y) {
    return (char)((0x4e54474341ULL >> (8 * seq_ord(r, kind, x, y))) & 0xff);       // "ACGTN"
}
// The SEQ as a stream of SEGMENTS off the walk that prints the CIGAR: F::seg(number, kind, position in SEQ, genome x, read y, bases)
template <class F> struct SegOps {
    F &f; u64 x, y = 0, p = 0; u32 k = 0;
    LNR_HD SegOps(F &f_, u64 x0) : f(f_), x(x0) {}
    LNR_HD void op(char o, u32 c, u32) {
        if (o == 'D') { x += c; return; }
        const u32 kind = o == '=' ? SEG_GENOME : (o == 'X' ? SEG_X : SEG_READ);
        f.seg(k++, kind, p, x, y, c);
        p += c; y += c;
        if (kind != SEG_READ) x += c;
    }
};
template <class F> LNR_HD inline void record_segs(F &f, const Params &P, const u64 *cs, const u64 *ce, u64 n, u64 lo, u64 L) {
    SegOps<F> s(f, cx(cs[lo]));
    record_ops(s, P, cs, ce, n, lo, L);
}
template <class S> struct SeqPrint {              // the serial form: base after base through the sink
    S &out; RecSrc r;
    LNR_HD void seg(u32, u32 kind, u64, u64 x, u64 y, u32 c) { for (u32 i = 0; i < c; i++) out.put(seq_char(r, kind, x + i, y + i)); }
};
template <class S> LNR_HD inline void sam_item_seq(S &out, const Params &P, const SeqSrc &q, const u64 *cs, const u64 *ce, u64 n, u64 lo, const char *qname, u64 it, u64 n_rec) {
    u64 bases = sam_head(out, P, cs, ce, n, lo, q.L, qname);
    if (bases == 0) out.put('*');
    else { SeqPrint<S> sp{out, rec_src(q, cs, lo)}; record_segs(sp, P, cs, ce, n, lo, q.L); }
    sam_tail(out, P, cs, ce, n, q.L, it, n_rec);
}

// ---- BAM records (-ot 4 / 8: the reference hands its records to SeqAn's writer, write_bam.h:99-203).  A record is the plain re-encoding of
// its SAM line, little endian: block_size, refID (index of RNAME, -1 for '*'), pos = POS - 1, l_read_name, mapq 255, bin, n_cigar_op, flag,
// l_seq, next_refID -1, next_pos -1, tlen 0, QNAME '\0', one word count << 4 | op per CIGAR element (MIDNSHP=X = 0..8), SEQ at two bases
// per byte (high nibble first, =ACMGRSVTWYHKDBN = 0..15), l_seq bytes 0xff, and where the line has one the tag SA:Z.  Without SEQ l_seq is 0.
// Fields narrower than their value take its low bits, as SeqAn's casts do: a QNAME of 255 or more characters (l_read_name is one byte) and
// more than 65535 CIGAR elements (n_cigar_op is two) give records no reader can walk; both are outside the tested ground.  How far real
// input stays from the second bound: the longest record of the `long` case (tests/cases.py, reads of up to 2^20 - 1 bases with 10 % errors)
// has 12 491 elements, from the error-free half of its 800 kb chimera (asserted in tests/test_gpu_long_reads.py); an error-free read of
// 2^20 - 1 bases, the most a read can bring, has 35 836 (tests/test_cli_golden_cpu.py).
// bam_head: block_size, core, QNAME, CIGAR words.  bam_tail: the tag.  Between them: packed SEQ and the 0xff run.
struct BamCount {                                 // one walk before the first byte: CIGAR elements, reference bases, SEQ bases
    u32 k = 0; u64 reflen = 0, seq = 0;
    LNR_HD void op(char o, u32 c, u32) { k++; if (o != 'D') seq += c; if (o == '=' || o == 'X' || o == 'D') reflen += c; }
};
LNR_HD inline u32 bam_op(char o) { return o == 'S' ? 4u : o == 'I' ? 1u : o == 'D' ? 2u : o == '=' ? 7u : o == 'X' ? 8u : 0u; }
template <class S> struct BamOps {                // the CIGAR words
    S &out;
    LNR_HD explicit BamOps(S &o) : out(o) {}
    LNR_HD void op(char o, u32 c, u32) { const u32 w = (c << 4) | bam_op(o); for (int b = 0; b < 4; b++) out.put((char)(w >> (8 * b))); }
};
template <class S> LNR_HD inline void put_le(S &s, u64 v, int bytes) { for (int b = 0; b < bytes; b++) s.put((char)(v >> (8 * b))); }
LNR_HD inline u32 reg2bin(u32 beg, u32 end) {     // the bin of [beg, end) in the usual BAM scheme
    --end;
    if (beg >> 14 == end >> 14) return 4681 + (beg >> 14);
    if (beg >> 17 == end >> 17) return 585 + (beg >> 17);
    if (beg >> 20 == end >> 20) return 73 + (beg >> 20);
    if (beg >> 23 == end >> 23) return 9 + (beg >> 23);
    if (beg >> 26 == end >> 26) return 1 + (beg >> 26);
    return 0;
}
LNR_HD inline u64 str_len(const char *z) { u64 n = 0; while (z[n]) n++; return n; }
// bytes of bam_head for a QNAME of qlen characters and k CIGAR elements
LNR_HD inline u64 bam_head_size(u64 qlen, u32 k) { return 36 + qlen + 1 + 4ULL * k; }
LNR_HD inline u64 bam_packed(u64 l_seq) { return (l_seq + 1) >> 1; }
// c: the record's counts; l_seq: the SEQ bases the record will carry (c.seq or 0); tag: bytes of bam_tail
template <class S> LNR_HD inline void bam_head(S &out, const Params &P, const u64 *cs, const u64 *ce, u64 n, u64 lo, u64 L, const char *qname, const BamCount &c, u64 l_seq, u64 tag) {
    const u64 qlen = str_len(qname), g = (u64)(int)cid(cs[lo]);
    const u32 pos = (u32)cx(cs[lo]);
    put_le(out, bam_head_size(qlen, c.k) - 4 + bam_packed(l_seq) + l_seq + tag, 4);
    put_le(out, g < P.nseq ? g : ~0ULL, 4);
    put_le(out, pos, 4);
    out.put((char)(qlen + 1)); out.put((char)255);
    put_le(out, reg2bin(pos, pos + (u32)c.reflen), 2);
    put_le(out, c.k, 2);
    put_le(out, rec_flag(cs, lo), 2);
    put_le(out, l_seq, 4);
    put_le(out, ~0ULL, 8);                        // next_refID, next_pos
    put_le(out, 0, 4);                            // tlen
    put_str(out, qname); out.put('\0');
    BamOps<S> w(out);
    record_ops(w, P, cs, ce, n, lo, L);
}
template <class S> LNR_HD inline void bam_tail(S &out, const Params &P, const u64 *cs, const u64 *ce, u64 n, u64 L, u64 it, u64 n_rec) {
    if (n_rec > 1) { put_str(out, "SAZ"); sa_entries(out, P, cs, ce, n, L, it); out.put('\0'); }
}
LNR_HD inline u32 seq_nib(const RecSrc &r, u32 kind, u64 x, u64 y) { return (0xf8421u >> (4 * seq_ord(r, kind, x, y))) & 15u; }     // A 1, C 2, G 4, T 8, N 15
template <class S> struct SeqPack {               // the serial form: two bases per byte through the sink
    S &out; RecSrc r; u32 half = 0; bool odd = false;
    LNR_HD void seg(u32, u32 kind, u64, u64 x, u64 y, u32 c) {
        for (u32 i = 0; i < c; i++) {
            const u32 nb = seq_nib(r, kind, x + i, y + i);
            if (odd) out.put((char)(half | nb)); else half = nb << 4;
            odd = !odd;
        }
    }
    LNR_HD void finish() { if (odd) out.put((char)half); }
};
// q == nullptr: no SEQ (l_seq 0)
template <class S> LNR_HD inline void bam_item(S &out, const Params &P, const SeqSrc *q, const u64 *cs, const u64 *ce, u64 n, u64 lo, u64 L, const char *qname, u64 it, u64 n_rec) {
    BamCount c;
    record_ops(c, P, cs, ce, n, lo, L);
    const u64 l_seq = q ? c.seq : 0;
    CountSink t;
    bam_tail(t, P, cs, ce, n, L, it, n_rec);
    bam_head(out, P, cs, ce, n, lo, L, qname, c, l_seq, t.n);
    if (l_seq) {
        SeqPack<S> sp{out, rec_src(*q, cs, lo)};
        record_segs(sp, P, cs, ce, n, lo, L);
        sp.finish();
        for (u64 i = 0; i < l_seq; i++) out.put((char)0xff);
    }
    bam_tail(out, P, cs, ce, n, L, it, n_rec);
}

// ---- PAF (lnr_writer_format_paf*: include/linear_amd.h has the line's definition).  One line per SAM record, from the same walk: the
// twelve columns need the sums of the record's elements, so a counting walk comes first and a printing walk writes the cg tag.  The two
// clips are taken where record_ops takes them -- from the first cord's y and the last cord's end -- because an element stream of one
// single S does not say which of the two it is.
struct PafCount {                                 // matches, block length, reference bases, elements of cg; first and last S
    u64 match = 0, block = 0, ref = 0, s_first = 0, s_last = 0; u32 k = 0;
    LNR_HD void op(char o, u32 c, u32) {
        if (o == 'S') return;
        k++; block += c;
        if (o == '=') match += c;
        if (o != 'I') ref += c;
    }
};
template <class S> struct PafCgOps {              // the elements of cg:Z: -- the CIGAR* without its S elements
    S &out;
    LNR_HD explicit PafCgOps(S &o) : out(o) {}
    LNR_HD void op(char o, u32 c, u32) { if (o != 'S') { put_u(out, c); out.put(o); } }
};
template <class S> LNR_HD inline void paf_item(S &out, const Params &P, const u64 *cs, const u64 *ce, u64 n, u64 lo, u64 L, const char *qname) {
    PafCount c;
    const u64 hi = record_ops(c, P, cs, ce, n, lo, L);
    const i64 clipped = (i64)(int)(L - cy(ce[hi]));
    c.s_first = cy(cs[lo]); c.s_last = clipped > 0 ? (u64)clipped : 0;
    const bool rev = cstrand(cs[lo]) != 0;
    const u64 g = (u64)(int)cid(cs[lo]), x = cx(cs[lo]);
    put_str(out, qname); out.put('\t');
    put_u(out, L); out.put('\t');
    put_u(out, rev ? c.s_last : c.s_first); out.put('\t');
    put_u(out, L - (rev ? c.s_first : c.s_last)); out.put('\t');
    out.put(rev ? '-' : '+'); out.put('\t');
    put_str(out, gname(P, g)); out.put('\t');
    put_u(out, g < P.nseq ? P.glen[g] : 0); out.put('\t');
    put_u(out, x); out.put('\t');
    put_u(out, x + c.ref); out.put('\t');
    put_u(out, c.match); out.put('\t');
    put_u(out, c.block); put_str(out, "\t255");
    if (c.k) { put_str(out, "\tcg:Z:"); PafCgOps<S> t(out); record_ops(t, P, cs, ce, n, lo, L); }
    out.put('\n');
}

// ---- one read, item after item (what the host shim runs; the kernels deal the items of a read to the lanes of a wave instead)
template <class S> LNR_HD inline void paf_read(S &out, const Params &P, const u64 *cs, const u64 *ce, u64 n, u64 L, const char *qname) {
    for (u64 j = 1; j < n; j++)
        if (rec_first(cs, ce, j, P.thd_large_X)) paf_item(out, P, cs, ce, n, j, L, qname);
}
template <class S> LNR_HD inline void apf_read(S &out, const Params &P, const u64 *c, u64 n, u64 L, const char *rid, bool blank_before) {
    for (u64 j = 1; j < n; j++) apf_item(out, P, c, n, j, L, rid, blank_before);
}
template <class S> LNR_HD inline void sam_read(S &out, const Params &P, const u64 *cs, const u64 *ce, u64 n, u64 L, const char *qname) {
    u64 n_rec = 0;
    for (u64 j = 1; j < n; j++) n_rec += rec_first(cs, ce, j, P.thd_large_X);
    u64 it = 0;
    for (u64 j = 1; j < n; j++)
        if (rec_first(cs, ce, j, P.thd_large_X)) sam_item(out, P, cs, ce, n, j, L, qname, it++, n_rec);
}
template <class S> LNR_HD inline void sam_read_seq(S &out, const Params &P, const SeqSrc &q, const u64 *cs, const u64 *ce, u64 n, const char *qname) {
    u64 n_rec = 0;
    for (u64 j = 1; j < n; j++) n_rec += rec_first(cs, ce, j, P.thd_large_X);
    u64 it = 0;
    for (u64 j = 1; j < n; j++)
        if (rec_first(cs, ce, j, P.thd_large_X)) sam_item_seq(out, P, q, cs, ce, n, j, qname, it++, n_rec);
}
template <class S> LNR_HD inline void bam_read(S &out, const Params &P, const SeqSrc *q, const u64 *cs, const u64 *ce, u64 n, u64 L, const char *qname) {
    u64 n_rec = 0;
    for (u64 j = 1; j < n; j++) n_rec += rec_first(cs, ce, j, P.thd_large_X);
    u64 it = 0;
    for (u64 j = 1; j < n; j++)
        if (rec_first(cs, ce, j, P.thd_large_X)) bam_item(out, P, q, cs, ce, n, j, L, qname, it++, n_rec);
}

// ---- the coordinate sort of a record stream (lnr_writer_sort_*): what decides a record's place, read from the raw record at ANY byte
// alignment (byte loads only).  end = pos + max(1, reference bases of the CIGAR: the counts of M D N = X), the end the index bins by.
// `avail`: bytes that may be read from rec (at least 36); CIGAR words past 4 + block_size or past avail are not looked at.
struct BamKey { int32_t ref, pos; u32 flag, block_size; i64 end; };
LNR_HD inline u32 le32_at(const uint8_t *p) { return (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24; }
LNR_HD inline BamKey bam_key(const uint8_t *rec, u64 avail) {
    BamKey k;
    k.block_size = le32_at(rec);
    k.ref = (int32_t)le32_at(rec + 4);
    k.pos = (int32_t)le32_at(rec + 8);
    k.flag = (u32)rec[18] | (u32)rec[19] << 8;
    const u64 lim = 4ULL + k.block_size < avail ? 4ULL + k.block_size : avail;
    u64 p = 36ULL + rec[12];                      // l_read_name holds the low 8 bits of a longer name's length: the name ends at its NUL
    while (p - 1 < lim && rec[12] && rec[p - 1] != 0) p += 256;
    u32 n = (u32)rec[16] | (u32)rec[17] << 8;
    u64 ref_bases = 0;
    for (; n && p + 4 <= lim; n--, p += 4) {
        const u32 w = le32_at(rec + p), op = w & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_bases += w >> 4;
    }
    k.end = (i64)k.pos + (i64)(ref_bases ? ref_bases : 1);
    return k;
}
// the sort key of the order's first two fields: (uint32)refID, then (uint32)pos -- refID -1 sorts last
LNR_HD inline u64 bam_sort_key(const BamKey &k) { return (u64)(u32)k.ref << 32 | (u64)(u32)k.pos; }
// The quality span of a raw record of `size` = 4 + block_size bytes (at least 36): the l_seq bytes at qoff = 36 + l_read_name + 4 n_cigar_op +
// (l_seq + 1) / 2, which this writer fills with 0xff (bam_item) -- what the sort mode does not hold and its gather puts back.  The name ends
// where bam_key finds its end.  A span that does not fit in the record (or l_seq 0): {0, 0}, the record is kept whole.
struct BamQual { u32 qoff, l_seq; };
LNR_HD inline BamQual bam_qual_span(const uint8_t *rec, u64 size) {
    const u64 l_seq = le32_at(rec + 20);
    u64 p = 36ULL + rec[12];
    while (p - 1 < size && rec[12] && rec[p - 1] != 0) p += 256;
    p += 4ULL * ((u32)rec[16] | (u32)rec[17] << 8) + ((l_seq + 1) >> 1);
    if (l_seq == 0 || p + l_seq > size || size > 0xffffffffULL) return BamQual{0, 0};
    return BamQual{(u32)p, (u32)l_seq};
}

}  // namespace lnr_out
